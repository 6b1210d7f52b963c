"""``deconvolve(adata_st, adata_ref, ...)``: the reference's scanpy-style entry (``flashdeconv/tl/_deconvolve.py:6-174``)
forwarding the same keyword arguments to the MI355X ``FlashDeconv``."""
import numpy as np


def deconvolve(adata_st, adata_ref, cell_type_key="cell_type", *, sketch_dim=512, lambda_spatial="auto", rho_sparsity=0.01,
               n_hvg=2000, n_markers_per_type=50, spatial_method="knn", k_neighbors=6, radius=None, preprocess="log_cpm",
               layer_st=None, layer_ref=None, spatial_key="spatial", key_added="flashdeconv", random_state=0, copy=False,
               spot_diagnostics=False, spatial_stats=False, n_niches=None, spatial_permutations=0, local_stats=False,
               correlogram=False, celltype_expression=False, spatial_genes=False, gene_pairs=None,
               gene_modules=False, niche_genes=False, gene_permutations=0, nhood_enrichment=False, ligrec_pairs=None,
               ligrec_permutations=999, co_occurrence=False):
    """Writes ``.obsm[key_added]`` (proportions DataFrame), ``.obs[key_added + '_dominant']`` and
    ``.uns[key_added + '_params']``; returns the modified copy when ``copy=True``, else ``None``.  ``spot_diagnostics=True``
    (additive) also writes ``.obs[key_added + '_residual']`` (relative sketch residual per spot) and
    ``.obs[key_added + '_roughness']`` (disagreement with the neighbours' abundances, ``neighbor_sq``).  ``spatial_stats=True``
    (additive) also writes ``.uns[key_added + '_moran']`` (DataFrame indexed by cell type: Moran's ``I`` of its proportions over
    the fit's graph and the ``z_score``) and ``.uns[key_added + '_colocalization']`` (cell type x cell type bivariate Moran
    matrix); with ``spatial_permutations=R`` > 0 beside it the rows are reassigned to the spots R times on the GPU
    (``utils.spatial_stats.spatial_permutation_test``, seeded by ``random_state``): the Moran table gains the columns ``p_value``
    and ``z_sim`` and ``.uns[key_added + '_colocalization_pvalue']`` holds the two-sided p value of every pair.
    ``n_niches=<int>`` (additive) also writes ``.obs[key_added + '_niche']`` (Categorical of niche indices: k-means of
    each spot's proportions beside its neighbours' mean proportions, ``FlashDeconv.get_spatial_niches``) and
    ``.uns[key_added + '_niche_composition']`` (DataFrame, niche x cell type: the mean proportions of each niche's spots).
    ``local_stats=True`` (additive) also writes ``.obsm[key_added + '_local_moran']`` (local Moran's I) and
    ``.obsm[key_added + '_hotspot']`` (Getis-Ord Gi*), DataFrames over ``obs_names`` x cell types
    (``FlashDeconv.get_local_spatial_statistics``); with ``spatial_permutations=R`` > 0 beside it also
    ``.obsm[key_added + '_hotspot_pvalue']``, the two-sided conditional-permutation p value of every spot and cell type.
    ``correlogram`` (additive): ``True`` (ten bands of the grid radius), an int (that many bands) or a sequence (the radii) also
    writes ``.uns[key_added + '_correlogram']``, a dict of ``radii``, ``n_pairs`` (unordered pairs per band), ``morans_i`` and
    ``z_score`` (DataFrames, band x cell type) and ``cross`` (band x cell type x cell type): Moran's I and the co-localisation
    matrix by distance band (``FlashDeconv.get_spatial_correlogram``).
    ``celltype_expression=True`` (additive) also writes ``.uns[key_added + '_expression']`` (DataFrame, common genes x cell types:
    what each cell type expresses in this tissue - the per-gene non-negative least squares of the spot matrix on the
    proportions scaled by each spot's row sum over the mean row sum, ``FlashDeconv.get_celltype_expression``) and
    ``.uns[key_added + '_expression_r2']`` (Series over the common genes: the share of each gene's variance the fitted
    composition explains).
    ``spatial_genes=True`` (additive) also writes ``.uns[key_added + '_spatial_genes']`` (DataFrame indexed by the common genes:
    Moran's ``I`` and Geary's ``C`` of each gene of the spot matrix over the fit's graph, the ``z_score`` under normality, the
    one-sided ``p_value`` under randomisation and its Benjamini-Hochberg ``q_value``, and - regressed on the proportions scaled by
    each spot's row sum over the mean row sum - ``residual_I``, ``residual_z_score`` of what the composition leaves and the
    ``r2`` it explains, ``FlashDeconv.get_spatially_variable_genes``); with ``gene_permutations=R`` > 0 beside it (an int >= 0,
    more than 0 only with ``spatial_genes=True``: a ``ValueError`` before the fit otherwise) every gene's values are reassigned to
    the spots R times on the GPU (``utils.gene_permutations.spatial_gene_permutation_test``, seeded by ``random_state``): the
    table gains the columns ``p_sim`` (the one-sided permutation p value of Moran's I), ``q_sim`` and ``z_sim``, and
    ``.uns[key_added + '_params']['gene_permutations']`` holds R.
    ``gene_pairs`` (additive): a non-empty sequence of ``(name_a, name_b)`` - a ligand and its receptor - of ``var_names`` common
    to both objects (an unknown name is a ``ValueError`` before the fit) also writes ``.uns[key_added + '_gene_pairs']``, a
    DataFrame with one row per pair in the caller's order and the columns ``gene_a``, ``gene_b``, ``R`` (the bivariate Moran's R
    of the two genes of the spot matrix over the fit's graph), ``pearson``, ``z_score`` (under the exact permutation variance),
    the one-sided ``p_value`` and its Benjamini-Hochberg ``q_value`` (``FlashDeconv.get_gene_pair_colocalisation``).
    ``gene_modules`` (additive): ``True`` (the 500 most spatially variable of the common genes at most) or an int (that many)
    groups the spatially variable genes of the spot matrix into modules - genes that vary together over the fit's graph,
    ``FlashDeconv.get_spatial_gene_modules`` - and also writes ``.var[key_added + '_module']`` (the module of every gene, -1 for
    one not selected or not assigned), ``.obsm[key_added + '_module_scores']`` (DataFrame, ``obs_names`` x module: the mean
    standardised expression of the module's genes), ``.uns[key_added + '_gene_modules']`` (DataFrame with one row per module:
    ``size``, ``mean_R`` - the mean bivariate Moran's R between its genes - and ``genes``, their names) and
    ``.uns[key_added + '_params']['gene_modules']``; anything else is a ``ValueError`` before the fit.
    ``niche_genes=True`` (additive; needs ``n_niches``, a ``ValueError`` before the fit otherwise) also writes
    ``.uns[key_added + '_niche_genes']``, a long DataFrame of the 50 genes that mark each niche best - the columns ``niche``,
    ``gene``, ``z_score`` and ``auc`` (Wilcoxon rank-sum test of the niche's spots against all others on the spot matrix),
    ``log2_fold_change``, ``pct``, ``pct_rest`` (the share of spots that express the gene, inside and outside the niche) and
    ``q_value`` (Benjamini-Hochberg over the genes), by decreasing ``z_score`` inside a niche
    (``FlashDeconv.get_niche_genes``) - and ``.uns[key_added + '_params']['niche_genes']``.
    ``nhood_enrichment=True`` (additive; anything but a bool is a ``ValueError`` before the fit) also writes
    ``.uns[key_added + '_nhood_enrichment']``, a dict of three DataFrames indexed both ways by niche index when ``n_niches`` is
    given, else by cell type (each spot labelled by its dominant one): ``count`` (how often a spot of the row's label has a
    neighbour of the column's over the fit's graph), ``zscore`` (the count against ``spatial_permutations`` random reassignments of
    the labels to the spots on the GPU, 999 when that is 0, seeded by ``random_state``) and ``pvalue`` (two-sided)
    (``FlashDeconv.get_neighborhood_enrichment``) - and ``.uns[key_added + '_params']['nhood_enrichment']``, the number of
    permutations.
    ``ligrec_pairs`` (additive): a non-empty sequence of ``(ligand, receptor)`` names, resolved as ``gene_pairs`` resolves them (an
    unknown name or a bad ``ligrec_permutations`` - an int >= 0 - is a ``ValueError`` before the fit), also writes
    ``.uns[key_added + '_ligrec']``, a dict of three DataFrames with one row per pair, named ``ligand_receptor``, and a
    (``source``, ``target``) MultiIndex of columns over the niche indices when ``n_niches`` is given, else over the cell types
    (each spot labelled by its dominant one): ``means`` (the mean of the ligand in the source's spots and of the receptor in the
    target's, halved), ``pvalues`` (one-sided, against ``ligrec_permutations`` random reassignments of the labels to the spots on
    the GPU, seeded by ``random_state``; NaN where a group is empty or expresses its gene in under 1 % of its spots) and
    ``qvalues`` (Benjamini-Hochberg over all of them) (``FlashDeconv.get_ligand_receptor``) - and
    ``.uns[key_added + '_params']['ligrec']``, the number of permutations.
    ``co_occurrence`` (additive): ``True`` (ten bands of the grid radius), an int (that many bands) or a sequence (the radii) -
    anything else is a ``ValueError`` before the fit - also writes ``.uns[key_added + '_co_occurrence']``, a dict of ``radii``,
    ``labels`` (the niche indices when ``n_niches`` is given, else the cell types: each spot labelled by its dominant one) and the
    (band, label, label) arrays ``count`` (how often a spot of the first label has one of the second at a distance in the band),
    ``ratio`` (the co-occurrence ratio: the share of the first label's band neighbours that carry the second, over the second's share
    of all the band's pair ends), ``z_score`` (analytic, under random reassignment) and ``p_value`` (two-sided, against as many
    random reassignments of the labels to the spots on the GPU as ``nhood_enrichment`` uses: ``spatial_permutations``, 999 when that
    is 0; seeded by ``random_state``) (``FlashDeconv.get_co_occurrence``) - and ``.uns[key_added + '_params']['co_occurrence']``,
    the request."""
    from ..core.deconv import FlashDeconv
    from ..io import prepare_data, result_to_anndata
    from ..utils.correlogram import correlogram_request
    correlogram_kw = correlogram_request(correlogram)          # a bad request fails here, not behind the fit
    from ..utils.cooccurrence import cooccurrence_request
    co_occurrence_kw = cooccurrence_request(co_occurrence)
    if not isinstance(celltype_expression, (bool, np.bool_)):
        raise ValueError(f"celltype_expression must be True or False, got {celltype_expression!r}")
    if not isinstance(spatial_genes, (bool, np.bool_)):
        raise ValueError(f"spatial_genes must be True or False, got {spatial_genes!r}")
    if isinstance(gene_permutations, (bool, np.bool_)) or not isinstance(gene_permutations, (int, np.integer)) or gene_permutations < 0:
        raise ValueError(f"gene_permutations must be an int >= 0, got {gene_permutations!r}")
    if gene_permutations > 0 and not spatial_genes:
        raise ValueError("gene_permutations > 0 needs spatial_genes=True: the table the permutation columns are added to")
    if not isinstance(gene_modules, (bool, np.bool_)):
        from ..utils.gene_modules import check_selection
        if not isinstance(gene_modules, (int, np.integer)):
            raise ValueError(f"gene_modules must be True, False or the number of genes to group, got {gene_modules!r}")
        module_genes = check_selection(gene_modules)
    else:
        module_genes = 500 if gene_modules else None
    if not isinstance(niche_genes, (bool, np.bool_)):
        raise ValueError(f"niche_genes must be True or False, got {niche_genes!r}")
    if not isinstance(nhood_enrichment, (bool, np.bool_)):
        raise ValueError(f"nhood_enrichment must be True or False, got {nhood_enrichment!r}")
    if niche_genes and n_niches is None:
        raise ValueError("niche_genes=True needs n_niches: the niches whose marker genes are asked for")
    gene_pairs = _pair_names("gene_pairs", gene_pairs, "(name_a, name_b)")
    ligrec_pairs = _pair_names("ligrec_pairs", ligrec_pairs, "(ligand, receptor)")
    if ligrec_pairs is not None:
        from ..utils._device import check_count
        check_count("ligrec_permutations", ligrec_permutations)

    adata = adata_st.copy() if copy else adata_st
    Y, X, coords, names, genes = prepare_data(adata, adata_ref, cell_type_key=cell_type_key, layer_st=layer_st,
                                          layer_ref=layer_ref, spatial_coord_key=spatial_key)
    if celltype_expression:
        from ..utils.expression import check_request
        check_request(tuple(Y.shape), len(names))                # more cell types than the solve takes: fails here too
    if spatial_genes:
        from ..utils.spatial_genes import check_request as check_spatial_genes
        check_spatial_genes(tuple(Y.shape), len(names))
    if niche_genes:
        from ..utils.group_genes import MAX_GROUPS, check_request as check_niche_genes
        check_niche_genes(tuple(Y.shape))
        if isinstance(n_niches, (int, np.integer)) and n_niches > MAX_GROUPS:
            raise ValueError(f"niche_genes is built for at most {MAX_GROUPS} niches, got n_niches = {n_niches}")
    if gene_pairs is not None:
        pair_idx = _pair_columns("gene_pairs", gene_pairs, genes, Y)
    if ligrec_pairs is not None:
        from ..utils.ligrec import check_request as check_ligrec
        ligrec_idx = _pair_columns("ligrec_pairs", ligrec_pairs, genes, Y)
        if n_niches is None:
            if len(names) > 64:
                raise ValueError(f"ligrec_pairs is built for at most 64 labels, got {len(names)} cell types: give n_niches")
            n_groups = len(names)
        else:
            from ..utils.niches import _check_n_niches
            n_groups = _check_n_niches(n_niches, int(Y.shape[0]))
        # the pairs, the caps (distinct genes, pairs x groups^2) and the permutation count: the labels themselves come with the fit
        check_ligrec(tuple(Y.shape), ligrec_idx, np.zeros(int(Y.shape[0]), dtype=np.int32), n_groups, ligrec_permutations)
    # like the reference, max_iter / tol / verbose are not exposed here (tl/_deconvolve.py:132-144)
    model = FlashDeconv(sketch_dim=sketch_dim, lambda_spatial=lambda_spatial, rho_sparsity=rho_sparsity, n_hvg=n_hvg,
                        n_markers_per_type=n_markers_per_type, spatial_method=spatial_method, k_neighbors=k_neighbors,
                        radius=radius, preprocess=preprocess, random_state=random_state, verbose=False)
    proportions = model.fit_transform(Y, X, coords, cell_type_names=names, spot_diagnostics=spot_diagnostics)
    result_to_anndata(proportions, adata, names, key_added=key_added)
    if spot_diagnostics:
        adata.obs[f"{key_added}_residual"] = model.get_spot_residuals()
        adata.obs[f"{key_added}_roughness"] = model.spot_diagnostics_["neighbor_sq"]
    adata.uns[f"{key_added}_params"] = {
        "sketch_dim": sketch_dim,
        "lambda_spatial": float(model.lambda_used_),
        "rho_sparsity": rho_sparsity,
        "n_hvg": n_hvg,
        "n_markers_per_type": n_markers_per_type,
        "spatial_method": spatial_method,
        "k_neighbors": k_neighbors,
        "radius": radius,
        "preprocess": preprocess,
        "n_genes_used": len(model.gene_idx_),
        "n_cell_types": len(names),
        "cell_type_names": list(names),
        "random_state": random_state,
        "converged": model.info_.get("converged", False),
        "n_iterations": model.info_.get("n_iterations", 0),
    }
    if spot_diagnostics:
        adata.uns[f"{key_added}_params"]["spot_diagnostics"] = True
    if spatial_stats:
        import pandas as pd
        stats = model.get_spatial_autocorrelation(n_permutations=spatial_permutations)
        types = [str(t) for t in names]
        moran = {"I": stats["morans_i"], "z_score": stats["z_score"]}
        if spatial_permutations:
            moran.update({"p_value": stats["p_value"], "z_sim": stats["z_sim"]})
            adata.uns[f"{key_added}_colocalization_pvalue"] = pd.DataFrame(stats["cross_p_value"], index=types, columns=types)
            adata.uns[f"{key_added}_params"]["spatial_permutations"] = int(spatial_permutations)
        adata.uns[f"{key_added}_moran"] = pd.DataFrame(moran, index=types)
        adata.uns[f"{key_added}_colocalization"] = pd.DataFrame(stats["cross"], index=types, columns=types)
        adata.uns[f"{key_added}_params"]["spatial_stats"] = True
    if n_niches is not None:
        import pandas as pd
        niches = model.get_spatial_niches(n_niches)
        index = list(range(int(n_niches)))
        adata.obs[f"{key_added}_niche"] = pd.Categorical(niches["labels"], categories=index)
        adata.uns[f"{key_added}_niche_composition"] = pd.DataFrame(niches["composition"], index=index,
                                                                   columns=[str(t) for t in names])
        adata.uns[f"{key_added}_params"]["n_niches"] = int(n_niches)
    if niche_genes:
        import pandas as pd
        ng = model.get_niche_genes(Y, groups=np.asarray(_host(niches["labels"])), n_groups=int(n_niches), n_top=50, output="numpy")
        top = ng["top"]
        niche_of = np.repeat(np.arange(top.shape[0]), top.shape[1])
        flat = top.ravel()
        table = {"niche": niche_of, "gene": [str(genes[j]) for j in flat]}
        for name in ("z_score", "auc", "log2_fold_change", "pct", "pct_rest", "q_value"):
            table[name] = ng[name][niche_of, flat]
        adata.uns[f"{key_added}_niche_genes"] = pd.DataFrame(table)
        adata.uns[f"{key_added}_params"]["niche_genes"] = True
    if nhood_enrichment:
        import pandas as pd
        n_perm = int(spatial_permutations) if spatial_permutations else 999
        if n_niches is not None:
            ne = model.get_neighborhood_enrichment(labels=niches["labels"], n_labels=int(n_niches), n_permutations=n_perm,
                                                   random_state=random_state)
            index = list(range(int(n_niches)))
        else:
            ne = model.get_neighborhood_enrichment(n_permutations=n_perm, random_state=random_state)
            index = [str(t) for t in names]
        adata.uns[f"{key_added}_nhood_enrichment"] = {
            "count": pd.DataFrame(ne["count"], index=index, columns=index),
            "zscore": pd.DataFrame(ne["z_sim"], index=index, columns=index),
            "pvalue": pd.DataFrame(ne["p_value"], index=index, columns=index)}
        adata.uns[f"{key_added}_params"]["nhood_enrichment"] = n_perm
    if co_occurrence_kw is not None:
        n_perm = int(spatial_permutations) if spatial_permutations else 999
        if n_niches is not None:
            co = model.get_co_occurrence(coords, labels=niches["labels"], n_labels=int(n_niches), n_permutations=n_perm,
                                         random_state=random_state, **co_occurrence_kw)
            index = list(range(int(n_niches)))
        else:
            co = model.get_co_occurrence(coords, n_permutations=n_perm, random_state=random_state, **co_occurrence_kw)
            index = [str(t) for t in names]
        adata.uns[f"{key_added}_co_occurrence"] = {"radii": co["radii"], "labels": index, "count": co["count"], "ratio": co["ratio"],
                                                   "z_score": co["z_score"], "p_value": co["p_value"]}
        adata.uns[f"{key_added}_params"]["co_occurrence"] = (True if not co_occurrence_kw else
                                                              co_occurrence_kw.get("n_bands", co_occurrence_kw.get("radii")))
    if ligrec_pairs is not None:
        import pandas as pd
        if n_niches is not None:
            lr = model.get_ligand_receptor(Y, ligrec_idx, labels=niches["labels"], n_labels=int(n_niches),
                                           n_permutations=int(ligrec_permutations), random_state=random_state)
            index = list(range(int(n_niches)))
        else:
            lr = model.get_ligand_receptor(Y, ligrec_idx, n_permutations=int(ligrec_permutations), random_state=random_state)
            index = [str(t) for t in names]
        rows = pd.Index([f"{a}_{b}" for a, b in ligrec_pairs], name="ligand_receptor")
        columns = pd.MultiIndex.from_product([index, index], names=["source", "target"])
        nan = np.full(lr["means"].shape, np.nan)
        adata.uns[f"{key_added}_ligrec"] = {
            name: pd.DataFrame(np.asarray(lr.get(key, nan)).reshape(len(ligrec_pairs), -1), index=rows, columns=columns)
            for name, key in (("means", "means"), ("pvalues", "p_greater"), ("qvalues", "q_value"))}
        adata.uns[f"{key_added}_params"]["ligrec"] = int(ligrec_permutations)
    if local_stats:
        import pandas as pd
        local = model.get_local_spatial_statistics(n_permutations=spatial_permutations)
        types = [str(t) for t in names]
        adata.obsm[f"{key_added}_local_moran"] = pd.DataFrame(local["local_i"], index=adata.obs_names, columns=types)
        adata.obsm[f"{key_added}_hotspot"] = pd.DataFrame(local["gi_star"], index=adata.obs_names, columns=types)
        if spatial_permutations:
            adata.obsm[f"{key_added}_hotspot_pvalue"] = pd.DataFrame(local["p_value"], index=adata.obs_names, columns=types)
            adata.uns[f"{key_added}_params"]["spatial_permutations"] = int(spatial_permutations)
        adata.uns[f"{key_added}_params"]["local_stats"] = True
    if correlogram_kw is not None:
        import pandas as pd
        cg = model.get_spatial_correlogram(coords, **correlogram_kw)
        types = [str(t) for t in names]
        bands = list(range(len(cg["radii"])))
        adata.uns[f"{key_added}_correlogram"] = {
            "radii": cg["radii"], "n_pairs": cg["n_pairs"],
            "morans_i": pd.DataFrame(cg["morans_i"], index=bands, columns=types),
            "z_score": pd.DataFrame(cg["z_score"], index=bands, columns=types),
            "cross": cg["cross"]}
        adata.uns[f"{key_added}_params"]["correlogram"] = (True if not correlogram_kw else
                                                            correlogram_kw.get("n_bands", correlogram_kw.get("radii")))
    if celltype_expression:
        import pandas as pd
        ex = model.get_celltype_expression(Y, spot_scale=_library_scale(Y))
        adata.uns[f"{key_added}_expression"] = pd.DataFrame(ex["expression"].T, index=[str(g) for g in genes],
                                                             columns=[str(t) for t in names])
        adata.uns[f"{key_added}_expression_r2"] = pd.Series(ex["r2"], index=[str(g) for g in genes])
        adata.uns[f"{key_added}_params"]["celltype_expression"] = True
    if spatial_genes:
        import pandas as pd
        sv = model.get_spatially_variable_genes(Y, residual=True, spot_scale=_library_scale(Y), n_permutations=int(gene_permutations),
                                                random_state=random_state)
        columns = {"I": sv["morans_i"], "C": sv["gearys_c"], "z_score": sv["z_score"], "p_value": sv["p_value"], "q_value": sv["q_value"],
                   "residual_I": sv["residual_morans_i"], "residual_z_score": sv["residual_z_score"], "r2": sv["r2"]}
        if gene_permutations:
            columns.update(p_sim=sv["p_sim"], q_sim=sv["q_sim"], z_sim=sv["z_sim"])
        adata.uns[f"{key_added}_spatial_genes"] = pd.DataFrame(columns, index=[str(g) for g in genes])
        adata.uns[f"{key_added}_params"]["spatial_genes"] = True
        if gene_permutations:
            adata.uns[f"{key_added}_params"]["gene_permutations"] = int(gene_permutations)
    if gene_pairs is not None:
        import pandas as pd
        gp = model.get_gene_pair_colocalisation(Y, pair_idx)
        adata.uns[f"{key_added}_gene_pairs"] = pd.DataFrame(
            {"gene_a": [str(a) for a, _ in gene_pairs], "gene_b": [str(b) for _, b in gene_pairs], "R": gp["morans_r"],
             "pearson": gp["pearson_r"], "z_score": gp["z_score"], "p_value": gp["p_value"], "q_value": gp["q_value"]})
        adata.uns[f"{key_added}_params"]["gene_pairs"] = len(gene_pairs)
    if module_genes is not None:
        import pandas as pd
        gm = model.get_spatial_gene_modules(Y, n_genes=module_genes)
        gene_names = [str(g) for g in genes]
        C, labels, R = gm["n_modules"], gm["labels"], gm["morans_r"]
        first = {}                                                # a duplicated name: the first occurrence is the gene used
        for i, name in enumerate(adata.var_names):
            first.setdefault(str(name), i)
        module_of = np.full(len(adata.var_names), -1, dtype=np.int64)
        module_of[[first[gene_names[j]] for j in gm["genes"]]] = labels
        adata.var[f"{key_added}_module"] = module_of
        adata.obsm[f"{key_added}_module_scores"] = pd.DataFrame(np.asarray(_host(gm["scores"])), index=adata.obs_names,
                                                                 columns=list(range(C)))
        within = []
        for c in range(C):
            block = R[np.ix_(labels == c, labels == c)]
            within.append(float(block[~np.eye(block.shape[0], dtype=bool)].mean()) if block.shape[0] > 1 else float("nan"))
        adata.uns[f"{key_added}_gene_modules"] = pd.DataFrame(
            {"size": gm["module_sizes"], "mean_R": within, "genes": [[gene_names[j] for j in members] for members in gm["modules"]]},
            index=list(range(C)))
        adata.uns[f"{key_added}_params"]["gene_modules"] = module_genes
    return adata if copy else None


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def _pair_names(what, pairs, form):
    """``pairs`` of the argument ``what`` as a list of 2-tuples (None stays None); ``ValueError`` for anything but a non-empty
    sequence of pairs."""
    if pairs is None:
        return None
    pairs = [tuple(pair) for pair in pairs]
    if not pairs or any(len(pair) != 2 for pair in pairs):
        raise ValueError(f"{what} must be a non-empty sequence of {form}, got {pairs!r}")
    return pairs


def _pair_columns(what, pairs, genes, Y):
    """The (P, 2) int32 columns of ``Y`` that the named ``pairs`` stand for; ``ValueError`` for a name that is not among ``genes``."""
    from ..utils.gene_pairs import check_request as check_gene_pairs
    column = {str(name): j for j, name in enumerate(genes)}
    for pair in pairs:
        for name in pair:
            if str(name) not in column:
                raise ValueError(f"{what} names the gene {name!r}, which is not among the genes common to both objects")
    return check_gene_pairs(tuple(Y.shape), np.array([[column[str(a)], column[str(b)]] for a, b in pairs], dtype=np.int64))


def _library_scale(Y):
    """Each spot's row sum of ``Y`` over the mean row sum (ones when the matrix is all zero), as a host float64 array."""
    from .. import _lib
    if _lib.is_torch_sparse_csr(Y):
        import torch
        crow = Y.crow_indices().to(torch.int64)
        row_of = torch.repeat_interleave(torch.arange(Y.shape[0], device=Y.device), crow[1:] - crow[:-1])
        rs = torch.zeros(Y.shape[0], dtype=torch.float64, device=Y.device)
        rs.index_add_(0, row_of, Y.values().to(torch.float64))     # (counts: exact in float64 whatever the order)
        rs = _lib.tensor_to_host(rs)
    elif getattr(Y, "is_cuda", False):
        import torch
        rs = _lib.tensor_to_host(Y.sum(dim=1, dtype=torch.float64))
    else:
        rs = np.asarray(Y.sum(axis=1), dtype=np.float64).ravel()
    mean = rs.mean() if rs.size else 0.0
    return rs / mean if mean > 0 else np.ones_like(rs)
