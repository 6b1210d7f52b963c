"""Spatial gene modules: which spatially variable genes vary TOGETHER over the tissue - the whole S x S matrix of bivariate Moran's
R of a list of genes over the model's graph, computed on the GPU's float64 matrix cores, the modules (spatial programmes) cut from
it by average-linkage clustering on the host, and a score of every module per spot (additive, not in the reference; Hotspot's
module workflow).

**Inputs.**  ``Y`` and ``graph`` are those of ``utils.gene_pairs``: ``Y`` (n, G) dense float32 or float64 (integers through the
upload rules of ``_lib.upload_matrix``), host or CUDA, any row stride, or CSR from scipy or a CUDA ``torch.sparse_csr`` tensor;
``graph`` a fitted ``FlashDeconv``, a ``_lib.Graph`` or a scipy sparse adjacency.  ``A`` is its symmetric binary adjacency,
``deg_i = sum_j A_ij``, ``W = sum_i deg_i``, ``sum_deg_sq = sum_i deg_i^2``.  ``genes`` is a 1-D array of S DISTINCT column
indices, ``1 <= S <= 4096``; a, b below are places in it.

**Sums.**  Raw sums in float64 on the value converted from its storage type (``fdx_gene_coexpr_sums_dev`` / ``_csr_dev``,
csrc/gene_module_kernels.cpp, on torch's current stream), with ``lag_g,i = sum_{j in N(i)} y_jg`` in the graph's stored neighbour
order::

    per gene (S,):     u = sum y    D = sum deg y    L = sum lag^2    DL = sum deg lag    ymin    ymax
    matrices (S, S):   S_ab = sum_i y_a,i y_b,i        X_ab = sum_i y_a,i lag_b,i

so ``sum y_a^2 = S_aa`` and ``sum y_a lag_a = X_aa``; entry for entry these are the planes of ``gene_pairs.gene_pair_sums``.  The
listed columns are gathered into one dense matrix of the storage type in the graph's order (a CSR entry that is not stored is the
value 0; no float64 copy of ``Y`` is made), and both matrices are contractions over the spots on ``v_mfma_f64_16x16x4_f64``.

**Statistics** (``assemble_coexpression``, pure NumPy float64): the formulas of ``gene_pairs.assemble_pairs`` - one shared
function - broadcast over (a, b) with ``Xab = X[a, b]`` and ``Xba = X[b, a]``::

    mean_a = u_a/n        m2_a = S_aa - u_a^2/n
    C_ab   = (X_ab + X_ba)/2 - mean_a D_b - mean_b D_a + mean_a mean_b W
    morans_r[a, b]  = (n/W) C_ab / sqrt(m2_a m2_b)              (the diagonal: each gene's Moran's I)
    pearson_r[a, b] = (S_ab - u_a u_b/n) / sqrt(m2_a m2_b)
    variance_moved_a = (n/W)^2 (LLc_a - s_a^2/n) / ((n - 1) m2_a),  LLc_a = L_a - 2 mean_a DL_a + mean_a^2 sum_deg_sq,  s_a = D_a - mean_a W
    z_score[a, b] = morans_r[a, b] / sqrt(max(variance_moved_a, variance_moved_b))
    p_value = erfc(z_score / sqrt 2) / 2  (one-sided)
    q_value = Benjamini-Hochberg over the pairs a < b whose p_value is not NaN, mirrored; its diagonal is NaN

``variance_moved_a`` is the pair entry's ``variance_b_moved`` of gene a: the exact variance of R over all reassignments of the
other gene's values to the spots.  **Conditioning**: the expansion in raw sums cancels - ``m2`` loses about ``eps * mean^2 / var``
of its relative accuracy (a gene with mean 100 and variance 1 keeps 12 of 16 digits), and ``C`` and ``LLc`` likewise.  Expression
matrices (counts, ``log1p`` of counts) have means of the order of their standard deviations; a matrix with a large common offset
should have it removed first.

A DEAD gene - ``ymin == ymax`` (decided exactly), ``m2 <= 0`` or a variance that is not positive - makes its whole row and column
NaN (and its ``variance_moved``); ``W == 0`` or ``n < 2`` makes everything NaN.  Nothing raises.

**Modules** (``modules_from_z``, host, scipy): over the alive genes, ``zmax`` the largest off-diagonal z, the dissimilarity
``d_ab = max(0, zmax - (z_ab + z_ba)/2)`` with a zero diagonal, ``scipy.cluster.hierarchy.linkage(squareform(d), "average")``.
Default cut: ``z_thr`` = the smallest z among the pairs a < b with ``q_value <= fdr``, ``fcluster(t = zmax - z_thr,
criterion="distance")`` - UPGMA is linear in z, so merging stops when the average z between two clusters falls below the
significance threshold; without a significant pair every gene is -1.  ``n_modules=C`` cuts with ``criterion="maxclust"`` instead.
A cluster of fewer than ``min_module_size`` genes becomes -1, as does a dead gene; the kept modules are numbered 0, 1, ... by
decreasing size, ties by the smallest place in ``genes``.  Deterministic.

**Scores** (``fdx_gene_module_scores_dev`` / ``_csr_dev``): ``score[i, c] = (1/|M_c|) sum_{a in M_c} (y_a,i - mean_a) / sd_a``,
``sd_a = sqrt(m2_a / n)``, (n, C) float64 in the caller's spot order, a module's genes added in their order in ``genes``.  A score
matrix is a legal ``values`` for ``spatial_autocorrelation``, ``local_spatial_statistics`` and ``spatial_niches``.

**Order.**  No floating-point atomics; two calls return the same bits; every entry of ``S`` and ``X`` and every per-gene number
depends only on the graph, its one or two columns and ``split_segments`` (the graph's positions are summed in splits of that many
segments of 256, default 16, and the split sums added in ascending order) - not on which other genes are listed or on their order;
``S`` is bitwise symmetric.

**Out of scope.**  Smoothing of the scores; permutation p values per pair; more than 4096 genes a call; ``ShardedFlashDeconv``;
normalising ``Y`` (the caller passes the matrix they want scored).
"""
import ctypes

import numpy as np

from .. import _lib
from ._device import device_of, matrix_on_device, resolved_graph
from .gene_pairs import _pair_arithmetic
from .spatial_genes import _benjamini_hochberg, _check_Y_rows

__all__ = ["spatial_gene_modules", "spatial_coexpression", "gene_coexpression_sums", "assemble_coexpression", "modules_from_z",
           "check_request", "GENE_PLANES", "MAX_GENES"]

GENE_PLANES = ("u", "D", "L", "DL", "ymin", "ymax")
MAX_GENES = 4096


def check_request(Y_shape, genes):
    """The genes of a request against the shape of ``Y``, before anything touches the GPU: ``genes`` as a C-contiguous int32 (S,)
    array; ``ValueError`` for a shape other than (S,), a non-integer dtype, ``S < 1``, ``S > 4096``, an index outside ``[0, G)``
    or a gene listed twice."""
    G = int(Y_shape[1])
    a = genes.detach().cpu().numpy() if _lib.is_torch(genes) else np.asarray(genes)
    if a.ndim != 1:
        raise ValueError(f"genes must be a 1-D array of gene indices, got shape {a.shape}")
    if a.dtype.kind not in "iu":
        raise ValueError(f"genes must be of an integer dtype, got {a.dtype}")
    if a.shape[0] < 1 or a.shape[0] > MAX_GENES:
        raise ValueError(f"genes must hold between 1 and {MAX_GENES} gene indices, got {a.shape[0]}")
    if int(a.min()) < 0 or int(a.max()) >= G:
        bad = a[(a < 0) | (a >= G)][0]
        raise ValueError(f"genes holds the gene index {int(bad)} outside [0, {G})")
    values, counts = np.unique(a, return_counts=True)
    if values.size != a.size:
        raise ValueError(f"genes lists the gene index {int(values[counts > 1][0])} twice")
    return np.ascontiguousarray(a, dtype=np.int32)


def _check_split(split_segments):
    if split_segments is None:
        return 0
    if isinstance(split_segments, (bool, np.bool_)) or not isinstance(split_segments, (int, np.integer)) or split_segments < 1:
        raise ValueError(f"split_segments must be None or a positive integer, got {split_segments!r}")
    return int(min(split_segments, 2 ** 31 - 1))


def _coexpr_sums(lib, g, m, n, G, genes, split, device, stream, max_gather_bytes=0):
    """The sums of one call on the staged matrix ``m`` (``matrix_on_device``) as the dict of ``gene_coexpression_sums``."""
    import torch
    S = genes.shape[0]
    counts = np.zeros(3, dtype=np.int64)
    gene_sums = torch.empty((len(GENE_PLANES), S), dtype=torch.float64, device=device)
    cross = torch.empty((2, S, S), dtype=torch.float64, device=device)
    if m[0] == "csr":
        _lib.check(lib.fdx_gene_coexpr_sums_csr_dev(g.handle, ctypes.byref(m[1].view), _lib.ptr_i32(genes), S, split, max_gather_bytes,
                                                    ctypes.c_void_p(gene_sums.data_ptr()), ctypes.c_void_p(cross.data_ptr()),
                                                    _lib.ptr_i64(counts), stream))
    else:
        _, ptr, code, ldy = m
        _lib.check(lib.fdx_gene_coexpr_sums_dev(g.handle, ptr, code, n, G, ldy, _lib.ptr_i32(genes), S, split, max_gather_bytes,
                                                ctypes.c_void_p(gene_sums.data_ptr()), ctypes.c_void_p(cross.data_ptr()),
                                                _lib.ptr_i64(counts), stream))
    host, mats = _lib.tensor_to_host(gene_sums), _lib.tensor_to_host(cross)
    out = {name: host[k] for k, name in enumerate(GENE_PLANES)}
    out.update(S=mats[0], X=mats[1], n=int(counts[0]), W=int(counts[1]), sum_deg_sq=int(counts[2]))
    return out


def _module_scores(lib, g, m, n, G, genes, labels, C, mean, m2, device, stream):
    """The (n, C) scores (CUDA tensor) of the modules ``labels`` (S,) from the genes' means and second moments."""
    import torch
    S = genes.shape[0]
    out = torch.empty((n, C), dtype=torch.float64, device=device)
    if C == 0:
        return out
    size = np.bincount(labels[labels >= 0], minlength=C).astype(np.float64)
    member = labels >= 0
    scale, shift = np.zeros(S), np.zeros(S)
    sd = np.sqrt(m2[member] / float(n))
    scale[member] = 1.0 / (sd * size[labels[member]])
    shift[member] = mean[member] * scale[member]
    inputs = torch.as_tensor(np.stack([scale, shift])).to(device)
    label = np.ascontiguousarray(labels, dtype=np.int32)
    sc, sh, op = (ctypes.c_void_p(t.data_ptr()) for t in (inputs[0], inputs[1], out))
    if m[0] == "csr":
        _lib.check(lib.fdx_gene_module_scores_csr_dev(g.handle, ctypes.byref(m[1].view), _lib.ptr_i32(genes), _lib.ptr_i32(label), S, C, 0,
                                                      sc, sh, op, C, stream))
    else:
        _, ptr, code, ldy = m
        _lib.check(lib.fdx_gene_module_scores_dev(g.handle, ptr, code, n, G, ldy, _lib.ptr_i32(genes), _lib.ptr_i32(label), S, C, sc, sh,
                                                  op, C, stream))
    torch.cuda.current_stream(device).synchronize()          # `inputs` goes back to the allocator with this frame
    return out


def gene_coexpression_sums(Y, graph, genes, split_segments=None):
    """The device half (module docstring): a dict of the six per-gene planes of ``GENE_PLANES`` - numpy float64 (S,) - the matrices
    ``S`` and ``X`` - numpy float64 (S, S) - and the integers ``n``, ``W``, ``sum_deg_sq``.  ``split_segments``: segments of 256
    positions summed as one split (None: 16); it changes the rounding, nothing else.  Shapes and dtypes are checked before
    anything touches the GPU."""
    import torch
    n, G = _check_Y_rows(Y)
    genes = check_request((n, G), genes)
    split = _check_split(split_segments)
    with resolved_graph(graph, n) as g:
        _lib.require_gpu()
        lib = _lib.load()
        device = device_of(Y)
        with torch.cuda.device(device):
            stream = _lib.current_stream(device)
            with matrix_on_device(Y, device) as m:
                return _coexpr_sums(lib, g, m, n, G, genes, split, device, stream)


def assemble_coexpression(n, W, sum_deg_sq, u, D, L, DL, ymin, ymax, S, X):
    """The statistics of the module docstring from the sums of one call (pure host arithmetic): a dict of ``mean``, ``m2``,
    ``variance_moved`` (S,) and ``morans_r``, ``pearson_r``, ``z_score``, ``p_value``, ``q_value`` (S, S)."""
    from scipy.special import erfc
    n, W, sum_deg_sq = int(n), int(W), int(sum_deg_sq)
    planes = [np.asarray(a, dtype=np.float64) for a in (u, D, L, DL, ymin, ymax)]
    S, X = np.asarray(S, dtype=np.float64), np.asarray(X, dtype=np.float64)
    if planes[0].ndim != 1 or any(a.shape != planes[0].shape for a in planes):
        raise ValueError(f"the six per-gene sums must be 1-D arrays of one length, got shapes {[a.shape for a in planes]}")
    k = planes[0].shape[0]
    if S.shape != (k, k) or X.shape != (k, k):
        raise ValueError(f"S and X must be ({k}, {k}) matrices, got shapes {S.shape} and {X.shape}")
    u, D, L, DL, ymin, ymax = planes
    q = np.diagonal(S).copy()
    col = lambda a: a[:, None]                                                   # noqa: E731
    row = lambda a: a[None, :]                                                   # noqa: E731
    m_a, _, m2_a, _, R, pearson, var_b_moved, _, z = _pair_arithmetic(
        n, W, sum_deg_sq, col(u), row(u), col(q), row(q), col(D), row(D), S, X, X.T, col(L), row(L), col(DL), row(DL),
        col(ymin), col(ymax), row(ymin), row(ymax))
    # of gene a alone: the entries of the pair (a, a) - the variance NaN exactly where the gene is dead
    mean, m2, variance_moved = (np.diagonal(np.broadcast_to(x, (k, k))).copy() for x in (m_a, m2_a, var_b_moved))
    p = np.where(np.isnan(z), np.nan, 0.5 * erfc(np.where(np.isnan(z), 0.0, z) / np.sqrt(2.0)))
    q_value = np.full((k, k), np.nan)
    ia, ib = np.triu_indices(k, 1)
    q_value[ia, ib] = _benjamini_hochberg(p[ia, ib])
    q_value[ib, ia] = q_value[ia, ib]
    return {"mean": mean, "m2": m2, "variance_moved": variance_moved, "morans_r": R, "pearson_r": pearson, "z_score": z,
            "p_value": p, "q_value": q_value}


def _check_cut(fdr, n_modules, min_module_size):
    if isinstance(fdr, (bool, np.bool_)) or not isinstance(fdr, (int, float, np.integer, np.floating)) or not 0.0 < float(fdr) <= 1.0:
        raise ValueError(f"fdr must be a number in (0, 1], got {fdr!r}")
    if n_modules is not None and (isinstance(n_modules, (bool, np.bool_)) or not isinstance(n_modules, (int, np.integer))
                                  or n_modules < 1):
        raise ValueError(f"n_modules must be None or a positive integer, got {n_modules!r}")
    if isinstance(min_module_size, (bool, np.bool_)) or not isinstance(min_module_size, (int, np.integer)) or min_module_size < 1:
        raise ValueError(f"min_module_size must be a positive integer, got {min_module_size!r}")
    return float(fdr), None if n_modules is None else int(n_modules), int(min_module_size)


def modules_from_z(z_score, q_value, fdr=0.05, n_modules=None, min_module_size=3):
    """The clustering rule of the module docstring on the (S, S) ``z_score`` and ``q_value`` of ``assemble_coexpression``:
    ``labels`` (S,) int64 - the module of every gene, -1 for a dead, unassigned or too small one; modules numbered by decreasing
    size, ties by the smallest place."""
    from scipy.cluster.hierarchy import fcluster, linkage
    from scipy.spatial.distance import squareform
    fdr, n_modules, min_module_size = _check_cut(fdr, n_modules, min_module_size)
    z, qv = np.asarray(z_score, dtype=np.float64), np.asarray(q_value, dtype=np.float64)
    k = z.shape[0]
    labels = np.full(k, -1, dtype=np.int64)
    alive = np.flatnonzero(~np.isnan(np.diagonal(z)))
    if alive.size < 2:
        return labels
    za, qa = z[np.ix_(alive, alive)], qv[np.ix_(alive, alive)]
    ia, ib = np.triu_indices(alive.size, 1)
    sym = 0.5 * (za + za.T)
    zmax = float(np.maximum(za[ia, ib], za[ib, ia]).max())
    d = np.maximum(zmax - sym, 0.0)
    np.fill_diagonal(d, 0.0)
    tree = linkage(squareform(d, checks=False), "average")
    if n_modules is None:
        significant = qa[ia, ib] <= fdr
        if not significant.any():
            return labels
        z_thr = float(za[ia, ib][significant].min())
        cluster = fcluster(tree, t=zmax - z_thr, criterion="distance")
    else:
        cluster = fcluster(tree, t=n_modules, criterion="maxclust")
    ids, first, sizes = np.unique(cluster, return_index=True, return_counts=True)
    kept = [j for j in range(ids.size) if sizes[j] >= min_module_size]
    kept.sort(key=lambda j: (-int(sizes[j]), int(first[j])))
    for c, j in enumerate(kept):
        labels[alive[cluster == ids[j]]] = c
    return labels


def _check_output(output):
    if output not in ("numpy", "torch"):
        raise ValueError(f"Unknown output: {output}. Choose from 'numpy', 'torch'.")


def spatial_coexpression(Y, graph, genes):
    """The S x S spatial co-expression of the listed genes (module docstring): a dict of ``morans_r``, ``pearson_r``, ``z_score``,
    ``p_value``, ``q_value`` (S, S), ``mean``, ``m2``, ``variance_moved`` (S,), ``genes`` (S,) int64, ``n`` and ``n_edges``.
    Arguments are checked before anything touches the GPU."""
    genes = check_request(_check_Y_rows(Y), genes)
    s = gene_coexpression_sums(Y, graph, genes)
    out = assemble_coexpression(s["n"], s["W"], s["sum_deg_sq"], *(s[name] for name in GENE_PLANES), s["S"], s["X"])
    out.update(genes=genes.astype(np.int64), n=s["n"], n_edges=s["W"] // 2)
    return out


def check_selection(n_genes):
    """``n_genes`` of ``spatial_gene_modules(genes=None)``: an integer in [1, 4096] (``ValueError`` otherwise)."""
    if isinstance(n_genes, (bool, np.bool_)) or not isinstance(n_genes, (int, np.integer)) or not 1 <= n_genes <= MAX_GENES:
        raise ValueError(f"n_genes must be an integer in [1, {MAX_GENES}], got {n_genes!r}")
    return int(n_genes)


def spatial_gene_modules(Y, graph, genes=None, n_genes=500, fdr=0.05, n_modules=None, min_module_size=3, scores=True, output="numpy"):
    """Which genes vary together over the tissue, and where: the spatial co-expression matrix of ``genes``, the gene modules cut
    from it and every module's score per spot (module docstring).

    ``Y``: (n_spots, n_genes) - dense numpy / CUDA tensor, float32, float64 or integer counts, or CSR (scipy, CUDA
    ``torch.sparse_csr``); scored as it is passed (not normalised).  ``graph``: a fitted ``FlashDeconv``, a ``_lib.Graph`` or a
    scipy sparse adjacency.  ``genes``: 1-D distinct gene indices (at most 4096), or None to select them:
    ``spatially_variable_genes(Y, graph)`` is called and the first ``n_genes`` of its ``order`` whose ``q_value <= fdr`` are kept;
    with fewer than 2 of them the result has zero modules.  ``fdr``: the significance level of the selection and of the default
    cut.  ``n_modules``: cut the tree into at most that many clusters instead.  ``min_module_size``: smaller clusters are
    unassigned (-1).  ``scores``: also compute the module scores.  ``output``: ``"numpy"``, or ``"torch"`` to leave ``scores`` a
    CUDA tensor.  Every argument is checked before anything touches the GPU.

    Returns the dict of ``spatial_coexpression`` plus ``labels`` (S,) int64, ``n_modules``, ``module_sizes`` (C,) int64,
    ``modules`` - a list of C int64 arrays of gene indices (columns of ``Y``), in the order of ``genes`` - and, with
    ``scores=True``, ``scores`` (n_spots, C) float64 in the caller's spot order: a legal ``values`` for
    ``spatial_autocorrelation``, ``local_spatial_statistics`` and ``spatial_niches``."""
    import torch
    n, G = _check_Y_rows(Y)
    if genes is not None:
        genes = check_request((n, G), genes)
    n_genes = check_selection(n_genes)
    fdr, n_modules, min_module_size = _check_cut(fdr, n_modules, min_module_size)
    if not isinstance(scores, (bool, np.bool_)):
        raise ValueError(f"scores must be True or False, got {scores!r}")
    _check_output(output)
    with resolved_graph(graph, n) as g:
        n_edges = None
        if genes is None:
            from .spatial_genes import spatially_variable_genes
            svg = spatially_variable_genes(Y, g)
            n_edges = svg["n_edges"]
            order = svg["order"][:]
            keep = order[svg["q_value"][order] <= fdr][:n_genes]        # (NaN compares false)
            genes = np.ascontiguousarray(keep, dtype=np.int32)
        _lib.require_gpu()
        lib = _lib.load()
        device = device_of(Y)
        with torch.cuda.device(device):
            stream = _lib.current_stream(device)
            if genes.size < 1:                                    # (a selection that kept nothing)
                out = _empty_result(genes, n, n_edges)
                labels = out["labels"]
                score = torch.empty((n, 0), dtype=torch.float64, device=device)
            else:
                with matrix_on_device(Y, device) as m:
                    s = _coexpr_sums(lib, g, m, n, G, genes, 0, device, stream)
                    out = assemble_coexpression(s["n"], s["W"], s["sum_deg_sq"], *(s[name] for name in GENE_PLANES), s["S"], s["X"])
                    out.update(genes=genes.astype(np.int64), n=s["n"], n_edges=s["W"] // 2)
                    labels = modules_from_z(out["z_score"], out["q_value"], fdr, n_modules, min_module_size)
                    C = int(labels.max()) + 1
                    score = _module_scores(lib, g, m, n, G, genes, labels, C, out["mean"], out["m2"], device, stream) if scores else None
    C = int(labels.max()) + 1 if labels.size else 0
    out.update(labels=labels, n_modules=C, module_sizes=np.bincount(labels[labels >= 0], minlength=C).astype(np.int64),
               modules=[out["genes"][labels == c] for c in range(C)])
    if scores:
        out["scores"] = score if output == "torch" else _lib.tensor_to_host(score)
    return out


def _empty_result(genes, n, n_edges):
    """What ``spatial_gene_modules`` returns where the selection kept no gene: empty statistics, no module."""
    k = genes.size
    nan1, nan2 = np.full(k, np.nan), np.full((k, k), np.nan)
    return {"mean": nan1.copy(), "m2": nan1.copy(), "variance_moved": nan1.copy(), "morans_r": nan2.copy(), "pearson_r": nan2.copy(),
            "z_score": nan2.copy(), "p_value": nan2.copy(), "q_value": nan2.copy(), "genes": genes.astype(np.int64), "n": int(n),
            "n_edges": n_edges, "labels": np.full(k, -1, dtype=np.int64)}
