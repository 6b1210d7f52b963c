"""CPU tests of the spatial gene modules (flashdeconv_amd/utils/gene_modules.py): the package's host arithmetic against the NumPy
definition in tests/gene_modules_ref.py, the centred textbook definitions and - bit for bit - ``assemble_pairs``; the NaN rules;
Benjamini-Hochberg over the upper triangle; the clustering rule; the conditions the GPU tests (tests/test_gpu_gene_modules.py) rest
on (the exact cases are exactly representable, the planted case separates in the reference alone); the argument checks and the
C ABI.  No GPU."""
import inspect

import numpy as np
import pytest
from scipy import sparse

import fdx_oracle as orc
import fit_tail_ref
import gene_modules_ref as mr
import gene_pairs_ref as gr
import spatial_genes_ref as sr


def _knn_adjacency(n, seed=11):
    return orc.knn_graph_kdtree(fit_tail_ref.tie_free_coords(n, 2, seed), 6)


def _assembled(module_assemble, s):
    return module_assemble(s["n"], s["W"], s["sum_deg_sq"], *(s[name] for name in mr.GENE_PLANES), s["S"], s["X"])


MATRIX_KEYS = ("morans_r", "pearson_r", "z_score", "p_value", "q_value")
VECTOR_KEYS = ("mean", "m2", "variance_moved")


# ---------------------------------------------------------------- the package's host arithmetic
def test_assemble_coexpression_agrees_with_the_centred_definitions():
    """A generic 600-spot case with mean^2 <= 4 var per gene (asserted), so conditioning cannot hide a wrong formula: rtol 1e-9."""
    from flashdeconv_amd.utils.gene_modules import assemble_coexpression
    A = _knn_adjacency(600)
    Y = sr.generic_case(600, 12, 1)
    assert np.all(Y.mean(axis=0) ** 2 <= 4.0 * Y.var(axis=0))
    genes = np.array([3, 0, 11, 7, 5, 9, 1])
    s = mr.planes(Y, A, genes)
    R, pearson = mr.centred(Y, A, genes)
    for mod in (assemble_coexpression, mr.assemble):
        out = _assembled(mod, s)
        np.testing.assert_allclose(out["morans_r"], R, rtol=1e-9, atol=0)
        np.testing.assert_allclose(out["pearson_r"], pearson, rtol=1e-9, atol=0)
        np.testing.assert_allclose(out["mean"], Y.mean(axis=0)[genes], rtol=1e-14, atol=0)
        np.testing.assert_allclose(np.diagonal(out["pearson_r"]), 1.0, rtol=1e-12)
        for key in MATRIX_KEYS:
            assert out[key].shape == (7, 7) and out[key].dtype == np.float64, key
        for key in VECTOR_KEYS:
            assert out[key].shape == (7,) and out[key].dtype == np.float64, key
        assert np.array_equal(out["morans_r"], out["morans_r"].T) and np.array_equal(out["z_score"], out["z_score"].T)
        off = ~np.eye(7, dtype=bool)
        assert np.all((out["p_value"] >= 0) & (out["p_value"] <= 1)) and np.all(out["q_value"][off] >= out["p_value"][off])
        assert np.isnan(np.diagonal(out["q_value"])).all() and np.array_equal(out["q_value"], out["q_value"].T, equal_nan=True)
    # the diagonal is each gene's Moran's I
    svg = sr.planes(Y[:, genes], A)
    morans_i = sr.assemble(svg["n"], svg["W"], svg["sum_deg_sq"], *(svg[name] for name in sr.PLANES))["morans_i"]
    np.testing.assert_allclose(np.diagonal(_assembled(assemble_coexpression, s)["morans_r"]), morans_i, rtol=1e-12)


def test_module_and_reference_agree():
    from flashdeconv_amd.utils.gene_modules import assemble_coexpression
    A = _knn_adjacency(257)
    Y = sr.generic_case(257, 9, 2, constant=(4,))
    s = mr.planes(Y, A, np.arange(9))
    got, want = _assembled(assemble_coexpression, s), _assembled(mr.assemble, s)
    assert set(got) == set(want) == set(MATRIX_KEYS) | set(VECTOR_KEYS)
    for key in MATRIX_KEYS + VECTOR_KEYS:
        assert np.array_equal(np.isnan(got[key]), np.isnan(want[key])), key
        np.testing.assert_allclose(got[key], want[key], rtol=1e-12, atol=0, err_msg=key)


def test_every_entry_equals_assemble_pairs_bit_for_bit():
    """The arithmetic is shared: fed the 17 planes built from the same sums, assemble_pairs returns the bits of the matrix entry."""
    from flashdeconv_amd.utils.gene_modules import assemble_coexpression
    from flashdeconv_amd.utils.gene_pairs import PLANES, assemble_pairs
    A = _knn_adjacency(600)
    Y = sr.generic_case(600, 10, 5, constant=(2,))
    genes = np.array([9, 2, 0, 5, 7, 1])
    s = mr.planes(Y, A, genes)
    out = _assembled(assemble_coexpression, s)
    pairs = np.array([(a, b) for a in range(6) for b in range(6)])
    pp = mr.pair_planes(s, pairs)
    flat = assemble_pairs(s["n"], s["W"], s["sum_deg_sq"], *(pp[name] for name in PLANES))
    dead_pair = np.isnan(flat["morans_r"])
    assert np.array_equal(dead_pair.reshape(6, 6), (np.arange(6)[:, None] == 1) | (np.arange(6)[None, :] == 1))
    for key in ("morans_r", "pearson_r", "z_score"):
        assert np.array_equal(out[key].ravel(), flat[key], equal_nan=True), key
    a, b = pairs[:, 0], pairs[:, 1]
    assert np.array_equal(out["variance_moved"][a][~dead_pair], flat["variance_b_moved"][~dead_pair])
    assert np.array_equal(out["variance_moved"][b][~dead_pair], flat["variance_a_moved"][~dead_pair])
    assert np.isnan(out["variance_moved"][1]) and np.isfinite(np.delete(out["variance_moved"], 1)).all()
    assert np.array_equal(out["mean"][a], flat["mean_a"]) and np.array_equal(out["m2"][b], flat["m2_b"])
    np.testing.assert_allclose(out["p_value"].ravel()[~dead_pair], flat["p_value"][~dead_pair], rtol=1e-13, atol=0)


def test_assemble_pairs_keeps_its_results():
    """The shared helper left assemble_pairs where it was: the reference of the pair entry, key by key."""
    from flashdeconv_amd.utils.gene_pairs import PLANES, assemble_pairs
    A = _knn_adjacency(257)
    Y = sr.generic_case(257, 9, 2, constant=(4,))
    s = gr.planes(Y, A, gr.pair_list(9, 40, 1))
    got = assemble_pairs(s["n"], s["W"], s["sum_deg_sq"], *(s[name] for name in PLANES))
    want = gr.assemble(s["n"], s["W"], s["sum_deg_sq"], *(s[name] for name in gr.PLANES))
    for key in want:
        assert np.array_equal(np.isnan(got[key]), np.isnan(want[key])), key
        np.testing.assert_allclose(got[key], want[key], rtol=1e-12, atol=0, err_msg=key)


# ---------------------------------------------------------------- NaN rules
def test_nan_rules():
    from flashdeconv_amd.utils.gene_modules import assemble_coexpression, modules_from_z
    A = _knn_adjacency(65)
    Y = sr.generic_case(65, 5, 3, constant=(2,))
    s = mr.planes(Y, A, np.arange(5))
    for mod in (assemble_coexpression, mr.assemble):
        out = _assembled(mod, s)
        dead = np.zeros((5, 5), dtype=bool)
        dead[2, :] = dead[:, 2] = True
        for key in ("morans_r", "pearson_r", "z_score", "p_value"):
            assert np.array_equal(np.isnan(out[key]), dead), key
        assert np.array_equal(np.isnan(out["q_value"]), dead | np.eye(5, dtype=bool))
        assert np.isnan(out["variance_moved"][2]) and np.isfinite(out["mean"]).all() and out["m2"][2] == 0
        # no edges; one spot; no spot
        for n, W in ((65, 0), (1, 0), (0, 0)):
            none = mod(n, W, 0, *(s[name] for name in mr.GENE_PLANES), s["S"], s["X"])
            assert all(np.isnan(none[key]).all() for key in MATRIX_KEYS + ("variance_moved",)), (n, W)
    out = _assembled(assemble_coexpression, s)
    labels = modules_from_z(out["z_score"], out["q_value"], min_module_size=1, n_modules=2)
    assert labels[2] == -1 and set(np.delete(labels, 2)) <= {0, 1}
    empty = assemble_coexpression(65, 0, 0, *(s[name] for name in mr.GENE_PLANES), s["S"], s["X"])
    assert (modules_from_z(empty["z_score"], empty["q_value"]) == -1).all()
    with pytest.raises(ValueError, match="six per-gene sums"):
        assemble_coexpression(65, 10, 20, s["u"], s["D"][:3], s["L"], s["DL"], s["ymin"], s["ymax"], s["S"], s["X"])
    with pytest.raises(ValueError, match="S and X must be"):
        assemble_coexpression(65, 10, 20, *(s[name] for name in mr.GENE_PLANES), s["S"][:3], s["X"])


def test_q_values_are_benjamini_hochberg_over_the_upper_triangle():
    from flashdeconv_amd.utils.gene_modules import assemble_coexpression
    A = _knn_adjacency(257)
    Y = sr.generic_case(257, 8, 4, constant=(6,))
    out = _assembled(assemble_coexpression, mr.planes(Y, A, np.arange(8)))
    p = out["p_value"]
    upper = [(a, b) for a in range(8) for b in range(a + 1, 8) if not np.isnan(p[a, b])]
    assert len(upper) == 21                                  # 7 alive genes
    ranked = sorted(upper, key=lambda ab: p[ab])
    m, q, running = len(ranked), {}, 1.0
    for j in range(m, 0, -1):                                # q_(j) = min_{k >= j} p_(k) m / k, at most 1
        running = min(running, p[ranked[j - 1]] * m / j)
        q[ranked[j - 1]] = running
    for (a, b), want in q.items():
        np.testing.assert_allclose(out["q_value"][a, b], want, rtol=1e-14, atol=0)
        assert out["q_value"][b, a] == out["q_value"][a, b]
    assert int(np.isnan(out["q_value"]).sum()) == 64 - 2 * 21


# ---------------------------------------------------------------- what the GPU tests rest on
def test_exact_cases_are_exact_in_any_order():
    """Integers in [0, 7] on the hub graph: the largest term of any sum is (7 * 299)^2 * 300 (L), the largest cross term
    49 * 299 * 300 (X), both far below 2^53, and the reference's sums are the integer sums."""
    A = fit_tail_ref.hub_and_spoke(300)
    Y = sr.exact_case(300, 40, 3)
    genes = mr.gene_list(40, 33, 0)
    s = mr.planes(Y, A, genes)
    Yi, Ai = Y.astype(np.int64)[:, genes], sparse.csr_matrix(A).astype(bool).astype(np.int64)
    lag, deg = Ai @ Yi, sr.degrees(A)
    for key, want in (("S", Yi.T @ Yi), ("X", Yi.T @ lag), ("L", (lag ** 2).sum(0)), ("DL", deg @ lag), ("D", deg @ Yi), ("u", Yi.sum(0))):
        assert np.array_equal(s[key], want), key
    assert np.array_equal(s["X"], s["X"].T) and np.array_equal(s["S"], s["S"].T)
    assert (7 * 299) ** 2 * 300 < 2 ** 53 and 49 * 299 * 300 < 2 ** 53 and s["L"].max() <= (7 * 299) ** 2 * 300
    assert Y.min() == 0 and Y.max() == 7 and np.array_equal(Y, np.round(Y))


def test_gene_lists_and_counts():
    assert mr.GENE_COUNTS == (1, 15, 16, 17, 63, 64, 65, 129) and mr.GM_TILE == 64
    source = open(__file__.replace("tests/test_gene_modules_host.py", "flashdeconv_amd/csrc/gene_module_kernels.cpp")).read()
    assert f"constexpr int GM_TILE = {mr.GM_TILE};" in source
    for G, S in ((1, 1), (40, 1), (40, 40), (1025, 129)):
        genes = mr.gene_list(G, S, 1)
        assert genes.shape == (S,) and len(set(genes.tolist())) == S and genes.min() >= 0 and genes.max() < G and genes[0] == 0
    assert not np.array_equal(mr.gene_list(1025, 129, 1), np.sort(mr.gene_list(1025, 129, 1)))


def test_the_planted_case_separates_in_the_reference_alone():
    """Three patterns of 12 genes and 20 noise genes on the 25 x 24 lattice: the default cut gives exactly the three modules, pure,
    every noise gene in a cluster of at most 2 genes (-1 at min_module_size=3), labels in the order of the tie rule."""
    from flashdeconv_amd.utils.gene_modules import assemble_coexpression, modules_from_z
    Y, truth = mr.planted_case()
    A = mr.lattice_adjacency()
    assert A.nnz == 2 * (25 * 23 + 24 * 24) and sorted(set(sr.degrees(A))) == [2, 3, 4] and (A != A.T).nnz == 0
    assert Y.shape == (600, 56) and (truth == -1).sum() == 20 and all((truth == k).sum() == 12 for k in range(3))
    s = mr.planes(Y, A, np.arange(56))
    ref = _assembled(mr.assemble, s)
    for labels in (mr.modules(ref["z_score"], ref["q_value"]),
                   modules_from_z(*(_assembled(assemble_coexpression, s)[key] for key in ("z_score", "q_value")))):
        assert labels.dtype == np.int64 and labels.max() == 2 and (labels[truth == -1] == -1).all()
        first = []
        for c in range(3):
            members = np.flatnonzero(labels == c)
            assert members.size == 12 and len(set(truth[members])) == 1 and truth[members[0]] >= 0
            first.append(members[0])
        assert first == sorted(first)                        # equal sizes: numbered by the smallest place
    loose = mr.modules(ref["z_score"], ref["q_value"], min_module_size=1)
    assert max(int((loose == loose[a]).sum()) for a in np.flatnonzero(truth == -1)) <= 2
    ia, ib = np.triu_indices(56, 1)
    significant = ref["q_value"][ia, ib] <= 0.05
    assert 150 < significant.sum() < 300 and 2.0 < ref["z_score"][ia, ib][significant].min() < 3.0
    # n_modules cuts the same tree; nothing significant: no module
    assert mr.modules(ref["z_score"], ref["q_value"], n_modules=3, min_module_size=1).max() == 2
    assert (mr.modules(ref["z_score"], np.where(np.isnan(ref["q_value"]), np.nan, 1.0)) == -1).all()
    # scores: a module's score follows its pattern
    sc = mr.scores(Y, np.arange(56), labels, ref["mean"], ref["m2"])
    assert sc.shape == (600, 3) and np.abs(sc.mean(axis=0)).max() < 1e-12


def test_modules_are_numbered_by_size_then_by_place():
    from flashdeconv_amd.utils.gene_modules import modules_from_z
    # three blocks: places {1, 4} (size 2), {0, 3, 5} (size 3), {2, 6, 7} (size 3); within a block z = 10, between the first two
    # z = 2, else 0
    block = np.array([0, 1, 2, 0, 1, 0, 2, 2])
    z = np.where(block[:, None] == block[None, :], 10.0, np.where((block[:, None] < 2) & (block[None, :] < 2), 2.0, 0.0))
    q = np.where(block[:, None] == block[None, :], 0.001, 0.9)
    np.fill_diagonal(q, np.nan)
    for fn in (modules_from_z, mr.modules):
        assert fn(z, q, min_module_size=2).tolist() == [0, 2, 1, 0, 2, 0, 1, 1]
        assert fn(z, q).tolist() == [0, -1, 1, 0, -1, 0, 1, 1]
        assert fn(z, q, n_modules=2).tolist() == [0, 0, 1, 0, 0, 0, 1, 1]
        zd = z.copy()
        zd[0, :] = zd[:, 0] = np.nan                          # a dead gene
        assert fn(zd, q, min_module_size=2).tolist() == [-1, 1, 0, 2, 1, 2, 0, 0]


# ---------------------------------------------------------------- argument checks (nothing touches a GPU)
def test_check_request_refusals():
    from flashdeconv_amd.utils.gene_modules import check_request
    for match, genes in (("1-D array", np.zeros((3, 2), dtype=np.int64)), ("1-D array", 3), ("integer dtype", [0.0, 1.0]),
                         ("integer dtype", np.zeros(2, dtype=bool)), ("between 1 and 4096", np.zeros(0, dtype=np.int64)),
                         ("between 1 and 4096", np.arange(4097)), ("gene index 4 outside \\[0, 4\\)", [0, 4]),
                         ("gene index -1 outside", [0, -1]), ("gene index 2 twice", [2, 0, 2])):
        with pytest.raises(ValueError, match=match):
            check_request((6, 4) if np.size(genes) < 100 else (6, 5000), genes)
    got = check_request((6, 4), [3, 0])
    assert got.dtype == np.int32 and got.flags.c_contiguous and got.tolist() == [3, 0]
    assert check_request((6, 4), np.array([1, 2], dtype=np.uint8)).dtype == np.int32
    assert check_request((6, 5000), np.arange(4096)).shape == (4096,)


def _bad_calls():
    Y = np.ones((6, 4), dtype=np.float32)
    A = sparse.csr_matrix(np.roll(np.eye(6), 1, axis=1) + np.roll(np.eye(6), -1, axis=1))
    ok = [0, 1]
    return [
        (ValueError, "Y must be a 2-D", dict(Y=np.ones(6), graph=A, genes=ok)),
        (ValueError, "at least one gene", dict(Y=np.ones((6, 0)), graph=A, genes=ok)),
        (ValueError, "at least one spot", dict(Y=np.ones((0, 4)), graph=sparse.csr_matrix((0, 0)), genes=ok)),
        (ValueError, "1-D array", dict(Y=Y, graph=A, genes=[(0, 1)])),
        (ValueError, "between 1 and 4096", dict(Y=Y, graph=A, genes=np.zeros(0, dtype=np.int32))),
        (ValueError, "between 1 and 4096", dict(Y=np.ones((6, 5000), dtype=np.float32), graph=A, genes=np.arange(4097))),
        (ValueError, "integer dtype", dict(Y=Y, graph=A, genes=[0.0, 1.0])),
        (ValueError, "outside \\[0, 4\\)", dict(Y=Y, graph=A, genes=[0, 4])),
        (ValueError, "twice", dict(Y=Y, graph=A, genes=[1, 1])),
        (ValueError, "values has 6 rows but the graph has 5 spots", dict(Y=Y, graph=A[:5, :5], genes=ok)),
        (ValueError, "must be symmetric", dict(Y=Y, graph=sparse.csr_matrix(np.roll(np.eye(6), 1, axis=1)), genes=ok)),
        (TypeError, "graph must be a fitted FlashDeconv", dict(Y=Y, graph=np.eye(6), genes=ok)),
        (ValueError, "n_genes must be an integer", dict(Y=Y, graph=A, n_genes=0)),
        (ValueError, "n_genes must be an integer", dict(Y=Y, graph=A, n_genes=4097)),
        (ValueError, "n_genes must be an integer", dict(Y=Y, graph=A, n_genes=2.0)),
        (ValueError, "fdr must be a number", dict(Y=Y, graph=A, genes=ok, fdr=0.0)),
        (ValueError, "fdr must be a number", dict(Y=Y, graph=A, genes=ok, fdr="0.05")),
        (ValueError, "n_modules must be None or a positive", dict(Y=Y, graph=A, genes=ok, n_modules=0)),
        (ValueError, "min_module_size must be a positive", dict(Y=Y, graph=A, genes=ok, min_module_size=0)),
        (ValueError, "scores must be True or False", dict(Y=Y, graph=A, genes=ok, scores=1)),
        (ValueError, "Unknown output", dict(Y=Y, graph=A, genes=ok, output="cupy")),
    ]


@pytest.mark.parametrize("error,match,kw", _bad_calls(), ids=[f"{i}" for i in range(len(_bad_calls()))])
def test_the_entries_check_their_arguments_before_the_gpu(error, match, kw, monkeypatch):
    from flashdeconv_amd import _lib
    from flashdeconv_amd.utils import gene_modules

    def no_gpu():
        raise AssertionError("the GPU was asked for before the arguments were checked")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    with pytest.raises(error, match=match):
        gene_modules.spatial_gene_modules(**kw)
    if set(kw) == {"Y", "graph", "genes"}:
        for entry in (gene_modules.gene_coexpression_sums, gene_modules.spatial_coexpression):
            with pytest.raises(error, match=match):
                entry(**kw)


def test_split_segments_is_checked():
    from flashdeconv_amd.utils.gene_modules import gene_coexpression_sums
    A = sparse.csr_matrix(np.roll(np.eye(6), 1, axis=1) + np.roll(np.eye(6), -1, axis=1))
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="split_segments must be None or a positive integer"):
            gene_coexpression_sums(np.ones((6, 4)), A, [0, 1], split_segments=bad)


def test_model_method_and_deconvolve_fail_early():
    import flashdeconv_amd as fd
    with pytest.raises(RuntimeError, match="has not been fitted"):
        fd.FlashDeconv().get_spatial_gene_modules(np.ones((3, 2)))
    for bad in ("yes", 2.0, None, [10]):
        with pytest.raises(ValueError, match="gene_modules must be True, False or the number"):
            fd.tl.deconvolve(None, None, gene_modules=bad)           # before the data is looked at, let alone fitted
    for bad in (0, -3, 4097):
        with pytest.raises(ValueError, match="n_genes must be an integer"):
            fd.tl.deconvolve(None, None, gene_modules=bad)
    assert inspect.signature(fd.tl.deconvolve).parameters["gene_modules"].default is False
    assert list(inspect.signature(fd.FlashDeconv.get_spatial_gene_modules).parameters) == ["self", "Y", "kw"]
    params = inspect.signature(fd.utils.spatial_gene_modules).parameters
    assert list(params) == ["Y", "graph", "genes", "n_genes", "fdr", "n_modules", "min_module_size", "scores", "output"]
    assert [params[k].default for k in list(params)[2:]] == [None, 500, 0.05, None, 3, True, "numpy"]


# ---------------------------------------------------------------- C ABI and exports
def test_symbols_version_and_exports():
    from flashdeconv_amd import _lib, utils
    from flashdeconv_amd.utils import gene_modules, gene_pairs
    lib = _lib.load()
    assert lib.fdx_version() >= 207
    header = open(_lib.LIB_PATH.replace("flashdeconv_amd/libfdx.so", "include/fdx.h")).read()
    for name, n_args in (("fdx_gene_coexpr_sums_dev", 14), ("fdx_gene_coexpr_sums_csr_dev", 10), ("fdx_gene_module_scores_dev", 15),
                         ("fdx_gene_module_scores_csr_dev", 12)):
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == n_args and name in header
    assert gene_modules.GENE_PLANES == mr.GENE_PLANES and gene_modules.MAX_GENES == 4096
    assert set(gene_modules.__all__) == {"spatial_gene_modules", "spatial_coexpression", "gene_coexpression_sums",
                                         "assemble_coexpression", "modules_from_z", "check_request", "GENE_PLANES", "MAX_GENES"}
    new = ["spatial_gene_modules", "spatial_coexpression", "gene_coexpression_sums", "assemble_coexpression"]
    assert utils.__all__[-4:] == new and all(callable(getattr(utils, name)) for name in new)
    assert utils.__all__[-7:-4] == ["spatial_gene_pairs", "gene_pair_sums", "assemble_pairs"]      # appended: nothing moved
    assert set(gene_pairs.__all__) == {"spatial_gene_pairs", "gene_pair_sums", "assemble_pairs", "check_request", "PLANES"}
    for text in ("eps * mean^2 / var", "Out of scope", "**Inputs.**", "**Sums.**", "**Statistics**", "**Modules**", "**Scores**",
                 "**Order.**", "spatial_autocorrelation", "local_spatial_statistics", "spatial_niches", "Smoothing"):
        assert text in gene_modules.__doc__, text
    for text in ("no floating-point atomics", "split_segments", "bitwise symmetric", "S must be in [1, 4096]", "gene listed twice"):
        assert text in header, text
