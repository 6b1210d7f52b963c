"""CPU tests of the spatially-variable-gene statistics (flashdeconv_amd/utils/spatial_genes.py): the NumPy definition in
tests/spatial_genes_ref.py against the centred textbook definitions, the package's host arithmetic against it, the NaN rules, the
conditions the GPU tests (tests/test_gpu_spatial_genes.py) rest on, the argument checks and the C ABI.  No GPU."""
import numpy as np
import pytest
from scipy import sparse

import fdx_oracle as orc
import fit_tail_ref
import spatial_genes_ref as sr


def _knn_adjacency(n, seed=11):
    return orc.knn_graph_kdtree(fit_tail_ref.tie_free_coords(n, 2, seed), 6)


def _assembled(module_assemble, s):
    return module_assemble(s["n"], s["W"], s["sum_deg_sq"], *(s[name] for name in sr.PLANES))


def _assert_same(got, want):
    assert set(got) == set(want)
    for key in want:
        a, b = np.asarray(got[key]), np.asarray(want[key])
        assert a.shape == b.shape and a.dtype == b.dtype, (key, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(a, b, equal_nan=True), key


# ---------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("n,G,seed", [(300, 7, 0), (600, 9, 1), (65, 5, 2)])
def test_reference_expansions_agree_with_the_centred_definitions(n, G, seed):
    """Moran's I, Geary's C, m2 and m4 expanded in the raw sums against Z = Y - mean, sum Z (A Z), the edge sum of Geary and
    sum Z^4, rtol 1e-10 - on inputs with mean^2 <= 4 var per gene (asserted), so conditioning cannot hide a wrong formula."""
    A = _knn_adjacency(n)
    Y = sr.generic_case(n, G, seed)
    assert np.all(Y.mean(axis=0) ** 2 <= 4.0 * Y.var(axis=0))
    out = _assembled(sr.assemble, sr.planes(Y, A))
    morans, geary, m2, m4 = sr.centred(Y, A)
    for key, want in (("morans_i", morans), ("gearys_c", geary), ("m2", m2), ("m4", m4)):
        np.testing.assert_allclose(out[key], want, rtol=1e-10, atol=0, err_msg=key)
    np.testing.assert_allclose(out["mean"], Y.mean(axis=0), rtol=1e-14, atol=0)
    # the moments of I against the entry the cell-type statistics use
    from flashdeconv_amd.utils import spatial_stats
    s = sr.planes(Y, A)
    base = spatial_stats.assemble(n, s["W"], s["sum_deg_sq"], m2, np.diag(m2))
    assert out["expected_i"] == base["expected_i"] and out["variance_i"] == base["variance_i"]
    np.testing.assert_allclose(out["variance_i_rand"], spatial_stats.randomization_variance(n, s["W"], s["sum_deg_sq"], m2, m4),
                               rtol=1e-9, atol=0)
    assert np.all((out["p_value"] >= 0) & (out["p_value"] <= 1)) and np.all(out["q_value"] >= out["p_value"])


def test_exact_cases_are_exact_in_any_order():
    """Integers in [0, 7] (one column negated): the largest partial sum of any plane is below 7^4 n (1 + max deg) << 2^53, so the
    planes do not depend on the order of summation and the device must return the reference's numbers."""
    for n, G in ((600, 9), (257, 513)):
        A = _knn_adjacency(n)
        Y = sr.exact_case(n, G, 3)
        Yi = Y.astype(np.int64)
        assert np.array_equal(Yi, Y) and Yi.min() >= 0 and Yi.max() <= 7
        s = sr.planes(Y, A)
        Ai = sparse.csr_matrix(A).astype(np.int64)
        deg = sr.degrees(A)
        for key, want in (("u", Yi.sum(0)), ("q", (Yi ** 2).sum(0)), ("c3", (Yi ** 3).sum(0)), ("c4", (Yi ** 4).sum(0)),
                          ("D", deg @ Yi), ("H", deg @ Yi ** 2), ("P", (Yi * (Ai.astype(bool).astype(np.int64) @ Yi)).sum(0))):
            assert np.array_equal(s[key], want), key
        assert 7 ** 4 * n * (1 + int(deg.max())) < 2 ** 40
    for variant in ("holes", "full"):
        m, Y = sr.csr_contents_case(65, 9, 1, variant)
        assert np.array_equal(np.rint(Y), Y) and np.abs(Y).max() <= 7
        assert (np.diff(m.indptr) == 0).any() == (variant == "holes") and not Y[:, 1].any()
        assert m[:, 1].nnz == (1 if variant == "full" else 0)      # empty but for the stored zero of the full row
        if variant == "full":
            assert (np.diff(m.tocsc().indptr)[[2, 5]] == 65).all() and (np.diff(m.indptr) == 9).any()
            assert sr.planes(Y, _knn_adjacency(65))["ymax"][5] < 0
        assert sr.planes(Y, _knn_adjacency(65))["ymax"][4] == 0 > sr.planes(Y, _knn_adjacency(65))["ymin"][4]


def test_planted_case_separates_the_smooth_gene_in_the_reference():
    """The condition the planted GPU test rests on, on the CPU: on the 25 x 24 grid the gradient leads, the shuffled copy of the
    same values does not autocorrelate, and the constant gene has no statistic."""
    yy, xx = np.mgrid[0:25, 0:24]
    A = orc.grid_graph(np.stack([xx.ravel(), yy.ravel()], 1).astype(np.float64))
    out = _assembled(sr.assemble, sr.planes(sr.planted_case(), A))
    assert out["order"][0] == 0 and out["morans_i"][0] > 0.8 > abs(out["morans_i"][1]) and np.isnan(out["morans_i"][2])
    assert out["gearys_c"][0] < 0.2 and out["q_value"][0] < 1e-6 < 0.05 < out["q_value"][1]


# ---------------------------------------------------------------- the package's host arithmetic
@pytest.mark.parametrize("n,G,seed,constant", [(300, 7, 0, ()), (600, 12, 1, (2, 5)), (65, 5, 2, (0,)), (4, 3, 3, ()), (3, 3, 4, ())])
def test_assemble_genes_equals_the_reference(n, G, seed, constant):
    from flashdeconv_amd.utils.spatial_genes import assemble_genes
    A = _knn_adjacency(n) if n > 4 else sparse.csr_matrix(np.ones((n, n)) - np.eye(n))
    for Y in (sr.generic_case(n, G, seed, constant), sr.exact_case(n, G, seed)):
        s = sr.planes(Y, A)
        want = _assembled(sr.assemble, s)
        _assert_same(_assembled(assemble_genes, s), want)
        assert int(np.isnan(want["morans_i"]).sum()) == (len(constant) if Y.max() > 7 else int((Y.min(0) == Y.max(0)).sum()))


def test_nan_rules():
    from flashdeconv_amd.utils.spatial_genes import assemble_genes
    stat_keys = ("morans_i", "gearys_c", "z_score", "variance_i_rand", "z_score_rand", "p_value", "q_value")
    # a constant gene beside a live one: decided by ymin == ymax, whatever m2 rounds to
    A = _knn_adjacency(100)
    Y = sr.generic_case(100, 3, 5)
    Y[:, 1] = np.float64(np.float32(0.1))
    s = sr.planes(Y, A)
    assert s["q"][1] - s["u"][1] ** 2 / 100 != 0.0           # the cancellation leaves rounding noise: no threshold would do
    for mod in (sr.assemble, assemble_genes):
        out = _assembled(mod, s)
        for key in stat_keys:
            assert np.isnan(out[key][1]) and not np.isnan(out[key][[0, 2]]).any(), key
        assert list(out["order"]) == sorted([0, 2], key=lambda g: -out["morans_i"][g]) + [1]
    # W = 0: nothing has a statistic; expected_i is still -1 / (n - 1)
    s0 = sr.planes(Y, sparse.csr_matrix((100, 100)))
    for mod in (sr.assemble, assemble_genes):
        out = _assembled(mod, s0)
        assert all(np.isnan(out[key]).all() for key in stat_keys) and np.isnan(out["variance_i"]) and out["expected_i"] == -1 / 99
        assert list(out["order"]) == [0, 1, 2]
    # n = 1, 2, 3: no randomisation variance below 4 spots, nothing at all below 2
    for n in (1, 2, 3):
        An = sparse.csr_matrix(np.ones((n, n)) - np.eye(n))
        Yn = sr.generic_case(n, 2, 6)
        for mod in (sr.assemble, assemble_genes):
            out = _assembled(mod, sr.planes(Yn, An))
            for key in ("variance_i_rand", "z_score_rand", "p_value", "q_value"):
                assert np.isnan(out[key]).all(), (n, key)
            assert np.isnan(out["morans_i"]).all() == (n == 1) and np.isnan(out["gearys_c"]).all() == (n == 1)
    _assert_same(_assembled(assemble_genes, sr.planes(Yn, An)), _assembled(sr.assemble, sr.planes(Yn, An)))
    with pytest.raises(ValueError, match="nine sums"):
        assemble_genes(3, 2, 2, *[np.ones(2)] * 8, np.ones(3))


def test_benjamini_hochberg_against_a_hand_case():
    from flashdeconv_amd.utils.spatial_genes import _benjamini_hochberg
    p = np.array([0.01, 0.04, 0.03, np.nan, 0.5])
    # m = 4; sorted 0.01, 0.03, 0.04, 0.5 -> p m / rank = 0.04, 0.06, 0.16 / 3, 0.5 -> running minimum from the right
    want = np.array([0.04, 0.16 / 3, 0.16 / 3, np.nan, 0.5])
    for bh in (_benjamini_hochberg, sr.benjamini_hochberg):
        np.testing.assert_allclose(bh(p), want, rtol=1e-15, atol=0)
        assert np.isnan(bh(np.full(3, np.nan))).all() and bh(np.zeros(0)).shape == (0,)
        assert np.array_equal(bh(np.array([0.9, 0.8])), [0.9, 0.9]) and np.array_equal(bh(np.array([0.7, 1.0])), [1.0, 1.0])


def test_order_with_nan_and_ties():
    from flashdeconv_amd.utils.spatial_genes import _decreasing_order
    x = np.array([0.2, np.nan, 0.5, 0.2, -0.1, np.nan, 0.5])
    for order in (_decreasing_order, sr.decreasing_order):
        got = order(x)
        assert got.dtype == np.int64 and list(got) == [2, 6, 0, 3, 4, 1, 5]


# ---------------------------------------------------------------- argument checks (nothing touches a GPU)
def _bad_calls():
    Y, W = np.ones((6, 4), dtype=np.float32), np.full((6, 3), 0.25)
    A = sparse.csr_matrix(np.roll(np.eye(6), 1, axis=1) + np.roll(np.eye(6), -1, axis=1))
    return [
        (ValueError, "Y must be a 2-D", dict(Y=np.ones(6), graph=A)),
        (ValueError, "at least one gene", dict(Y=np.ones((6, 0)), graph=A)),
        (ValueError, "at least one spot", dict(Y=np.ones((0, 4)), graph=sparse.csr_matrix((0, 0)))),
        (ValueError, "values has 6 rows but the graph has 5 spots", dict(Y=Y, graph=A[:5, :5])),
        (ValueError, "square adjacency", dict(Y=Y, graph=A[:, :5])),
        (ValueError, "must be symmetric", dict(Y=Y, graph=sparse.csr_matrix(np.roll(np.eye(6), 1, axis=1)))),
        (ValueError, "no self loops", dict(Y=Y, graph=A + sparse.identity(6))),
        (TypeError, "graph must be a fitted FlashDeconv", dict(Y=Y, graph=np.eye(6))),
        (ValueError, "weights must be a 2-D", dict(Y=Y, graph=A, weights=np.ones(6))),
        (ValueError, "Y has 6 rows but weights has 5", dict(Y=Y, graph=A, weights=W[:5])),
        (ValueError, "1 to 272 columns", dict(Y=Y, graph=A, weights=np.ones((6, 273)))),
        (ValueError, "weights must be finite", dict(Y=Y, graph=A, weights=np.where(np.eye(6, 3) > 0, np.nan, W))),
        (ValueError, "weights must be non-negative", dict(Y=Y, graph=A, weights=W - np.eye(6, 3))),
        (ValueError, "ridge must be a finite number >= 0", dict(Y=Y, graph=A, weights=W, ridge=-1.0)),
        (ValueError, "max_iter must be an int >= 1", dict(Y=Y, graph=A, weights=W, max_iter=0)),
        (ValueError, "tol must be a finite number > 0", dict(Y=Y, graph=A, weights=W, tol=0.0)),
        (ValueError, "n_top must be an int >= 0 or None", dict(Y=Y, graph=A, n_top=-1)),
        (ValueError, "n_top must be an int >= 0 or None", dict(Y=Y, graph=A, n_top=2.0)),
    ]


@pytest.mark.parametrize("error,match,kw", _bad_calls(), ids=[f"{i}" for i in range(len(_bad_calls()))])
def test_the_entries_check_their_arguments_before_the_gpu(error, match, kw, monkeypatch):
    from flashdeconv_amd import _lib
    from flashdeconv_amd.utils import spatial_genes

    def no_gpu():
        raise AssertionError("the GPU was asked for before the arguments were checked")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    with pytest.raises(error, match=match):
        spatial_genes.spatially_variable_genes(**kw)
    if set(kw) == {"Y", "graph"}:
        with pytest.raises(error, match=match):
            spatial_genes.gene_spatial_sums(**kw)


def test_model_method_and_deconvolve_fail_early():
    import flashdeconv_amd as fd
    with pytest.raises(RuntimeError, match="has not been fitted"):
        fd.FlashDeconv().get_spatially_variable_genes(np.ones((3, 2)))
    with pytest.raises(ValueError, match="residual must be True or False"):
        fd.FlashDeconv().get_spatially_variable_genes(np.ones((3, 2)), residual=1)
    with pytest.raises(ValueError, match="spatial_genes must be True or False"):
        fd.tl.deconvolve(None, None, spatial_genes="yes")               # before the data is looked at, let alone fitted
    from flashdeconv_amd.utils.spatial_genes import check_request
    for match, args in (("2-D", ((5,), 3)), ("at least one gene", ((5, 0), 3)), ("1 to 272 cell types", ((5, 4), 273)),
                        ("at least one spot", ((0, 4), 3))):
        with pytest.raises(ValueError, match=match):
            check_request(*args)


# ---------------------------------------------------------------- C ABI and exports
def test_symbols_version_and_exports():
    from flashdeconv_amd import _lib, utils
    from flashdeconv_amd.utils import spatial_genes
    lib = _lib.load()
    assert lib.fdx_version() >= 205
    for name, n_args in (("fdx_gene_spatial_sums_dev", 10), ("fdx_gene_spatial_sums_csr_dev", 6)):
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == n_args
    header = open(_lib.LIB_PATH.replace("flashdeconv_amd/libfdx.so", "include/fdx.h")).read()
    for name in ("fdx_gene_spatial_sums_dev", "fdx_gene_spatial_sums_csr_dev", "FDX_GENE_SPATIAL_SEGMENT_POSITIONS 256"):
        assert name in header
    assert spatial_genes.PLANES == sr.PLANES
    assert set(spatial_genes.__all__) == {"spatially_variable_genes", "gene_spatial_sums", "assemble_genes", "check_request", "PLANES"}
    for name in ("spatially_variable_genes", "gene_spatial_sums", "assemble_genes"):
        assert name in utils.__all__ and callable(getattr(utils, name))
    # the module and the reference state the same definition
    for text in ("m  = u / n                  m2 = q - u*u/n                 m4 = c4 - 4 m c3 + 6 m^2 q - 3 n m^4",
                 "morans_i = (n / W) (P - 2 m D + m^2 W) / m2", "gearys_c = ((n - 1) / (2 W)) (2 H - 2 P) / m2"):
        assert text in spatial_genes.__doc__ and text in sr.__doc__
    for text in ("eps * mean^2 / var", "Out of scope", "permutation p values per gene", "ShardedFlashDeconv"):
        assert text in spatial_genes.__doc__
