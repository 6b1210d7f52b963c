"""CPU tests of the gene-pair co-expression statistics (flashdeconv_amd/utils/gene_pairs.py): the exact permutation variance
against the enumeration of every permutation, the package's host arithmetic against the NumPy definition in
tests/gene_pairs_ref.py and the centred textbook definitions, the NaN rules, the planted case the GPU tests
(tests/test_gpu_gene_pairs.py) rest on, the argument checks and the C ABI.  No GPU."""
import inspect

import numpy as np
import pytest
from scipy import sparse

import fdx_oracle as orc
import fit_tail_ref
import gene_pairs_ref as gr
import spatial_genes_ref as sr


def _knn_adjacency(n, seed=11):
    return orc.knn_graph_kdtree(fit_tail_ref.tie_free_coords(n, 2, seed), 6)


def _assembled(module_assemble, s):
    return module_assemble(s["n"], s["W"], s["sum_deg_sq"], *(s[name] for name in gr.PLANES))


def _grid_adjacency():
    """The 4-neighbour adjacency of the 25 x 24 grid, spot i at x = i % 24, y = i // 24."""
    i = np.arange(600)
    right, up = i[i % 24 < 23], i[i // 24 < 24]
    rows, cols = np.concatenate([right, up]), np.concatenate([right + 1, up + 24])
    A = sparse.csr_matrix((np.ones(rows.size), (rows, cols)), shape=(600, 600))
    A = sparse.csr_matrix(A + A.T)
    assert A.nnz == 2 * (25 * 23 + 24 * 24) and sorted(set(sr.degrees(A))) == [2, 3, 4]
    return A


# ---------------------------------------------------------------- the variance is exact
def test_permutation_variance_equals_the_enumeration_of_all_720_permutations():
    """Six spots on an irregular graph (degrees 1 to 4), lognormal values: over all 6! reassignments of one gene's values the mean
    of R is 0 and its variance is variance_b_moved (gene b moved) / variance_a_moved (gene a moved)."""
    from flashdeconv_amd.utils.gene_pairs import assemble_pairs
    edges = [(0, 1), (0, 2), (0, 3), (0, 4), (1, 2), (2, 3), (4, 5)]
    A = sparse.lil_matrix((6, 6))
    for i, j in edges:
        A[i, j] = A[j, i] = 1
    A = sparse.csr_matrix(A)
    assert sorted(sr.degrees(A)) == [1, 2, 2, 2, 3, 4]
    Y = np.random.RandomState(3).lognormal(0.0, 1.0, size=(6, 2))
    s = gr.planes(Y, A, [(0, 1)])
    mean_b, var_b = gr.enumerate_moves(Y[:, 0], Y[:, 1], A)
    mean_a, var_a = gr.enumerate_moves(Y[:, 1], Y[:, 0], A)
    assert abs(mean_b) < 1e-14 and abs(mean_a) < 1e-14
    for mod in (assemble_pairs, gr.assemble):
        out = _assembled(mod, s)
        np.testing.assert_allclose(out["variance_b_moved"][0], var_b, rtol=1e-12, atol=0)
        np.testing.assert_allclose(out["variance_a_moved"][0], var_a, rtol=1e-12, atol=0)
        assert out["z_score"][0] == out["morans_r"][0] / np.sqrt(max(out["variance_b_moved"][0], out["variance_a_moved"][0]))
    assert var_a != var_b


# ---------------------------------------------------------------- the package's host arithmetic
def test_assemble_pairs_agrees_with_the_centred_definitions():
    """A generic 600-spot case with mean^2 <= 4 var per gene (asserted), so conditioning cannot hide a wrong formula: rtol 1e-9."""
    from flashdeconv_amd.utils.gene_pairs import assemble_pairs
    A = _knn_adjacency(600)
    Y = sr.generic_case(600, 9, 1)
    assert np.all(Y.mean(axis=0) ** 2 <= 4.0 * Y.var(axis=0))
    pairs = gr.pair_list(9, 30, 0)
    s = gr.planes(Y, A, pairs)
    R, pearson, local = gr.centred(Y, A, pairs)
    for mod in (assemble_pairs, gr.assemble):
        out = _assembled(mod, s)
        np.testing.assert_allclose(out["morans_r"], R, rtol=1e-9, atol=0)
        np.testing.assert_allclose(out["pearson_r"], pearson, rtol=1e-9, atol=0)
        np.testing.assert_allclose(out["mean_a"], Y.mean(axis=0)[pairs[:, 0]], rtol=1e-14, atol=0)
        assert np.all((out["p_value"] >= 0) & (out["p_value"] <= 1)) and np.all(out["q_value"] >= out["p_value"])
    np.testing.assert_allclose(local.sum(axis=0), R, rtol=1e-9, atol=0)
    same = pairs[:, 0] == pairs[:, 1]
    assert same.any()
    np.testing.assert_allclose(out["pearson_r"][same], 1.0, rtol=1e-12)
    np.testing.assert_allclose(out["morans_r"][same], sr.centred(Y, A)[0][pairs[same, 0]], rtol=1e-9)


@pytest.mark.parametrize("n,G,seed,constant", [(300, 7, 0, ()), (600, 12, 1, (2, 5)), (65, 5, 2, (0,)), (3, 3, 4, ()), (2, 3, 5, ())])
def test_assemble_pairs_equals_the_reference(n, G, seed, constant):
    from flashdeconv_amd.utils.gene_pairs import assemble_pairs
    A = _knn_adjacency(n) if n > 4 else sparse.csr_matrix(np.ones((n, n)) - np.eye(n))
    pairs = gr.pair_list(G, 40, seed)
    for Y in (sr.generic_case(n, G, seed, constant), sr.exact_case(n, G, seed)):
        s = gr.planes(Y, A, pairs)
        got, want = _assembled(assemble_pairs, s), _assembled(gr.assemble, s)
        assert set(got) == set(want)
        for key in want:
            a, b = np.asarray(got[key]), np.asarray(want[key])
            assert a.shape == b.shape and a.dtype == b.dtype, key
            if key in ("order", "mean_a", "mean_b", "m2_a", "m2_b"):
                assert np.array_equal(a, b, equal_nan=True), key
            else:
                assert np.array_equal(np.isnan(a), np.isnan(b)), key
                np.testing.assert_allclose(a, b, rtol=1e-13, atol=0, err_msg=key)


def test_nan_rules():
    from flashdeconv_amd.utils.gene_pairs import assemble_pairs
    stat_keys = ("morans_r", "pearson_r", "variance_b_moved", "variance_a_moved", "z_score", "p_value", "q_value")
    # a constant gene on either side of a pair: decided by min == max, whatever m2 rounds to
    A = _knn_adjacency(100)
    Y = sr.generic_case(100, 3, 5)
    Y[:, 1] = np.float64(np.float32(0.1))
    pairs = np.array([(0, 2), (0, 1), (1, 2), (1, 1), (2, 0)])
    s = gr.planes(Y, A, pairs)
    assert s["qa"][3] - s["ua"][3] ** 2 / 100 != 0.0        # the cancellation leaves rounding noise: no threshold would do
    for mod in (gr.assemble, assemble_pairs):
        out = _assembled(mod, s)
        for key in stat_keys:
            assert np.isnan(out[key][[1, 2, 3]]).all() and not np.isnan(out[key][[0, 4]]).any(), key
        assert sorted(out["order"][:2]) == [0, 4] and list(out["order"][2:]) == [1, 2, 3]
    # W = 0 and n < 2: nothing has a statistic
    for Yn, An in ((Y, sparse.csr_matrix((100, 100))), (Y[:1], sparse.csr_matrix((1, 1)))):
        for mod in (gr.assemble, assemble_pairs):
            out = _assembled(mod, gr.planes(Yn, An, pairs))
            assert all(np.isnan(out[key]).all() for key in stat_keys) and list(out["order"]) == [0, 1, 2, 3, 4]
    with pytest.raises(ValueError, match="seventeen sums"):
        assemble_pairs(3, 2, 2, *[np.ones(2)] * 16, np.ones(3))


def test_q_values_and_order_follow_the_plain_python_versions():
    from flashdeconv_amd.utils.gene_pairs import assemble_pairs
    A = _knn_adjacency(300)
    Y = sr.generic_case(300, 8, 2, constant=(3,))
    pairs = gr.pair_list(8, 60, 1)
    out = _assembled(assemble_pairs, gr.planes(Y, A, pairs))
    assert np.isnan(out["p_value"]).any() and not np.isnan(out["p_value"]).all()
    assert np.array_equal(out["q_value"], sr.benjamini_hochberg(out["p_value"]), equal_nan=True)
    assert out["order"].dtype == np.int64 and np.array_equal(out["order"], sr.decreasing_order(out["morans_r"]))
    assert out["morans_r"][3] == out["morans_r"][4]          # the repeated pair: a tie, kept in index order
    assert list(out["order"]).index(3) + 1 == list(out["order"]).index(4)


def test_planted_pairs_separate():
    """On the 25 x 24 grid with the 4-neighbour adjacency: the partner co-localises with the smooth gene (R = 0.956, z = 24), the
    shuffled copy does not (|R| = 0.024), the constant has no statistic, the mirrored gene is anti-co-localised (R = -0.957) and
    a gene with itself has the Moran's I of the gene (0.957)."""
    from flashdeconv_amd.utils.gene_pairs import assemble_pairs
    A = _grid_adjacency()
    Y, pairs = gr.planted_case()
    for mod in (gr.assemble, assemble_pairs):
        out = _assembled(mod, gr.planes(Y, A, pairs))
        R, q = out["morans_r"], out["q_value"]
        print("planted R", R, "z", out["z_score"], "q", q)
        assert R[0] > 0.8 > abs(R[1]) and R[3] < -0.8 and q[0] < 1e-6 and q[1] > 0.05
        assert all(np.isnan(out[key][2]) for key in ("morans_r", "pearson_r", "z_score", "p_value", "q_value"))
        morans_i = _assembled_genes(Y, A)
        np.testing.assert_allclose(R[4], morans_i[0], rtol=1e-12)
        assert list(out["order"]) == [4, 0, 1, 3, 2] and out["z_score"][0] > 20


def _assembled_genes(Y, A):
    s = sr.planes(Y, A)
    return sr.assemble(s["n"], s["W"], s["sum_deg_sq"], *(s[name] for name in sr.PLANES))["morans_i"]


def test_exact_cases_are_exact_in_any_order():
    """Integers in [0, 7] on the hub graph: the largest term of any plane, (7 * 299)^2 * 300, is far below 2^53, and the reference's
    planes are the integer sums."""
    A = fit_tail_ref.hub_and_spoke(300)
    Y = sr.exact_case(300, 40, 3)
    pairs = gr.pair_list(40, 257, 0)
    s = gr.planes(Y, A, pairs)
    Yi, Ai = Y.astype(np.int64), sparse.csr_matrix(A).astype(bool).astype(np.int64)
    lag, deg = Ai @ Yi, sr.degrees(A)
    a, b = pairs[:, 0], pairs[:, 1]
    for key, want in (("S", (Yi[:, a] * Yi[:, b]).sum(0)), ("Xab", (Yi[:, a] * lag[:, b]).sum(0)), ("Xba", (Yi[:, b] * lag[:, a]).sum(0)),
                      ("La", (lag[:, a] ** 2).sum(0)), ("DLb", deg @ lag[:, b]), ("Da", deg @ Yi[:, a])):
        assert np.array_equal(s[key], want), key
    assert np.array_equal(s["Xab"], s["Xba"]) and (7 * 299) ** 2 * 300 < 2 ** 40


# ---------------------------------------------------------------- argument checks (nothing touches a GPU)
def test_check_request_refusals():
    from flashdeconv_amd.utils.gene_pairs import check_request
    for match, pairs in (("must be a \\(P, 2\\)", np.zeros((3, 3), dtype=np.int64)), ("must be a \\(P, 2\\)", np.arange(4)),
                         ("must be a \\(P, 2\\)", []), ("at least one pair", np.zeros((0, 2), dtype=np.int64)),
                         ("integer dtype", np.zeros((2, 2))), ("integer dtype", np.zeros((2, 2), dtype=bool)),
                         ("gene index 4 outside \\[0, 4\\)", [(0, 1), (4, 0)]), ("gene index -1 outside", [(0, -1)])):
        with pytest.raises(ValueError, match=match):
            check_request((6, 4), pairs)
    got = check_request((6, 4), [(0, 3), (3, 3)])
    assert got.dtype == np.int32 and got.flags.c_contiguous and got.tolist() == [[0, 3], [3, 3]]
    assert check_request((6, 4), np.array([[1, 2]], dtype=np.uint8)).dtype == np.int32


def _bad_calls():
    Y = np.ones((6, 4), dtype=np.float32)
    A = sparse.csr_matrix(np.roll(np.eye(6), 1, axis=1) + np.roll(np.eye(6), -1, axis=1))
    ok = [(0, 1)]
    return [
        (ValueError, "Y must be a 2-D", dict(Y=np.ones(6), graph=A, pairs=ok)),
        (ValueError, "at least one gene", dict(Y=np.ones((6, 0)), graph=A, pairs=ok)),
        (ValueError, "at least one spot", dict(Y=np.ones((0, 4)), graph=sparse.csr_matrix((0, 0)), pairs=ok)),
        (ValueError, "must be a \\(P, 2\\)", dict(Y=Y, graph=A, pairs=[0, 1])),
        (ValueError, "at least one pair", dict(Y=Y, graph=A, pairs=np.zeros((0, 2), dtype=np.int32))),
        (ValueError, "integer dtype", dict(Y=Y, graph=A, pairs=[(0.0, 1.0)])),
        (ValueError, "outside \\[0, 4\\)", dict(Y=Y, graph=A, pairs=[(0, 4)])),
        (ValueError, "values has 6 rows but the graph has 5 spots", dict(Y=Y, graph=A[:5, :5], pairs=ok)),
        (ValueError, "must be symmetric", dict(Y=Y, graph=sparse.csr_matrix(np.roll(np.eye(6), 1, axis=1)), pairs=ok)),
        (TypeError, "graph must be a fitted FlashDeconv", dict(Y=Y, graph=np.eye(6), pairs=ok)),
        (ValueError, "local must be True or False", dict(Y=Y, graph=A, pairs=ok, local=1)),
        (ValueError, "n_top must be an int >= 0 or None", dict(Y=Y, graph=A, pairs=ok, n_top=-1)),
        (ValueError, "Unknown output", dict(Y=Y, graph=A, pairs=ok, output="cupy")),
    ]


@pytest.mark.parametrize("error,match,kw", _bad_calls(), ids=[f"{i}" for i in range(len(_bad_calls()))])
def test_the_entries_check_their_arguments_before_the_gpu(error, match, kw, monkeypatch):
    from flashdeconv_amd import _lib
    from flashdeconv_amd.utils import gene_pairs

    def no_gpu():
        raise AssertionError("the GPU was asked for before the arguments were checked")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    with pytest.raises(error, match=match):
        gene_pairs.spatial_gene_pairs(**kw)
    if set(kw) == {"Y", "graph", "pairs"}:
        with pytest.raises(error, match=match):
            gene_pairs.gene_pair_sums(**kw)


def test_model_method_and_deconvolve_fail_early():
    import flashdeconv_amd as fd
    with pytest.raises(RuntimeError, match="has not been fitted"):
        fd.FlashDeconv().get_gene_pair_colocalisation(np.ones((3, 2)), [(0, 1)])
    for bad in ([], [("a",)], [("a", "b", "c")]):
        with pytest.raises(ValueError, match="gene_pairs must be a non-empty sequence"):
            fd.tl.deconvolve(None, None, gene_pairs=bad)             # before the data is looked at, let alone fitted
    assert inspect.signature(fd.tl.deconvolve).parameters["gene_pairs"].default is None
    params = inspect.signature(fd.FlashDeconv.get_gene_pair_colocalisation).parameters
    assert list(params) == ["self", "Y", "pairs", "local", "n_top"] and params["local"].default is False


# ---------------------------------------------------------------- C ABI and exports
def test_symbols_version_and_exports():
    from flashdeconv_amd import _lib, utils
    from flashdeconv_amd.utils import gene_pairs
    lib = _lib.load()
    assert lib.fdx_version() >= 206
    header = open(_lib.LIB_PATH.replace("flashdeconv_amd/libfdx.so", "include/fdx.h")).read()
    for name, n_args in (("fdx_gene_pair_sums_dev", 11), ("fdx_gene_pair_sums_csr_dev", 8), ("fdx_gene_pair_local_dev", 14),
                         ("fdx_gene_pair_local_csr_dev", 11)):
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == n_args and name in header
    assert gene_pairs.PLANES == gr.PLANES and len(gr.PLANES) == 17
    assert set(gene_pairs.__all__) == {"spatial_gene_pairs", "gene_pair_sums", "assemble_pairs", "check_request", "PLANES"}
    for name in ("spatial_gene_pairs", "gene_pair_sums", "assemble_pairs"):
        assert name in utils.__all__ and callable(getattr(utils, name))
    # the module and the reference state the same definition
    for text in ("C   = (Xab + Xba)/2 - m_a Db - m_b Da + m_a m_b W", "morans_r  = (n/W) C / sqrt(m2_a m2_b)",
                 "variance_b_moved = (n/W)^2 (LLc_a - s_a^2/n) / ((n - 1) m2_a)",
                 "z_score = morans_r / sqrt(max(variance_b_moved, variance_a_moved))"):
        assert text in gene_pairs.__doc__ and text in gr.__doc__
    for text in ("eps * mean^2 / var", "Out of scope", "ermutation p values per pair", "multi-subunit complexes", "cell types",
                 "ShardedFlashDeconv", "normalising ``Y``"):
        assert text in gene_pairs.__doc__
