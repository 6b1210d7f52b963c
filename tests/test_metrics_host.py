"""utils.metrics without a GPU: the module imports, the reference's re-exports are there, and bad shapes are refused before
anything touches the device."""
import numpy as np
import pytest


def test_module_imports_with_reference_names():
    from flashdeconv_amd.utils import metrics
    for name in ("compute_rmse", "compute_mae", "compute_correlation", "compute_jsd", "evaluate_deconvolution",
                 "compute_rare_cell_detection"):
        assert callable(getattr(metrics, name))


def test_utils_reexports_rmse_and_correlation():
    import flashdeconv_amd.utils as utils
    from flashdeconv_amd.utils import compute_correlation, compute_rmse
    assert "compute_rmse" in utils.__all__ and "compute_correlation" in utils.__all__
    assert compute_rmse is utils.metrics.compute_rmse and compute_correlation is utils.metrics.compute_correlation


def test_metrics_symbols_are_bound():
    from flashdeconv_amd import _lib
    for name in ("fdx_metrics_moments_dev", "fdx_metrics_spearman_dev", "fdx_metrics_evaluate_dev"):
        assert name in _lib.SIGNATURES


@pytest.fixture
def no_gpu_calls(monkeypatch):
    """Any attempt to reach the device library fails the test: validation must come first."""
    from flashdeconv_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the GPU library was reached before the shapes were checked")
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(_lib, "require_gpu", boom)


@pytest.mark.parametrize("fn", ["compute_rmse", "compute_mae", "compute_correlation", "compute_jsd", "evaluate_deconvolution",
                                "compute_rare_cell_detection"])
def test_shape_errors_before_gpu(fn, no_gpu_calls):
    from flashdeconv_amd.utils import metrics
    f = getattr(metrics, fn)
    with pytest.raises(ValueError, match=r"\(10, 3\).*\(10, 4\)"):
        f(np.zeros((10, 3)), np.zeros((10, 4)))
    with pytest.raises(ValueError, match=r"2-D.*\(10,\)"):
        f(np.zeros(10), np.zeros(10))
    with pytest.raises(ValueError, match="2-D"):
        f(np.zeros((2, 3, 4)), np.zeros((2, 3, 4)))


def test_size_limit_is_a_value_error(no_gpu_calls):
    from flashdeconv_amd.utils import metrics

    class Big:                               # a shape only: nothing of this size is allocated
        shape = (2 ** 26, 32)
        ndim = 2
    with pytest.raises(ValueError, match="2\\*\\*31 - 1"):
        metrics.compute_rmse(Big(), Big())


# ------------------------------------------------------------------------------------------------ the plain reference
# tests/metrics_ref.py is the oracle of tests/test_gpu_metrics_fields.py.  What licenses it: built from its pieces, every
# function of the reference's utils/metrics.py reproduces the recorded outputs of the real thing (golden/metrics.npz), at the
# tolerances tests/test_gpu_metrics.py holds the device to.
GOLDEN_CASES = ["dirichlet", "tied", "negzero", "constcol", "allconst", "nan", "zerorows", "k1", "n1", "f32", "nearconst", "norare"]


@pytest.fixture(scope="module")
def gold():
    from conftest import load_golden
    return load_golden("metrics.npz")


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_reference_reproduces_the_recorded_outputs(gold, case):
    import metrics_ref as R
    g = lambda key: gold[f"{case}__{key}"]
    res = R.results(g("pred"), g("true"))
    for key in ("rmse", "rmse_per", "mae", "mae_per"):
        np.testing.assert_allclose(res[key], g(key), rtol=1e-12, atol=0, equal_nan=True, err_msg=key)
    for key in ("pearson", "pearson_per", "spearman", "spearman_per"):
        np.testing.assert_allclose(res[key], g(key), rtol=0, atol=1e-12, equal_nan=True, err_msg=key)
    np.testing.assert_allclose(res["pearson"], g("kendall"), rtol=0, atol=1e-12, equal_nan=True)
    for key in ("jsd", "jsd_e3"):
        np.testing.assert_allclose(res[key], g(key), rtol=1e-10, atol=1e-14, equal_nan=True, err_msg=key)
    for key in ("rare_t05", "rare_t20"):
        np.testing.assert_array_equal(res[key], g(key), err_msg=key)
    per = g("eval_per")
    np.testing.assert_allclose(res["mean_proportion_true"], per[:, 4], rtol=1e-12, atol=0, equal_nan=True)
    np.testing.assert_allclose(res["mean_proportion_pred"], per[:, 5], rtol=1e-12, atol=0, equal_nan=True)
    np.testing.assert_allclose(np.mean(res["jsd"]), g("eval_overall")[4], rtol=1e-10, atol=1e-14, equal_nan=True)


def test_reference_inputs_are_what_the_gpu_tests_say_they_are():
    import metrics_ref as R
    p, t = R.pair(2721, 3)
    for a in (p, t):
        assert a.min() >= 0 and np.array_equal(a, np.round(a, 3)) and not a.flags.writeable
        assert 0.5 < np.mean(a[:, [0, 2]] == 0) < 0.75
    assert np.ptp(p[:, 1]) == 0 and np.ptp(p[:, 0]) > 0
    p32, _ = R.pair(2721, 3, "float32")
    assert p32.dtype == np.float32
    jp, jt = R.jsd_pair(5, 1)
    assert not jp[0].any() and not jt[4].any() and not jp[1].any() and not jt[1].any()


# ---- the comparator bites: each perturbation of the reference's own output must fail the comparator of the GPU tests, and
# ---- the unperturbed output must pass it
@pytest.fixture(scope="module")
def stats_case():
    import metrics_ref as R
    p, t = R.pair(300, 5)
    ref = R.reference(p, t, 0.05)
    blk = R.block_of(ref)
    R.check_stats(blk, ref, "self-test, reference against itself")
    blk.setflags(write=False)
    return p, t, ref, blk


def test_comparator_fails_on_one_entry_dropped_from_a_columns_sse(stats_case):
    import metrics_ref as R
    p, t, ref, blk = stats_case
    c = 3
    d2 = (p[:, c] - t[:, c]) ** 2
    drop = np.min(d2[d2 > 0])                                     # the smallest entry the column can lose
    bad = blk.copy()
    bad[c, R.SSE] -= drop
    assert 0 < drop < 1e-4 * blk[c, R.SSE]
    with pytest.raises(AssertionError, match="sse off"):
        R.check_stats(bad, ref, "self-test, dropped entry")


def test_comparator_fails_on_the_second_smallest_as_minimum(stats_case):
    import metrics_ref as R
    p, t, ref, blk = stats_case
    c = 2
    bad = blk.copy()
    bad[c, R.MIN_P] = np.unique(p[:, c])[1]
    assert bad[5, R.MIN_P] == blk[5, R.MIN_P]
    with pytest.raises(AssertionError, match="min_p of row 2"):
        R.check_stats(bad, ref, "self-test, second smallest")


def test_comparator_fails_on_tp_and_fn_swapped_in_one_column(stats_case):
    import metrics_ref as R
    p, t, ref, blk = stats_case
    c = 0
    assert blk[c, R.TP] != blk[c, R.FN] and blk[c, R.TP] > 0 and blk[c, R.FP] > 0
    bad = blk.copy()
    bad[c, [R.TP, R.FN]] = blk[c, [R.FN, R.TP]]                   # row K, all Python reads, is unchanged
    with pytest.raises(AssertionError, match="tp of row 0"):
        R.check_stats(bad, ref, "self-test, tp and fn swapped")


@pytest.fixture(scope="module")
def rank_case():
    import metrics_ref as R
    p, t, _ = R.tie_pair()
    n, K = p.shape
    ranks = dict(cp=R.column_twice_ranks(p), ct=R.column_twice_ranks(t), ap=R.twice_ranks(p.ravel(), n * K).reshape(n, K),
                 at=R.twice_ranks(t.ravel(), n * K).reshape(n, K))
    want = R.rho_from_ranks(ranks["cp"], ranks["ct"], ranks["ap"], ranks["at"], 3)
    R.check_rho(want.copy(), want, "self-test, reference against itself")
    assert np.isnan(want[0]) and not np.isnan(want[1:]).any()     # true's column 0 is constant: raw 0 / 0
    return p, t, ranks, want


def test_comparator_fails_on_one_twice_rank_off_by_one(rank_case):
    import metrics_ref as R
    p, t, ranks, want = rank_case
    cp = ranks["cp"].copy()
    cp[17, 2] += 1
    with pytest.raises(AssertionError, match="rho of row 2"):
        R.check_rho(R.rho_from_ranks(cp, ranks["ct"], ranks["ap"], ranks["at"], 3), want, "self-test, rank off by one")
    ap = ranks["ap"].copy()
    ap[40, 1] -= 1
    with pytest.raises(AssertionError, match="rho of row 4"):
        R.check_rho(R.rho_from_ranks(ranks["cp"], ranks["ct"], ap, ranks["at"], 3), want, "self-test, overall rank off by one")


def test_comparator_fails_on_a_tie_run_merged_across_a_column_boundary(rank_case):
    """Column 1's maximum is column 2's minimum: without the segment test of the run heads, the four 0.5 that end segment 1 and the
    five that start segment 2 would be one run of nine with one average rank."""
    import metrics_ref as R
    p, t, ranks, want = rank_case
    n = p.shape[0]
    a, b = int(np.sum(p[:, 1] == 0.5)), int(np.sum(p[:, 2] == 0.5))
    assert (a, b) == (4, 5) and p[:, 1].max() == 0.5 == p[:, 2].min()
    assert np.all(ranks["cp"][p[:, 1] == 0.5, 1] == (n - a + 1) + n) and np.all(ranks["cp"][p[:, 2] == 0.5, 2] == 1 + b)
    merged = (n - a + 1) + (n + b)                                # first and last 1-based position of the run of nine, from segment 1
    cp = ranks["cp"].copy()
    cp[p[:, 1] == 0.5, 1] = merged
    cp[p[:, 2] == 0.5, 2] = merged
    with pytest.raises(AssertionError, match="rho of row 1"):
        R.check_rho(R.rho_from_ranks(cp, ranks["ct"], ranks["ap"], ranks["at"], 3), want, "self-test, merged run")


def test_comparator_fails_on_a_spot_scored_against_its_neighbours_truth():
    import metrics_ref as R
    p, t = R.jsd_pair(257, 8)
    for eps in (1e-10, 1e-3):
        j, S = R.jsd(p, t, eps)
        R.check_jsd(j, float(np.sum(j)), j, S, 8, f"self-test, reference against itself, eps {eps:g}")
        r = 100
        assert not np.array_equal(t[r], t[r + 1])
        bad = j.copy()
        bad[r] = R.jsd(p[r:r + 1], t[r + 1:r + 2], eps)[0][0]
        with pytest.raises(AssertionError, match="jsd of spot 100"):
            R.check_jsd(bad, None, j, S, 8, "self-test, neighbour's truth")
        with pytest.raises(AssertionError, match="jsd sum"):
            R.check_jsd(j, float(np.sum(bad)), j, S, 8, "self-test, neighbour's truth in the sum")
