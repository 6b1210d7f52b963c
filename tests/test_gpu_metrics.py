"""utils.metrics on the GPU against the reference's utils/metrics.py (golden/metrics.npz, make_metrics_golden.py), for numpy
and for device-tensor inputs, and at 1M x 30 against an independent numpy + scipy restatement."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
from metrics_ref import rankdata_spearman as _rankdata_spearman

pytestmark = pytest.mark.gpu

CASES = ["dirichlet", "tied", "negzero", "constcol", "allconst", "nan", "zerorows", "k1", "n1", "f32", "nearconst", "norare"]
PER_KEYS = ["rmse", "mae", "pearson", "spearman", "mean_proportion_true", "mean_proportion_pred"]
OVERALL_KEYS = ["rmse", "mae", "pearson", "spearman", "mean_jsd"]


@pytest.fixture(scope="module")
def gold():
    return load_golden("metrics.npz")


def _torch(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(x):
    if type(x).__module__.split(".")[0] == "torch":
        return x.cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def close_moment(got, want):
    np.testing.assert_allclose(np.asarray(got, dtype=np.float64), want, rtol=1e-12, atol=0, equal_nan=True)


def close_corr(got, want):
    np.testing.assert_allclose(np.asarray(got, dtype=np.float64), want, rtol=0, atol=1e-12, equal_nan=True)


def close_jsd(got, want):
    np.testing.assert_allclose(_host(got), want, rtol=1e-10, atol=1e-14, equal_nan=True)


def _inputs(gold, case, kind):
    p, t = gold[f"{case}__pred"], gold[f"{case}__true"]
    return (p, t) if kind == "numpy" else (_torch(p), _torch(t))


def check_evaluate(ev, overall, per, names):
    assert list(ev) == ["overall", "per_cell_type"]
    assert list(ev["overall"]) == OVERALL_KEYS
    assert list(ev["per_cell_type"]) == list(names)
    for i, key in enumerate(OVERALL_KEYS):
        (close_corr if key in ("pearson", "spearman") else close_jsd if key == "mean_jsd" else close_moment)(ev["overall"][key], overall[i])
    for k, name in enumerate(names):
        d = ev["per_cell_type"][name]
        assert list(d) == PER_KEYS
        for j, key in enumerate(PER_KEYS):
            (close_corr if key in ("pearson", "spearman") else close_moment)(d[key], per[k, j])


@pytest.mark.parametrize("kind", ["numpy", "torch"])
@pytest.mark.parametrize("case", CASES)
def test_against_reference(gold, case, kind):
    from flashdeconv_amd.utils import metrics as M
    p, t = _inputs(gold, case, kind)
    g = lambda key: gold[f"{case}__{key}"]
    for per in (False, True):
        sfx = "_per" if per else ""
        close_moment(M.compute_rmse(p, t, per_cell_type=per), g("rmse" + sfx))
        close_moment(M.compute_mae(p, t, per_cell_type=per), g("mae" + sfx))
        for meth in ("pearson", "spearman", "kendall"):
            close_corr(M.compute_correlation(p, t, method=meth, per_cell_type=per), g(meth + sfx))
    close_corr(M.compute_correlation(p, t), g("pearson"))
    j = M.compute_jsd(p, t)
    assert type(j).__module__.split(".")[0] == ("torch" if kind == "torch" else "numpy")
    assert tuple(j.shape) == (g("jsd").shape[0],)
    close_jsd(j, g("jsd"))
    close_jsd(M.compute_jsd(p, t, epsilon=1e-3), g("jsd_e3"))
    np.testing.assert_array_equal(np.asarray(M.compute_rare_cell_detection(p, t), dtype=np.float64), g("rare_t05"))
    np.testing.assert_array_equal(np.asarray(M.compute_rare_cell_detection(p, t, threshold=0.2), dtype=np.float64), g("rare_t20"))
    K = g("pred").shape[1]
    check_evaluate(M.evaluate_deconvolution(p, t), g("eval_overall"), g("eval_per"), [f"CellType_{k}" for k in range(K)])


@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_evaluate_with_names(gold, kind):
    from flashdeconv_amd.utils import metrics as M
    p, t = _inputs(gold, "dirichlet", kind)
    names = gold["names"]
    check_evaluate(M.evaluate_deconvolution(p, t, cell_type_names=names), gold["named__eval_overall"], gold["named__eval_per"], names)


def test_no_rare_entry_gives_nan_tuple(gold):
    from flashdeconv_amd.utils import metrics as M
    res = M.compute_rare_cell_detection(gold["norare__pred"], gold["norare__true"])
    assert len(res) == 3 and all(np.isnan(v) for v in res)


def test_reexports_work_on_device(gold):
    from flashdeconv_amd.utils import compute_correlation, compute_rmse
    p, t = gold["dirichlet__pred"], gold["dirichlet__true"]
    close_moment(compute_rmse(p, t), gold["dirichlet__rmse"])
    close_corr(compute_correlation(p, t, "spearman", per_cell_type=True), gold["dirichlet__spearman_per"])


def test_spearman_entry(gold):
    """fdx_metrics_spearman_dev on its own: per-type and overall rho of a pair without constant columns or NaNs."""
    import torch
    from flashdeconv_amd import _lib
    p, t = _torch(gold["tied__pred"]), _torch(gold["tied__true"])
    n, K = p.shape
    rho = np.zeros(K + 1)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.load().fdx_metrics_spearman_dev(ctypes.c_void_p(p.data_ptr()), ctypes.c_void_p(t.data_ptr()), _lib.FDX_F64, n, K,
                                                    K, K, 3, _lib.ptr_f64(rho), st))
    close_corr(rho[:K], gold["tied__spearman_per"])
    close_corr(rho[K], gold["tied__spearman"])


def _flat(ev):
    out = [ev["overall"][k] for k in OVERALL_KEYS]
    for d in ev["per_cell_type"].values():
        out += [d[k] for k in PER_KEYS]
    return np.array(out)


def _bits_equal(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("case", ["dirichlet", "tied", "nan", "f32"])
def test_numpy_and_device_inputs_bit_identical_and_repeatable(gold, case):
    from flashdeconv_amd.utils import metrics as M
    p, t = gold[f"{case}__pred"], gold[f"{case}__true"]
    a = _flat(M.evaluate_deconvolution(p, t))
    b = _flat(M.evaluate_deconvolution(_torch(p), _torch(t)))
    c = _flat(M.evaluate_deconvolution(_torch(p), _torch(t)))
    _bits_equal(a, b)
    _bits_equal(b, c)
    _bits_equal(M.compute_jsd(p, t), _host(M.compute_jsd(_torch(p), _torch(t))))


def test_large_heavily_tied_against_numpy_scipy():
    """1M x 30 with ~85 % exact-zero truth: evaluate_deconvolution against numpy and scipy.stats.rankdata restated here."""
    import torch
    from flashdeconv_amd.utils import metrics as M
    rng = np.random.default_rng(7)
    n, K = 1_000_000, 30
    t = np.round(rng.dirichlet(np.full(K, 0.3), size=n), 3) * (rng.random((n, K)) > 0.85)
    p = np.clip(t + rng.normal(0, 0.02, (n, K)), 0, None)
    p[rng.random((n, K)) < 0.5] = 0.0
    P, T = _torch(p), _torch(t)
    ev = M.evaluate_deconvolution(P, T)
    _bits_equal(_flat(ev), _flat(M.evaluate_deconvolution(P, T)))
    o = ev["overall"]
    close_moment(o["rmse"], np.sqrt(np.mean((p - t) ** 2)))
    close_moment(o["mae"], np.mean(np.abs(p - t)))
    close_corr(o["pearson"], np.corrcoef(p.ravel(), t.ravel())[0, 1])
    close_corr(o["spearman"], _rankdata_spearman(p.ravel(), t.ravel()))
    pc, tc = np.clip(p, 1e-10, 1 - 1e-10), np.clip(t, 1e-10, 1 - 1e-10)
    pc, tc = pc / pc.sum(1, keepdims=True), tc / tc.sum(1, keepdims=True)
    m = 0.5 * (pc + tc)
    jsd = 0.5 * (np.sum(pc * np.log(pc / m), 1) + np.sum(tc * np.log(tc / m), 1))
    close_jsd(o["mean_jsd"], np.mean(jsd))
    for k in (0, 7, 29):
        d = ev["per_cell_type"][f"CellType_{k}"]
        close_moment(d["rmse"], np.sqrt(np.mean((p[:, k] - t[:, k]) ** 2)))
        close_corr(d["pearson"], np.corrcoef(p[:, k], t[:, k])[0, 1])
        close_corr(d["spearman"], _rankdata_spearman(p[:, k], t[:, k]))
        close_moment(d["mean_proportion_true"], np.mean(t[:, k]))
    del P, T
    torch.cuda.empty_cache()


def test_fit_output_torch_then_evaluate_on_device():
    import datagen
    from flashdeconv_amd import FlashDeconv
    from flashdeconv_amd.utils import metrics as M
    Y, X, coords, B = datagen.count_like(800, 300, 6, 0.1, 3)
    P = FlashDeconv(sketch_dim=64, max_iter=25).fit(Y, X, coords, output="torch").proportions_
    assert P.is_cuda
    Bd = _torch(B)
    dev = M.evaluate_deconvolution(P, Bd)
    host = M.evaluate_deconvolution(P.cpu().numpy(), B)
    _bits_equal(_flat(dev), _flat(host))
    _bits_equal(_host(M.compute_jsd(P, Bd)), M.compute_jsd(P.cpu().numpy(), B))
    assert M.compute_rare_cell_detection(P, Bd) == M.compute_rare_cell_detection(P.cpu().numpy(), B) or \
        all(np.isnan(M.compute_rare_cell_detection(P, Bd)))


@pytest.mark.parametrize("K", [300, 2100])
def test_wide_rows_against_numpy(K):
    """More columns than a workgroup has threads (column groups), and rows too wide for the staged JSD tile."""
    from flashdeconv_amd.utils import metrics as M
    rng = np.random.default_rng(K)
    n = 40
    t = np.round(rng.dirichlet(np.full(K, 0.5), size=n), 4)
    p = np.clip(t + rng.normal(0, 1e-3, t.shape), 0, None)
    ev = M.evaluate_deconvolution(p, t)
    close_moment(M.compute_rmse(p, t, per_cell_type=True), np.sqrt(np.mean((p - t) ** 2, axis=0)))
    close_moment(ev["overall"]["mae"], np.mean(np.abs(p - t)))
    close_corr(ev["overall"]["pearson"], np.corrcoef(p.ravel(), t.ravel())[0, 1])
    close_corr(ev["overall"]["spearman"], _rankdata_spearman(p.ravel(), t.ravel()))
    for k in (0, K // 2, K - 1):
        d = ev["per_cell_type"][f"CellType_{k}"]
        want_p = np.corrcoef(p[:, k], t[:, k])[0, 1] if np.ptp(p[:, k]) and np.ptp(t[:, k]) else 0.0
        want_s = _rankdata_spearman(p[:, k], t[:, k]) if np.ptp(p[:, k]) and np.ptp(t[:, k]) else 0.0
        close_corr(d["pearson"], want_p)
        close_corr(d["spearman"], want_s)
        close_moment(d["mean_proportion_pred"], np.mean(p[:, k]))
    pc, tc = np.clip(p, 1e-10, 1 - 1e-10), np.clip(t, 1e-10, 1 - 1e-10)
    pc, tc = pc / pc.sum(1, keepdims=True), tc / tc.sum(1, keepdims=True)
    m = 0.5 * (pc + tc)
    close_jsd(M.compute_jsd(p, t), 0.5 * (np.sum(pc * np.log(pc / m), 1) + np.sum(tc * np.log(tc / m), 1)))
