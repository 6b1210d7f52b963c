"""Evaluation metrics of deconvolution results (utils/metrics.py:12-266), computed on the GPU.

Same names, signatures, defaults and return structure as the reference.  Inputs are 2-D ``(n_spots, n_types)`` arrays: numpy,
or CUDA ``torch`` tensors such as ``FlashDeconv.fit(..., output="torch")`` leaves in HBM, float32 or float64; arithmetic is
float64 throughout.  Device tensors are never copied to the host, numpy arrays are uploaded once each, and only scalars and
length-K vectors come back (plus the per-spot JSD, which stays a device tensor when both inputs are device tensors).  The
work goes on torch's current stream through the C ABI entries ``fdx_metrics_*_dev`` (csrc/metrics_kernels.cpp).
"""
import ctypes
from typing import Optional, Tuple

import numpy as np

from .. import _lib
from ._device import device_of, values_on_device

N_MAX = 2 ** 31 - 1                      # n_spots * n_types limit of the device path (int32 sort payloads)

# fields of a stats row (include/fdx.h FDX_MX_*)
_SSE, _SAE, _SUM_P, _SUM_T, _MIN_P, _MAX_P, _MIN_T, _MAX_T, _NAN_P, _NAN_T = range(10)
_JSD_SUM, _C_PT, _C_PP, _C_TT = 14, 15, 16, 17
_FIELDS = 18
_SPEARMAN_OVERALL, _SPEARMAN_PER_TYPE = 1, 2


def _shape(x):
    if _lib.is_torch(x):
        return tuple(x.shape)
    return np.shape(x)


def _validate(pred, true):
    """Shapes only, before anything touches the GPU."""
    sp, st = _shape(pred), _shape(true)
    if len(sp) != 2 or len(st) != 2:
        raise ValueError(f"pred and true must be 2-D (n_spots, n_cell_types) arrays, got shapes {sp} and {st}")
    if sp != st:
        raise ValueError(f"pred and true must have the same shape, got {sp} and {st}")
    n, K = sp
    if n < 1 or K < 1:
        raise ValueError(f"pred and true must not be empty, got shape {sp}")
    if n * K > N_MAX:
        raise ValueError(f"n_spots * n_cell_types = {n * K} exceeds the device limit of 2**31 - 1 = {N_MAX} entries")
    return n, K


class _Pair:
    """pred / true as device matrices of one dtype (float32 only when both are float32), on torch's current stream."""

    def __init__(self, pred, true):
        self.n, self.K = _validate(pred, true)
        import torch
        self.device_out = _lib.is_cuda_tensor(pred) and _lib.is_cuda_tensor(true)
        devs = [x.device for x in (pred, true) if _lib.is_cuda_tensor(x)]
        if len(devs) == 2 and devs[0] != devs[1]:
            raise ValueError(f"pred and true are on different devices ({devs[0]} and {devs[1]})")
        self.device = device_of(pred, true)
        if not devs:
            _lib.require_gpu()
        f32 = all(str(x.dtype).replace("torch.", "") == "float32" for x in (pred, true))
        self.tdtype = torch.float32 if f32 else torch.float64
        self.code = _lib.FDX_F32 if f32 else _lib.FDX_F64
        with torch.cuda.device(self.device):
            self.stream = _lib.current_stream(self.device)
            self.P, self.ldp = values_on_device(pred, self.device, self.stream, self.tdtype)
            self.T, self.ldt = values_on_device(true, self.device, self.stream, self.tdtype)

    def run(self, moments=True, threshold=0.05, epsilon=1e-10, jsd=False, spearman=0):
        """(stats (K+1, FIELDS), rare int64 [n_rare, tp, fp, fn], rho (K+1), jsd device tensor or None): one device sequence,
        one host sync."""
        import torch
        lib = _lib.load()
        K = self.K
        stats = np.zeros((K + 1, _FIELDS))
        rare = np.zeros(4, dtype=np.int64)
        rho = np.full(K + 1, np.nan)
        with torch.cuda.device(self.device):
            jsd_t = torch.empty(self.n, dtype=torch.float64, device=self.device) if jsd else None
            jp = ctypes.c_void_p(jsd_t.data_ptr()) if jsd else None
            P, T = ctypes.c_void_p(self.P.data_ptr()), ctypes.c_void_p(self.T.data_ptr())
            if moments:
                _lib.check(lib.fdx_metrics_evaluate_dev(P, T, self.code, self.n, K, self.ldp, self.ldt, float(threshold),
                                                        float(epsilon), int(spearman), jp, _lib.ptr_f64(stats), _lib.ptr_i64(rare),
                                                        _lib.ptr_f64(rho), self.stream))
            else:
                _lib.check(lib.fdx_metrics_spearman_dev(P, T, self.code, self.n, K, self.ldp, self.ldt, int(spearman),
                                                        _lib.ptr_f64(rho), self.stream))
        return stats, rare, rho, jsd_t


def _ptp(row, mn, mx, nan):
    return np.nan if row[nan] else row[mx] - row[mn]


def _safe(row, value):
    """_safe_corr (metrics.py:98-103): 0.0 when either ptp is 0; a NaN ptp (a NaN entry) makes the correlation NaN."""
    if _ptp(row, _MIN_P, _MAX_P, _NAN_P) == 0 or _ptp(row, _MIN_T, _MAX_T, _NAN_T) == 0:
        return 0.0
    if row[_NAN_P] or row[_NAN_T]:
        return np.nan
    return value


def _pearson(row, N):
    """np.corrcoef(a, b)[0, 1] from the centred sums: covariance with ddof 1 divided by both standard deviations, clipped."""
    den = N - 1.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.float64(row[_C_PT] / den) / np.sqrt(np.float64(row[_C_PP] / den)) / np.sqrt(np.float64(row[_C_TT] / den))
    return np.clip(r, -1.0, 1.0)


def _correlations(stats, rho, n, K, method, per_cell_type):
    spearman = method == "spearman"
    if per_cell_type:
        out = np.zeros(K)
        for k in range(K):
            out[k] = _safe(stats[k], rho[k] if spearman else _pearson(stats[k], n))
        return out
    return _safe(stats[K], np.float64(rho[K]) if spearman else _pearson(stats[K], n * K))


def compute_rmse(pred, true, per_cell_type: bool = False):
    """Root mean squared error (metrics.py:12-41): per column with ``per_cell_type``, else over all entries."""
    pair = _Pair(pred, true)
    stats = pair.run()[0]
    if per_cell_type:
        return np.sqrt(stats[:pair.K, _SSE] / pair.n)
    return np.sqrt(np.float64(stats[pair.K, _SSE] / (pair.n * pair.K)))


def compute_mae(pred, true, per_cell_type: bool = False):
    """Mean absolute error (metrics.py:44-68)."""
    pair = _Pair(pred, true)
    stats = pair.run()[0]
    if per_cell_type:
        return stats[:pair.K, _SAE] / pair.n
    return np.float64(stats[pair.K, _SAE] / (pair.n * pair.K))


def compute_correlation(pred, true, method: str = "pearson", per_cell_type: bool = False):
    """Pearson or Spearman correlation (metrics.py:71-122): per column, or over ``pred.flatten()`` vs ``true.flatten()``.
    Any ``method`` other than ``"spearman"`` is Pearson, as in the reference."""
    pair = _Pair(pred, true)
    flags = (_SPEARMAN_PER_TYPE if per_cell_type else _SPEARMAN_OVERALL) if method == "spearman" else 0
    stats, _, rho, _ = pair.run(spearman=flags)
    return _correlations(stats, rho, pair.n, pair.K, method, per_cell_type)


def compute_jsd(pred, true, epsilon: float = 1e-10):
    """Per-spot Jensen-Shannon divergence (metrics.py:125-157): a float64 device tensor when both inputs are device tensors,
    else a numpy array."""
    pair = _Pair(pred, true)
    jsd = pair.run(epsilon=epsilon, jsd=True)[3]
    return jsd if pair.device_out else _lib.tensor_to_host(jsd)


def evaluate_deconvolution(pred, true, cell_type_names: Optional[np.ndarray] = None) -> dict:
    """Overall and per-cell-type RMSE, MAE, Pearson, Spearman, mean JSD and mean proportions (metrics.py:160-217), from one
    device sequence and one host sync."""
    pair = _Pair(pred, true)
    n, K = pair.n, pair.K
    if cell_type_names is None:
        cell_type_names = [f"CellType_{i}" for i in range(K)]
    stats, _, rho, _ = pair.run(jsd=True, spearman=_SPEARMAN_OVERALL | _SPEARMAN_PER_TYPE)
    N = n * K
    metrics = {
        "overall": {
            "rmse": float(np.sqrt(stats[K, _SSE] / N)),
            "mae": float(stats[K, _SAE] / N),
            "pearson": float(_correlations(stats, rho, n, K, "pearson", False)),
            "spearman": float(_correlations(stats, rho, n, K, "spearman", False)),
            "mean_jsd": float(stats[K, _JSD_SUM] / n),
        },
        "per_cell_type": {},
    }
    pearson_per = _correlations(stats, rho, n, K, "pearson", True)
    spearman_per = _correlations(stats, rho, n, K, "spearman", True)
    for k, name in enumerate(cell_type_names):
        if k >= K:
            raise IndexError(f"index {k} is out of bounds for axis 0 with size {K}")
        metrics["per_cell_type"][name] = {
            "rmse": float(np.sqrt(stats[k, _SSE] / n)),
            "mae": float(stats[k, _SAE] / n),
            "pearson": float(pearson_per[k]),
            "spearman": float(spearman_per[k]),
            "mean_proportion_true": float(stats[k, _SUM_T] / n),
            "mean_proportion_pred": float(stats[k, _SUM_P] / n),
        }
    return metrics


def compute_rare_cell_detection(pred, true, threshold: float = 0.05) -> Tuple[float, float, float]:
    """Precision, recall and F1 of detecting rare entries (0 < true < threshold) by pred > threshold / 2 (metrics.py:220-266);
    (nan, nan, nan) when no entry is rare."""
    pair = _Pair(pred, true)
    n_rare, tp, fp, fn = pair.run(threshold=threshold)[1]
    if n_rare == 0:
        return np.nan, np.nan, np.nan
    precision = tp / (tp + fp + 1e-10)
    recall = tp / (tp + fn + 1e-10)
    f1 = 2 * precision * recall / (precision + recall + 1e-10)
    return precision, recall, f1
