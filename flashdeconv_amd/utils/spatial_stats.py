"""Spatial autocorrelation and co-localisation of per-spot values over the model's graph, computed on the GPU (additive, not in
the reference).

With ``V`` the (n, K) values, ``A`` the symmetric binary adjacency without self loops, ``W = nnz(A)`` and ``deg_i = sum_j A_ij``::

    mean_a = (1/n) sum_i V_ia        Z = V - mean        m2_a = sum_i Z_ia^2        C = Z' (A Z)
    cross_ab   = (n / W) C_ab / sqrt(m2_a m2_b)          bivariate Moran ("neighbourhood co-localisation")
    morans_i_a = cross_aa                                Moran's I
    E = -1 / (n - 1)      S1 = 2 W      S2 = 4 sum_i deg_i^2
    Var = (n^2 S1 - n S2 + 3 W^2) / ((n^2 - 1) W^2) - E^2          (normality assumption)
    z_score_a = (morans_i_a - E) / sqrt(Var)
    neighbor_mean_ia = (sum_j A_ij V_ja) / deg_i                   (0 where deg_i = 0)

The sums (``mean``, ``m2``, ``C``, ``W``, ``sum deg^2``, ``neighbor_mean``) come from ``fdx_spatial_autocorr_dev``
(csrc/spatial_stats_kernels.cpp) on torch's current stream, float64 throughout and in a fixed order: two calls return the same
bits.  ``assemble`` forms the statistics from them on the host.  Entries whose definition divides by zero (``W == 0``,
``m2_a == 0``, ``n < 2``, ``Var <= 0``) are NaN; nothing raises.
"""
import ctypes

import numpy as np

from .. import _lib

__all__ = ["spatial_autocorrelation", "spatial_sums", "assemble"]


def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


def _is_cuda_tensor(x):
    return _is_torch(x) and getattr(x, "is_cuda", False)


def assemble(n, W, sum_deg_sq, m2, C):
    """``cross``, ``morans_i``, ``expected_i``, ``variance_i`` and ``z_score`` from the sums of one call (pure host arithmetic).

    ``n`` spots, ``W = nnz(A)``, ``sum_deg_sq = sum_i deg_i^2``, ``m2`` (K,), ``C`` (K, K).  ``variance_i`` is reported as the
    formula gives it (NaN where ``n < 2`` or ``W == 0``); ``z_score`` is NaN where it is not positive."""
    n, W, sum_deg_sq = int(n), int(W), int(sum_deg_sq)
    m2 = np.asarray(m2, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    K = m2.shape[0]
    if m2.ndim != 1 or C.shape != (K, K):
        raise ValueError(f"m2 must be (K,) and C (K, K), got shapes {m2.shape} and {C.shape}")
    nan = np.float64(np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        den = np.sqrt(np.outer(m2, m2))
        if W > 0 and n >= 2:
            cross = np.where(den > 0, (float(n) / float(W)) * C / den, nan)
        else:
            cross = np.full((K, K), nan)
        # a column without variance has no statistic, whatever the product of the two m2 underflows or rounds to
        dead = ~(m2 > 0)
        cross[dead, :] = nan
        cross[:, dead] = nan
    morans = np.diagonal(cross).copy()
    expected = -1.0 / (n - 1.0) if n >= 2 else nan
    if n >= 2 and W > 0:
        nf, Wf = float(n), float(W)
        S1, S2 = 2.0 * Wf, 4.0 * float(sum_deg_sq)
        variance = np.float64((nf * nf * S1 - nf * S2 + 3.0 * Wf * Wf) / ((nf * nf - 1.0) * Wf * Wf) - expected * expected)
    else:
        variance = nan
    if np.isfinite(variance) and variance > 0:
        z = (morans - expected) / np.sqrt(variance)
    else:
        z = np.full(K, nan)
    return {"cross": cross, "morans_i": morans, "expected_i": np.float64(expected), "variance_i": np.float64(variance),
            "z_score": z}


def _check_adjacency(A, n_rows):
    """A scipy sparse adjacency as canonical CSR; shape, symmetry and the empty diagonal are checked on the host."""
    if A.ndim != 2 or A.shape[0] != A.shape[1]:
        raise ValueError(f"graph must be a square adjacency matrix, got shape {A.shape}")
    if A.shape[0] != n_rows:
        raise ValueError(f"values has {n_rows} rows but the graph has {A.shape[0]} spots")
    A = A.tocsr().astype(bool).astype(np.int8)        # binary weights: stored values only mark the edges
    A.eliminate_zeros()
    A.sum_duplicates()
    A.sort_indices()
    if A.diagonal().any():
        raise ValueError("graph must have no self loops (a non-zero diagonal entry was found)")
    if (A != A.T).nnz != 0:
        raise ValueError("graph must be symmetric")
    return A


def _resolve_graph(graph, n_rows):
    """(_lib.Graph, owned): the device graph behind `graph`; owned graphs are closed by the caller."""
    if isinstance(graph, _lib.Graph):
        g, owned = graph, False
    elif hasattr(graph, "_graph") and hasattr(graph, "_require_fitted"):      # a FlashDeconv
        graph._require_fitted()
        if graph._graph is None:
            raise RuntimeError("Model has not been fitted. Call fit() first.")
        g, owned = graph._graph, False
    elif hasattr(graph, "tocsr"):
        A = _check_adjacency(graph, n_rows)
        _lib.require_gpu()
        return _lib.Graph.from_csr(A.indptr, A.indices, A.shape[0]), True
    else:
        raise TypeError("graph must be a fitted FlashDeconv, a flashdeconv_amd._lib.Graph or a scipy sparse adjacency matrix, "
                        f"got {type(graph).__name__}")
    n = g.info()[0]
    if n != n_rows:
        raise ValueError(f"values has {n_rows} rows but the graph has {n} spots")
    return g, owned


def _values_on_device(values, device, stream):
    """(float64 device tensor with unit column stride, row stride)."""
    import torch
    if _is_cuda_tensor(values):
        v = values.detach()
        if v.dtype != torch.float64:
            v = v.to(torch.float64)
        if v.stride(1) != 1 or v.stride(0) < v.shape[1]:
            v = v.contiguous()
        return v, v.stride(0)
    if _is_torch(values):
        values = values.detach().numpy()
    a = np.asarray(values)
    a = np.ascontiguousarray(a, dtype=np.float32 if a.dtype == np.float32 else np.float64)
    d = torch.empty(a.shape, dtype=torch.float64, device=device)
    _lib.check(_lib.load().fdx_upload_convert_dev(ctypes.c_void_p(d.data_ptr()), _lib.FDX_F64, a.ctypes.data_as(ctypes.c_void_p),
                                                  _lib.SRC_CODES[a.dtype.name], a.size, None, stream))
    return d, a.shape[1]


def spatial_sums(values, graph, neighbor_mean=False):
    """The device half of ``spatial_autocorrelation``: a dict of ``mean``, ``m2`` (K,), ``C`` (K, K) - numpy - and the integers
    ``n``, ``W``, ``sum_deg_sq``, plus ``neighbor_mean`` (n, K) on request.  Same arguments and checks."""
    shape = tuple(values.shape) if _is_torch(values) else np.shape(values)
    if len(shape) != 2:
        raise ValueError(f"values must be a 2-D (n_spots, n_columns) array, got shape {shape}")
    n, K = shape
    if n < 1 or K < 1:
        raise ValueError(f"values must not be empty, got shape {shape}")
    dtype = str(values.dtype).replace("torch.", "") if hasattr(values, "dtype") else "float64"
    if _is_cuda_tensor(values) and dtype not in ("float32", "float64"):
        raise ValueError(f"values must be float32 or float64, got {dtype}")
    g, owned = _resolve_graph(graph, n)
    try:
        import torch
        device_out = _is_cuda_tensor(values)
        device = values.device if device_out else torch.device("cuda", torch.cuda.current_device())
        mean, m2, C = np.empty(K), np.empty(K), np.empty((K, K))
        counts = np.zeros(3, dtype=np.int64)
        with torch.cuda.device(device):
            stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
            V, ldv = _values_on_device(values, device, stream)
            nm = torch.empty((n, K), dtype=torch.float64, device=device) if neighbor_mean else None
            _lib.check(_lib.load().fdx_spatial_autocorr_dev(
                g.handle, ctypes.c_void_p(V.data_ptr()), int(ldv), int(K), _lib.ptr_f64(mean), _lib.ptr_f64(m2), _lib.ptr_f64(C),
                _lib.ptr_i64(counts), ctypes.c_void_p(nm.data_ptr()) if neighbor_mean else None, stream))
            out = {"mean": mean, "m2": m2, "C": C, "n": int(counts[0]), "W": int(counts[1]), "sum_deg_sq": int(counts[2])}
            if neighbor_mean:
                out["neighbor_mean"] = nm if device_out else _lib.tensor_to_host(nm)
    finally:
        if owned:
            g.close()
    return out


def spatial_autocorrelation(values, graph, neighbor_mean=False):
    """Moran's I per column of ``values``, the K x K bivariate Moran matrix and, on request, each spot's neighbour-averaged values.

    ``values``: 2-D (n_spots, K) numpy array or CUDA torch tensor, float32 or float64 (converted to float64 on the device; a numpy
    array is uploaded once).  ``graph``: a fitted ``FlashDeconv`` (its device graph is used as it stands), a ``_lib.Graph``, or a
    scipy sparse adjacency - square, symmetric, no diagonal, any non-zero counts as an edge - which is uploaded for the call.
    Shapes are checked before anything touches the GPU (``ValueError``).

    Returns a dict: ``morans_i``, ``z_score``, ``mean``, ``m2`` (K,), ``cross`` (K, K), ``expected_i``, ``variance_i``, ``n``,
    ``n_edges`` (undirected edges: ``W = 2 n_edges``), all numpy / Python scalars; with ``neighbor_mean=True`` also
    ``neighbor_mean`` (n, K), a CUDA tensor when ``values`` was one, else numpy."""
    s = spatial_sums(values, graph, neighbor_mean)
    out = {"mean": s["mean"], "m2": s["m2"], "n": s["n"], "n_edges": s["W"] // 2}
    out.update(assemble(s["n"], s["W"], s["sum_deg_sq"], s["m2"], s["C"]))
    if neighbor_mean:
        out["neighbor_mean"] = s["neighbor_mean"]
    return out
