"""Cell-type expression in tissue: per-gene non-negative least squares of a spot-by-gene matrix on the fitted abundances, computed on
the GPU from one pass over ``Y`` (additive, not in the reference).  What does each cell type express in THIS tissue, which genes
does the fitted composition explain - over all spots or per group of spots (the niches of ``get_spatial_niches``, say).

**Inputs.**  ``Y`` is (n, G): dense float32 or float64 (integers through the upload rules of ``_lib.upload_matrix``), host or CUDA,
any row stride; or CSR from scipy or a CUDA ``torch.sparse_csr`` tensor (rows with distinct columns, sorted or not), kept sparse.
``W`` is (n, K) float64, finite and non-negative, 1 <= K <= 272.  ``groups`` is optional: (n,) integers in ``[-1, C)``; ``-1``
leaves a spot out; ``None`` means one group of all rows.  Scalars: ``ridge >= 0``, ``max_iter >= 1``, ``tol > 0``.

**Sums.**  For each group c, with its rows R_c taken in ascending row index, everything in float64::

    n_c    = |R_c|
    A_c    = sum_i w_i w_i'            (K, K)
    B_c    = sum_i w_i y_i'            (K, G)
    q_c[g] = sum_i y_ig^2      u_c[g] = sum_i y_ig

**Solve.**  For each (c, g), with ``D_k = A_c[k,k] + ridge * mean(diag A_c)`` (the diagonal added in ascending k, divided by K) and
``b = B_c[:, g]``, cyclic coordinate descent from ``s = 0``::

    for it = 1 .. max_iter:
        dmax = 0
        for k = 0 .. K-1:
            new  = max(0, (b_k - sum_{j != k} A_c[k,j] s_j) / D_k)   if D_k > 0 else 0
            dmax = max(dmax, |new - s_k|);  s_k = new
        if dmax <= tol * max_k s_k: converged, stop        (all-zero s: 0 <= 0, converged)

The device keeps the running gradient ``A s - b`` and updates it by ``A[:,k] * delta_k`` instead of forming the dot product each
step: results agree up to rounding, not bit for bit.

**Outputs.**  ``expression`` (C, K, G);  ``rss = max(0, q - 2 s.b + s' A_c s)`` with ``A_c`` without the ridge;
``tss = max(0, q - u^2 / n_c)`` (0 for an empty group);  ``r2 = 1 - rss / tss``, NaN where ``tss == 0``;  ``n_iter`` (C, G) int32;
``converged`` (C, G) bool;  ``gram`` (C, K, K), ``n_rows`` (C,);  ``estimable`` (C, K) = ``A_c[k,k] > 0`` - a type absent from a
group gets ``s_k = 0`` and ``estimable`` False; nothing raises.  With ``groups=None`` the leading C axis is dropped.

The sums come from ``fdx_weighted_gene_sums_dev`` / ``fdx_weighted_gene_sums_csr_dev`` and the solves from ``fdx_nnls_gram_dev``
(csrc/expression_kernels.cpp) on torch's current stream: float64 arithmetic, no floating-point atomics, a fixed summation order (the
rows of a group in segments of 2048, the segments in ascending order) - two calls return the same bits, whatever the launch looks
like.  No float64 copy of ``Y`` is made.
"""
import ctypes

import numpy as np

from .. import _lib
from ._device import check_matrix as _check_Y, device_of, matrix_on_device

__all__ = ["celltype_expression", "weighted_gene_sums", "nnls_gram", "check_request", "MAX_TYPES"]

MAX_TYPES = 272


def _check_weights(W, n):
    """K of the (n, K) float64 weights: shape, dtype, and for host weights finiteness and sign."""
    shape = tuple(W.shape) if hasattr(W, "shape") else np.shape(W)
    if len(shape) != 2:
        raise ValueError(f"weights must be a 2-D (n_spots, n_types) array, got shape {shape}")
    if shape[0] != n:
        raise ValueError(f"Y has {n} rows but weights has {shape[0]}")
    K = int(shape[1])
    if K < 1 or K > MAX_TYPES:
        raise ValueError(f"weights must have 1 to {MAX_TYPES} columns, got {K}")
    if _lib.is_cuda_tensor(W):
        if str(W.dtype) != "torch.float64":
            raise ValueError(f"weights on the device must be float64, got {W.dtype}")
        return K
    Wh = W.detach().numpy() if _lib.is_torch(W) else np.asarray(W)
    if Wh.dtype.kind not in "fiub":
        raise ValueError(f"weights must be numeric, got dtype {Wh.dtype}")
    if not np.all(np.isfinite(Wh)):
        raise ValueError("weights must be finite")
    if np.any(Wh < 0):
        raise ValueError("weights must be non-negative")
    return K


def _check_scalars(ridge, max_iter, tol):
    if isinstance(ridge, (bool, np.bool_)) or not isinstance(ridge, (int, float, np.integer, np.floating)) or not ridge >= 0 \
            or not np.isfinite(ridge):
        raise ValueError(f"ridge must be a finite number >= 0, got {ridge!r}")
    if isinstance(max_iter, (bool, np.bool_)) or not isinstance(max_iter, (int, np.integer)) or max_iter < 1:
        raise ValueError(f"max_iter must be an int >= 1, got {max_iter!r}")
    if isinstance(tol, (bool, np.bool_)) or not isinstance(tol, (int, float, np.integer, np.floating)) or not tol > 0 \
            or not np.isfinite(tol):
        raise ValueError(f"tol must be a finite number > 0, got {tol!r}")
    return float(ridge), int(max_iter), float(tol)


def _check_n_groups(n_groups):
    if n_groups is None:
        return None
    if isinstance(n_groups, (bool, np.bool_)) or not isinstance(n_groups, (int, np.integer)) or n_groups < 1 or n_groups > 65535:
        raise ValueError(f"n_groups must be an int from 1 to 65535, got {n_groups!r}")
    return int(n_groups)


def _check_groups(groups, n, n_groups):
    """The labels checked as far as the host can: (labels or None, C or None - None when CUDA labels must tell it)."""
    C = _check_n_groups(n_groups)
    if groups is None:
        if C not in (None, 1):
            raise ValueError(f"n_groups = {C} without groups")
        return None, 1
    shape = tuple(groups.shape) if hasattr(groups, "shape") else np.shape(groups)
    if len(shape) != 1 or shape[0] != n:
        raise ValueError(f"groups must be a 1-D array of {n} labels, got shape {shape}")
    if _lib.is_cuda_tensor(groups):
        if groups.dtype.is_floating_point or str(groups.dtype) == "torch.bool":
            raise ValueError(f"groups must be integers, got {groups.dtype}")
        return groups, C
    g = groups.detach().numpy() if _lib.is_torch(groups) else np.asarray(groups)
    if g.dtype.kind not in "iu":
        raise ValueError(f"groups must be integers, got dtype {g.dtype}")
    g = g.astype(np.int64)
    lo, hi = (int(g.min()), int(g.max())) if n else (0, -1)
    if C is None:
        C = max(hi + 1, 1)
        if C > 65535:
            raise ValueError(f"at most 65535 groups, got labels up to {hi}")
    if lo < -1 or hi >= C:
        raise ValueError(f"groups must lie in [-1, {C}), got labels from {lo} to {hi}")
    return g, C


def check_request(Y_shape, n_types, groups=None, n_groups=None, ridge=0.0, max_iter=10000, tol=1e-10):
    """What ``tl.deconvolve(..., celltype_expression=True)`` can check before the fit: the shape of ``Y``, the number of cell types
    and the keywords of ``celltype_expression``.  ``ValueError`` on the first that fails."""
    if len(Y_shape) != 2 or Y_shape[1] < 1:
        raise ValueError(f"Y must be a 2-D (n_spots, n_genes) matrix with at least one gene, got shape {tuple(Y_shape)}")
    if n_types < 1 or n_types > MAX_TYPES:
        raise ValueError(f"cell-type expression is built for 1 to {MAX_TYPES} cell types, got {n_types}")
    _check_groups(groups, int(Y_shape[0]), n_groups)
    _check_scalars(ridge, max_iter, tol)


def _sort_groups(labels, C, n, device, stream):
    """(rows int32 device tensor or None, group_off int32 host array, C): a stable sort of the labels, the ``-1`` rows dropped."""
    import torch
    if labels is None:
        return None, np.array([0, n], dtype=np.int32), 1
    if _lib.is_cuda_tensor(labels):
        lab = labels.detach().to(device=device, dtype=torch.int64)
        lo, hi = (int(lab.min().item()), int(lab.max().item())) if n else (0, -1)
        if C is None:
            C = max(hi + 1, 1)
        if lo < -1 or hi >= C or C > 65535:
            raise ValueError(f"groups must lie in [-1, {C}) with at most 65535 groups, got labels from {lo} to {hi}")
        order = torch.sort(lab, stable=True).indices
        counts = _lib.tensor_to_host(torch.bincount(lab + 1, minlength=C + 1))
        rows = order[int(counts[0]):].to(torch.int32).contiguous()
    else:
        order = np.argsort(labels, kind="stable")
        counts = np.bincount(labels + 1, minlength=C + 1)
        rows_h = np.ascontiguousarray(order[int(counts[0]):], dtype=np.int32)
        rows = torch.empty(max(rows_h.size, 1), dtype=torch.int32, device=device)
        if rows_h.size:
            _lib.check(_lib.load().fdx_memcpy_h2d(ctypes.c_void_p(rows.data_ptr()), rows_h.ctypes.data_as(ctypes.c_void_p),
                                                  rows_h.nbytes, stream))
    off = np.zeros(C + 1, dtype=np.int32)
    off[1:] = np.cumsum(counts[1:])
    return rows, off, C


def _weights_on_device(W, device, stream):
    """(float64 device tensor with unit column stride, row stride)."""
    import torch
    if _lib.is_cuda_tensor(W):
        w = W.detach().to(device)
        if w.stride(1) != 1 or w.stride(0) < w.shape[1]:
            w = w.contiguous()
        return w, w.stride(0)
    Wh = _lib.as_f64(W.detach().numpy() if _lib.is_torch(W) else W)
    d = torch.empty(Wh.shape, dtype=torch.float64, device=device)
    if Wh.size:
        _lib.check(_lib.load().fdx_memcpy_h2d(ctypes.c_void_p(d.data_ptr()), Wh.ctypes.data_as(ctypes.c_void_p), Wh.nbytes, stream))
    return d, Wh.shape[1]


def _sums_device(Y, W, labels, C, n, G, K):
    """The sums as device tensors: (A (C, K, K), B (C, K, G), q, u (C, G), n_rows (C,) host int64)."""
    import torch
    _lib.require_gpu()
    lib = _lib.load()
    device = device_of(Y, W, labels)
    with torch.cuda.device(device):
        stream = _lib.current_stream(device)
        rows, off, C = _sort_groups(labels, C, n, device, stream)
        Wd, ldw = _weights_on_device(W, device, stream)
        A = torch.empty((C, K, K), dtype=torch.float64, device=device)
        B = torch.empty((C, K, G), dtype=torch.float64, device=device)
        q = torch.empty((C, G), dtype=torch.float64, device=device)
        u = torch.empty((C, G), dtype=torch.float64, device=device)
        out = [ctypes.c_void_p(t.data_ptr()) for t in (A, B, q, u)]
        rows_p = ctypes.c_void_p(rows.data_ptr()) if rows is not None else None
        with matrix_on_device(Y, device) as m:
            if m[0] == "csr":
                _lib.check(lib.fdx_weighted_gene_sums_csr_dev(ctypes.byref(m[1].view), ctypes.c_void_p(Wd.data_ptr()), int(ldw), K,
                                                              rows_p, _lib.ptr_i32(off), C, *out, stream))
            else:
                _, ptr, code, ldy = m
                _lib.check(lib.fdx_weighted_gene_sums_dev(ptr, code, n, G, ldy, ctypes.c_void_p(Wd.data_ptr()), int(ldw), K, rows_p,
                                                          _lib.ptr_i32(off), C, *out, stream))
    return A, B, q, u, np.diff(off.astype(np.int64))


def weighted_gene_sums(Y, weights, groups=None, n_groups=None):
    """The sufficient statistics of the regressions (module docstring): a dict of ``A`` (C, K, K), ``B`` (C, K, G), ``q``, ``u``
    (C, G) float64 and ``n_rows`` (C,) int64 - CUDA tensors when ``weights`` is one, else numpy (``n_rows`` always numpy); without
    ``groups`` the C axis is dropped.  Shapes, dtypes, host weights and host labels are checked before anything touches the GPU."""
    n, G = _check_Y(Y)
    K = _check_weights(weights, n)
    labels, C = _check_groups(groups, n, n_groups)
    A, B, q, u, n_rows = _sums_device(Y, weights, labels, C, n, G, K)
    out = {"A": A, "B": B, "q": q, "u": u}
    if groups is None:
        out = {k: v[0] for k, v in out.items()}
    if not _lib.is_cuda_tensor(weights):
        out = {k: _lib.tensor_to_host(v) for k, v in out.items()}
    out["n_rows"] = n_rows if groups is not None else n_rows[0]
    return out


def _solve_device(A, B, q, ridge, max_iter, tol):
    """``fdx_nnls_gram_dev`` on contiguous float64 device tensors A (C, K, K), B (C, K, G), q (C, G) or None."""
    import torch
    C, K, G = B.shape
    device = B.device
    with torch.cuda.device(device):
        stream = _lib.current_stream(device)
        S = torch.empty((C, K, G), dtype=torch.float64, device=device)
        n_iter = torch.empty((C, G), dtype=torch.int32, device=device)
        conv = torch.empty((C, G), dtype=torch.int32, device=device)
        rss = torch.empty((C, G), dtype=torch.float64, device=device) if q is not None else None
        _lib.check(_lib.load().fdx_nnls_gram_dev(
            ctypes.c_void_p(A.data_ptr()), ctypes.c_void_p(B.data_ptr()), ctypes.c_void_p(q.data_ptr()) if q is not None else None,
            int(C), int(K), int(G), float(ridge), int(max_iter), float(tol), ctypes.c_void_p(S.data_ptr()),
            ctypes.c_void_p(n_iter.data_ptr()), ctypes.c_void_p(conv.data_ptr()),
            ctypes.c_void_p(rss.data_ptr()) if rss is not None else None, stream))
    return S, n_iter, conv.to(torch.bool), rss


def nnls_gram(A, B, ridge=0.0, max_iter=10000, tol=1e-10, q=None):
    """The solves alone (module docstring), from sums the caller has: ``A`` (K, K) or (C, K, K), symmetric, ``B`` (K, G) or
    (C, K, G), ``q`` (G,) or (C, G) or None - numpy arrays or float64 CUDA tensors.  Returns a dict of ``expression`` like ``B``,
    ``n_iter`` int32, ``converged`` bool and, with ``q``, ``rss`` - CUDA tensors when ``B`` is one, else numpy."""
    ridge, max_iter, tol = _check_scalars(ridge, max_iter, tol)
    sa, sb = tuple(A.shape), tuple(B.shape)
    grouped = len(sb) == 3
    if len(sb) not in (2, 3) or len(sa) != len(sb):
        raise ValueError(f"A must be (K, K) and B (K, G), or (C, K, K) and (C, K, G); got shapes {sa} and {sb}")
    K, G = sb[-2], sb[-1]
    if sa[-1] != K or sa[-2] != K or (grouped and sa[0] != sb[0]):
        raise ValueError(f"A must be (K, K) and B (K, G), or (C, K, K) and (C, K, G); got shapes {sa} and {sb}")
    if K < 1 or K > MAX_TYPES or G < 1 or (grouped and not 1 <= sb[0] <= 65535):
        raise ValueError(f"1 to {MAX_TYPES} types, at least one gene and 1 to 65535 groups; got shapes {sa} and {sb}")
    if q is not None and tuple(q.shape) != sb[:-2] + (G,):
        raise ValueError(f"q must have shape {sb[:-2] + (G,)}, got {tuple(q.shape)}")
    for name, x in (("A", A), ("B", B), ("q", q)):
        if x is None:
            continue
        if _lib.is_cuda_tensor(x):
            if str(x.dtype) != "torch.float64":
                raise ValueError(f"{name} on the device must be float64, got {x.dtype}")
        elif not np.all(np.isfinite(np.asarray(x, dtype=np.float64))):
            raise ValueError(f"{name} must be finite")
    if not _lib.is_cuda_tensor(A):
        Ah = np.asarray(A, dtype=np.float64)
        if not np.array_equal(Ah, np.swapaxes(Ah, -1, -2)):
            raise ValueError("A must be symmetric")
    _lib.require_gpu()
    import torch
    device = device_of(B, A, q)

    def dev(x, shape):
        if x is None:
            return None
        if _lib.is_cuda_tensor(x):
            return x.detach().to(device).reshape(shape).contiguous()
        h = _lib.as_f64(x).reshape(shape)
        d = torch.empty(shape, dtype=torch.float64, device=device)
        _lib.check(_lib.load().fdx_memcpy_h2d(ctypes.c_void_p(d.data_ptr()), h.ctypes.data_as(ctypes.c_void_p), h.nbytes,
                                              _lib.current_stream(device)))
        return d
    C = sb[0] if grouped else 1
    with torch.cuda.device(device):
        S, n_iter, conv, rss = _solve_device(dev(A, (C, K, K)), dev(B, (C, K, G)), dev(q, (C, G)), ridge, max_iter, tol)
    out = {"expression": S, "n_iter": n_iter, "converged": conv}
    if rss is not None:
        out["rss"] = rss
    if not grouped:
        out = {k: v[0] for k, v in out.items()}
    if not _lib.is_cuda_tensor(B):
        out = {k: _lib.tensor_to_host(v) for k, v in out.items()}
    return out


def celltype_expression(Y, weights, groups=None, n_groups=None, ridge=0.0, max_iter=10000, tol=1e-10, output="numpy"):
    """What each cell type expresses in the tissue ``Y`` was measured on, given each spot's weights (module docstring).

    ``Y``: (n_spots, n_genes) - dense numpy / CUDA tensor, float32, float64 or integer counts, or CSR (scipy, CUDA
    ``torch.sparse_csr``).  ``weights``: (n_spots, K) float64, non-negative - proportions or abundances, possibly scaled by each
    spot's library size.  ``groups``: (n_spots,) integer labels in ``[-1, n_groups)``, ``-1`` = left out (``n_groups`` None: the
    largest label + 1).  ``output``: ``"numpy"`` or ``"torch"`` (the arrays stay on the device).  Arguments are checked before
    anything touches the GPU (``ValueError``).

    Returns a dict: ``expression`` (C, K, G), ``rss``, ``tss``, ``r2`` (C, G), ``n_iter`` (C, G) int32, ``converged`` (C, G) bool,
    ``gram`` (C, K, K), ``n_rows`` (C,) int64, ``estimable`` (C, K) bool; without ``groups`` the C axis is dropped."""
    if output not in ("numpy", "torch"):
        raise ValueError(f"Unknown output: {output}. Choose from 'numpy', 'torch'.")
    n, G = _check_Y(Y)
    K = _check_weights(weights, n)
    labels, C = _check_groups(groups, n, n_groups)
    ridge, max_iter, tol = _check_scalars(ridge, max_iter, tol)
    import torch
    A, B, q, u, n_rows = _sums_device(Y, weights, labels, C, n, G, K)
    S, n_iter, conv, rss = _solve_device(A, B, q, ridge, max_iter, tol)
    with torch.cuda.device(A.device):
        cnt = torch.as_tensor(n_rows, dtype=torch.float64).to(A.device)[:, None]
        tss = torch.clamp(q - (u * u) / torch.where(cnt > 0, cnt, torch.ones_like(cnt)), min=0.0)
        r2 = torch.where(tss > 0, 1.0 - rss / torch.where(tss > 0, tss, torch.ones_like(tss)), torch.full_like(tss, float("nan")))
        estimable = torch.diagonal(A, dim1=1, dim2=2) > 0
        n_rows_t = torch.as_tensor(n_rows, dtype=torch.int64).to(A.device)
    out = {"expression": S, "rss": rss, "tss": tss, "r2": r2, "n_iter": n_iter, "converged": conv, "gram": A, "n_rows": n_rows_t,
           "estimable": estimable}
    if groups is None:
        out = {k: v[0] for k, v in out.items()}
    if output == "numpy":
        out = {k: _lib.tensor_to_host(v) if v.dim() else v.item() for k, v in out.items()}
    return out
