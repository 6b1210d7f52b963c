"""Gene-pair spatial co-expression: the bivariate Moran's R of pairs of genes - a ligand and its receptor - of a spot-by-gene matrix
over the model's graph, globally and per spot, computed on the GPU from one pass over the pairs' columns (additive, not in the
reference; the global and local R of SpatialDM).

**Inputs.**  ``Y`` and ``graph`` are those of ``utils.spatial_genes``: ``Y`` (n, G) dense float32 or float64 (integers through the
upload rules of ``_lib.upload_matrix``), host or CUDA, any row stride, or CSR from scipy or a CUDA ``torch.sparse_csr`` tensor (rows
with distinct columns, sorted or not); ``graph`` a fitted ``FlashDeconv``, a ``_lib.Graph`` or a scipy sparse adjacency.  ``A`` is
its symmetric binary adjacency, ``deg_i = sum_j A_ij``, ``W = sum_i deg_i``, ``sum_deg_sq = sum_i deg_i^2``.  ``pairs`` is (P, 2)
of integers, row p = ``(a, b)`` with ``0 <= a, b < G``; ``a == b`` is allowed and the same pair may occur twice.

**Sums.**  Per pair, in float64 on the value converted from its storage type (``fdx_gene_pair_sums_dev`` / ``_csr_dev``,
csrc/gene_pair_kernels.cpp, on torch's current stream), with ``lag_g,i = sum_{j in N(i)} y_jg`` in the graph's stored neighbour
order - the 17 planes of ``PLANES``::

    0 ua = sum y_a      1 ub = sum y_b      2 qa = sum y_a^2     3 qb = sum y_b^2     4 Da = sum deg y_a   5 Db = sum deg y_b
    6 S  = sum y_a y_b  7 Xab = sum y_a lag_b   8 Xba = sum y_b lag_a
    9 La = sum lag_a^2   10 Lb = sum lag_b^2      11 DLa = sum deg lag_a   12 DLb = sum deg lag_b
    13 amin  14 amax  15 bmin  16 bmax

A CSR entry that is not stored is the value 0 (the distinct genes of the pairs are gathered into a dense matrix of the storage type
on the device, in chunks of about 1 GiB).  No floating-point atomics and a fixed summation order (the graph's positions in segments
of 256, the segments in ascending order): two calls return the same bits, and a pair's numbers depend only on the graph and its two
columns - not on the other pairs of the call or on their order.  No float64 copy of ``Y`` is made.

**Statistics** (``assemble_pairs``, pure NumPy float64)::

    m_a = ua/n            m2_a = qa - ua^2/n                                  (likewise b)
    C   = (Xab + Xba)/2 - m_a Db - m_b Da + m_a m_b W                        (= Z_a' A Z_b, Z = Y - mean)
    morans_r  = (n/W) C / sqrt(m2_a m2_b)                                    bivariate Moran's R
    pearson_r = (S - ua ub/n) / sqrt(m2_a m2_b)
    LLc_a = La - 2 m_a DLa + m_a^2 sum_deg_sq          s_a = Da - m_a W      (sum_i (A Z_a)_i^2, sum_i (A Z_a)_i)
    variance_b_moved = (n/W)^2 (LLc_a - s_a^2/n) / ((n - 1) m2_a)
    variance_a_moved = the same with a and b exchanged
    z_score = morans_r / sqrt(max(variance_b_moved, variance_a_moved))
    p_value = erfc(z_score / sqrt 2) / 2          q_value = Benjamini-Hochberg over the pairs whose p_value is not NaN
    order   = pairs by decreasing morans_r, NaN last, ties by ascending index (int64)

``variance_b_moved`` is the EXACT variance of R over all n! reassignments of gene b's values to the spots while gene a stays in
place (the exact mean is 0); ``variance_a_moved`` is its mirror, and ``z_score`` takes the larger - the conservative - of the two.
``p_value`` is one-sided, for co-localisation.  These are the centred definitions expanded in the raw sums, which is what lets one
pass serve.  **Conditioning**: the expansion cancels - ``m2`` loses about ``eps * mean^2 / var`` of its relative accuracy (a gene
with mean 100 and variance 1 keeps 12 of 16 digits), and ``C`` and ``LLc`` likewise.  Expression matrices (counts, ``log1p`` of
counts) have means of the order of their standard deviations; a matrix with a large common offset should have it removed first.

Everything of a pair is NaN where ``amin == amax`` or ``bmin == bmax`` (a constant gene - decided exactly, not by a threshold),
where ``m2 <= 0``, ``W == 0``, ``n < 2``, or where the variance is not positive.  Nothing raises.

**Local score** (``local=True``), (n, P) float64 in the caller's spot order (``fdx_gene_pair_local_dev`` / ``_csr_dev``; it runs
after the sums, whose means and scales are its inputs)::

    local_i = (n / (2W)) [ (y_a,i - m_a)(lag_b,i - m_b deg_i) + (y_b,i - m_b)(lag_a,i - m_a deg_i) ] / sqrt(m2_a m2_b)

``sum_i local_i = morans_r`` up to rounding; a column is NaN for a pair whose statistics are NaN.

**Out of scope.**  Permutation p values per pair; multi-subunit complexes (the caller passes a combined column); attribution of a
pair to cell types; ``ShardedFlashDeconv``; normalising ``Y`` (the caller passes the matrix they want scored).
"""
import ctypes
import math

import numpy as np

from .. import _lib
from ._device import device_of, matrix_on_device, resolved_graph
from .spatial_genes import _benjamini_hochberg, _check_n_top, _check_Y_rows, _decreasing_order

__all__ = ["spatial_gene_pairs", "gene_pair_sums", "assemble_pairs", "check_request", "PLANES"]

PLANES = ("ua", "ub", "qa", "qb", "Da", "Db", "S", "Xab", "Xba", "La", "Lb", "DLa", "DLb", "amin", "amax", "bmin", "bmax")


def check_request(Y_shape, pairs):
    """The pairs of a request against the shape of ``Y``, before anything touches the GPU: ``pairs`` as a C-contiguous int32 (P, 2)
    array; ``ValueError`` for a shape other than (P, 2), ``P < 1``, a non-integer dtype or an index outside ``[0, G)``."""
    G = int(Y_shape[1])
    a = pairs.detach().cpu().numpy() if _lib.is_torch(pairs) else np.asarray(pairs)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError(f"pairs must be a (P, 2) array of gene indices, got shape {a.shape}")
    if a.shape[0] < 1:
        raise ValueError("pairs must hold at least one pair (P >= 1), got shape (0, 2)")
    if a.dtype.kind not in "iu":
        raise ValueError(f"pairs must be of an integer dtype, got {a.dtype}")
    if int(a.min()) < 0 or int(a.max()) >= G:
        bad = a[(a < 0) | (a >= G)][0]
        raise ValueError(f"pairs holds the gene index {int(bad)} outside [0, {G})")
    return np.ascontiguousarray(a, dtype=np.int32)


def _pair_sums(lib, g, m, n, G, pairs, device, stream):
    """The (17, P) sums (CUDA tensor) and the three integers of one call on the staged matrix ``m`` (``matrix_on_device``)."""
    import torch
    P = pairs.shape[0]
    counts = np.zeros(3, dtype=np.int64)
    sums = torch.empty((len(PLANES), P), dtype=torch.float64, device=device)
    if m[0] == "csr":
        _lib.check(lib.fdx_gene_pair_sums_csr_dev(g.handle, ctypes.byref(m[1].view), _lib.ptr_i32(pairs), P, 0,
                                                  ctypes.c_void_p(sums.data_ptr()), _lib.ptr_i64(counts), stream))
    else:
        _, ptr, code, ldy = m
        _lib.check(lib.fdx_gene_pair_sums_dev(g.handle, ptr, code, n, G, ldy, _lib.ptr_i32(pairs), P, ctypes.c_void_p(sums.data_ptr()),
                                              _lib.ptr_i64(counts), stream))
    host = _lib.tensor_to_host(sums)
    out = {name: host[k] for k, name in enumerate(PLANES)}
    out.update(n=int(counts[0]), W=int(counts[1]), sum_deg_sq=int(counts[2]))
    return out


def _pair_local(lib, g, m, n, G, pairs, stats, W, device, stream):
    """The (n, P) local scores (CUDA tensor) from the statistics of the sums."""
    import torch
    P = pairs.shape[0]
    dead = np.isnan(stats["morans_r"])
    with np.errstate(divide="ignore", invalid="ignore"):
        coef = np.where(dead, np.nan, (float(n) / (2.0 * float(W)) if W > 0 else np.nan) / np.sqrt(np.where(dead, 1.0, stats["m2_a"] * stats["m2_b"])))
    inputs = torch.as_tensor(np.stack([stats["mean_a"], stats["mean_b"], coef])).to(device)
    out = torch.empty((n, P), dtype=torch.float64, device=device)
    ma, mb, cf = (ctypes.c_void_p(inputs[k].data_ptr()) for k in range(3))
    if m[0] == "csr":
        _lib.check(lib.fdx_gene_pair_local_csr_dev(g.handle, ctypes.byref(m[1].view), _lib.ptr_i32(pairs), P, 0, ma, mb, cf,
                                                   ctypes.c_void_p(out.data_ptr()), P, stream))
    else:
        _, ptr, code, ldy = m
        _lib.check(lib.fdx_gene_pair_local_dev(g.handle, ptr, code, n, G, ldy, _lib.ptr_i32(pairs), P, ma, mb, cf,
                                               ctypes.c_void_p(out.data_ptr()), P, stream))
    torch.cuda.current_stream(device).synchronize()          # `inputs` goes back to the allocator with this frame
    return out


def _on_graph(Y, g, n, G, pairs, local):
    """(sums, statistics or None, local scores or None) on a resolved graph; ``local``: None (sums only), False or True."""
    import torch
    _lib.require_gpu()
    lib = _lib.load()
    device = device_of(Y)
    with torch.cuda.device(device):
        stream = _lib.current_stream(device)
        with matrix_on_device(Y, device) as m:
            s = _pair_sums(lib, g, m, n, G, pairs, device, stream)
            if local is None:
                return s, None, None
            stats = assemble_pairs(s["n"], s["W"], s["sum_deg_sq"], *(s[name] for name in PLANES))
            scores = _pair_local(lib, g, m, n, G, pairs, stats, s["W"], device, stream) if local else None
    return s, stats, scores


def gene_pair_sums(Y, graph, pairs):
    """The device half (module docstring): a dict of the 17 planes of ``PLANES`` - numpy float64 (P,) - and the integers ``n``,
    ``W``, ``sum_deg_sq``.  Shapes and dtypes are checked before anything touches the GPU."""
    n, G = _check_Y_rows(Y)
    pairs = check_request((n, G), pairs)
    with resolved_graph(graph, n) as g:
        return _on_graph(Y, g, n, G, pairs, None)[0]


def _pair_arithmetic(n, W, sum_deg_sq, ua, ub, qa, qb, Da, Db, S, Xab, Xba, La, Lb, DLa, DLb, amin, amax, bmin, bmax):
    """The arithmetic of the module docstring, element by element over float64 arrays that broadcast against each other (the (P,)
    planes of ``assemble_pairs``; (S, 1) / (1, S) / (S, S) for ``gene_modules.assemble_coexpression``): ``(mean_a, mean_b, m2_a,
    m2_b, morans_r, pearson_r, variance_b_moved, variance_a_moved, z_score)``, NaN by the rules stated there."""
    shape = np.broadcast(ua, ub).shape
    nan = np.full(shape, np.nan)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if n > 0:
            m_a, m_b, m2_a, m2_b = ua / n, ub / n, qa - ua * ua / n, qb - ub * ub / n
        else:
            m_a, m_b, m2_a, m2_b = nan, nan, nan, nan
        dead = (amin == amax) | (bmin == bmax) | ~(m2_a > 0) | ~(m2_b > 0)
        if W > 0 and n >= 2:
            nf, Wf = float(n), float(W)
            scale = np.sqrt(np.where(dead, 1.0, m2_a * m2_b))
            C = 0.5 * (Xab + Xba) - m_a * Db - m_b * Da + m_a * m_b * Wf
            R = (nf / Wf) * C / scale
            pearson = (S - ua * ub / nf) / scale
            LLc_a = La - 2.0 * m_a * DLa + m_a * m_a * float(sum_deg_sq)
            LLc_b = Lb - 2.0 * m_b * DLb + m_b * m_b * float(sum_deg_sq)
            s_a, s_b = Da - m_a * Wf, Db - m_b * Wf
            var_b_moved = (nf / Wf) ** 2 * (LLc_a - s_a * s_a / nf) / ((nf - 1.0) * m2_a)
            var_a_moved = (nf / Wf) ** 2 * (LLc_b - s_b * s_b / nf) / ((nf - 1.0) * m2_b)
            var = np.maximum(var_b_moved, var_a_moved)
            dead = dead | ~(np.isfinite(var) & (var > 0))
            z = R / np.sqrt(np.where(dead, 1.0, var))
        else:
            dead = np.ones(shape, dtype=bool)
            R = pearson = var_b_moved = var_a_moved = z = nan
    R, pearson, var_b_moved, var_a_moved, z = (np.where(dead, np.nan, x) for x in (R, pearson, var_b_moved, var_a_moved, z))
    return m_a, m_b, m2_a, m2_b, R, pearson, var_b_moved, var_a_moved, z


def assemble_pairs(n, W, sum_deg_sq, ua, ub, qa, qb, Da, Db, S, Xab, Xba, La, Lb, DLa, DLb, amin, amax, bmin, bmax):
    """The statistics of the module docstring from the sums of one call (pure host arithmetic): a dict of ``mean_a``, ``mean_b``,
    ``m2_a``, ``m2_b``, ``morans_r``, ``pearson_r``, ``variance_b_moved``, ``variance_a_moved``, ``z_score``, ``p_value``,
    ``q_value`` (P,) and ``order`` (P,) int64."""
    n, W, sum_deg_sq = int(n), int(W), int(sum_deg_sq)
    planes = [np.asarray(a, dtype=np.float64) for a in (ua, ub, qa, qb, Da, Db, S, Xab, Xba, La, Lb, DLa, DLb, amin, amax, bmin, bmax)]
    if planes[0].ndim != 1 or any(a.shape != planes[0].shape for a in planes):
        raise ValueError(f"the seventeen sums must be 1-D arrays of one length, got shapes {[a.shape for a in planes]}")
    m_a, m_b, m2_a, m2_b, R, pearson, var_b_moved, var_a_moved, z = _pair_arithmetic(n, W, sum_deg_sq, *planes)
    p = np.array([0.5 * math.erfc(v / math.sqrt(2.0)) if not math.isnan(v) else math.nan for v in z.tolist()], dtype=np.float64)
    return {"mean_a": m_a, "mean_b": m_b, "m2_a": m2_a, "m2_b": m2_b, "morans_r": R, "pearson_r": pearson,
            "variance_b_moved": var_b_moved, "variance_a_moved": var_a_moved, "z_score": z, "p_value": p,
            "q_value": _benjamini_hochberg(p), "order": _decreasing_order(R)}


def spatial_gene_pairs(Y, graph, pairs, local=False, n_top=None, output="numpy"):
    """Which pairs of genes are expressed next to each other, and where: the bivariate Moran's R of every pair of ``pairs`` over
    ``graph`` with Pearson's r, the z score under the exact permutation variance, one-sided p values and Benjamini-Hochberg q
    values and, with ``local=True``, the per-spot score whose column sums are R (module docstring).

    ``Y``: (n_spots, n_genes) - dense numpy / CUDA tensor, float32, float64 or integer counts, or CSR (scipy, CUDA
    ``torch.sparse_csr``); scored as it is passed (not normalised).  ``graph``: a fitted ``FlashDeconv``, a ``_lib.Graph`` or a
    scipy sparse adjacency.  ``pairs``: (P, 2) integer gene indices.  ``n_top``: also return ``top = order[:n_top]``.  ``output``:
    ``"numpy"``, or ``"torch"`` to leave ``local`` a CUDA tensor.  Arguments are checked before anything touches the GPU.

    Returns a dict of numpy arrays and Python scalars: ``morans_r``, ``pearson_r``, ``variance_b_moved``, ``variance_a_moved``,
    ``z_score``, ``p_value``, ``q_value``, ``mean_a``, ``mean_b``, ``m2_a``, ``m2_b`` (P,), ``order`` (P,) int64, ``pairs``
    (P, 2) int64, ``n``, ``n_edges``; with ``local=True`` also ``local`` (n_spots, P) float64 in the caller's spot order."""
    n, G = _check_Y_rows(Y)
    pairs = check_request((n, G), pairs)
    if not isinstance(local, (bool, np.bool_)):
        raise ValueError(f"local must be True or False, got {local!r}")
    n_top = _check_n_top(n_top)
    if output not in ("numpy", "torch"):
        raise ValueError(f"Unknown output: {output}. Choose from 'numpy', 'torch'.")
    with resolved_graph(graph, n) as g:
        s, out, scores = _on_graph(Y, g, n, G, pairs, bool(local))
    out.update(n=s["n"], n_edges=s["W"] // 2, pairs=pairs.astype(np.int64))
    if local:
        out["local"] = scores if output == "torch" else _lib.tensor_to_host(scores)
    if n_top is not None:
        out["top"] = out["order"][:n_top]
    return out
