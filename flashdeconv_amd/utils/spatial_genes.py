"""Spatially variable genes: Moran's I and Geary's C per gene of a spot-by-gene matrix over the model's graph, and what the fitted
composition leaves of a gene's spatial pattern, computed on the GPU from one pass over ``Y`` (additive, not in the reference).

**Inputs.**  ``Y`` is (n, G): dense float32 or float64 (integers through the upload rules of ``_lib.upload_matrix``), host or CUDA,
any row stride; or CSR from scipy or a CUDA ``torch.sparse_csr`` tensor (rows with distinct columns, sorted or not), kept sparse -
the routes of ``utils.expression``.  ``graph`` is the argument of ``spatial_autocorrelation``: a fitted ``FlashDeconv``, a
``_lib.Graph`` or a scipy sparse adjacency.  ``A`` is its symmetric binary adjacency, ``deg_i = sum_j A_ij``, ``W = sum_i deg_i``.

**Sums.**  Per gene, in float64 on the value converted from its storage type (``fdx_gene_spatial_sums_dev`` / ``_csr_dev``,
csrc/gene_spatial_kernels.cpp, on torch's current stream)::

    u = sum_i y_i       q = sum_i y_i^2       c3 = sum_i y_i^3       c4 = sum_i y_i^4
    D = sum_i deg_i y_i                       H = sum_i deg_i y_i^2
    P = sum_i y_i lag_i,   lag_i = sum_{j in N(i)} y_j
    ymin = min_i y_i      ymax = max_i y_i

A CSR entry that is not stored is the value 0.  No floating-point atomics and a fixed summation order (the graph's positions in
segments of 256, the segments in ascending order): two calls return the same bits, whatever the launch looks like.  No float64 copy
of ``Y`` is made.

**Statistics** (``assemble_genes``, pure NumPy float64)::

    m  = u / n                  m2 = q - u*u/n                 m4 = c4 - 4 m c3 + 6 m^2 q - 3 n m^4
    morans_i = (n / W) (P - 2 m D + m^2 W) / m2
    gearys_c = ((n - 1) / (2 W)) (2 H - 2 P) / m2
    expected_i, variance_i, z_score        as spatial_stats.assemble (normality)
    variance_i_rand = spatial_stats.randomization_variance(n, W, sum_deg_sq, m2, m4)       z_score_rand from it
    p_value = erfc(z_score_rand / sqrt 2) / 2        (one-sided: positive autocorrelation)
    q_value = Benjamini-Hochberg over the genes whose p_value is not NaN
    order   = genes by decreasing morans_i, NaN last, ties by ascending index (int64)

These are the centred definitions (``Z = Y - m``: ``I = (n / W) sum Z (A Z) / sum Z^2``, Geary's C over the edges,
``m4 = sum Z^4``) expanded in the raw sums, which is what lets one pass over ``Y`` serve.  **Conditioning**: the expansion cancels -
``m2`` loses about ``eps * mean^2 / var`` of its relative accuracy (a gene with mean 100 and variance 1 keeps 12 of 16 digits) and
``m4`` more (about ``eps * mean^4 / (m4 / n)``).  Expression matrices (counts, ``log1p`` of counts) have means of the order of
their standard deviations; a matrix with a large common offset should have it removed first.

A statistic is NaN where ``ymin == ymax`` (a constant gene - decided exactly, not by a threshold), where ``m2 <= 0``, ``W == 0``,
``n < 2`` (``n < 4`` for the randomisation variance), or where its variance is not positive.  Nothing raises.

**Residual mode** (``weights`` (n, K) given, under the checks of ``celltype_expression``): the composition is fitted per gene,
``E = nnls_gram(weights' weights, weights' Y)`` (K, G), and the same statistics are formed for the residual ``R = Y - weights E``
without ever forming it: with ``N = A weights``, ``B = weights' Y``, ``M = N' Y``, ``A_w = weights' weights``, ``C_w = weights' N``,
``s_w = sum_i w_i``, ``d_w = sum_i deg_i w_i`` and ``e`` a column of ``E``::

    u_r = u - s_w.e      q_r = q - 2 e.B + e' A_w e      D_r = D - d_w.e      P_r = P - 2 e.M + e' C_w e

A gene with a spatial pattern of its own - a gradient or a state inside a cell type - keeps a high ``residual_morans_i``; one whose
pattern is where its cell types sit does not.

**Out of scope.**  Normalising ``Y`` (the caller passes the matrix they want scored; ``log1p`` on a CSR's data keeps it sparse);
permutation p values per gene (``utils.gene_permutations`` has them); Geary's C and the randomisation variance of the residual; ``ShardedFlashDeconv``.
"""
import ctypes
import math

import numpy as np

from .. import _lib
from ._device import check_matrix, device_of, matrix_on_device, resolved_graph
from .spatial_stats import assemble, randomization_variance

__all__ = ["spatially_variable_genes", "gene_spatial_sums", "assemble_genes", "check_request", "PLANES"]

PLANES = ("u", "q", "c3", "c4", "D", "H", "P", "ymin", "ymax")


def _sums_on_graph(Y, g, n, G, return_degree):
    """``gene_spatial_sums`` on a resolved graph."""
    import torch
    _lib.require_gpu()
    lib = _lib.load()
    device = device_of(Y)
    counts = np.zeros(3, dtype=np.int64)
    with torch.cuda.device(device):
        stream = _lib.current_stream(device)
        sums = torch.empty((len(PLANES), G), dtype=torch.float64, device=device)
        degree = torch.empty(n, dtype=torch.int32, device=device) if return_degree else None
        deg_p = ctypes.c_void_p(degree.data_ptr()) if return_degree else None
        with matrix_on_device(Y, device) as m:
            if m[0] == "csr":
                _lib.check(lib.fdx_gene_spatial_sums_csr_dev(g.handle, ctypes.byref(m[1].view), ctypes.c_void_p(sums.data_ptr()), deg_p,
                                                             _lib.ptr_i64(counts), stream))
            else:
                _, ptr, code, ldy = m
                _lib.check(lib.fdx_gene_spatial_sums_dev(g.handle, ptr, code, n, G, ldy, ctypes.c_void_p(sums.data_ptr()), deg_p,
                                                         _lib.ptr_i64(counts), stream))
        host = _lib.tensor_to_host(sums)
    out = {name: host[k] for k, name in enumerate(PLANES)}
    out.update(n=int(counts[0]), W=int(counts[1]), sum_deg_sq=int(counts[2]))
    if return_degree:
        out["degree"] = degree
    return out


def _check_Y_rows(Y):
    n, G = check_matrix(Y)
    if n < 1:
        raise ValueError(f"Y must have at least one spot, got shape {(n, G)}")
    return n, G


def gene_spatial_sums(Y, graph, return_degree=False):
    """The device half (module docstring): a dict of ``u``, ``q``, ``c3``, ``c4``, ``D``, ``H``, ``P``, ``ymin``, ``ymax`` - numpy
    float64 (G,) - and the integers ``n``, ``W``, ``sum_deg_sq``; with ``return_degree=True`` also ``degree``, an int32 CUDA tensor
    (n,) of ``deg_i`` in the caller's spot order.  Shapes and dtypes are checked before anything touches the GPU."""
    n, G = _check_Y_rows(Y)
    with resolved_graph(graph, n) as g:
        return _sums_on_graph(Y, g, n, G, bool(return_degree))


def _benjamini_hochberg(p):
    """q values over the entries of ``p`` that are not NaN (NaN elsewhere): ``q_(i) = min_{j >= i} p_(j) m / j``, at most 1."""
    q = np.full(p.shape, np.nan)
    idx = np.flatnonzero(~np.isnan(p))
    if idx.size:
        order = idx[np.argsort(p[idx], kind="stable")]
        scaled = p[order] * (float(idx.size) / np.arange(1, idx.size + 1))
        q[order] = np.minimum(1.0, np.minimum.accumulate(scaled[::-1])[::-1])
    return q


def _decreasing_order(x):
    """Indices by decreasing ``x``, NaN last, ties by ascending index (int64)."""
    return np.argsort(np.where(np.isnan(x), np.inf, -x), kind="stable").astype(np.int64)


def _z(stat, expected, variance):
    """``(stat - expected) / sqrt(variance)`` where the variance is positive and finite, else NaN (variance: scalar or (G,))."""
    variance = np.broadcast_to(np.asarray(variance, dtype=np.float64), stat.shape)
    ok = np.isfinite(variance) & (variance > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ok, (stat - expected) / np.sqrt(np.where(ok, variance, 1.0)), np.nan)


def _morans(n, W, u, q, D, P, dead):
    """(mean, m2, morans_i) from the raw sums; ``dead`` genes and genes without variance are NaN."""
    with np.errstate(divide="ignore", invalid="ignore"):
        m = u / n if n > 0 else np.full(u.shape, np.nan)
        m2 = q - u * u / n if n > 0 else np.full(u.shape, np.nan)
        if W > 0 and n >= 2:
            morans = np.where(dead | ~(m2 > 0), np.nan, (float(n) / float(W)) * (P - 2.0 * m * D + m * m * float(W)) / m2)
        else:
            morans = np.full(u.shape, np.nan)
    return m, m2, morans


def assemble_genes(n, W, sum_deg_sq, u, q, c3, c4, D, H, P, ymin, ymax):
    """The statistics of the module docstring from the sums of one call (pure host arithmetic): a dict of ``mean``, ``m2``, ``m4``,
    ``morans_i``, ``gearys_c``, ``z_score``, ``variance_i_rand``, ``z_score_rand``, ``p_value``, ``q_value`` (G,), ``order`` (G,)
    int64 and the scalars ``expected_i``, ``variance_i``."""
    n, W, sum_deg_sq = int(n), int(W), int(sum_deg_sq)
    u, q, c3, c4, D, H, P, ymin, ymax = (np.asarray(a, dtype=np.float64) for a in (u, q, c3, c4, D, H, P, ymin, ymax))
    if u.ndim != 1 or any(a.shape != u.shape for a in (q, c3, c4, D, H, P, ymin, ymax)):
        raise ValueError(f"the nine sums must be 1-D arrays of one length, got shapes {[a.shape for a in (u, q, c3, c4, D, H, P, ymin, ymax)]}")
    constant = ymin == ymax
    m, m2, morans = _morans(n, W, u, q, D, P, constant)
    dead = np.isnan(morans)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        m4 = c4 - 4.0 * m * c3 + 6.0 * (m * m) * q - 3.0 * n * (m * m) * (m * m)
        if W > 0 and n >= 2:
            geary = np.where(dead, np.nan, ((n - 1.0) / (2.0 * float(W))) * (2.0 * H - 2.0 * P) / m2)
        else:
            geary = np.full(u.shape, np.nan)
    norm = assemble(n, W, sum_deg_sq, np.ones(1), np.zeros((1, 1)))          # the two scalars of the normality assumption
    expected, variance = norm["expected_i"], norm["variance_i"]
    z = _z(morans, expected, variance)
    var_rand = np.where(dead, np.nan, randomization_variance(n, W, sum_deg_sq, np.where(dead, np.nan, m2), m4))
    z_rand = _z(morans, expected, var_rand)
    p = np.array([0.5 * math.erfc(v / math.sqrt(2.0)) if not math.isnan(v) else math.nan for v in z_rand.tolist()], dtype=np.float64)
    return {"mean": m, "m2": m2, "m4": m4, "morans_i": morans, "gearys_c": geary, "expected_i": expected, "variance_i": variance,
            "z_score": z, "variance_i_rand": var_rand, "z_score_rand": z_rand, "p_value": p, "q_value": _benjamini_hochberg(p),
            "order": _decreasing_order(morans)}


def _check_n_top(n_top):
    if n_top is None:
        return None
    if isinstance(n_top, (bool, np.bool_)) or not isinstance(n_top, (int, np.integer)) or n_top < 0:
        raise ValueError(f"n_top must be an int >= 0 or None, got {n_top!r}")
    return int(n_top)


def check_request(Y_shape, n_types):
    """What ``tl.deconvolve(..., spatial_genes=True)`` can check before the fit: the shape of ``Y`` and the number of cell types
    the residual columns regress on.  ``ValueError`` on the first that fails."""
    from .expression import check_request as check_expression
    check_expression(Y_shape, n_types)
    if Y_shape[0] < 1:
        raise ValueError(f"Y must have at least one spot, got shape {tuple(Y_shape)}")


def _host(x):
    return _lib.tensor_to_host(x) if _lib.is_torch(x) else np.asarray(x)


def _residual(Y, g, weights, s, base, ridge, max_iter, tol):
    """The residual keys (module docstring) from the sums ``s`` (with ``degree``) and the statistics ``base`` of ``Y`` itself."""
    from .expression import nnls_gram, weighted_gene_sums
    from .spatial_stats import spatial_sums
    n, W = s["n"], s["W"]
    on_device = _lib.is_cuda_tensor(weights)
    ws = weighted_gene_sums(Y, weights)
    sol = nnls_gram(ws["A"], ws["B"], ridge=ridge, max_iter=max_iter, tol=tol, q=ws["q"])
    sp = spatial_sums(weights, g, neighbor_mean=True)
    nm = sp["neighbor_mean"]
    if on_device:
        import torch
        N = torch.clamp(nm * s["degree"].to(device=nm.device, dtype=torch.float64)[:, None], min=0.0)
    else:                                                  # A weights; the mean was formed around the column mean, so rounding
        N = np.maximum(nm * _host(s["degree"]).astype(np.float64)[:, None], 0.0)    # may leave -1e-17 where it is 0
    # the K-sized sums through the gene pass as well, N as its matrix: B = weights' N, u = sum_i N_i = sum_i deg_i w_i (A is
    # symmetric) - a (K, n) x (n, K) float64 product is the shape BLAS libraries serve worst
    ns = weighted_gene_sums(N, weights)
    C_w, d_w, s_w = _host(ns["B"]), _host(ns["u"]), sp["mean"] * float(n)
    M = _host(weighted_gene_sums(Y, N)["B"])
    A_w, B, E, rss = _host(ws["A"]), _host(ws["B"]), _host(sol["expression"]), _host(sol["rss"])
    u_r = s["u"] - s_w @ E
    q_r = s["q"] - 2.0 * (E * B).sum(axis=0) + np.einsum("kg,kl,lg->g", E, A_w, E)
    D_r = s["D"] - d_w @ E
    P_r = s["P"] - 2.0 * (E * M).sum(axis=0) + np.einsum("kg,kl,lg->g", E, C_w, E)
    _, _, morans_r = _morans(n, W, u_r, q_r, D_r, P_r, np.isnan(base["morans_i"]))
    with np.errstate(divide="ignore", invalid="ignore"):
        q_w, u_w = _host(ws["q"]), _host(ws["u"])                          # the regression's own sums: celltype_expression's r2
        tss = np.maximum(q_w - (u_w * u_w) / n, 0.0)
        r2 = np.where(tss > 0, 1.0 - rss / np.where(tss > 0, tss, 1.0), np.nan)
    return {"residual_morans_i": morans_r, "residual_z_score": _z(morans_r, base["expected_i"], base["variance_i"]),
            "residual_order": _decreasing_order(morans_r), "r2": r2, "expression": E,
            "residual_sums": {"u": u_r, "q": q_r, "D": D_r, "P": P_r}}


def spatially_variable_genes(Y, graph, weights=None, ridge=0.0, max_iter=10000, tol=1e-10, n_top=None):
    """Which genes vary over the tissue - Moran's I and Geary's C per gene of ``Y`` over ``graph`` with their z scores, one-sided
    p values and Benjamini-Hochberg q values - and, with ``weights`` (n_spots, K), which still do once the composition is accounted
    for (module docstring).

    ``Y``: (n_spots, n_genes) - dense numpy / CUDA tensor, float32, float64 or integer counts, or CSR (scipy, CUDA
    ``torch.sparse_csr``); scored as it is passed (not normalised).  ``graph``: a fitted ``FlashDeconv``, a ``_lib.Graph`` or a
    scipy sparse adjacency.  ``weights``: float64, finite, non-negative, 1 to 272 columns - proportions or abundances, possibly
    scaled by each spot's library size; ``ridge``, ``max_iter``, ``tol`` go to the per-gene solve (``nnls_gram``).  ``n_top``: also
    return ``top = order[:n_top]``.  Arguments are checked before anything touches the GPU (``ValueError`` / ``TypeError``).

    Returns a dict of numpy arrays and Python scalars: ``morans_i``, ``gearys_c``, ``z_score``, ``variance_i_rand``,
    ``z_score_rand``, ``p_value``, ``q_value``, ``mean``, ``m2``, ``m4`` (G,), ``order`` (G,) int64, ``expected_i``,
    ``variance_i``, ``n``, ``n_edges``; with ``weights`` also ``residual_morans_i``, ``residual_z_score`` (normality),
    ``residual_order``, ``r2`` (as ``celltype_expression`` defines it) (G,), ``expression`` (K, G) and ``residual_sums`` (a dict of
    ``u``, ``q``, ``D``, ``P`` of the residual).  A gene that is NaN in ``morans_i`` is NaN in the residual keys as well."""
    from .expression import _check_scalars, _check_weights
    n, G = _check_Y_rows(Y)
    n_top = _check_n_top(n_top)
    if weights is not None:
        _check_weights(weights, n)
        ridge, max_iter, tol = _check_scalars(ridge, max_iter, tol)
    with resolved_graph(graph, n) as g:
        s = _sums_on_graph(Y, g, n, G, weights is not None)
        out = assemble_genes(s["n"], s["W"], s["sum_deg_sq"], *(s[name] for name in PLANES))
        out.update(n=s["n"], n_edges=s["W"] // 2)
        if weights is not None:
            out.update(_residual(Y, g, weights, s, out, ridge, max_iter, tol))
    if n_top is not None:
        out["top"] = out["order"][:n_top]
    return out
