"""Spatial correlogram: Moran's I and the co-localisation matrix by distance band, computed on the GPU in one walk over the
pairs within the largest radius, with no graph built (additive, not in the reference).

Inputs are ``coords`` (n, dim), 1 <= dim <= 3 as for radius graphs, and values ``V`` (n, K).  The radii satisfy
``0 < r_1 < ... < r_B``, all finite, 1 <= B <= 32.  The distance is ``d_ij = sqrt((dx*dx + dy*dy) + dz*dz)``, every operation
rounded (the radius graph's ``dist2_exact`` followed by ``sqrt``).  Ordered pairs i != j go into bands::

    band 1:  d_ij <= r_1                 (coincident spots, d = 0, land here)
    band b:  r_{b-1} < d_ij <= r_b

so the union of bands 1 .. b is the adjacency of ``build_radius_graph(coords, r_b)``, entry for entry.  Per band, with
``Z = V - mean`` and ``A_b`` the band's binary adjacency::

    deg_{b,i}     = #{j in band b of i}
    W_b           = sum_i deg_{b,i}
    sum_deg_sq_b  = sum_i deg_{b,i}^2
    C_b           = Z' A_b Z                      (K, K)

and each band is assembled by ``spatial_stats.assemble(n, W_b, sum_deg_sq_b, m2, C_b)``: ``cross`` (B, K, K), ``morans_i``,
``z_score`` (B, K), ``expected_i`` and ``variance_i`` (B,); with ``m4 = sum_i Z^4``, ``spatial_stats.randomization_variance``
gives ``variance_i_rand`` and ``z_score_rand`` (B, K).  The NaN rules are ``assemble``'s: an empty band, ``m2_a == 0`` or
``n < 2`` gives NaN; nothing raises.

The sums come from ``fdx_spatial_correlogram_dev`` (csrc/correlogram_kernels.cpp) on torch's current stream: float64 throughout,
no floating-point atomics, a fixed order - two calls return the same bits, and nothing depends on how many bands are processed per
pass.  The walk examines ``sum over grid cells of count(cell) * count(the 3^dim block of cells around it)`` candidate pairs (cell
edge just above r_B); that number is computed first and a call where it exceeds ``max_candidates`` fails before any pair is
walked - a careless radius on a large slide is an n^2 kernel otherwise.
"""
import ctypes

import numpy as np

from .. import _lib
from ._device import check_count, check_values, device_of, values_on_device
from .spatial_stats import assemble, randomization_variance

__all__ = ["spatial_correlogram", "correlogram_sums", "assemble_correlogram", "correlogram_request", "MAX_BANDS"]

MAX_BANDS = 32


def _check_radii(radii):
    """The radii as a float64 array: 1-D, 1 to 32 of them, finite, positive, strictly ascending."""
    r = np.asarray(radii, dtype=np.float64)
    if r.ndim != 1 or r.size == 0:
        raise ValueError(f"radii must be a non-empty 1-D sequence, got shape {r.shape}")
    if r.size > MAX_BANDS:
        raise ValueError(f"at most {MAX_BANDS} radii, got {r.size}")
    if not np.all(np.isfinite(r)):
        raise ValueError("radii must be finite")
    if not np.all(r > 0):
        raise ValueError("radii must be positive")
    if not np.all(np.diff(r) > 0):
        raise ValueError("radii must be strictly ascending")
    return np.ascontiguousarray(r)


def _check_n_bands(n_bands):
    nb = check_count("n_bands", n_bands, 1)
    if nb > MAX_BANDS:
        raise ValueError(f"at most {MAX_BANDS} bands, got n_bands = {nb}")
    return nb


def correlogram_request(arg):
    """What ``tl.deconvolve(..., correlogram=arg)`` asks for, checked without a GPU: None when it is off (``False``, ``None``),
    else the keywords of ``spatial_correlogram`` - ``{}`` for ``True`` (default radii), ``{"n_bands": arg}`` for an int from 1 to
    32, ``{"radii": ...}`` for a sequence that passes the radii checks.  ``ValueError`` for anything else."""
    if arg is None or (isinstance(arg, (bool, np.bool_)) and not arg):
        return None
    if isinstance(arg, (bool, np.bool_)):
        return {}
    if isinstance(arg, (int, np.integer)):
        return {"n_bands": _check_n_bands(arg)}
    if isinstance(arg, (str, bytes)) or not hasattr(arg, "__len__"):
        raise ValueError(f"correlogram must be a bool, a number of bands or a sequence of radii, got {arg!r}")
    return {"radii": [float(r) for r in _check_radii(arg)]}


def _check_coords(coords, n_rows):
    """(n, dim) of ``coords``: a 2-D numpy array (anything numeric) or float64 CUDA tensor with 1 to 3 columns and ``n_rows`` rows."""
    shape = tuple(coords.shape) if _lib.is_torch(coords) else np.shape(coords)
    if len(shape) != 2 or shape[1] == 0:
        raise ValueError(f"coords must be 2D with at least 1 coordinate dimension, got shape {shape}")
    if shape[1] > 3:
        raise ValueError(f"coords has {shape[1]} dimensions: the correlogram is built for 1 to 3 coordinate dimensions")
    if shape[0] != n_rows:
        raise ValueError(f"values has {n_rows} rows but coords has {shape[0]}")
    if _lib.is_cuda_tensor(coords) and str(coords.dtype) != "torch.float64":
        raise ValueError(f"coords on the device must be float64, got {coords.dtype}")
    return shape


def _check_common(values, coords, max_bands_per_pass, max_candidates):
    n, K = check_values(values)
    _check_coords(coords, n)
    check_count("max_bands_per_pass", max_bands_per_pass, 0)
    if max_candidates is not None:
        check_count("max_candidates", max_candidates, 1)
    return n, K


def _coords_host(coords):
    if _lib.is_cuda_tensor(coords):
        return _lib.tensor_to_host(coords)
    if _lib.is_torch(coords):
        coords = coords.detach().numpy()
    return _lib.as_f64(coords)


def correlogram_sums(values, coords, radii, max_bands_per_pass=0, degree=False, max_candidates=None):
    """The device half of ``spatial_correlogram``: a dict of ``mean``, ``m2``, ``m4`` (K,), ``C`` (B, K, K) - numpy float64 -
    ``W``, ``sum_deg_sq`` (B,) int64, the integers ``n``, ``bands_per_pass`` (bands whose lag planes were in flight at once:
    what the scratch budget holds, at most ``max_bands_per_pass`` when that is positive; no value depends on it) and
    ``candidates`` (the candidate pairs the walk examined), plus ``degree`` (n, B) int32 on request.  Same arguments and checks
    as ``spatial_correlogram``, with ``radii`` given."""
    n, K = _check_common(values, coords, max_bands_per_pass, max_candidates)
    r = _check_radii(radii)
    B = r.size
    _lib.require_gpu()
    import torch
    device_out = _lib.is_cuda_tensor(values)
    device = device_of(values, coords)
    mean, m2, m4, C = np.empty(K), np.empty(K), np.empty(K), np.empty((B, K, K))
    W, sds = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    bpp, cand = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int64)
    with torch.cuda.device(device):
        stream = _lib.current_stream(device)
        V, ldv = values_on_device(values, device, stream)
        if _lib.is_cuda_tensor(coords):
            xy = coords.detach().to(device).contiguous()
        else:
            ch = _coords_host(coords)
            xy = torch.empty(ch.shape, dtype=torch.float64, device=device)
            _lib.check(_lib.load().fdx_memcpy_h2d(ctypes.c_void_p(xy.data_ptr()), ch.ctypes.data_as(ctypes.c_void_p), ch.nbytes,
                                                  stream))
        deg = torch.empty((n, B), dtype=torch.int32, device=device) if degree else None
        _lib.check(_lib.load().fdx_spatial_correlogram_dev(
            ctypes.c_void_p(xy.data_ptr()), int(n), int(xy.shape[1]), ctypes.c_void_p(V.data_ptr()), int(ldv), int(K),
            _lib.ptr_f64(r), int(B), int(max_bands_per_pass), 0 if max_candidates is None else int(max_candidates),
            _lib.ptr_f64(mean), _lib.ptr_f64(m2), _lib.ptr_f64(m4), _lib.ptr_f64(C), _lib.ptr_i64(W), _lib.ptr_i64(sds),
            ctypes.c_void_p(deg.data_ptr()) if degree else None, _lib.ptr_i32(bpp), _lib.ptr_i64(cand), stream))
        out = {"mean": mean, "m2": m2, "m4": m4, "C": C, "W": W, "sum_deg_sq": sds, "n": int(n), "bands_per_pass": int(bpp[0]),
               "candidates": int(cand[0])}
        if degree:
            out["degree"] = deg if device_out else _lib.tensor_to_host(deg)
    return out


def assemble_correlogram(n, W, sum_deg_sq, m2, m4, C):
    """The statistics of every band from the sums of one call (pure host arithmetic): ``spatial_stats.assemble`` and
    ``spatial_stats.randomization_variance`` per band, stacked.  ``W``, ``sum_deg_sq`` (B,), ``m2``, ``m4`` (K,), ``C`` (B, K, K).
    Returns ``cross`` (B, K, K), ``morans_i``, ``z_score``, ``variance_i_rand``, ``z_score_rand`` (B, K), ``expected_i`` and
    ``variance_i`` (B,).  ``z_score_rand`` is NaN where the randomisation variance is not positive."""
    W = np.asarray(W).astype(np.int64)
    sds = np.asarray(sum_deg_sq).astype(np.int64)
    m2 = np.asarray(m2, dtype=np.float64)
    m4 = np.asarray(m4, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    if W.ndim != 1 or sds.shape != W.shape:
        raise ValueError(f"W and sum_deg_sq must be (B,), got shapes {W.shape} and {sds.shape}")
    B = W.shape[0]
    if m2.ndim != 1 or m4.shape != m2.shape or C.shape != (B, m2.shape[0], m2.shape[0]):
        raise ValueError(f"m2 and m4 must be (K,) and C (B, K, K), got shapes {m2.shape}, {m4.shape} and {C.shape}")
    K = m2.shape[0]
    out = {"cross": np.empty((B, K, K)), "morans_i": np.empty((B, K)), "z_score": np.empty((B, K)), "expected_i": np.empty(B),
           "variance_i": np.empty(B), "variance_i_rand": np.empty((B, K)), "z_score_rand": np.empty((B, K))}
    for b in range(B):
        a = assemble(n, W[b], sds[b], m2, C[b])
        for key in ("cross", "morans_i", "z_score", "expected_i", "variance_i"):
            out[key][b] = a[key]
        var = randomization_variance(n, W[b], sds[b], m2, m4)
        with np.errstate(divide="ignore", invalid="ignore"):
            z = np.where(var > 0, (a["morans_i"] - a["expected_i"]) / np.sqrt(np.where(var > 0, var, 1.0)), np.nan)
        out["variance_i_rand"][b] = var
        out["z_score_rand"][b] = z
    return out


def spatial_correlogram(values, coords, radii=None, n_bands=10, degree=False, max_candidates=None):
    """Moran's I per column of ``values`` and the K x K bivariate Moran matrix in every distance band of ``radii``.

    ``values``: as for ``spatial_autocorrelation`` - a 2-D (n_spots, K) numpy array or CUDA torch tensor, float32 or float64, any
    row stride.  ``coords``: (n_spots, dim) numpy array or float64 CUDA tensor, 1 <= dim <= 3, rows in the order of ``values``.
    ``radii``: 1 to 32 finite values, ``0 < r_1 < ... < r_B``; None: ``grid_radius(coords) * (1 .. n_bands)``, so that band 1 is
    the adjacency of ``build_grid_graph(coords)``.  ``max_candidates``: the most candidate pairs the walk may examine (None: the
    library's default - about ten seconds of walking, the walks that K columns and B bands need counted in); a call that
    would exceed it raises.  Shapes, row counts, the dimension and the
    radii are checked before anything touches the GPU (``ValueError``).

    Returns a dict: ``radii`` (B,), ``n_pairs`` (B,) int64 (unordered pairs per band, ``W_b / 2``), ``n``, ``mean``, ``m2`` (K,),
    everything ``assemble_correlogram`` returns and, with ``degree=True``, ``degree`` (n, B) int32 - a CUDA tensor when
    ``values`` was one, else numpy."""
    _check_common(values, coords, 0, max_candidates)
    if radii is None:
        nb = _check_n_bands(n_bands)
        from .graph import grid_radius
        r = grid_radius(_coords_host(coords)) * np.arange(1, nb + 1, dtype=np.float64)
        r = _check_radii(r)
    else:
        r = _check_radii(radii)
    s = correlogram_sums(values, coords, r, degree=degree, max_candidates=max_candidates)
    out = {"radii": r, "n_pairs": s["W"] // 2, "n": s["n"], "mean": s["mean"], "m2": s["m2"]}
    out.update(assemble_correlogram(s["n"], s["W"], s["sum_deg_sq"], s["m2"], s["m4"], s["C"]))
    if degree:
        out["degree"] = s["degree"]
    return out
