"""Spatial niches (tissue domains): k-means of per-spot compositions, of their neighbourhood's composition or of both, on the GPU
(additive, not in the reference).

With ``F`` the (n, D) features and ``M`` the (C, D) centres, ``d2(i, c) = sum_k (F_ik - M_ck)^2`` - the difference formed first,
never the expanded form, which cancels on nearly collinear proportions - and Lloyd's loop is::

    labels = -1
    for it = 1 .. max_iter:
        labels, changed, inertia = assign(F, centres)        label_i = the smallest c attaining min_c d2(i, c)
        if changed == 0: converged, stop
        if it == max_iter: stop
        sums, counts = label_sums(F, labels)
        centres[c] = sums[c] / counts[c]   where counts[c] > 0      (an empty niche keeps its centre)

so the labels returned are always the arg-min of the centres returned.  The loop (``fdx_kmeans_dev``), the k-means++ distances
(``fdx_kmeans_seed_dist_dev``) and the per-niche sums (``fdx_label_sums_dev``) run in csrc/niche_kernels.cpp on torch's current
stream, float64 throughout and in a fixed summation order: two calls return the same bits.  The k-means++ draw itself is host
arithmetic on at most 1024 block sums and one block of distances (``pick_row``).
"""
import contextlib
import ctypes

import numpy as np

from .. import _lib
from .random import check_random_state
from ._device import check_values, device_of, resolved_graph, values_on_device
from .spatial_stats import spatial_sums

__all__ = ["spatial_niches", "kmeans", "kmeans_plusplus", "pick_row"]

MAX_NICHES = 64
FEATURE_MODES = ("composition", "neighborhood", "both")


def pick_row(block_sums, fetch_block, t):
    """The row a k-means++ draw ``t`` falls on: with ``d2`` the per-row weights cut into blocks of consecutive rows, the first row
    whose running sum of ``d2`` exceeds ``t`` - so rows of weight 0 are never drawn.  ``block_sums[b]`` is the sum of block b and
    ``fetch_block(b)`` returns ``(first_row, d2_of_the_block)``; only the block the draw falls in is fetched.  The running sum is
    carried over the block sums in ascending order and continued inside the block row by row.  Where the rounding of a block's own
    sum leaves the draw past its last row, the block's last row of positive weight is taken.  ``t`` must be below the total."""
    block_sums = np.asarray(block_sums, dtype=np.float64)
    running = np.float64(0.0)
    for b in range(block_sums.shape[0]):
        upto = running + block_sums[b]
        if upto > t:
            break
        running = upto
    else:
        raise ValueError(f"the draw {t!r} is not below the total weight {float(running)!r}")
    first, d2 = fetch_block(b)
    d2 = np.asarray(d2, dtype=np.float64)
    within = np.cumsum(np.concatenate(([running], d2)))[1:]          # sequential, continued from the blocks before
    j = int(np.searchsorted(within, t, side="right"))
    if j >= d2.shape[0]:
        j = int(np.flatnonzero(d2 > 0)[-1])
    return int(first) + j


def _check_n_niches(n_niches, n):
    if isinstance(n_niches, bool) or not isinstance(n_niches, (int, np.integer)):
        raise ValueError(f"n_niches must be an integer, got {n_niches!r}")
    if not 1 <= n_niches <= MAX_NICHES:
        raise ValueError(f"n_niches must be between 1 and {MAX_NICHES}, got {n_niches}")
    if n_niches > n:
        raise ValueError(f"n_niches ({n_niches}) must not exceed the number of spots ({n})")
    return int(n_niches)


def _check_max_iter(max_iter):
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 1:
        raise ValueError(f"max_iter must be a positive integer, got {max_iter!r}")
    return int(max_iter)


def _check_init(init, n, D):
    shape = check_values(init, "init")
    if shape[1] != D:
        raise ValueError(f"init must have the features' {D} columns, got shape {shape}")
    _check_n_niches(shape[0], n)
    return shape[0]


def _lloyd(F, ldf, n, D, init, max_iter, device, stream):
    """fdx_kmeans_dev on the device matrix F: (labels - a CUDA int32 tensor -, the rest of the result dict)."""
    import torch
    C = (tuple(init.shape) if _lib.is_torch(init) else np.shape(init))[0]
    centres, _ = values_on_device(init, device, stream)
    if _lib.is_cuda_tensor(init) or not centres.is_contiguous():
        centres = centres.clone(memory_format=torch.contiguous_format)          # updated in place: never the caller's tensor
    labels = torch.empty(n, dtype=torch.int32, device=device)
    counts = np.zeros(C, dtype=np.int64)
    inertia = ctypes.c_double(0.0)
    n_iter, converged = ctypes.c_int32(0), ctypes.c_int32(0)
    _lib.check(_lib.load().fdx_kmeans_dev(
        ctypes.c_void_p(F.data_ptr()), int(ldf), int(n), int(D), int(C), int(max_iter), ctypes.c_void_p(centres.data_ptr()),
        ctypes.c_void_p(labels.data_ptr()), _lib.ptr_i64(counts), ctypes.byref(inertia), ctypes.byref(n_iter),
        ctypes.byref(converged), stream))
    return labels, {"centers": _lib.tensor_to_host(centres), "counts": counts, "inertia": float(inertia.value),
                    "n_iter": int(n_iter.value), "converged": bool(converged.value)}


def _seed(F, ldf, n, D, C, rs, device, stream):
    """k-means++ on the device matrix F: the C chosen row indices."""
    import torch
    lib = _lib.load()
    d2 = torch.full((n,), float("inf"), dtype=torch.float64, device=device)
    block_sums = np.zeros(1024)
    block_rows, n_blocks = ctypes.c_int64(0), ctypes.c_int32(0)

    def fetch_block(b):
        first = b * block_rows.value
        return first, _lib.tensor_to_host(d2[first:min(n, first + block_rows.value)])

    rows = [int(rs.randint(n))]
    while len(rows) < C:
        _lib.check(lib.fdx_kmeans_seed_dist_dev(
            ctypes.c_void_p(F.data_ptr()), int(ldf), int(n), int(D), ctypes.c_void_p(F.data_ptr() + rows[-1] * int(ldf) * 8),
            ctypes.c_void_p(d2.data_ptr()), _lib.ptr_f64(block_sums), ctypes.byref(block_rows), ctypes.byref(n_blocks), stream))
        sums = block_sums[:n_blocks.value]
        total = np.float64(0.0)
        for s in sums:
            total = total + s
        if not total > 0:
            rows.append(int(rs.randint(n)))
            continue
        rows.append(pick_row(sums, fetch_block, rs.random_sample() * total))
    return rows


def kmeans(features, init, max_iter=100):
    """Lloyd's k-means of the rows of ``features`` from the centres ``init`` (the device half of ``spatial_niches``).

    ``features``: 2-D (n, D) numpy array or CUDA torch tensor, float32 or float64 (converted to float64 on the device; a numpy
    array is uploaded once; a tensor with unit column stride is read in place).  ``init``: (C, D), 1 <= C <= min(64, n).
    Returns a dict: ``labels`` (n,) int32 - a CUDA tensor when ``features`` was one, else numpy -, ``centers`` (C, D), ``counts``
    (C,) int64, ``inertia``, ``n_iter`` (assign passes) and ``converged``.  Shapes are checked before the GPU is touched."""
    n, D = check_values(features, "features")
    _check_init(init, n, D)
    max_iter = _check_max_iter(max_iter)
    import torch
    device_out = _lib.is_cuda_tensor(features)
    device = device_of(features)
    with torch.cuda.device(device):
        stream = _lib.current_stream(device)
        F, ldf = values_on_device(features, device, stream)
        labels, out = _lloyd(F, ldf, n, D, init, max_iter, device, stream)
        out["labels"] = labels if device_out else _lib.tensor_to_host(labels)
    return out


def kmeans_plusplus(features, n_niches, random_state=0):
    """k-means++ seeding: (n_niches, D) float64 numpy rows of ``features``.  The first is row ``rs.randint(n)``; each further one is
    drawn with probability proportional to its squared distance to the nearest row chosen so far (``pick_row`` on the device's
    block sums with ``t = rs.random_sample() * total``), so a row at distance 0 of a chosen one is never drawn; where every row is
    (``total == 0``), row ``rs.randint(n)``."""
    n, D = check_values(features, "features")
    C = _check_n_niches(n_niches, n)
    rs = check_random_state(random_state)
    import torch
    device = device_of(features)
    with torch.cuda.device(device):
        stream = _lib.current_stream(device)
        F, ldf = values_on_device(features, device, stream)
        rows = _seed(F, ldf, n, D, C, rs, device, stream)
        return _lib.tensor_to_host(F[torch.as_tensor(rows, device=device)])


def spatial_niches(values, n_niches, graph=None, features="composition", neighbor_weight=1.0, init="k-means++", max_iter=100,
                   random_state=0):
    """Groups spots into ``n_niches`` niches by k-means of their composition (``features="composition"``: the rows of ``values``),
    of their neighbours' mean composition (``"neighborhood"``: ``neighbor_mean`` of ``spatial_stats.spatial_sums`` over ``graph``)
    or of both (``"both"``: ``[values | neighbor_weight * neighbor_mean]``).

    ``values``: 2-D (n_spots, K) numpy array or CUDA torch tensor, float32 or float64.  ``graph`` (needed by the two neighbourhood
    modes): a fitted ``FlashDeconv``, a ``_lib.Graph`` or a scipy sparse adjacency, as ``spatial_autocorrelation`` takes it.
    ``init``: ``"k-means++"`` (seeded by ``random_state``) or the (n_niches, D) initial centres, D the width of the features.
    Returns the dict of ``kmeans`` plus ``composition`` (n_niches, K): the mean of ``values`` over each niche's spots, NaN rows
    for empty niches.  Every shape and argument check raises ``ValueError`` before the GPU is touched."""
    n, K = check_values(values, "values")
    C = _check_n_niches(n_niches, n)
    if features not in FEATURE_MODES:
        raise ValueError(f"Unknown features: {features!r}. Choose from {', '.join(repr(m) for m in FEATURE_MODES)}.")
    needs_graph = features != "composition"
    if needs_graph and graph is None:
        raise ValueError(f"features={features!r} needs a graph (a fitted FlashDeconv, a _lib.Graph or a scipy sparse adjacency)")
    w = float(neighbor_weight)
    if not np.isfinite(w):
        raise ValueError(f"neighbor_weight must be finite, got {neighbor_weight!r}")
    D = 2 * K if features == "both" else K
    plusplus = isinstance(init, str)
    if plusplus:
        if init != "k-means++":
            raise ValueError(f"Unknown init: {init!r}. Pass 'k-means++' or the ({C}, {D}) initial centres.")
        rs = check_random_state(random_state)
    elif _check_init(init, n, D) != C:
        raise ValueError(f"init must hold n_niches = {C} centres, got shape {tuple(np.shape(init))}")
    max_iter = _check_max_iter(max_iter)

    with (resolved_graph(graph, n) if needs_graph else contextlib.nullcontext()) as g:
        import torch
        device_out = _lib.is_cuda_tensor(values)
        device = device_of(values)
        with torch.cuda.device(device):
            stream = _lib.current_stream(device)
            V, ldv = values_on_device(values, device, stream)
            if needs_graph:
                nm = spatial_sums(V, g, neighbor_mean=True)["neighbor_mean"]
                F = nm if features == "neighborhood" else torch.cat([V, nm if w == 1.0 else w * nm], dim=1)
                ldf = F.stride(0)
            else:
                F, ldf = V, ldv
            if plusplus:
                rows = _seed(F, ldf, n, D, C, rs, device, stream)
                init = F[torch.as_tensor(rows, device=device)]
            labels, out = _lloyd(F, ldf, n, D, init, max_iter, device, stream)
            sums, counts = np.empty((C, K)), np.zeros(C, dtype=np.int64)
            _lib.check(_lib.load().fdx_label_sums_dev(ctypes.c_void_p(V.data_ptr()), int(ldv), int(n), int(K),
                                                      ctypes.c_void_p(labels.data_ptr()), int(C), _lib.ptr_f64(sums),
                                                      _lib.ptr_i64(counts), stream))
            with np.errstate(divide="ignore", invalid="ignore"):
                out["composition"] = np.where(counts[:, None] > 0, sums / counts[:, None], np.nan)
            out["labels"] = labels if device_out else _lib.tensor_to_host(labels)
    return out
