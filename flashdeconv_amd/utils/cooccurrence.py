"""Label co-occurrence by distance band: at which distances two niches, cell types or clusters occur together more often than
chance, and where the association stops - the join counts of ``utils.neighborhoods`` in every distance band of
``utils.correlogram``, with their exact moments and a permutation null, counted on the GPU with no graph built (additive, not in
the reference).  The ``co_occurrence`` entry of the usual spatial toolkits.

**Definitions.**  ``coords`` (n, dim), 1 <= dim <= 3; radii ``0 < r_1 < ... < r_B``, all finite, 1 <= B <= 32.  Distance and band
membership are exactly the correlogram's: ``d_ij = sqrt((dx*dx + dy*dy) + dz*dz)``, every operation rounded (the radius graph's
``dist2_exact`` followed by ``sqrt``), and ordered pairs i != j go into bands::

    band 1:  d_ij <= r_1                 (coincident spots, d = 0, land here)
    band b:  r_{b-1} < d_ij <= r_b

so the union of bands 1 .. b is the adjacency of ``build_radius_graph(coords, r_b)``, entry for entry.  Labels ``l_i`` in
``{-1, 0 .. C - 1}``, C <= 64, follow the convention of ``utils.neighborhoods``: a spot labelled ``-1`` is shuffled with the rest,
is never counted, and still counts in ``n`` and in the degrees.  Per band::

    N_b[a][c]        = #{(i, j) in band b : l_i = a, l_j = c}
    deg_{b,i}        = #{j in band b of i}        W_b = sum_i deg_{b,i}        sum_deg_sq_b = sum_i deg_{b,i}^2

and cumulatively ("within r_b")::

    Ncum_b = sum_{b' <= b} N_{b'}        Wcum_b = sum_{b' <= b} W_{b'}        sum_deg_sq_cum_b = sum_i (sum_{b' <= b} deg_{b',i})^2

(the last is no function of the per-band sums: the device forms it from the per-spot degrees).  The null: under permutation ``r``
of ``seed`` the labels are ``l^r_i = l[pi_r(i)]`` with ``pi_r = utils.spatial_stats.permutation_indices(seed, r, n)`` in the
caller's spot order - the same ``(seed, r)`` is the same relabelling as in ``label_pair_counts`` - and ``N^r_b``, ``Ncum^r_b`` are
the counts of ``l^r``.

**Device half** (``label_band_counts``: ``fdx_label_cooccurrence_dev``, csrc/label_band_kernels.cpp, on torch's current stream).  A
pair's band does not depend on the permutation, so one distance computation serves the 8 or 16 permutations of a group.  Every
count is an exact integer; nothing depends on the batching, on the bands per pass, on the grid or on how a range of permutations
is split into calls; two calls return the same bits.  The walk examines ``sum over grid cells of count(cell) * count(the 3^dim
block of cells around it)`` candidate pairs (cell edge just above r_B); that number is computed first and a call where it exceeds
``max_candidates`` fails before any pair is walked.

**Statistics** (``assemble_cooccurrence``, pure NumPy), per band or per cumulative band, from ``join_count_moments(n, W,
sum_deg_sq, n_a)`` with the matching sums::

    z_score     = (N - E) / sqrt(Var)                          NaN where Var is not positive
    interaction = N_ac / sum_c N_ac                            the share of label a's band-b neighbours that carry c; NaN for empty rows
    ratio       = N_ac N_.. / (N_a. N_.c)                      that share over c's share of all band-b pair ends; NaN where a row or
                                                               column is empty
    p_greater, p_less, p_value, null_mean, null_std, z_sim     as ``assemble_enrichment`` defines them, through ``rank_against_null``

**Out of scope.**  Edge-corrected Ripley functions; sharded coordinates; conditional shuffles that keep the ``-1`` spots fixed;
weights other than binary; more than 64 labels or 32 bands.
"""
import ctypes

import numpy as np

from .. import _lib
from ._device import check_count, device_of
from ._permutation import _permutation_seed, check_permutation_counts
from .correlogram import _check_coords, _check_n_bands, _check_radii, _coords_host
from .neighborhoods import _check_flag, _labels_on_device, assemble_enrichment, check_labels

__all__ = ["label_cooccurrence", "label_band_counts", "assemble_cooccurrence", "cooccurrence_request", "MODES"]

MODES = ("band", "cumulative")
_NULL_KEYS = ("count_ge", "count_le", "sum_d", "sumsq_d")


def _check_mode(mode):
    if mode not in MODES:
        raise ValueError(f"Unknown mode: {mode}. Choose from 'band', 'cumulative'.")
    return mode


def cooccurrence_request(arg):
    """What ``tl.deconvolve(..., co_occurrence=arg)`` asks for, checked without a GPU: None when it is off (``False``, ``None``),
    else the keywords of ``label_cooccurrence`` - ``{}`` for ``True`` (default radii), ``{"n_bands": arg}`` for an int from 1 to
    32, ``{"radii": ...}`` for a sequence that passes the radii checks.  ``ValueError`` for anything else."""
    if arg is None or (isinstance(arg, (bool, np.bool_)) and not arg):
        return None
    if isinstance(arg, (bool, np.bool_)):
        return {}
    if isinstance(arg, (int, np.integer)):
        return {"n_bands": _check_n_bands(arg)}
    if isinstance(arg, (str, bytes)) or not hasattr(arg, "__len__"):
        raise ValueError(f"co_occurrence must be a bool, a number of bands or a sequence of radii, got {arg!r}")
    return {"radii": [float(r) for r in _check_radii(arg)]}


def _check_common(labels, coords, n_labels, max_candidates):
    n, labels, C = check_labels(labels, n_labels)
    try:
        _check_coords(coords, n)
    except ValueError as e:                                    # (the correlogram's check speaks of its values)
        raise ValueError(str(e).replace("values has", "labels has")) from None
    if max_candidates is not None:
        check_count("max_candidates", max_candidates, 1)
    return n, labels, C


def label_band_counts(labels, coords, radii, n_labels=None, seed=0, first_perm=0, n_permutations=0, max_batch=0,
                      max_bands_per_pass=0, max_blocks=0, max_candidates=None, degree=False, return_null=False):
    """The device half of ``label_cooccurrence`` (``fdx_label_cooccurrence_dev``): a dict of ``count`` (B, C, C) and
    ``label_counts`` (C,) int64, the integer ``n``, ``W``, ``sum_deg_sq``, ``sum_deg_sq_cum`` (B,) int64, and over permutations
    ``first_perm .. first_perm + n_permutations - 1`` of ``seed`` the (B, C, C) arrays ``count_ge``, ``count_le`` (int64),
    ``sum_d``, ``sumsq_d`` (float64) of ``d = N^r_b - N_b`` and ``count_ge_cum``, ``count_le_cum``, ``sum_d_cum``, ``sumsq_d_cum``
    of ``d = Ncum^r_b - Ncum_b``, the sums added in permutation order; ``batch`` (permutations per launch chain), ``bands_per_pass``
    (bands counted per walk) and ``candidates`` (the candidate pairs one walk examines) report what ran; ``degree=True`` adds
    ``degree`` (n, B) int32 and ``return_null=True`` adds ``null`` (n_permutations, B, C, C) int64 with every ``N^r_b`` - CUDA
    tensors when ``labels`` was one, else numpy.

    ``labels``: (n,) integers in ``[-1, n_labels)``, numpy or a CUDA tensor of any integer dtype; ``n_labels``: 1 .. 64 (None: the
    largest label + 1).  ``coords``: (n, dim) numpy array or float64 CUDA tensor, 1 <= dim <= 3, rows in the order of ``labels``.
    ``radii``: 1 to 32 finite values, strictly ascending.  ``max_batch``, ``max_bands_per_pass`` and ``max_blocks`` cap the
    permutations of a launch chain, the bands of a walk and the workgroups of a group (0: the plan's choice; the blocks a
    workgroup's 32-bit bins need go before ``max_blocks``); no result depends on any of them, nor on how a range of permutations
    is split into calls.  ``max_candidates``: the most candidate pairs a walk may examine (None: the library's default, the walks
    this call needs counted in).  Everything checkable is checked before the GPU is touched."""
    n, labels, C = _check_common(labels, coords, n_labels, max_candidates)
    r = _check_radii(radii)
    n_perm, first_perm, max_batch = check_permutation_counts(n_permutations, first_perm, max_batch)
    max_bpp = check_count("max_bands_per_pass", max_bands_per_pass, 0)
    max_blocks = check_count("max_blocks", max_blocks, 0)
    degree, return_null = _check_flag("degree", degree), _check_flag("return_null", return_null)
    seed = _permutation_seed(seed)
    B = r.size
    _lib.require_gpu()
    import torch
    device_out = _lib.is_cuda_tensor(labels)
    device = device_of(labels, coords)
    with torch.cuda.device(device):
        stream = _lib.current_stream(device)
        lab, C = _labels_on_device(labels, C, device)
        if _lib.is_cuda_tensor(coords):
            xy = coords.detach().to(device).contiguous()
        else:
            ch = _coords_host(coords)
            xy = torch.empty(ch.shape, dtype=torch.float64, device=device)
            _lib.check(_lib.load().fdx_memcpy_h2d(ctypes.c_void_p(xy.data_ptr()), ch.ctypes.data_as(ctypes.c_void_p), ch.nbytes,
                                                  stream))
        label_counts, pair, deg_sums = np.zeros(C, dtype=np.int64), np.zeros((B, C, C), dtype=np.int64), np.zeros((3, B), dtype=np.int64)
        ge, le = np.zeros((2, B, C, C), dtype=np.int64), np.zeros((2, B, C, C), dtype=np.int64)
        sd, sq = np.zeros((2, B, C, C)), np.zeros((2, B, C, C))
        batch, bpp, cand = ctypes.c_int32(0), ctypes.c_int32(0), np.zeros(1, dtype=np.int64)
        deg = torch.empty((n, B), dtype=torch.int32, device=device) if degree else None
        null = torch.empty((n_perm, B, C, C), dtype=torch.int64, device=device) if return_null else None
        try:
            _lib.check(_lib.load().fdx_label_cooccurrence_dev(
                ctypes.c_void_p(xy.data_ptr()), int(n), int(xy.shape[1]), ctypes.c_void_p(lab.data_ptr()), int(C), _lib.ptr_f64(r),
                int(B), ctypes.c_uint64(seed), int(first_perm), int(n_perm), int(max_batch), int(max_bpp), int(max_blocks),
                0 if max_candidates is None else int(max_candidates), ctypes.c_void_p(deg.data_ptr()) if degree else None,
                ctypes.c_void_p(null.data_ptr()) if return_null and n_perm > 0 else None, _lib.ptr_i64(label_counts),
                _lib.ptr_i64(pair), _lib.ptr_i64(deg_sums), _lib.ptr_i64(ge), _lib.ptr_i64(le), _lib.ptr_f64(sd), _lib.ptr_f64(sq),
                ctypes.byref(batch), ctypes.byref(bpp), _lib.ptr_i64(cand), stream))
        except _lib.FdxError as e:
            if "outside [-1, C)" in str(e):
                raise ValueError(f"labels must lie in [-1, {C}): the device found one that does not") from e
            raise
        out = {"count": pair, "label_counts": label_counts, "n": int(n), "W": deg_sums[0].copy(), "sum_deg_sq": deg_sums[1].copy(),
               "sum_deg_sq_cum": deg_sums[2].copy(), "n_permutations": int(n_perm), "batch": int(batch.value),
               "bands_per_pass": int(bpp.value), "candidates": int(cand[0])}
        for key, arr in zip(_NULL_KEYS, (ge, le, sd, sq)):
            out[key], out[key + "_cum"] = arr[0].copy(), arr[1].copy()
        if degree:
            out["degree"] = deg if device_out else _lib.tensor_to_host(deg)
        if return_null:
            out["null"] = null if device_out else _lib.tensor_to_host(null)
    return out


def assemble_cooccurrence(count, label_counts, n, W, sum_deg_sq, sum_deg_sq_cum=None, count_ge=None, count_le=None, sum_d=None,
                          sumsq_d=None, n_permutations=0, mode="band"):
    """The statistics of the module docstring from the sums of ``label_band_counts`` (pure host arithmetic).  ``count`` (B, C, C),
    ``W`` and ``sum_deg_sq`` (B,) are the PER-BAND values in both modes; ``mode="cumulative"`` forms their running sums over the
    bands itself, takes ``sum_deg_sq_cum`` (B,) in the place of ``sum_deg_sq`` and needs it.  With ``n_permutations`` R >= 1 the
    four (B, C, C) arrays ``count_ge``, ``count_le``, ``sum_d``, ``sumsq_d`` of the mode are needed (the ``_cum`` ones of
    ``label_band_counts`` for ``"cumulative"``).

    Returns a dict of ``count`` (B, C, C) int64 (the mode's), ``label_counts`` (C,), ``W`` (B,) int64 (the mode's), ``expected``,
    ``variance``, ``z_score``, ``interaction``, ``ratio`` (B, C, C) float64 and with R >= 1 ``p_greater``, ``p_less``,
    ``p_value``, ``null_mean``, ``null_std``, ``z_sim`` (B, C, C) and ``n_permutations``.  Nothing raises on a degenerate input;
    the NaN rules are ``assemble_enrichment``'s per band - ``z_score`` where the variance is not positive (``n < 4`` and an empty
    band among it), ``z_sim`` where the null does not vary, a row of ``interaction`` without counted pairs - and ``ratio`` is NaN
    where its row or its column is empty."""
    mode = _check_mode(mode)
    count = np.asarray(count)
    na = np.asarray(label_counts)
    if count.ndim != 3 or count.shape[1] != count.shape[2] or na.shape != (count.shape[1],):
        raise ValueError(f"count must be (B, C, C) and label_counts (C,), got shapes {count.shape} and {na.shape}")
    if not np.issubdtype(count.dtype, np.integer):
        raise ValueError(f"count must be an integer array, got dtype {count.dtype}")
    B, C = count.shape[0], count.shape[1]
    W = np.asarray(W).astype(np.int64)
    sds = np.asarray(sum_deg_sq).astype(np.int64)
    if W.shape != (B,) or sds.shape != (B,):
        raise ValueError(f"W and sum_deg_sq must be (B,) = {(B,)}, got shapes {W.shape} and {sds.shape}")
    R = check_count("n_permutations", n_permutations)
    count = count.astype(np.int64)
    if mode == "cumulative":
        if sum_deg_sq_cum is None:
            raise ValueError("sum_deg_sq_cum is needed for mode='cumulative'")
        sds = np.asarray(sum_deg_sq_cum).astype(np.int64)
        if sds.shape != (B,):
            raise ValueError(f"sum_deg_sq_cum must be (B,) = {(B,)}, got shape {sds.shape}")
        count, W = np.cumsum(count, axis=0), np.cumsum(W)
    arrs = [count_ge, count_le, sum_d, sumsq_d]
    if R >= 1:
        if any(a is None for a in arrs):
            raise ValueError("count_ge, count_le, sum_d and sumsq_d are needed when n_permutations >= 1")
        arrs = [np.asarray(a) for a in arrs]
        if any(a.shape != (B, C, C) for a in arrs):
            raise ValueError(f"the counts and sums must be (B, C, C) = {(B, C, C)}, got shapes {[a.shape for a in arrs]}")
    bands = [assemble_enrichment(count[b], na, n, W[b], sds[b], *([a[b] for a in arrs] if R >= 1 else [None] * 4), R)
             for b in range(B)]
    out = {"count": count, "label_counts": na.astype(np.int64), "W": W}
    for key in bands[0]:
        if key not in ("count", "label_counts", "n_permutations"):
            out[key] = np.stack([band[key] for band in bands])
    cf = count.astype(np.float64)
    rows, cols, total = cf.sum(axis=2)[:, :, None], cf.sum(axis=1)[:, None, :], cf.sum(axis=(1, 2))[:, None, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        ok = (rows > 0) & (cols > 0)
        out["ratio"] = np.where(ok, cf * total / np.where(ok, rows * cols, 1.0), np.nan)
    if R >= 1:
        out["n_permutations"] = R
    return out


def label_cooccurrence(labels, coords, radii=None, n_bands=10, n_labels=None, n_permutations=999, random_state=0, mode="band",
                       max_candidates=None, return_null=False):
    """At which distances the labels of ``labels`` occur together more often than chance: their join counts in every distance
    band of ``radii``, the exact expectation and variance under random reassignment, the analytic z score, the interaction
    matrix, the co-occurrence ratio and a permutation test on the GPU (module docstring).

    ``labels``: (n_spots,) integers in ``[-1, n_labels)``, numpy or a CUDA tensor - the ``labels`` of ``spatial_niches``, the
    dominant cell type, cluster labels; ``-1`` is shuffled with the rest and never counted.  ``n_labels``: 1 .. 64 (None: the
    largest label + 1).  ``coords``: (n_spots, dim) numpy array or float64 CUDA tensor, 1 <= dim <= 3, rows in the order of
    ``labels``.  ``radii``: 1 to 32 finite values, ``0 < r_1 < ... < r_B``; None: ``grid_radius(coords) * (1 .. n_bands)``, so that
    band 1 is the adjacency of ``build_grid_graph(coords)``.  ``mode``: ``"band"`` (pairs with ``r_{b-1} < d <= r_b``) or
    ``"cumulative"`` (pairs within ``r_b``).  ``n_permutations``: an int >= 0; ``random_state``: as in
    ``neighborhood_enrichment``.  ``max_candidates``: the most candidate pairs a walk may examine (None: the library's default);
    a call that would exceed it raises.  Every argument and shape check raises ``ValueError`` or ``TypeError`` before the GPU is
    touched.

    Returns the dict of ``assemble_cooccurrence`` for ``mode`` plus ``radii`` (B,), ``n_pairs`` (B,) int64 (unordered pairs per
    band, or within ``r_b``), ``n`` and, with ``return_null=True`` and R >= 1, ``null`` (R, B, C, C) int64 - the mode's counts of
    every permutation, a CUDA tensor when ``labels`` was one, else numpy."""
    _check_common(labels, coords, n_labels, max_candidates)
    R = check_count("n_permutations", n_permutations)
    mode = _check_mode(mode)
    return_null = _check_flag("return_null", return_null)
    seed = _permutation_seed(random_state)
    if radii is None:
        nb = _check_n_bands(n_bands)
        from .graph import grid_radius
        r = _check_radii(grid_radius(_coords_host(coords)) * np.arange(1, nb + 1, dtype=np.float64))
    else:
        r = _check_radii(radii)
    s = label_band_counts(labels, coords, r, n_labels=n_labels, seed=seed, n_permutations=R, max_candidates=max_candidates,
                          return_null=return_null and R >= 1)
    tail = "_cum" if mode == "cumulative" else ""
    out = assemble_cooccurrence(s["count"], s["label_counts"], s["n"], s["W"], s["sum_deg_sq"], s["sum_deg_sq_cum"],
                                *(s[key + tail] for key in _NULL_KEYS), n_permutations=R, mode=mode)
    out.update(radii=r, n_pairs=out["W"] // 2, n=s["n"])
    if return_null and R >= 1:
        out["null"] = s["null"].cumsum(1) if mode == "cumulative" else s["null"]
    return out
