"""Local indicators of spatial association of per-spot values over the model's graph, computed on the GPU (additive, not in the
reference): where a spatially clustered column is clustered.

``V`` is (n, K), ``A`` the symmetric binary adjacency without self loops; ``deg_i``, ``W = nnz(A)``, ``mean_a``,
``m2_a = sum_i Z_ia^2`` and ``Z = V - mean`` are exactly as in ``utils/spatial_stats.py``.  Observed, no randomness::

    neighbor_sum_ia = S_ia = sum_{j in N(i)} V_ja            lag_ia = S_ia - deg_i mean_a
    local_i_ia  = (n^2 / W) Z_ia lag_ia / m2_a               local Moran's I; its mean over the spots is the global morans_i_a
                                                             NaN where W == 0, n < 2 or m2_a is not positive
    quadrant_ia = 1 HH (Z > 0, lag > 0)   2 LH (Z < 0, lag > 0)   3 LL (Z < 0, lag < 0)   4 HL (Z > 0, lag < 0)   0 otherwise (int8)
    gi_star_ia  = (S_ia + V_ia - w_i mean_a) / (s_a sqrt((n w_i - w_i^2) / (n - 1)))      Getis-Ord Gi*
                  w_i = deg_i + 1, s_a = sqrt(m2_a / n); NaN where the denominator is not positive

Conditional permutation null: spot i keeps its own value and its ``deg_i`` neighbours are replaced by a random ``deg_i``-subset of
the other n - 1 spots.  The draw is a function, as ``spatial_stats.permutation_indices`` is - no index array, no host random
stream: ``conditional_indices(seed, r, spot, n, count)`` is the first ``count`` values not equal to ``spot`` among
``F_key(0), F_key(1), ..., F_key(count)`` (``count + 1`` evaluations: a bijection meets ``spot`` at most once), where ``F_key`` is
the 8-round unbalanced Feistel bijection of [0, n) with cycle-walking that ``permutation_indices`` defines, under the key::

    key = mix64(key_r + (spot + 1) * 0x9e3779b97f4a7c15)  mod 2^64        key_r = mix64(mix64(seed) + (r + 1) * 0x9e3779b97f4a7c15)

(``key_r`` is ``permutation_indices``' key of ``(seed, r)``); ``0 <= count <= n - 1``.  The NumPy function below is the definition
and the device matches it bit for bit (``fdx_conditional_indices_dev``).  Then::

    S_ia,r = sum_t V[c_t][a]   over c = conditional_indices(seed, r, i, n, deg_i), added in slot order

Everything is ranked on the raw neighbour sum S, not on Z: with ``deg_i`` fixed ``S_r >= S`` is the same event as
``lag_r >= lag``, zeros add exactly (the many exact ties of zero-inflated data stay exact), and the ranking does not depend on the
device's rounding of the mean.  Per (i, a) the device keeps over the permutations ``first_perm .. first_perm + n_perm - 1``
(``fdx_local_stats_dev``, csrc/local_stats_kernels.cpp)::

    count_ge = #{S_r >= S}      count_le = #{S_r <= S}      sum_d, sumsq_d = sum_r d, sum_r d^2 with d = S_r - S

and ``assemble_local`` forms on the host, with R the number of permutations::

    p_greater = (1 + count_ge) / (R + 1)      the hot-spot side; it serves Gi* as well, whose self term is fixed
    p_less    = (1 + count_le) / (R + 1)
    p_value   = min(1, 2 min(p_greater, p_less))
    z_sim     = -mean_d / sqrt(var_d)         mean_d = sum_d / R, var_d = max(sumsq_d / R - mean_d^2, 0)   (ddof = 0)
    local_i_p_greater = p_greater where Z > 0, p_less where Z < 0, 1 where Z == 0      (one-sided p of local_i)

All of these are NaN where ``deg_i == 0``; ``z_sim`` is also NaN where the null does not vary (a spot adjacent to every other
spot draws everybody: ``count_ge = count_le = R``).
"""
import ctypes

import numpy as np

from .. import _lib
from ._device import check_values, device_of, resolved_graph, values_on_device
from ._permutation import (_GOLDEN, _keyed_bijection, _mix64_int, _permutation_seed, check_permutation_counts, permutation_key,
                           rank_against_null)

__all__ = ["local_spatial_statistics", "local_sums", "assemble_local", "conditional_indices"]

_PERM_KEYS = ("count_ge", "count_le", "sum_d", "sumsq_d")


def conditional_indices(seed, r, spot, n, count):
    """The ``count`` spots that conditional permutation ``r`` of ``seed`` draws for ``spot`` among ``n``, an int64 array in slot
    order (module docstring): distinct, in [0, n), never ``spot``.  ``ValueError`` unless ``seed >= 0``, ``r >= 0``,
    ``0 <= spot < n < 2^31 - 128`` and ``0 <= count <= n - 1``."""
    seed, r, spot, n, count = int(seed), int(r), int(spot), int(n), int(count)
    if seed < 0 or r < 0:
        raise ValueError(f"seed and r must not be negative, got seed = {seed}, r = {r}")
    if not 0 <= spot < n or n >= (1 << 31) - 128:
        raise ValueError(f"spot must be in [0, n) and n below 2^31 - 128, got spot = {spot}, n = {n}")
    if not 0 <= count <= n - 1:
        raise ValueError(f"count must be in [0, n - 1] = [0, {n - 1}], got {count}")
    key = _mix64_int(permutation_key(seed, r) + (spot + 1) * _GOLDEN)
    c = _keyed_bijection(key, np.arange(count + 1, dtype=np.uint64), n)
    return c[c != spot][:count]


def _assemble(xp, V, S, deg, mean, m2, n, W, perm):
    """The assembly in the array namespace ``xp`` (numpy, or torch on the device of the arrays): the same expressions in the same
    order for both.  Divisors are 0-d arrays of the namespace, never Python scalars: torch divides by a host scalar through its
    reciprocal, which is not the quotient NumPy forms.  The ranking is ``_permutation.rank_against_null``."""
    nan = float("nan")
    nf, Wf = float(n), float(W)

    def c(v):
        return xp.zeros_like(mean[0]) + v

    degf = deg.reshape(-1, 1)                                      # (n, 1) float64
    Z = V - mean
    lag = S - degf * mean
    alive = (m2 > 0) & (W > 0 and n >= 2)                          # (K,)
    m2_safe = xp.where(alive, m2, m2 * 0.0 + 1.0)
    local_i = xp.where(alive, ((nf * nf / Wf) if W > 0 else nan) * Z * lag / m2_safe, nan)
    quadrant = ((Z > 0) & (lag > 0)) * 1 + ((Z < 0) & (lag > 0)) * 2 + ((Z < 0) & (lag < 0)) * 3 + ((Z > 0) & (lag < 0)) * 4
    w = degf + 1.0
    if n >= 2:
        den = xp.sqrt(xp.where(m2 > 0, m2, m2 * 0.0) / c(nf)) * xp.sqrt((nf * w - w * w) / c(nf - 1.0))
        ok = den > 0
        gi = xp.where(ok, (S + V - w * mean) / xp.where(ok, den, den * 0.0 + 1.0), nan)
    else:
        gi = V * 0.0 + nan
    out = {"local_i": local_i, "gi_star": gi, "quadrant": quadrant}
    if perm is None:
        return out
    ge, le, sd, sq, R = perm
    isolated = degf == 0
    greater, less, p, _, _, z_sim = rank_against_null(xp, ge, le, sd, sq, R)
    own = xp.where(Z > 0, greater, xp.where(Z < 0, less, greater * 0.0 + 1.0))
    z_sim = xp.where(xp.isfinite(sq), z_sim, nan)                  # an overflowed sum of squares has no deviation to divide by
    out.update({"n_permutations": int(R)})
    out.update({k: xp.where(isolated, nan, v) for k, v in (("p_greater", greater), ("p_less", less), ("p_value", p),
                                                           ("z_sim", z_sim), ("local_i_p_greater", own))})
    return out


def assemble_local(values, neighbor_sum, degree, mean, m2, n, W, count_ge=None, count_le=None, sum_d=None, sumsq_d=None,
                   n_permutations=0):
    """``local_i``, ``gi_star`` (n, K) and ``quadrant`` (n, K) int8 from the sums of ``local_sums``, and with
    ``n_permutations`` R >= 1 and the four (n, K) counts and sums also ``n_permutations``, ``p_greater``, ``p_less``, ``p_value``,
    ``z_sim`` and ``local_i_p_greater`` (module docstring).  Pure NumPy; nothing raises on a zero division, the entry is NaN."""
    V = np.asarray(values, dtype=np.float64)
    S = np.asarray(neighbor_sum, dtype=np.float64)
    deg = np.asarray(degree)
    mean, m2 = np.asarray(mean, dtype=np.float64), np.asarray(m2, dtype=np.float64)
    n, W, R = int(n), int(W), int(n_permutations)
    if V.ndim != 2 or S.shape != V.shape or deg.shape != V.shape[:1] or mean.shape != V.shape[1:] or m2.shape != mean.shape:
        raise ValueError(f"values and neighbor_sum must be (n, K), degree (n,), mean and m2 (K,), got shapes {V.shape}, {S.shape}, "
                         f"{deg.shape}, {mean.shape}, {m2.shape}")
    if n != V.shape[0]:
        raise ValueError(f"n = {n} but values has {V.shape[0]} rows")
    if R < 0:
        raise ValueError(f"n_permutations must not be negative, got {n_permutations}")
    perm = None
    if R >= 1:
        arrs = [None if a is None else np.asarray(a) for a in (count_ge, count_le, sum_d, sumsq_d)]
        if any(a is None or a.shape != V.shape for a in arrs):
            raise ValueError(f"with n_permutations >= 1 the counts and sums must be (n, K) = {V.shape}")
        perm = tuple(a.astype(np.float64) for a in arrs) + (R,)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = _assemble(np, V, S, deg.astype(np.float64), mean, m2, n, W, perm)
    out["quadrant"] = out["quadrant"].astype(np.int8)
    return out


def _assemble_torch(V, s):
    """``assemble_local`` on the device of ``V`` for the tensors of ``_local_calls``."""
    import torch
    mean = torch.as_tensor(s["mean"], device=V.device)
    m2 = torch.as_tensor(s["m2"], device=V.device)
    R = s["n_permutations"]
    perm = tuple(s[k].to(torch.float64) for k in _PERM_KEYS) + (R,) if R >= 1 else None
    out = _assemble(torch, V, s["neighbor_sum"], s["degree"].to(torch.float64), mean, m2, s["n"], s["W"], perm)
    out["quadrant"] = out["quadrant"].to(torch.int8)
    return out


def _local_calls(values, g, seed, first_perm, n_perm):
    """``fdx_local_stats_dev`` on a resolved graph: (the float64 device copy of ``values``, a dict of device tensors and host
    sums)."""
    import torch
    n, K = check_values(values)
    device = device_of(values)
    mean, m2 = np.empty(K), np.empty(K)
    counts = np.zeros(3, dtype=np.int64)
    with torch.cuda.device(device):
        stream = _lib.current_stream(device)
        V, ldv = values_on_device(values, device, stream)
        S = torch.empty((n, K), dtype=torch.float64, device=device)
        deg = torch.empty((n,), dtype=torch.int32, device=device)
        perm = {}
        if n_perm > 0:
            perm = {"count_ge": torch.empty((n, K), dtype=torch.int32, device=device),
                    "count_le": torch.empty((n, K), dtype=torch.int32, device=device),
                    "sum_d": torch.empty((n, K), dtype=torch.float64, device=device),
                    "sumsq_d": torch.empty((n, K), dtype=torch.float64, device=device)}
        ptrs = [ctypes.c_void_p(perm[k].data_ptr()) if perm else None for k in _PERM_KEYS]
        _lib.check(_lib.load().fdx_local_stats_dev(
            g.handle, ctypes.c_void_p(V.data_ptr()), int(ldv), int(K), ctypes.c_uint64(seed), int(first_perm), int(n_perm),
            ctypes.c_void_p(S.data_ptr()), ctypes.c_void_p(deg.data_ptr()), *ptrs, _lib.ptr_f64(mean), _lib.ptr_f64(m2),
            _lib.ptr_i64(counts), stream))
    out = {"mean": mean, "m2": m2, "n": int(counts[0]), "W": int(counts[1]), "sum_deg_sq": int(counts[2]), "neighbor_sum": S,
           "degree": deg, "n_permutations": int(n_perm)}
    out.update(perm)
    return V, out


def _device_sums(values, graph, seed, first_perm, n_permutations):
    n, _ = check_values(values)
    n_perm, first_perm, _ = check_permutation_counts(n_permutations, first_perm)
    if n_perm >= 1 << 31:
        raise ValueError(f"n_permutations must be below 2^31, got {n_perm}")
    seed = _permutation_seed(seed)
    with resolved_graph(graph, n) as g:
        return _local_calls(values, g, seed, first_perm, n_perm)


def local_sums(values, graph, seed=0, first_perm=0, n_permutations=0):
    """The device half of ``local_spatial_statistics`` (``fdx_local_stats_dev``): a dict of ``mean``, ``m2`` (K,) - numpy - and the
    integers ``n``, ``W``, ``sum_deg_sq``, bit for bit what ``spatial_stats.spatial_sums`` returns; ``neighbor_sum`` (n, K)
    float64 and ``degree`` (n,) int32 in the caller's spot order; ``n_permutations``; and with ``n_permutations`` >= 1, over the
    conditional permutations ``first_perm .. first_perm + n_permutations - 1`` of ``seed``, the (n, K) arrays ``count_ge``,
    ``count_le`` (int32), ``sum_d``, ``sumsq_d`` (float64).  The arrays are CUDA tensors when ``values`` was one, else numpy.
    Same arguments and checks as ``local_spatial_statistics``.  The counts do not depend on how a range of permutations is split
    into calls; the sums of split calls add up to the rounding of their additions."""
    device_out = _lib.is_cuda_tensor(values)
    _, out = _device_sums(values, graph, seed, first_perm, n_permutations)
    if not device_out:
        for k in ("neighbor_sum", "degree") + _PERM_KEYS:
            if k in out:
                out[k] = _lib.tensor_to_host(out[k])
    return out


def local_spatial_statistics(values, graph, n_permutations=0, random_state=0):
    """Local Moran's I with its quadrant and the Getis-Ord Gi* score per spot and column of ``values``, and with
    ``n_permutations`` R >= 1 their conditional-permutation p values (module docstring).

    ``values`` and ``graph`` as for ``spatial_stats.spatial_autocorrelation``: a 2-D (n_spots, K) numpy array or CUDA torch
    tensor, float32 or float64; a fitted ``FlashDeconv``, a ``_lib.Graph`` or a scipy sparse adjacency (square, symmetric, no
    diagonal).  ``n_permutations``: an int in [0, 2^31); ``random_state``: an int in [0, 2^64) used as the seed as it stands, or
    None / a ``RandomState`` from which one seed is drawn.  Everything is checked before anything touches the GPU
    (``ValueError`` / ``TypeError``).

    Returns a dict: ``local_i``, ``gi_star``, ``neighbor_sum`` (n, K) float64, ``quadrant`` (n, K) int8, ``degree`` (n,) int32,
    ``mean``, ``m2`` (K,) numpy, ``n``, ``n_edges``; with R >= 1 also ``n_permutations`` and the (n, K) arrays ``p_greater``,
    ``p_less``, ``p_value``, ``z_sim``, ``local_i_p_greater``.  The per-spot arrays are CUDA tensors when ``values`` was one (the
    assembly then runs in torch on the device), else numpy."""
    device_out = _lib.is_cuda_tensor(values)
    V, s = _device_sums(values, graph, random_state, 0, n_permutations)
    if device_out:
        out = _assemble_torch(V, s)
        out["neighbor_sum"], out["degree"] = s["neighbor_sum"], s["degree"]
    else:
        host = {k: _lib.tensor_to_host(s[k]) for k in ("neighbor_sum", "degree") + _PERM_KEYS if k in s}
        host_values = values.detach().numpy() if _lib.is_torch(values) else values
        out = assemble_local(host_values, host["neighbor_sum"], host["degree"], s["mean"], s["m2"], s["n"], s["W"],
                             *(host.get(k) for k in _PERM_KEYS), n_permutations=s["n_permutations"])
        out["neighbor_sum"], out["degree"] = host["neighbor_sum"], host["degree"]
    if s["n_permutations"] < 1:
        out.pop("n_permutations", None)
    out.update({"mean": s["mean"], "m2": s["m2"], "n": s["n"], "n_edges": s["W"] // 2})
    return out
