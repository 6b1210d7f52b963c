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

Significance without the normality assumption (``spatial_permutation_test``): the rows of ``V`` are reassigned to the spots at
random, ``V_pi[i] = V[pi_r(i)]``, and ``C_r = Z_pi' (A Z_pi)`` is recomputed for r = 0 .. R - 1 (``fdx_spatial_perm_dev``; mean and
m2 do not change).  ``pi_r`` is a keyed bijection of [0, n) evaluated inside the kernels - no index array, no host random stream -
and ``permutation_indices`` (utils/_permutation.py) is its definition, in NumPy integer arithmetic::

    p_greater_ab = (1 + #{r: C_r,ab >= C_ab}) / (R + 1)      p_less likewise with <=      p_value = min(1, 2 min(greater, less))
    z_sim_ab     = (cross_ab - mean_r cross_r,ab) / std_r cross_r,ab                      (std with ddof = 0)

Beside them ``randomization_variance`` gives the exact variance of I over all n! reassignments (Cliff and Ord), which needs
``m4 = sum_i Z_ia^4`` from the same call.
"""
import ctypes

import numpy as np

from .. import _lib
from ._device import check_count, check_values, device_of, resolved_graph, values_on_device
from ._permutation import (_NULL_CALL_BYTES, _permutation_seed, check_permutation_counts, permutation_chunks,
                           permutation_indices, rank_against_null)

__all__ = ["spatial_autocorrelation", "spatial_sums", "assemble", "spatial_permutation_test", "spatial_permutation_sums",
           "permutation_indices", "randomization_variance", "assemble_permutation"]


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


def randomization_variance(n, W, sum_deg_sq, m2, m4):
    """The variance of Moran's I over all n! reassignments of the values to the spots (Cliff and Ord), per column: with
    ``S0 = W``, ``S1 = 2 W``, ``S2 = 4 sum deg^2`` (binary symmetric weights) and ``b2 = n m4 / m2^2``::

        E[I^2] = {n [(n^2 - 3n + 3) S1 - n S2 + 3 S0^2] - b2 [(n^2 - n) S1 - 2n S2 + 6 S0^2]} / [(n - 1)(n - 2)(n - 3) S0^2]
        Var    = E[I^2] - 1 / (n - 1)^2

    NaN for ``n < 4``, ``W == 0`` and where ``m2`` is not positive."""
    n, W, sum_deg_sq = int(n), int(W), int(sum_deg_sq)
    m2 = np.asarray(m2, dtype=np.float64)
    m4 = np.asarray(m4, dtype=np.float64)
    if m2.ndim != 1 or m4.shape != m2.shape:
        raise ValueError(f"m2 and m4 must be (K,), got shapes {m2.shape} and {m4.shape}")
    if n < 4 or W <= 0:
        return np.full(m2.shape, np.nan)
    nf, S0 = float(n), float(W)
    S1, S2 = 2.0 * S0, 4.0 * float(sum_deg_sq)
    with np.errstate(divide="ignore", invalid="ignore"):
        b2 = np.where(m2 > 0, nf * m4 / (m2 * m2), np.nan)
        e2 = (nf * ((nf * nf - 3.0 * nf + 3.0) * S1 - nf * S2 + 3.0 * S0 * S0)
              - b2 * ((nf * nf - nf) * S1 - 2.0 * nf * S2 + 6.0 * S0 * S0)) / ((nf - 1.0) * (nf - 2.0) * (nf - 3.0) * S0 * S0)
    return e2 - 1.0 / ((nf - 1.0) * (nf - 1.0))


def assemble_permutation(n, W, m2, C, count_ge, count_le, sum_d, sumsq_d, n_permutations):
    """The permutation keys of ``spatial_permutation_test`` from the merged counts and sums of R = ``n_permutations`` >= 1
    permutations (pure host arithmetic): ``count_ge`` / ``count_le`` (K, K) count ``C_r >= C`` / ``C_r <= C``, ``sum_d`` /
    ``sumsq_d`` are the sums of ``d = C_r - C`` and ``d^2``.  Every entry that is NaN in ``cross`` is NaN here; ``cross_z_sim`` is
    also NaN where the null standard deviation is 0."""
    R = int(n_permutations)
    if R < 1:
        raise ValueError(f"n_permutations must be at least 1 here, got {n_permutations}")
    cross = assemble(n, W, 0, m2, C)["cross"]
    K = cross.shape[0]
    arrs = [np.asarray(a) for a in (count_ge, count_le, sum_d, sumsq_d)]
    if any(a.shape != (K, K) for a in arrs):
        raise ValueError(f"the counts and sums must be (K, K) = {(K, K)}, got shapes {[a.shape for a in arrs]}")
    ge, le = arrs[0].astype(np.float64), arrs[1].astype(np.float64)
    sd, sq = arrs[2].astype(np.float64), arrs[3].astype(np.float64)
    dead = np.isnan(cross)
    nan = np.float64(np.nan)
    m2 = np.asarray(m2, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        greater, less, p, mean_d, std_d, z_sim = rank_against_null(np, ge, le, sd, sq, R)
        scale = (float(n) / float(W)) / np.sqrt(np.outer(m2, m2)) if W > 0 else np.full((K, K), nan)   # cross = scale * C
        null_mean = np.where(dead, nan, scale * (C + mean_d))
        null_std = np.where(dead, nan, scale * std_d)
        z_sim = np.where(dead | ~(null_std > 0), nan, z_sim)      # the scaled deviation decides: it is what is reported
    out = {"n_permutations": R, "cross_p_greater": np.where(dead, nan, greater), "cross_p_less": np.where(dead, nan, less),
           "cross_p_value": np.where(dead, nan, p), "cross_null_mean": null_mean, "cross_null_std": null_std, "cross_z_sim": z_sim}
    for name in ("p_value", "p_greater", "p_less", "z_sim"):
        out[name] = np.diagonal(out["cross_" + name]).copy()
    return out


def spatial_sums(values, graph, neighbor_mean=False):
    """The device half of ``spatial_autocorrelation``: a dict of ``mean``, ``m2`` (K,), ``C`` (K, K) - numpy - and the integers
    ``n``, ``W``, ``sum_deg_sq``, plus ``neighbor_mean`` (n, K) on request.  Same arguments and checks."""
    n, K = check_values(values)
    with resolved_graph(graph, n) as g:
        import torch
        device_out = _lib.is_cuda_tensor(values)
        device = device_of(values)
        mean, m2, C = np.empty(K), np.empty(K), np.empty((K, K))
        counts = np.zeros(3, dtype=np.int64)
        with torch.cuda.device(device):
            stream = _lib.current_stream(device)
            V, ldv = values_on_device(values, device, stream)
            nm = torch.empty((n, K), dtype=torch.float64, device=device) if neighbor_mean else None
            _lib.check(_lib.load().fdx_spatial_autocorr_dev(
                g.handle, ctypes.c_void_p(V.data_ptr()), int(ldv), int(K), _lib.ptr_f64(mean), _lib.ptr_f64(m2), _lib.ptr_f64(C),
                _lib.ptr_i64(counts), ctypes.c_void_p(nm.data_ptr()) if neighbor_mean else None, stream))
            out = {"mean": mean, "m2": m2, "C": C, "n": int(counts[0]), "W": int(counts[1]), "sum_deg_sq": int(counts[2])}
            if neighbor_mean:
                out["neighbor_mean"] = nm if device_out else _lib.tensor_to_host(nm)
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


def _permutation_calls(values, g, seed, first_perm, n_perm, max_batch, return_null, chunk):
    """The calls of ``spatial_permutation_sums`` on a resolved graph: permutations ``first_perm .. first_perm + n_perm - 1`` in
    calls of at most ``chunk``, counts and sums merged in order."""
    import torch
    n, K = check_values(values)
    device_out = _lib.is_cuda_tensor(values)
    device = device_of(values)
    mean, m2, m4, C = np.empty(K), np.empty(K), np.empty(K), np.empty((K, K))
    counts = np.zeros(3, dtype=np.int64)
    tot_ge, tot_le = np.zeros((K, K), dtype=np.int64), np.zeros((K, K), dtype=np.int64)
    tot_sd, tot_sq = np.zeros((K, K)), np.zeros((K, K))
    ge, le, sd, sq = np.empty_like(tot_ge), np.empty_like(tot_le), np.empty_like(tot_sd), np.empty_like(tot_sq)
    batch = ctypes.c_int32(0)
    batches, null = [], None
    with torch.cuda.device(device):
        stream = _lib.current_stream(device)
        V, ldv = values_on_device(values, device, stream)
        if return_null:
            if device_out:
                null = torch.empty((n_perm, K, K), dtype=torch.float64, device=device)
            else:
                null = np.empty((n_perm, K, K))
                buf = torch.empty((min(chunk, max(n_perm, 1)), K, K), dtype=torch.float64, device=device)
        for done, cnt in permutation_chunks(n_perm, chunk):   # (one call even without permutations: the observed sums and m4)
            if return_null and cnt > 0:
                null_ptr = ctypes.c_void_p((null[done:] if device_out else buf).data_ptr())
            else:
                null_ptr = None
            _lib.check(_lib.load().fdx_spatial_perm_dev(
                g.handle, ctypes.c_void_p(V.data_ptr()), int(ldv), int(K), ctypes.c_uint64(seed), int(first_perm + done), int(cnt),
                int(max_batch), null_ptr, _lib.ptr_f64(mean), _lib.ptr_f64(m2), _lib.ptr_f64(C), _lib.ptr_i64(counts),
                _lib.ptr_f64(m4), _lib.ptr_i64(ge), _lib.ptr_i64(le), _lib.ptr_f64(sd), _lib.ptr_f64(sq), ctypes.byref(batch),
                stream))
            if return_null and cnt > 0 and not device_out:
                null[done:done + cnt] = _lib.tensor_to_host(buf[:cnt])
            tot_ge += ge
            tot_le += le
            tot_sd += sd
            tot_sq += sq
            batches.append(int(batch.value))
    out = {"mean": mean, "m2": m2, "m4": m4, "C": C, "n": int(counts[0]), "W": int(counts[1]), "sum_deg_sq": int(counts[2]),
           "count_ge": tot_ge, "count_le": tot_le, "sum_d": tot_sd, "sumsq_d": tot_sq, "n_permutations": int(n_perm),
           "batch": max(batches)}
    if return_null:
        out["null"] = null
    return out


def spatial_permutation_sums(values, graph, seed=0, first_perm=0, n_permutations=0, max_batch=0, return_null=False):
    """The device half of ``spatial_permutation_test`` (``fdx_spatial_perm_dev``): everything ``spatial_sums`` returns, bit for
    bit, ``m4`` (K,), and over permutations ``first_perm .. first_perm + n_permutations - 1`` of ``seed`` the (K, K) arrays
    ``count_ge``, ``count_le`` (int64), ``sum_d``, ``sumsq_d`` of ``d = C_r - C``; ``batch`` is the number of permutations the
    device ran per launch chain (``max_batch`` caps it, 0: chosen from the scratch budget), and with ``return_null=True`` ``null``
    (n_permutations, K, K) holds every ``C_r`` - a CUDA tensor when ``values`` was one, else numpy.  The counts and the null do
    not depend on ``max_batch`` or on how a range of permutations is split into calls."""
    n, K = check_values(values)
    n_perm, first_perm, max_batch = check_permutation_counts(n_permutations, first_perm, max_batch)
    seed = _permutation_seed(seed)
    with resolved_graph(graph, n) as g:
        chunk = max(1, n_perm)
        if return_null and not _lib.is_cuda_tensor(values):
            chunk = max(1, min(chunk, _NULL_CALL_BYTES // (8 * K * K)))
        return _permutation_calls(values, g, seed, first_perm, n_perm, max_batch, return_null, chunk)


def spatial_permutation_test(values, graph, n_permutations=999, random_state=0, return_null=False):
    """``spatial_autocorrelation`` with a permutation test of Moran's I and of every entry of the co-localisation matrix: the
    rows of ``values`` are reassigned to the spots ``n_permutations`` times on the GPU and the observed statistics ranked against
    that null (module docstring); no normality is assumed, which matters for proportions (zero-inflated, bounded, summing to one).

    ``values`` and ``graph`` as for ``spatial_autocorrelation``, with the same checks before anything touches the GPU;
    ``n_permutations``: an int >= 0 (``ValueError`` otherwise); ``random_state``: an int in [0, 2^64) used as the seed as it
    stands, or None / a ``RandomState`` from which one 63-bit seed is drawn.  The same seed gives the same permutations, on any
    input of the same length.

    Returns every key of ``spatial_autocorrelation`` and ``m4``, ``variance_i_rand``, ``z_score_rand`` (K,): the variance of I
    under randomisation (``randomization_variance``) and the z score it gives.  With ``n_permutations`` R >= 1 also
    ``n_permutations``, the (K, K) arrays ``cross_p_greater = (1 + #{C_r >= C}) / (R + 1)``, ``cross_p_less`` (``<=``),
    ``cross_p_value = min(1, 2 min(greater, less))``, ``cross_null_mean``, ``cross_null_std`` (ddof = 0; both in the units of
    ``cross``), ``cross_z_sim``, their diagonals ``p_value``, ``p_greater``, ``p_less``, ``z_sim`` (K,), and with
    ``return_null=True`` ``cross_null`` (R, K, K), the null in the units of ``cross`` (a CUDA tensor when ``values`` was one, else
    numpy).  Entries that are NaN in ``cross`` are NaN in all of these, ``z_sim`` also where the null does not vary."""
    check_values(values)
    R = check_count("n_permutations", n_permutations)
    s = spatial_permutation_sums(values, graph, seed=_permutation_seed(random_state), n_permutations=R,
                                 return_null=bool(return_null) and R >= 1)
    out = {"mean": s["mean"], "m2": s["m2"], "m4": s["m4"], "n": s["n"], "n_edges": s["W"] // 2}
    out.update(assemble(s["n"], s["W"], s["sum_deg_sq"], s["m2"], s["C"]))
    var = randomization_variance(s["n"], s["W"], s["sum_deg_sq"], s["m2"], s["m4"])
    out["variance_i_rand"] = var
    with np.errstate(divide="ignore", invalid="ignore"):
        out["z_score_rand"] = np.where(var > 0, (out["morans_i"] - out["expected_i"]) / np.sqrt(np.where(var > 0, var, 1.0)), np.nan)
    if R >= 1:
        out.update(assemble_permutation(s["n"], s["W"], s["m2"], s["C"], s["count_ge"], s["count_le"], s["sum_d"], s["sumsq_d"], R))
        if return_null:
            dead = np.isnan(out["cross"])
            with np.errstate(divide="ignore", invalid="ignore"):
                scale = np.where(dead, np.nan, (float(s["n"]) / max(float(s["W"]), 1.0)) / np.sqrt(np.outer(s["m2"], s["m2"])))
            null = s["null"]
            if _lib.is_torch(null):
                import torch
                null = null * torch.as_tensor(scale, device=null.device)
            else:
                null = null * scale
            out["cross_null"] = null
    return out
