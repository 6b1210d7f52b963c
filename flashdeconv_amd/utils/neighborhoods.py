"""Neighbourhood enrichment of spot labels: which niches, dominant cell types or clusters border each other more often than chance
and which avoid each other - join counts over the model's graph with their exact moments and a permutation null, counted on the
GPU (additive, not in the reference).  The ``nhood_enrichment`` / ``interaction_matrix`` pair of the usual spatial toolkits.

**Definitions.**  ``A`` is the graph's symmetric binary adjacency with no self loops; ``l_i`` in ``{-1, 0 .. C - 1}`` is the label of
spot i in the caller's spot order (the convention of ``utils.group_genes``: ``-1`` means left out); ``n_a = #{i : l_i = a}``;
``W = sum_i deg_i`` is the number of directed edges and::

    N_ab = #{(i, j) : A_ij = 1, l_i = a, l_j = b}        over ordered pairs, a, b in [0, C)

so ``N`` is symmetric and ``N_aa`` is twice the number of undirected a-a edges.  Under permutation ``r`` of ``seed`` the labels are
``l^r_i = l[pi_r(i)]`` with ``pi_r = utils.spatial_stats.permutation_indices(seed, r, n)`` - the convention of
``V_pi[i] = V[pi_r(i)]`` in ``fdx_spatial_perm_dev`` - and ``N^r`` is the count matrix of ``l^r``.  Spots labelled ``-1`` take part
in the shuffle like any other label and are never counted: ``-1`` is one more class that is not reported, which keeps one bijection
of ``[0, n)`` and makes the moments below exact with ``n`` equal to all spots.

**Exact moments** over all ``n!`` reassignments (Cliff and Ord, k-colour join counts, binary weights), with ``x^(k)`` the falling
factorial, ``S0 = W``, ``S1 = 2 W`` and ``S2 = 4 sum_i deg_i^2``::

    E[N_aa]   = S0 n_a^(2) / n^(2)
    Var[N_aa] = S1 n_a^(2)/n^(2) + (S2 - 2 S1) n_a^(3)/n^(3) + (S0^2 + S1 - S2) n_a^(4)/n^(4) - E^2
    E[N_ab]   = S0 n_a n_b / n^(2)                                                   (a != b)
    Var[N_ab] = 1/4 [ 2 S1 n_a n_b/n^(2) + (S2 - 2 S1) n_a n_b (n_a + n_b - 2)/n^(3)
                      + 4 (S0^2 + S1 - S2) n_a^(2) n_b^(2)/n^(4) ] - E^2

(``join_count_moments``; NaN for ``n < 4`` or ``W = 0``.)

**Device half** (``label_pair_counts``: ``fdx_label_pair_counts_dev``, csrc/label_pair_kernels.cpp, on torch's current stream): the
observed ``N``, ``n_a``, ``n``, ``W``, ``sum deg^2`` and over permutations ``first_perm .. first_perm + R - 1`` the counts
``#{r : N^r >= N}``, ``#{r : N^r <= N}`` (int64) and the float64 sums of ``d = N^r - N`` and ``d^2`` in permutation order.  Every
count is an exact integer and does not depend on the batching or on how a range of permutations is split into calls.

**Statistics** (``assemble_enrichment``, pure NumPy)::

    z_score     = (N - E) / sqrt(Var)                          NaN where Var is not positive
    interaction = N_ab / sum_b N_ab                            the share of label a's neighbours that carry label b; NaN for rows without edges
    p_greater   = (1 + #{r : N^r >= N}) / (R + 1)              p_less likewise with <=        p_value = min(1, 2 min(p_greater, p_less))
    null_mean   = N + mean_r d      null_std = std_r d (ddof = 0)      z_sim = (N - null_mean) / null_std      NaN where null_std = 0

**Distance bands.**  The same counts, moments and null in every distance band of a set of radii, with no graph built, are
``utils.cooccurrence.label_cooccurrence``.

**Out of scope.**  Per-spot neighbour label counts (``spatial_sums`` on a one-hot matrix gives them); sharded graphs (refused);
conditional shuffles that keep the ``-1`` spots fixed.
"""
import ctypes

import numpy as np

from .. import _lib
from ._device import check_count, device_of, resolved_graph
from ._permutation import _permutation_seed, check_permutation_counts, rank_against_null

__all__ = ["neighborhood_enrichment", "label_pair_counts", "join_count_moments", "assemble_enrichment", "MAX_LABELS"]

MAX_LABELS = 64


def _falling(x, k):
    """``x (x - 1) .. (x - k + 1)`` in float64, elementwise."""
    x = np.asarray(x, dtype=np.float64)
    out = np.ones_like(x)
    for j in range(k):
        out = out * (x - float(j))
    return out


def join_count_moments(n, W, sum_deg_sq, label_counts):
    """``(expected, variance)`` of the join counts ``N_ab`` over all ``n!`` reassignments of the labels to the spots (module
    docstring), (C, C) float64 each, from ``n`` spots, ``W = sum deg``, ``sum_deg_sq = sum deg^2`` and ``label_counts`` (C,) - the
    spots labelled ``-1`` count in ``n`` and in no ``n_a``.  NaN for ``n < 4`` or ``W = 0``.  A variance within rounding of zero
    (64 ulp of the terms it is the difference of) is reported as 0: a count that cannot vary - every spot in one label, a label of
    one spot with itself - has no z score."""
    n, W, sum_deg_sq = int(n), int(W), int(sum_deg_sq)
    na = np.asarray(label_counts)
    if na.ndim != 1 or na.shape[0] < 1 or not np.issubdtype(na.dtype, np.integer):
        raise ValueError(f"label_counts must be a non-empty 1-D integer array, got shape {na.shape} and dtype {na.dtype}")
    if np.any(na < 0) or int(na.sum()) > n:
        raise ValueError(f"label_counts must be non-negative and sum to at most n = {n}, got {na.tolist()}")
    C = na.shape[0]
    if n < 4 or W <= 0:
        return np.full((C, C), np.nan), np.full((C, C), np.nan)
    S0 = float(W)
    S1, S2 = 2.0 * S0, 4.0 * float(sum_deg_sq)
    nf = float(n)
    d2, d3, d4 = (float(_falling(nf, k)) for k in (2, 3, 4))
    a1 = na.astype(np.float64)
    a2, a3, a4 = _falling(a1, 2), _falling(a1, 3), _falling(a1, 4)
    # diagonal
    e_d = S0 * a2 / d2
    t_d = (S1 * a2 / d2, (S2 - 2.0 * S1) * a3 / d3, (S0 * S0 + S1 - S2) * a4 / d4)
    # off-diagonal
    nab = np.outer(a1, a1)
    e_o = S0 * nab / d2
    t_o = (0.25 * 2.0 * S1 * nab / d2, 0.25 * (S2 - 2.0 * S1) * nab * (a1[:, None] + a1[None, :] - 2.0) / d3,
           0.25 * 4.0 * (S0 * S0 + S1 - S2) * np.outer(a2, a2) / d4)
    expected = e_o.copy()
    expected[np.diag_indices(C)] = e_d
    terms = [t.copy() for t in t_o]
    for t, td in zip(terms, t_d):
        t[np.diag_indices(C)] = td
    variance = terms[0] + terms[1] + terms[2] - expected * expected
    scale = np.abs(terms[0]) + np.abs(terms[1]) + np.abs(terms[2]) + expected * expected
    variance = np.where(np.abs(variance) <= 64.0 * np.finfo(np.float64).eps * scale, 0.0, variance)
    return expected, variance


def assemble_enrichment(count, label_counts, n, W, sum_deg_sq, count_ge=None, count_le=None, sum_d=None, sumsq_d=None,
                        n_permutations=0):
    """The statistics of the module docstring from the sums of ``label_pair_counts`` (pure host arithmetic): a dict of ``count``
    (C, C) and ``label_counts`` (C,) int64, ``expected``, ``variance``, ``z_score`` and ``interaction`` (C, C) float64, and with
    ``n_permutations`` R >= 1 - then ``count_ge``, ``count_le``, ``sum_d``, ``sumsq_d`` (C, C) are needed - also ``p_greater``,
    ``p_less``, ``p_value``, ``null_mean``, ``null_std``, ``z_sim`` and ``n_permutations``.  Nothing raises on a degenerate input:
    ``z_score`` is NaN where the variance is not positive, ``z_sim`` where the null does not vary, a row of ``interaction`` where
    the label has no counted neighbour."""
    count = np.asarray(count)
    na = np.asarray(label_counts)
    if count.ndim != 2 or count.shape[0] != count.shape[1] or na.shape != (count.shape[0],):
        raise ValueError(f"count must be (C, C) and label_counts (C,), got shapes {count.shape} and {na.shape}")
    if not np.issubdtype(count.dtype, np.integer):
        raise ValueError(f"count must be an integer array, got dtype {count.dtype}")
    R = check_count("n_permutations", n_permutations)
    C = count.shape[0]
    count = count.astype(np.int64)
    expected, variance = join_count_moments(n, W, sum_deg_sq, na)
    cf = count.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ok = variance > 0
        z = np.where(ok, (cf - expected) / np.sqrt(np.where(ok, variance, 1.0)), np.nan)
        rows = count.sum(axis=1).astype(np.float64)[:, None] + np.zeros((1, C))
        interaction = np.where(rows > 0, cf / np.where(rows > 0, rows, 1.0), np.nan)
    out = {"count": count, "label_counts": na.astype(np.int64), "expected": expected, "variance": variance, "z_score": z,
           "interaction": interaction}
    if R >= 1:
        arrs = [count_ge, count_le, sum_d, sumsq_d]
        if any(a is None for a in arrs):
            raise ValueError("count_ge, count_le, sum_d and sumsq_d are needed when n_permutations >= 1")
        arrs = [np.asarray(a) for a in arrs]
        if any(a.shape != (C, C) for a in arrs):
            raise ValueError(f"the counts and sums must be (C, C) = {(C, C)}, got shapes {[a.shape for a in arrs]}")
        ge, le, sd, sq = (a.astype(np.float64) for a in arrs)
        with np.errstate(divide="ignore", invalid="ignore"):
            greater, less, p, mean_d, null_std, z_sim = rank_against_null(np, ge, le, sd, sq, R)
        out.update({"p_greater": greater, "p_less": less, "p_value": p, "null_mean": cf + mean_d, "null_std": null_std,
                    "z_sim": z_sim, "n_permutations": R})
    return out


def _check_n_labels(n_labels):
    if isinstance(n_labels, (bool, np.bool_)) or not isinstance(n_labels, (int, np.integer)) or not 1 <= n_labels <= MAX_LABELS:
        raise ValueError(f"n_labels must be an int from 1 to {MAX_LABELS}, got {n_labels!r}")
    return int(n_labels)


def _check_flag(name, v):
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError(f"{name} must be True or False, got {v!r}")
    return bool(v)


def check_labels(labels, n_labels=None):
    """``(n, labels, C or None)``: what can be checked of the labels without touching the GPU.  Host labels come back as a
    contiguous int32 array, checked to lie in ``[-1, C)`` with ``C = n_labels`` (None: the largest label + 1, at least 1); a CUDA
    tensor comes back as it is, its length and dtype checked (its range is checked on the device).  ``TypeError`` for what is no
    array of integers, ``ValueError`` for the rest."""
    C = None if n_labels is None else _check_n_labels(n_labels)
    if _lib.is_torch(labels):
        shape, dtype = tuple(labels.shape), str(labels.dtype).replace("torch.", "")
        integer = dtype in ("int8", "int16", "int32", "int64", "uint8")
    else:
        if not hasattr(labels, "dtype"):
            labels = np.asarray(labels)
        shape, dtype = tuple(labels.shape), str(labels.dtype)
        integer = np.issubdtype(labels.dtype, np.integer)
    if not integer:
        raise TypeError(f"labels must be integers, got dtype {dtype}")
    if len(shape) != 1 or shape[0] < 1:
        raise ValueError(f"labels must be a non-empty 1-D (n_spots,) array, got shape {shape}")
    if _lib.is_cuda_tensor(labels):
        return shape[0], labels, C
    lab = labels.detach().numpy() if _lib.is_torch(labels) else np.asarray(labels)
    lo, hi = int(lab.min()), int(lab.max())
    if C is None:
        if hi >= MAX_LABELS:
            raise ValueError(f"at most {MAX_LABELS} labels, got labels up to {hi}")
        C = max(hi + 1, 1)
    if lo < -1 or hi >= C:
        raise ValueError(f"labels must lie in [-1, {C}), got labels from {lo} to {hi}")
    return shape[0], np.ascontiguousarray(lab, dtype=np.int32), C


def _labels_on_device(labels, C, device):
    """(int32 device tensor, C): host labels uploaded, CUDA labels converted where they lie - values outside int32 are clamped
    to -2 / 64 first, so they stay outside every valid range and the device's check reports them."""
    import torch
    if not _lib.is_cuda_tensor(labels):
        return torch.as_tensor(labels).to(device), C
    lab = labels.detach().to(device)
    if C is None:
        hi = int(lab.max().item())
        if hi >= MAX_LABELS:
            raise ValueError(f"at most {MAX_LABELS} labels, got labels up to {hi}")
        C = max(hi + 1, 1)
    if lab.dtype == torch.uint8:                      # (every value fits; a negative bound cannot clamp an unsigned dtype)
        lab = lab.to(torch.int32)
    elif lab.dtype != torch.int32:
        lab = lab.clamp(-2, MAX_LABELS).to(torch.int32)
    return lab.contiguous(), C


def label_pair_counts(labels, graph, n_labels=None, seed=0, first_perm=0, n_permutations=0, max_batch=0, return_null=False):
    """The device half of ``neighborhood_enrichment`` (``fdx_label_pair_counts_dev``): a dict of ``count`` (C, C) and
    ``label_counts`` (C,) int64, the integers ``n``, ``W``, ``sum_deg_sq``, and over permutations
    ``first_perm .. first_perm + n_permutations - 1`` of ``seed`` the (C, C) arrays ``count_ge``, ``count_le`` (int64), ``sum_d``,
    ``sumsq_d`` (float64) of ``d = N^r - N``; ``batch`` is the number of permutations the device ran per launch chain
    (``max_batch`` caps it, 0: chosen from the scratch budget), and with ``return_null=True`` ``null`` (n_permutations, C, C)
    int64 holds every ``N^r`` - a CUDA tensor when ``labels`` was one, else numpy.

    ``labels``: (n,) integers in ``[-1, n_labels)``, numpy or a CUDA tensor, any integer dtype (converted to int32; floats are a
    ``TypeError``); ``n_labels``: 1 .. 64 (None: the largest label + 1).  ``graph``: a fitted ``FlashDeconv``, a ``_lib.Graph`` or
    a scipy sparse adjacency, as ``spatial_autocorrelation`` takes it.  Every count is exact and depends neither on ``max_batch``
    nor on how a range of permutations is split into calls.  Everything checkable is checked before the GPU is touched."""
    n, labels, C = check_labels(labels, n_labels)
    n_perm, first_perm, max_batch = check_permutation_counts(n_permutations, first_perm, max_batch)
    return_null = _check_flag("return_null", return_null)
    seed = _permutation_seed(seed)
    with resolved_graph(graph, n) as g:
        import torch
        device_out = _lib.is_cuda_tensor(labels)
        device = device_of(labels)
        with torch.cuda.device(device):
            stream = _lib.current_stream(device)
            lab, C = _labels_on_device(labels, C, device)
            CC = (C, C)
            label_counts, pair, counts = np.zeros(C, dtype=np.int64), np.zeros(CC, dtype=np.int64), np.zeros(3, dtype=np.int64)
            ge, le, sd, sq = np.zeros(CC, dtype=np.int64), np.zeros(CC, dtype=np.int64), np.zeros(CC), np.zeros(CC)
            batch = ctypes.c_int32(0)
            null = torch.empty((n_perm, C, C), dtype=torch.int64, device=device) if return_null else None
            try:
                _lib.check(_lib.load().fdx_label_pair_counts_dev(
                    g.handle, ctypes.c_void_p(lab.data_ptr()), int(C), ctypes.c_uint64(seed), int(first_perm), int(n_perm),
                    int(max_batch), ctypes.c_void_p(null.data_ptr()) if return_null and n_perm > 0 else None,
                    _lib.ptr_i64(label_counts), _lib.ptr_i64(pair), _lib.ptr_i64(counts), _lib.ptr_i64(ge), _lib.ptr_i64(le),
                    _lib.ptr_f64(sd), _lib.ptr_f64(sq), ctypes.byref(batch), stream))
            except _lib.FdxError as e:
                if "outside [-1, C)" in str(e):
                    raise ValueError(f"labels must lie in [-1, {C}): the device found one that does not") from e
                raise
            out = {"count": pair, "label_counts": label_counts, "n": int(counts[0]), "W": int(counts[1]),
                   "sum_deg_sq": int(counts[2]), "count_ge": ge, "count_le": le, "sum_d": sd, "sumsq_d": sq,
                   "n_permutations": int(n_perm), "batch": int(batch.value)}
            if return_null:
                out["null"] = null if device_out else _lib.tensor_to_host(null)
    return out


def neighborhood_enrichment(labels, graph, n_labels=None, n_permutations=999, random_state=0, return_null=False):
    """Which labels border each other more often than chance, and which avoid each other: the join counts ``N_ab`` of ``labels``
    over ``graph``, their exact expectation and variance under random reassignment, the analytic z score, the row-normalised
    interaction matrix and a permutation test on the GPU (module docstring).

    ``labels``: (n_spots,) integers in ``[-1, n_labels)``, numpy or a CUDA tensor - the ``labels`` of ``spatial_niches``, the
    dominant cell type, cluster labels; ``-1`` is shuffled with the rest and never counted.  ``n_labels``: 1 .. 64 (None: the
    largest label + 1).  ``graph``: a fitted ``FlashDeconv``, a ``_lib.Graph`` or a scipy sparse adjacency.  ``n_permutations``:
    an int >= 0; ``random_state``: an int in [0, 2^64) used as the seed as it stands, or None / a ``RandomState`` from which one
    63-bit seed is drawn - as in ``spatial_permutation_test``.  Every argument and shape check raises ``ValueError`` or
    ``TypeError`` before the GPU is touched.

    Returns the dict of ``assemble_enrichment`` - ``count``, ``label_counts``, ``expected``, ``variance``, ``z_score``,
    ``interaction`` and, with ``n_permutations`` R >= 1, ``p_greater``, ``p_less``, ``p_value``, ``null_mean``, ``null_std``,
    ``z_sim``, ``n_permutations`` - plus ``n``, ``n_edges`` (undirected: ``W = 2 n_edges``) and, with ``return_null=True`` and
    R >= 1, ``null`` (R, C, C) int64 (a CUDA tensor when ``labels`` was one, else numpy)."""
    check_labels(labels, n_labels)
    R = check_count("n_permutations", n_permutations)
    return_null = _check_flag("return_null", return_null)
    s = label_pair_counts(labels, graph, n_labels=n_labels, seed=_permutation_seed(random_state), n_permutations=R,
                          return_null=return_null and R >= 1)
    out = assemble_enrichment(s["count"], s["label_counts"], s["n"], s["W"], s["sum_deg_sq"], s["count_ge"], s["count_le"],
                              s["sum_d"], s["sumsq_d"], R)
    out.update(n=s["n"], n_edges=s["W"] // 2)
    if return_null and R >= 1:
        out["null"] = s["null"]
    return out
