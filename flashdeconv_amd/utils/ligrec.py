"""Ligand-receptor test between spot groups: between which niches, dominant cell types or clusters a ligand-receptor pair acts - for
every pair and every ordered pair of groups (a, b) the mean of the ligand in a and of the receptor in b, ranked against the same
statistic under random reassignment of the group labels to the spots, summed on the GPU (additive, not in the reference).  The
``ligrec`` test of CellPhoneDB and of the usual spatial toolkits.  No graph is involved: with ``utils.neighborhoods`` ("which niches
touch") this answers "which niches talk".

**Inputs.**  ``Y`` (n, G) is that of ``utils.group_genes``: dense float32 or float64 (integers through the upload rules of
``_lib.upload_matrix``), host or CUDA, any row stride, or CSR from scipy or a CUDA ``torch.sparse_csr`` tensor, kept sparse.
``labels`` is (n,) integers in ``[-1, C)`` with ``1 <= C <= 64``, checked by ``neighborhoods.check_labels``: ``-1`` is shuffled with
the rest and never counted, so one bijection of ``[0, n)`` is used and every group size ``n_c`` is the same under every permutation.
``pairs`` is (P, 2) integer columns of ``Y``, ligand then receptor (``gene_pairs.check_request``): the same gene may stand on both
sides and a pair may occur twice.  ``genes`` is the sorted distinct columns in ``pairs``, ``S = len(genes) <= MAX_GENES`` = 4096, and
``P * C^2 <= MAX_STATISTICS`` = 2^22; a request above either is a ``ValueError`` before the GPU is touched.

**Sums** (``label_gene_sums``: ``fdx_label_gene_sums_dev`` / ``_csr_dev``, csrc/label_gene_kernels.cpp, on torch's current stream), all
float64 on the value converted from storage.  Under permutation ``r`` of ``seed`` the labels are ``l^r_i = l[pi_r(i)]`` with
``pi_r = permutation_indices(seed, r, n)`` and::

    u^r[c, s] = sum_{i : l^r_i = c} y[i, genes[s]]

The observed ``u`` is the same sum with the identity in place of ``pi_r``, through the same kernel, so it shares the summation
order.  For the observed labelling ``nnz[c, s] = #{i in c : y != 0}`` (int64) and ``label_counts[c] = n_c``.

**Statistic**::

    m^r[c, s]    = u^r[c, s] / n_c
    T^r[p, a, b] = (m^r[a, lig_p] + m^r[b, rec_p]) * 0.5

and ``T`` is the observed value of the same expression: one IEEE division per mean, one addition and one multiplication by 0.5, in
that order, on the device as here.  Where ``n_a < 1`` or ``n_b < 1`` the device counts nothing and adds nothing; the host reports NaN.

**Null accumulation**, on the device in permutation order over ``r = first_perm .. first_perm + R - 1``:
``count_ge[p, a, b] = #{r : T^r >= T}`` and ``count_le`` likewise (int64), ``sum_d`` and ``sumsq_d`` the float64 sums of
``d = T^r - T`` and of ``d^2`` (the square rounded on its own, then added).

**Order.**  A spot's value is added to the cell of its label by the one thread that owns the cell, the spots of a segment of 2,048 in
ascending order, the segments in ascending order; an exact zero is skipped, which changes no bit.  No floating-point atomics; every
``u^r[c, s]`` depends only on the labels, the column and the permutation - not on the gene tile, the batch (``max_batch``), the
stripe (``max_gather_bytes``), the other genes, the other pairs or how a range of permutations is split into calls; two calls
return the same bits.

**Statistics** (``assemble_ligrec``, pure NumPy through ``rank_against_null``)::

    means     = T
    pct[c, s] = nnz / n_c
    expressed[p, a, b] = pct[a, lig_p] >= threshold and pct[b, rec_p] >= threshold          threshold = 0.01 by default, in [0, 1]
    p_greater = (1 + count_ge) / (R + 1)        p_less likewise with count_le        p_value = min(1, 2 min(p_greater, p_less))
    null_mean = T + mean_r d      null_std = std_r d (ddof = 0)      z_sim = (T - null_mean) / null_std      NaN where null_std = 0
    q_value   = Benjamini-Hochberg of p_greater over all entries that are not NaN
    order     = the (pair, a, b) triples by ascending p_greater, then descending means; NaN last, ties by ascending flat index

Everything of the test (``p_*``, ``z_sim``, ``null_*``, ``q_value``) is NaN where not ``expressed`` or where a group is empty.  Two
deliberate differences from squidpy's ``ligrec``: p is ``(1 + count) / (R + 1)``, this project's rule for every permutation test, not
``count / R`` (a p value is never 0); and ``means`` is not zeroed where one of the two means is 0.

**Out of scope.**  Multi-subunit complexes (the caller passes a combined column); pairs resolved from a database;
``ShardedFlashDeconv``; NaN in ``Y``; normalising ``Y``; more than 64 labels.
"""
import ctypes

import numpy as np

from .. import _lib
from ._device import check_count, device_of, matrix_on_device
from ._permutation import _NULL_CALL_BYTES, _permutation_seed, check_permutation_counts, permutation_chunks, rank_against_null
from .gene_pairs import check_request as _check_pairs
from .neighborhoods import MAX_LABELS, _check_flag, _labels_on_device, check_labels
from .spatial_genes import _benjamini_hochberg, _check_n_top, _check_Y_rows

__all__ = ["ligand_receptor_test", "label_gene_sums", "assemble_ligrec", "check_request", "MAX_GENES", "MAX_STATISTICS", "MAX_SPOTS",
           "GENE_TILE", "GROUP", "SEGMENT"]

MAX_GENES = 4096                                  # the MAX_GENES of gene_modules
MAX_STATISTICS = 1 << 22                          # P * C^2: the (pair, a, b) triples of a request
MAX_SPOTS = 1 << 24
GENE_TILE = 16                                    # genes of a workgroup
GROUP = 16                                        # permutations of a workgroup
SEGMENT = 2048                                    # spots of a workgroup: the constant of the summation order


def _check_threshold(threshold):
    if isinstance(threshold, (bool, np.bool_)) or not isinstance(threshold, (int, float, np.integer, np.floating)) \
            or not 0.0 <= threshold <= 1.0:
        raise ValueError(f"threshold must be a number in [0, 1], got {threshold!r}")
    return float(threshold)


def check_request(Y_shape, pairs, labels, n_labels=None, n_permutations=0, first_perm=0, max_batch=0, threshold=0.01):
    """Every check of a request that needs no GPU (``ValueError``, or ``TypeError`` for labels that are no integers, on the first
    that fails): the shape of ``Y``, the pairs against it, the labels (``neighborhoods.check_labels``) and their length, the caps
    ``MAX_GENES`` and ``MAX_STATISTICS``, the counts and ``threshold``.  Returns ``(pairs as int32 (P, 2), genes - the sorted
    distinct columns, int32 -, labels, C or None - CUDA labels whose count is not given are ranged on the device -,
    n_permutations, first_perm, max_batch, threshold)``."""
    if len(Y_shape) != 2 or Y_shape[1] < 1:
        raise ValueError(f"Y must be a 2-D (n_spots, n_genes) matrix with at least one gene, got shape {tuple(Y_shape)}")
    n = int(Y_shape[0])
    if not 1 <= n <= MAX_SPOTS:
        raise ValueError(f"Y must have between 1 and {MAX_SPOTS} spots, got shape {tuple(Y_shape)}")
    pairs = _check_pairs(Y_shape, pairs)
    genes = np.unique(pairs).astype(np.int32)
    if genes.shape[0] > MAX_GENES:
        raise ValueError(f"pairs may name at most {MAX_GENES} distinct genes, got {genes.shape[0]}")
    n_lab, labels, C = check_labels(labels, n_labels)
    if n_lab != n:
        raise ValueError(f"labels must have one entry per spot of Y ({n}), got {n_lab}")
    if pairs.shape[0] * (C if C is not None else 1) ** 2 > MAX_STATISTICS:
        raise ValueError(f"P * C^2 must be at most {MAX_STATISTICS}, got P = {pairs.shape[0]} and C = {C if C is not None else 1}")
    R, first, batch = check_permutation_counts(n_permutations, first_perm, max_batch)
    return pairs, genes, labels, C, R, first, batch, _check_threshold(threshold)


def _check_gather(max_gather_bytes):
    return 0 if max_gather_bytes is None else check_count("max_gather_bytes", max_gather_bytes, 1)


def _one_call(lib, m, n, G, lab, C, genes, pairs, seed, first, cnt, max_batch, max_gather, null, stream):
    """One call of the entry on the staged matrix ``m``: (u, nnz, label_counts, count_ge, count_le, sum_d, sumsq_d, batch)."""
    S, P = genes.shape[0], pairs.shape[0]
    u, nnz, counts = np.zeros((C, S)), np.zeros((C, S), dtype=np.int64), np.zeros(C, dtype=np.int64)
    ge, le = np.zeros((P, C, C), dtype=np.int64), np.zeros((P, C, C), dtype=np.int64)
    sd, sq = np.zeros((P, C, C)), np.zeros((P, C, C))
    batch = ctypes.c_int32(0)
    tail = (ctypes.c_void_p(lab.data_ptr()), int(C), _lib.ptr_i32(genes), S, _lib.ptr_i32(pairs), P, ctypes.c_uint64(seed), int(first),
            int(cnt), int(max_batch), int(max_gather), ctypes.c_void_p(null.data_ptr()) if null is not None and cnt > 0 else None,
            _lib.ptr_f64(u), _lib.ptr_i64(nnz), _lib.ptr_i64(counts), _lib.ptr_i64(ge), _lib.ptr_i64(le), _lib.ptr_f64(sd),
            _lib.ptr_f64(sq), ctypes.byref(batch), stream)
    try:
        if m[0] == "csr":
            _lib.check(lib.fdx_label_gene_sums_csr_dev(ctypes.byref(m[1].view), *tail))
        else:
            _, ptr, code, ldy = m
            _lib.check(lib.fdx_label_gene_sums_dev(ptr, code, n, G, ldy, *tail))
    except _lib.FdxError as e:
        if "outside [-1, C)" in str(e):
            raise ValueError(f"labels must lie in [-1, {C}): the device found one that does not") from e
        raise
    return u, nnz, counts, ge, le, sd, sq, int(batch.value)


def _sums_device(Y, n, G, pairs, genes, labels, C, seed, first, R, max_batch, max_gather, return_null):
    import torch
    _lib.require_gpu()
    lib = _lib.load()
    device = device_of(Y, labels)
    device_out = return_null and (_lib.is_cuda_tensor(Y) or _lib.is_cuda_tensor(labels))
    with torch.cuda.device(device):
        stream = _lib.current_stream(device)
        lab, C = _labels_on_device(labels, C, device)
        P, S = pairs.shape[0], genes.shape[0]
        if P * C * C > MAX_STATISTICS:                          # (CUDA labels whose count was not given: known only now)
            raise ValueError(f"P * C^2 must be at most {MAX_STATISTICS}, got P = {P} and C = {C}")
        # device inputs keep the whole null on the device in one call; host inputs get it in calls of at most _NULL_CALL_BYTES
        chunk = R if device_out or not return_null else max(1, min(R, _NULL_CALL_BYTES // (8 * C * S)))
        null_dev = torch.empty((R if device_out else min(chunk, R), C, S), dtype=torch.float64, device=device) if return_null else None
        null_host = np.empty((R, C, S)) if return_null and not device_out else None
        out, batches = None, [0]
        with matrix_on_device(Y, device) as m:
            for done, cnt in permutation_chunks(R, max(chunk, 1)):
                part = None if null_dev is None else null_dev[done:done + cnt] if device_out else null_dev[:cnt]
                u, nnz, counts, ge, le, sd, sq, batch = _one_call(lib, m, n, G, lab, C, genes, pairs, seed, first + done, cnt, max_batch,
                                                                  max_gather, part, stream)
                batches.append(batch)
                if out is None:
                    out = {"genes": genes.astype(np.int64), "u": u, "nnz": nnz, "label_counts": counts, "n": int(n), "count_ge": ge,
                           "count_le": le, "sum_d": sd, "sumsq_d": sq}
                else:                                           # the counts add exactly; the sums continue call after call
                    out["count_ge"] += ge
                    out["count_le"] += le
                    out["sum_d"] += sd
                    out["sumsq_d"] += sq
                if null_host is not None and cnt > 0:
                    null_host[done:done + cnt] = _lib.tensor_to_host(part)
    out.update(n_permutations=int(R), batch=max(batches))
    if return_null:
        out["null"] = null_dev if device_out else null_host
    return out


def label_gene_sums(Y, labels, pairs, n_labels=None, seed=0, first_perm=0, n_permutations=0, max_batch=0, return_null=False,
                    max_gather_bytes=None):
    """The device half (module docstring): a dict of ``genes`` (S,) int64 - the sorted distinct columns of ``pairs`` -, ``u`` (C, S)
    float64, ``nnz`` (C, S) and ``label_counts`` (C,) int64, ``n``, and over permutations
    ``first_perm .. first_perm + n_permutations - 1`` of ``seed`` the (P, C, C) arrays ``count_ge``, ``count_le`` (int64), ``sum_d``,
    ``sumsq_d`` (float64) of ``d = T^r - T`` (all 0 where a group is empty); ``n_permutations``; ``batch``, the permutations the
    device ran per launch chain (``max_batch`` caps it, 0: chosen from the scratch budget).  With ``return_null=True`` ``null``
    (n_permutations, C, S) float64 holds every ``u^r`` - a CUDA tensor when ``Y`` or ``labels`` was one, else numpy, and then the
    permutations go in calls whose null is at most 256 MiB (the counts of the calls add exactly, their sums one after the other).
    ``max_gather_bytes`` (None: about 1 GiB) bounds the gathered copy of a stripe of columns; neither it nor ``max_batch`` moves a
    bit of ``u``, ``null`` or the counts.  Everything checkable is checked before the GPU is touched."""
    n, G = _check_Y_rows(Y)
    pairs, genes, labels, C, R, first, max_batch, _ = check_request((n, G), pairs, labels, n_labels, n_permutations, first_perm, max_batch)
    return_null = _check_flag("return_null", return_null)
    max_gather = _check_gather(max_gather_bytes)
    seed = _permutation_seed(seed)
    return _sums_device(Y, n, G, pairs, genes, labels, C, seed, first, R, max_batch, max_gather, return_null)


def _order(p_greater, means):
    """Flat places by ascending ``p_greater``, then descending ``means``, NaN last, ties by ascending place (int64)."""
    p = np.where(np.isnan(p_greater), np.inf, p_greater).ravel()
    m = np.where(np.isnan(means), np.inf, -means).ravel()
    return np.lexsort((np.arange(p.size), m, p)).astype(np.int64)


def assemble_ligrec(pairs, genes, u, nnz, label_counts, count_ge=None, count_le=None, sum_d=None, sumsq_d=None, n_permutations=0,
                    threshold=0.01):
    """The statistics of the module docstring from the sums of ``label_gene_sums`` (pure host arithmetic): a dict of ``means``
    (P, C, C) float64, ``pct`` (C, S), ``expressed`` (P, C, C) bool, ``order`` (P C C, 3) int64 - the triples (pair, a, b) - and, with
    ``n_permutations`` R >= 1 - then ``count_ge``, ``count_le``, ``sum_d``, ``sumsq_d`` (P, C, C) are needed - also ``p_greater``,
    ``p_less``, ``p_value``, ``null_mean``, ``null_std``, ``z_sim``, ``q_value`` and ``n_permutations``.  With R = 0 the order is by
    descending ``means`` alone.  Nothing raises on a degenerate input: an empty group gives NaN in ``means`` and in the test, a
    pair that is not ``expressed`` NaN in the test, a null that does not vary NaN in ``z_sim``."""
    pairs = np.asarray(pairs)
    genes = np.asarray(genes)
    u = np.asarray(u, dtype=np.float64)
    nnz, na = np.asarray(nnz), np.asarray(label_counts)
    if pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.shape[0] < 1 or genes.ndim != 1:
        raise ValueError(f"pairs must be (P, 2) with P >= 1 and genes (S,), got shapes {pairs.shape} and {genes.shape}")
    if u.ndim != 2 or u.shape[1] != genes.shape[0] or nnz.shape != u.shape or na.shape != (u.shape[0],):
        raise ValueError(f"u and nnz must be (C, S) and label_counts (C,) with S = {genes.shape[0]}, got shapes "
                         f"{[a.shape for a in (u, nnz, na)]}")
    slot = np.searchsorted(genes, pairs)
    if np.any(slot >= genes.shape[0]) or np.any(genes[np.minimum(slot, genes.shape[0] - 1)] != pairs):
        raise ValueError("a pair names a column that genes does not list")
    R = check_count("n_permutations", n_permutations)
    threshold = _check_threshold(threshold)
    P, C = pairs.shape[0], u.shape[0]
    lig, rec = slot[:, 0], slot[:, 1]
    nc = na.astype(np.float64)
    filled = na >= 1
    with np.errstate(divide="ignore", invalid="ignore"):
        m = u / nc[:, None]                                     # one division per mean
        pct = np.where(filled[:, None], nnz.astype(np.float64) / np.where(filled, nc, 1.0)[:, None], np.nan)
        means = (m[:, lig].T[:, :, None] + m[:, rec].T[:, None, :]) * 0.5
    both = filled[None, :, None] & filled[None, None, :] & np.ones((P, 1, 1), dtype=bool)
    means = np.where(both, means, np.nan)
    with np.errstate(invalid="ignore"):
        expressed = both & (pct[:, lig].T[:, :, None] >= threshold) & (pct[:, rec].T[:, None, :] >= threshold)
    out = {"means": means, "pct": pct, "expressed": expressed}
    p_greater = np.full((P, C, C), np.nan)
    if R >= 1:
        arrs = [count_ge, count_le, sum_d, sumsq_d]
        if any(a is None for a in arrs):
            raise ValueError("count_ge, count_le, sum_d and sumsq_d are needed when n_permutations >= 1")
        arrs = [np.asarray(a) for a in arrs]
        if any(a.shape != (P, C, C) for a in arrs):
            raise ValueError(f"the counts and sums must be (P, C, C) = {(P, C, C)}, got shapes {[a.shape for a in arrs]}")
        ge, le, sd, sq = (a.astype(np.float64) for a in arrs)
        with np.errstate(divide="ignore", invalid="ignore"):
            greater, less, p, mean_d, null_std, z_sim = rank_against_null(np, ge, le, sd, sq, R)
            null_mean = means + mean_d
        nan = np.float64(np.nan)
        p_greater = np.where(expressed, greater, nan)
        out.update({"p_greater": p_greater, "p_less": np.where(expressed, less, nan), "p_value": np.where(expressed, p, nan),
                    "null_mean": np.where(expressed, null_mean, nan), "null_std": np.where(expressed, null_std, nan),
                    "z_sim": np.where(expressed, z_sim, nan), "n_permutations": R})
        out["q_value"] = _benjamini_hochberg(p_greater.ravel()).reshape(P, C, C)
    flat = _order(p_greater, means)
    out["order"] = np.stack(np.unravel_index(flat, (P, C, C)), axis=1).astype(np.int64)
    return out


def ligand_receptor_test(Y, labels, pairs, n_labels=None, n_permutations=999, random_state=0, threshold=0.01, n_top=None,
                         return_null=False):
    """Between which groups of spots a ligand-receptor pair acts: for every pair of ``pairs`` and every ordered pair of labels
    (a, b) the mean of the ligand in a and of the receptor in b against ``n_permutations`` random reassignments of the labels to the
    spots, on the GPU (module docstring).

    ``Y``: (n_spots, n_genes) - dense numpy / CUDA tensor, float32, float64 or integer counts, or CSR (scipy, CUDA
    ``torch.sparse_csr``); tested as it is passed (not normalised).  ``labels``: (n_spots,) integers in ``[-1, n_labels)``, numpy or
    a CUDA tensor - the ``labels`` of ``spatial_niches``, the dominant cell type, cluster labels; ``-1`` is shuffled with the rest
    and never counted.  ``n_labels``: 1 .. 64 (None: the largest label + 1).  ``pairs``: (P, 2) integer columns of ``Y``, ligand
    then receptor.  ``n_permutations``: an int >= 0; ``random_state``: an int in [0, 2^64) used as the seed as it stands, or None / a
    ``RandomState`` from which one 63-bit seed is drawn.  ``threshold``: the share of a group's spots that must express a gene for
    the pair to be tested there.  ``n_top``: also ``top = order[:n_top]``.  Every argument check raises before the GPU is touched.

    Returns the dict of ``assemble_ligrec`` - ``means``, ``pct``, ``expressed``, ``order`` and, with R >= 1, ``p_greater``,
    ``p_less``, ``p_value``, ``null_mean``, ``null_std``, ``z_sim``, ``q_value``, ``n_permutations`` - plus ``pairs`` (P, 2) and
    ``genes`` (S,) int64, ``label_counts``, ``n`` and, with ``return_null=True`` and R >= 1, ``null`` (R, C, S) - every ``u^r``."""
    n, G = _check_Y_rows(Y)
    pairs, genes, labels, C, R, _, _, threshold = check_request((n, G), pairs, labels, n_labels, n_permutations, 0, 0, threshold)
    n_top = _check_n_top(n_top)
    return_null = _check_flag("return_null", return_null)
    s = _sums_device(Y, n, G, pairs, genes, labels, C, _permutation_seed(random_state), 0, R, 0, 0, return_null and R >= 1)
    out = assemble_ligrec(pairs, s["genes"], s["u"], s["nnz"], s["label_counts"], s["count_ge"], s["count_le"], s["sum_d"],
                          s["sumsq_d"], R, threshold)
    out.update(pairs=pairs.astype(np.int64), genes=s["genes"], label_counts=s["label_counts"], n=s["n"])
    if return_null and R >= 1:
        out["null"] = s["null"]
    if n_top is not None:
        out["top"] = out["order"][:n_top]
    return out
