"""Permutation test per gene for Moran's I and Geary's C: the observed statistics of the listed genes of a spot-by-gene matrix
ranked against the null of R random reassignments of each gene's values to the spots, computed on the GPU with the gene columns
held in LDS (additive, not in the reference).  No normality is assumed, which matters for sparse, zero-inflated counts: there the
analytic z score of ``utils.spatial_genes`` is at its weakest.

**Inputs.**  ``Y`` and ``graph`` are those of ``utils.spatial_genes``: ``Y`` (n, G) dense float32 or float64 (integers through the
upload rules of ``_lib.upload_matrix``), host or CUDA, any row stride, or CSR from scipy or a CUDA ``torch.sparse_csr`` tensor;
``graph`` a fitted ``FlashDeconv``, a ``_lib.Graph`` or a scipy sparse adjacency.  ``genes`` is a 1-D array of S DISTINCT column
indices (None: every column).

**Definition.**  ``A`` is the graph's symmetric binary adjacency, ``deg_i = sum_j A_ij``, ``W = sum_i deg_i``; ``y`` is one gene
column, converted from its storage type to float64; ``pi_r = permutation_indices(seed, r, n)``.  The permuted column is
``v_i = y[pi_r(i)]``, in the caller's spot order (the convention of ``spatial_permutation_test``).  Per gene and permutation r::

    P_r = sum_i v_i sum_{j in N(i)} v_j      D_r = sum_i deg_i v_i      H_r = sum_i deg_i v_i^2

``u``, ``q``, ``ymin``, ``ymax`` and hence ``m = u/n`` and ``m2 = q - u*u/n`` do not change under a permutation.  The observed
``P``, ``D``, ``H`` are the same sums with the identity in place of ``pi_r``.  With
``I(P, D) = (n / W) (P - 2 m D + m^2 W) / m2`` and ``C(P, H) = ((n - 1) / (2 W)) (2 H - 2 P) / m2``::

    p_sim        = (1 + #{r : I_r >= I_obs}) / (R + 1)          one-sided, positive autocorrelation, as p_value of spatial_genes
    p_sim_less   = (1 + #{r : I_r <= I_obs}) / (R + 1)
    gearys_p_sim = (1 + #{r : C_r <= C_obs}) / (R + 1)          small C = positive autocorrelation
    null_mean, null_std (ddof 0) of I_r       z_sim = (I_obs - null_mean) / null_std   (NaN where null_std == 0)
    q_sim        = Benjamini-Hochberg of p_sim over the tested genes that are not NaN

``null_mean = (sum_r I_r) / R`` and ``null_std = sqrt(max((sum_r I_r^2) / R - null_mean^2, 0))``, both sums added in the order
r = 0, 1, ..., so they can be merged chunk by chunk without keeping the null.  NaN rules follow ``assemble_genes``: a constant gene
(``ymin == ymax``, decided exactly), ``m2 <= 0``, ``W == 0`` or ``n < 2`` gives NaN in every key.  Nothing raises.  ``R = 0`` is
allowed and returns the observed part only.

**Device** (``fdx_gene_spatial_perm_dev`` / ``_csr_dev``, csrc/gene_perm_kernels.cpp, on torch's current stream): the listed
columns are gathered once in the storage type and the graph's order; per permutation a table of n positions is computed once
(one evaluation of the keyed bijection per spot, shared by every gene); a workgroup owns a tile of genes and a range of
permutations, and where the tile and the table fit the CU's LDS (``max_lds_bytes``, default the device's 160 KiB: 20 n bytes for
four float32 genes) every one of the ``R * S * n * (1 + deg)`` reads of the statistic is an LDS read; otherwise the same loop reads
through L2.  ``Y`` is read once.  The device returns the raw sums ``obs`` (7, S) and ``null`` (R, 3, S); counting is done here on
the host in float64.

**Order.**  No floating-point atomics; every (gene, permutation) sum depends only on the graph, the column and the permutation -
not on the gene tile, how many permutations a workgroup walks at a time, the permutation batch (``max_batch``), the stripe
(``max_gather_bytes``), the route, the other genes of the list or their order; two calls and
a range of permutations split into several calls return the same bits.

**Out of scope.**  Permutation p values for gene pairs and for the co-expression matrix; permutations of the residual statistic;
``ShardedFlashDeconv``; NaN in ``Y``; normalising ``Y``.
"""
import ctypes

import numpy as np

from .. import _lib
from ._device import check_count, device_of, matrix_on_device, resolved_graph
from .spatial_genes import _benjamini_hochberg, _check_n_top, _check_Y_rows
from ._permutation import (_NULL_CALL_BYTES, _permutation_seed, check_permutation_counts, null_moments, p_from_count,
                           permutation_chunks)

__all__ = ["spatial_gene_permutation_test", "gene_permutation_sums", "assemble_gene_permutation", "merge_null_counts", "check_request",
           "OBS_PLANES", "NULL_PLANES", "ROUTES", "GENE_TILE"]

OBS_PLANES = ("u", "q", "D", "H", "P", "ymin", "ymax")
NULL_PLANES = ("P", "D", "H")
ROUTES = ("global", "lds", "lds_table")
GENE_TILE = 4                                     # float32 genes of a workgroup where they fit LDS, and on the global route (float64: 2)
STAT_KEYS = ("p_sim", "p_sim_less", "gearys_p_sim", "z_sim", "null_mean", "null_std", "q_sim")


def check_request(Y_shape, genes=None, n_permutations=0, first_perm=0, max_batch=0, max_lds_bytes=None, max_gather_bytes=None):
    """Everything of a request that can be checked before the GPU is touched (``ValueError`` on the first that fails): the shape of
    ``Y``; ``genes`` - None (every column) or a 1-D integer array of distinct indices in ``[0, G)``, at least one; the counts
    ``n_permutations``, ``first_perm``, ``max_batch`` (ints >= 0), ``max_lds_bytes`` and ``max_gather_bytes`` (None or an int >= 1).
    Returns ``(genes as a C-contiguous int32 array, n_permutations, first_perm, max_batch, max_lds_bytes or 0, max_gather_bytes
    or 0)``."""
    if len(Y_shape) != 2:
        raise ValueError(f"Y must be a 2-D spot-by-gene matrix, got shape {tuple(Y_shape)}")
    n, G = int(Y_shape[0]), int(Y_shape[1])
    if G < 1:
        raise ValueError(f"Y must have at least one gene, got shape {(n, G)}")
    if n < 1:
        raise ValueError(f"Y must have at least one spot, got shape {(n, G)}")
    if genes is None:
        a = np.arange(G, dtype=np.int32)
    else:
        a = genes.detach().cpu().numpy() if _lib.is_torch(genes) else np.asarray(genes)
        if a.ndim != 1:
            raise ValueError(f"genes must be a 1-D array of gene indices, got shape {a.shape}")
        if a.dtype.kind not in "iu":
            raise ValueError(f"genes must be of an integer dtype, got {a.dtype}")
        if a.shape[0] < 1:
            raise ValueError("genes must hold at least one gene index")
        if int(a.min()) < 0 or int(a.max()) >= G:
            bad = a[(a < 0) | (a >= G)][0]
            raise ValueError(f"genes holds the gene index {int(bad)} outside [0, {G})")
        values, counts = np.unique(a, return_counts=True)
        if values.size != a.size:
            raise ValueError(f"genes lists the gene index {int(values[counts > 1][0])} twice")
    R, first, batch = check_permutation_counts(n_permutations, first_perm, max_batch)
    lds = 0 if max_lds_bytes is None else check_count("max_lds_bytes", max_lds_bytes, 1)
    gather = 0 if max_gather_bytes is None else check_count("max_gather_bytes", max_gather_bytes, 1)
    return np.ascontiguousarray(a, dtype=np.int32), R, first, batch, lds, gather


def _statistics(n, W, m, m2, dead, P, D, H):
    """(I, C) of the sums ``P``, ``D``, ``H`` ((S,) or (R, S)) of genes with mean ``m`` and second moment ``m2``; NaN where ``dead``:
    ``(n / W) (P - (2 m) D + m m W) / m2`` and ``((n - 1) / (2 W)) (2 H - 2 P) / m2``, operation for operation, in place (the null
    of 1,000 permutations of 2,000 genes is 16 MB a plane)."""
    if not (W > 0 and n >= 2):
        return np.full(np.shape(P), np.nan), np.full(np.shape(P), np.nan)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        I = np.multiply(2.0 * m, D)
        np.subtract(P, I, out=I)
        I += m * m * float(W)
        I *= float(n) / float(W)
        I /= m2
        C = np.multiply(2.0, H)
        C -= 2.0 * P
        C *= (n - 1.0) / (2.0 * float(W))
        C /= m2
    I[..., dead] = np.nan
    C[..., dead] = np.nan
    return I, C


def _observed(n, W, u, q, D, H, P, ymin, ymax):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        m = u / n if n > 0 else np.full(u.shape, np.nan)
        m2 = q - u * u / n if n > 0 else np.full(u.shape, np.nan)
    dead = (ymin == ymax) | ~(m2 > 0) | (W <= 0) | (n < 2)
    I, C = _statistics(n, W, m, m2, dead, P, D, H)
    return m, m2, dead, I, C


def merge_null_counts(counts, n, W, u, q, D, H, P, ymin, ymax, null):
    """The counts of ``assemble_gene_permutation`` after the permutations of ``null`` (r, 3, S) - the planes ``P_r``, ``D_r``,
    ``H_r`` of the NEXT r permutations - are merged into ``counts`` (None: none so far): a dict of ``count_ge``, ``count_le``,
    ``count_c_le`` (int64 (S,)), ``sum_i``, ``sumsq_i`` (float64 (S,), added permutation after permutation) and
    ``n_permutations``.  Pure NumPy float64."""
    n, W = int(n), int(W)
    u, q, D, H, P, ymin, ymax = (np.asarray(a, dtype=np.float64) for a in (u, q, D, H, P, ymin, ymax))
    null = np.asarray(null, dtype=np.float64)
    S = u.shape[0]
    if null.ndim != 3 or null.shape[1:] != (3, S):
        raise ValueError(f"null must be (R, 3, S) with S = {S}, got shape {null.shape}")
    if counts is None:
        counts = {"count_ge": np.zeros(S, dtype=np.int64), "count_le": np.zeros(S, dtype=np.int64),
                  "count_c_le": np.zeros(S, dtype=np.int64), "sum_i": np.zeros(S), "sumsq_i": np.zeros(S), "n_permutations": 0}
    m, m2, dead, I, C = _observed(n, W, u, q, D, H, P, ymin, ymax)
    Ir, Cr = _statistics(n, W, m, m2, dead, null[:, 0], null[:, 1], null[:, 2])
    with np.errstate(invalid="ignore"):
        out = {"count_ge": counts["count_ge"] + (Ir >= I).sum(axis=0), "count_le": counts["count_le"] + (Ir <= I).sum(axis=0),
               "count_c_le": counts["count_c_le"] + (Cr <= C).sum(axis=0), "n_permutations": counts["n_permutations"] + null.shape[0]}
        s, sq = counts["sum_i"].copy(), counts["sumsq_i"].copy()
        for r in range(null.shape[0]):                          # in the order of the permutations: no chunking moves a bit
            s += Ir[r]
        np.multiply(Ir, Ir, out=Ir)
        for r in range(null.shape[0]):
            sq += Ir[r]
    out.update(sum_i=s, sumsq_i=sq)
    return out


def assemble_gene_permutation(n, W, u, q, D, H, P, ymin, ymax, null=None, counts=None):
    """The keys of the module docstring from the observed sums of one call and EITHER the whole ``null`` (R, 3, S) OR the merged
    ``counts`` of ``merge_null_counts`` (pure host arithmetic): a dict of ``morans_i``, ``gearys_c`` (S,), ``n_permutations`` and,
    for R >= 1, ``p_sim``, ``p_sim_less``, ``gearys_p_sim``, ``z_sim``, ``null_mean``, ``null_std``, ``q_sim`` (S,)."""
    n, W = int(n), int(W)
    planes = [np.asarray(a, dtype=np.float64) for a in (u, q, D, H, P, ymin, ymax)]
    if planes[0].ndim != 1 or any(a.shape != planes[0].shape for a in planes):
        raise ValueError(f"the seven sums must be 1-D arrays of one length, got shapes {[a.shape for a in planes]}")
    if null is not None and counts is not None:
        raise ValueError("give the null or the merged counts, not both")
    if null is not None:
        counts = merge_null_counts(None, n, W, *planes, null)
    _, _, dead, I, C = _observed(n, W, *planes)
    R = 0 if counts is None else int(counts["n_permutations"])
    out = {"morans_i": I, "gearys_c": C, "n_permutations": R}
    if R < 1:
        return out
    nan = np.float64(np.nan)
    ge, le, c_le, s, sq = (np.asarray(counts[k], dtype=np.float64) for k in ("count_ge", "count_le", "count_c_le", "sum_i", "sumsq_i"))
    out["p_sim"] = np.where(dead, nan, p_from_count(np, ge, R))
    out["p_sim_less"] = np.where(dead, nan, p_from_count(np, le, R))
    out["gearys_p_sim"] = np.where(dead, nan, p_from_count(np, c_le, R))
    with np.errstate(divide="ignore", invalid="ignore"):
        mean, std = null_moments(np, s, sq, R)                  # of I_r itself, not of a difference: z_sim keeps its own form
        out["null_mean"] = np.where(dead, nan, mean)
        out["null_std"] = np.where(dead, nan, std)
        out["z_sim"] = np.where(dead | ~(std > 0), nan, (I - mean) / np.where(std > 0, std, 1.0))
    out["q_sim"] = _benjamini_hochberg(out["p_sim"])
    return out


def _one_call(lib, g, m, n, G, genes, seed, first, cnt, max_batch, max_lds, max_gather, obs, null, stream):
    """One call of the entry on the staged matrix ``m`` into ``obs`` (7, S) and ``null`` (at least (cnt, 3, S); None for cnt = 0),
    CUDA float64: (counts, info)."""
    S = genes.shape[0]
    counts, info = np.zeros(3, dtype=np.int64), np.zeros(6, dtype=np.int64)
    null_p = ctypes.c_void_p(null.data_ptr()) if cnt > 0 else None
    tail = (_lib.ptr_i32(genes), S, ctypes.c_uint64(seed), int(first), int(cnt), int(max_batch), int(max_lds), int(max_gather),
            ctypes.c_void_p(obs.data_ptr()), null_p, _lib.ptr_i64(counts), _lib.ptr_i64(info), stream)
    if m[0] == "csr":
        _lib.check(lib.fdx_gene_spatial_perm_csr_dev(g.handle, ctypes.byref(m[1].view), *tail))
    else:
        _, ptr, code, ldy = m
        _lib.check(lib.fdx_gene_spatial_perm_dev(g.handle, ptr, code, n, G, ldy, *tail))
    return counts, info


def _sums_on_graph(Y, g, n, G, genes, seed, first, R, max_batch, max_lds, max_gather, return_null):
    import torch
    _lib.require_gpu()
    lib = _lib.load()
    device = device_of(Y)
    device_out = _lib.is_cuda_tensor(Y) and return_null
    S = genes.shape[0]
    chunk = max(1, min(R, _NULL_CALL_BYTES // (24 * S)))        # a call's null: what is copied to the host and counted in one piece
    merged, batches = None, [0]
    with torch.cuda.device(device):
        stream = _lib.current_stream(device)
        obs = torch.empty((len(OBS_PLANES), S), dtype=torch.float64, device=device)
        # a CUDA Y keeps the whole null on the device and every call writes its slice of it; else one call's worth, reused
        null_dev = torch.empty((R if device_out else min(chunk, R), 3, S), dtype=torch.float64, device=device)
        null_host = np.empty((R, 3, S)) if return_null and not device_out else None
        with matrix_on_device(Y, device) as m:
            for done, cnt in permutation_chunks(R, chunk):      # (one call even without permutations: the observed sums)
                part = null_dev[done:done + cnt] if device_out else null_dev[:cnt]
                counts, info = _one_call(lib, g, m, n, G, genes, seed, first + done, cnt, max_batch, max_lds, max_gather, obs, part, stream)
                if done == 0:
                    host = _lib.tensor_to_host(obs)
                    out = {name: host[k] for k, name in enumerate(OBS_PLANES)}
                    out.update(n=int(counts[0]), W=int(counts[1]), sum_deg_sq=int(counts[2]), genes=genes.astype(np.int64),
                               tile=int(info[0]), route=ROUTES[int(info[2])], stripes=int(info[3]), ways=int(info[4]),
                               chunk=int(info[5]))
                batches.append(int(info[1]))
                if cnt > 0:
                    block = _lib.tensor_to_host(part)
                    if null_host is not None:
                        null_host[done:done + cnt] = block
                    merged = merge_null_counts(merged, out["n"], out["W"], *(out[name] for name in OBS_PLANES), block)
    out.update(n_permutations=R, batch=max(batches), counts=merged)
    if return_null:
        out["null"] = null_dev if device_out else null_host
    return out


def gene_permutation_sums(Y, graph, genes=None, seed=0, first_perm=0, n_permutations=0, max_batch=0, max_lds_bytes=None,
                          return_null=True, max_gather_bytes=None):
    """The device half (module docstring): a dict of the observed planes ``u``, ``q``, ``D``, ``H``, ``P``, ``ymin``, ``ymax`` -
    numpy float64 (S,) - the integers ``n``, ``W``, ``sum_deg_sq``, ``genes`` (S,) int64, ``n_permutations``, what ran (``tile`` -
    the genes of a workgroup -, ``batch`` - the permutations whose tables were in flight -, ``route`` - one of ``ROUTES`` -,
    ``stripes`` - the pieces the gathered copy of the columns went in -, ``ways`` and ``chunk`` - the permutations a workgroup of
    the first launch walked at a time and in all), ``counts`` (``merge_null_counts`` over the permutations ``first_perm ..
    first_perm + n_permutations - 1`` of ``seed``; None without permutations) and, with ``return_null=True``, ``null``
    (n_permutations, 3, S) holding ``P_r``, ``D_r``, ``H_r`` - a CUDA tensor when ``Y`` was one, else numpy.  The permutations go
    in calls whose null is at most 256 MiB: that much is copied to the host and counted in one piece (every call gathers the
    columns again).  ``max_batch`` caps the permutations in flight (0: from the scratch budget), ``max_lds_bytes`` the LDS a
    workgroup may use (None: the device's), ``max_gather_bytes`` the gathered copy of a stripe (None: about 1 GiB); none of them
    moves a bit of the result.  Arguments are checked before anything touches the GPU."""
    n, G = _check_Y_rows(Y)
    genes, R, first, max_batch, max_lds, max_gather = check_request((n, G), genes, n_permutations, first_perm, max_batch, max_lds_bytes,
                                                                   max_gather_bytes)
    seed = _permutation_seed(seed)
    with resolved_graph(graph, n) as g:
        return _sums_on_graph(Y, g, n, G, genes, seed, first, R, max_batch, max_lds, max_gather, bool(return_null))


def _order(p_sim, z_sim):
    """Places by increasing ``p_sim``, then decreasing ``z_sim``, NaN last, ties by ascending place (int64)."""
    p = np.where(np.isnan(p_sim), np.inf, p_sim)
    z = np.where(np.isnan(z_sim), np.inf, -z_sim)
    return np.lexsort((np.arange(p.size), z, p)).astype(np.int64)


def spatial_gene_permutation_test(Y, graph, genes=None, n_permutations=999, random_state=0, return_null=False, n_top=None):
    """Which of the listed genes are spatially autocorrelated beyond chance: Moran's I and Geary's C of every gene of ``genes``
    ranked against ``n_permutations`` random reassignments of its values to the spots, on the GPU (module docstring).

    ``Y``: (n_spots, n_genes) - dense numpy / CUDA tensor, float32, float64 or integer counts, or CSR (scipy, CUDA
    ``torch.sparse_csr``); tested as it is passed.  ``graph``: a fitted ``FlashDeconv``, a ``_lib.Graph`` or a scipy sparse
    adjacency.  ``genes``: 1-D distinct column indices, None for every column.  ``n_permutations``: an int >= 0.  ``random_state``:
    an int in [0, 2^64) used as the seed as it stands, or None / a ``RandomState`` from which one 63-bit seed is drawn; the same
    seed gives the same permutations.  ``return_null``: also ``null_i`` (R, S), the null of Moran's I (numpy).  ``n_top``: also
    ``top = order[:n_top]``.  Arguments are checked before anything touches the GPU (``ValueError``).

    Returns a dict: ``morans_i``, ``gearys_c``, ``p_sim``, ``p_sim_less``, ``gearys_p_sim``, ``z_sim``, ``null_mean``,
    ``null_std``, ``q_sim`` (S,), ``genes`` (S,) int64, ``n_permutations``, ``n``, ``n_edges`` and ``order`` (S,) int64 - places
    in ``genes`` by increasing ``p_sim``, then decreasing ``z_sim``, NaN last.  With ``n_permutations=0`` the permutation keys
    are all NaN."""
    n, G = _check_Y_rows(Y)
    genes, R = check_request((n, G), genes, n_permutations)[:2]
    n_top = _check_n_top(n_top)
    seed = _permutation_seed(random_state)
    with resolved_graph(graph, n) as g:
        s = _sums_on_graph(Y, g, n, G, genes, seed, 0, R, 0, 0, 0, bool(return_null) and R >= 1)
    out = assemble_gene_permutation(s["n"], s["W"], *(s[name] for name in OBS_PLANES), counts=s["counts"])
    for key in STAT_KEYS:
        out.setdefault(key, np.full(genes.shape[0], np.nan))
    out.update(genes=s["genes"], n=s["n"], n_edges=s["W"] // 2, order=_order(out["p_sim"], out["z_sim"]))
    if return_null and R >= 1:
        null = _lib.tensor_to_host(s["null"]) if _lib.is_torch(s["null"]) else s["null"]
        m, m2, dead, _, _ = _observed(s["n"], s["W"], *(s[name] for name in OBS_PLANES))
        out["null_i"] = _statistics(s["n"], s["W"], m, m2, dead, null[:, 0], null[:, 1], null[:, 2])[0]
    if n_top is not None:
        out["top"] = out["order"][:n_top]
    return out
