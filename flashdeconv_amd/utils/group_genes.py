"""Marker genes of groups of spots: a Wilcoxon rank-sum test and a Welch t test per gene of "group c against the rest", with the
descriptives and the ranking of scanpy's ``rank_genes_groups``, from sums and exact tie-aware ranks computed on the GPU (additive,
not in the reference).  Which genes mark niche c - the groups being the ``labels`` of ``get_spatial_niches``, the spots a module
score lights up, or labels the caller brings.

**Inputs.**  ``Y`` is (n, G): dense float32 or float64 (integers through the upload rules of ``_lib.upload_matrix``), host or CUDA,
any row stride; or CSR from scipy or a CUDA ``torch.sparse_csr`` tensor (rows with distinct columns, sorted or not), kept sparse -
the routes of ``utils.expression``.  ``groups`` is (n,) integers in ``[-1, C)``, host or CUDA; ``-1`` leaves a spot out; ``None``
means one group of all rows; ``C = n_groups`` (None: the largest label + 1), ``1 <= C <= 256``.  ``n <= 2 000 000``.

**Sums** (``fdx_gene_group_sums_dev`` / ``_csr_dev``, csrc/gene_group_kernels.cpp, on torch's current stream).  With ``N`` the
number of used spots, ``n_c`` the size of group c and a gene's values compared as converted to float64 from their storage type
(every bit of a float64 counts)::

    u[c, g]   = sum_{i in c} y_ig          q[c, g] = sum_{i in c} y_ig^2                     float64
    nnz[c, g] = #{i in c : y_ig != 0}                                                        int64
    R2[c, g]  = sum_{i in c} 2 midrank_ig                                                    int64
    T[g]      = sum over the tie runs of gene g's N used values of (t^3 - t)                 int64

``midrank_ig`` is the 1-based average rank of ``y_ig`` among the N used values of gene g (``scipy.stats.rankdata(method=
"average")``); a CSR entry that is not stored is the value 0, and ``-0.0`` and a stored zero are zeros.  ``u`` and ``q`` are,
bit for bit, what ``weighted_gene_sums(Y, ones((n, 1)), groups)`` returns - the same pass runs; the integers are exact.  The
kernels never sort a zero: the nonzeros of a stripe of genes are compacted, sorted by value and then stably by gene, and the zero
run's ranks follow from the counts; two calls return the same bits, and so does a call cut into more stripes.

**Statistics** (``assemble_group_tests``, pure NumPy float64), group c against the rest - all OTHER used spots:
``n_r = N - n_c`` and every sum of the rest is the total, added over c in ascending order, minus the group's::

    mean = u / n_c                         var  = max(0, q - u^2 / n_c) / (n_c - 1)           (ddof 1; _rest alike)
    pct  = nnz / n_c                       log2_fold_change = log2((mean + pseudocount) / (mean_rest + pseudocount))
    t       = (mean - mean_rest) / sqrt(var / n_c + var_rest / n_r)                           (Welch)
    t_dof   = (var/n_c + var_rest/n_r)^2 / ((var/n_c)^2 / (n_c - 1) + (var_rest/n_r)^2 / (n_r - 1))
    t_p_value = 2 stdtr(t_dof, -|t|)
    U       = R2 / 2 - n_c (n_c + 1) / 2   auc = U / (n_c n_r)
    sigma^2 = n_c n_r / 12 * ((N + 1) - T / (N (N - 1)))        formed as (N^3 - N - T) / (N (N - 1)) from the exact integer
    z_score = (U - n_c n_r / 2) / sigma    (tie correction, no continuity correction)
    p_value = erfc(|z_score| / sqrt 2)     (two-sided)
    q_value, t_q_value = Benjamini-Hochberg over the genes of each group whose p value is not NaN
    order[c] = genes by decreasing z_score, NaN last, ties by ascending index (int64)

These are ``scipy.stats.mannwhitneyu(method="asymptotic", use_continuity=False)`` and ``ttest_ind(equal_var=False)``.
**Conditioning**: the variances are raw sums expanded, ``q - u^2 / n``, and the rest's come by subtraction from the totals: both
cancel, like ``m2`` of the spatial entries - about ``eps * mean^2 / var`` of the relative accuracy goes, and a small group inside
a large total loses nothing while a small REST does (its sums are differences of nearly equal numbers).  Expression matrices have
means of the order of their standard deviations.  The rank statistics have no such loss: they are integers until the last step.

**NaN rules.**  Nothing raises.  ``mean``, ``pct`` are NaN where ``n_c < 1`` (``_rest``: ``n_r < 1``), variances where the count is
below 2; ``auc``, ``z_score``, ``p_value``, ``log2_fold_change`` and the t statistics are NaN where ``n_c < 1`` or ``n_r < 1``
(one group of everything, an empty group, no used spot); ``z_score`` and ``p_value`` also where ``sigma == 0`` (a constant gene,
an all-zero one among them - decided on the exact integer); ``t``, ``t_dof``, ``t_p_value`` also where the t denominator is 0 or
a variance is NaN.

**Out of scope.**  NaN in ``Y``; contrasts of one group against one other group; normalising ``Y`` (the caller passes the matrix
they want tested - ``log1p`` on a CSR's data keeps it sparse); ``ShardedFlashDeconv``; more than 2 000 000 spots.
"""
import ctypes

import numpy as np

from .. import _lib
from ._device import check_matrix, device_of, matrix_on_device
from .expression import _check_groups
from .spatial_genes import _benjamini_hochberg, _check_n_top, _decreasing_order

__all__ = ["rank_genes_groups", "gene_group_sums", "assemble_group_tests", "check_request", "MAX_GROUPS", "MAX_SPOTS"]

MAX_GROUPS = 256
MAX_SPOTS = 2_000_000


def _check_labels(groups, n, n_groups):
    """(labels or None, C or None): the checks of ``expression._check_groups`` with at most ``MAX_GROUPS`` groups."""
    if n_groups is not None and not isinstance(n_groups, (bool, np.bool_)) and isinstance(n_groups, (int, np.integer)) \
            and n_groups > MAX_GROUPS:
        raise ValueError(f"n_groups must be an int from 1 to {MAX_GROUPS}, got {n_groups!r}")
    labels, C = _check_groups(groups, n, n_groups)
    if C is not None and C > MAX_GROUPS:
        raise ValueError(f"at most {MAX_GROUPS} groups, got labels up to {C - 1}")
    return labels, C


def _check_pseudocount(pseudocount):
    if isinstance(pseudocount, (bool, np.bool_)) or not isinstance(pseudocount, (int, float, np.integer, np.floating)) \
            or not pseudocount >= 0 or not np.isfinite(pseudocount):
        raise ValueError(f"pseudocount must be a finite number >= 0, got {pseudocount!r}")
    return float(pseudocount)


def _check_max_sort_bytes(max_sort_bytes):
    if max_sort_bytes is None:
        return 0
    if isinstance(max_sort_bytes, (bool, np.bool_)) or not isinstance(max_sort_bytes, (int, np.integer)) or max_sort_bytes < 1:
        raise ValueError(f"max_sort_bytes must be an int >= 1 or None, got {max_sort_bytes!r}")
    return int(max_sort_bytes)


def check_request(Y_shape, groups=None, n_groups=None, pseudocount=1e-9, n_top=None):
    """What can be checked of a ``rank_genes_groups`` call from the shape of ``Y`` alone, before anything touches the GPU (and, for
    ``tl.deconvolve``, before the fit): ``ValueError`` on the first that fails; returns ``(labels or None, C or None)``."""
    if len(Y_shape) != 2 or Y_shape[1] < 1:
        raise ValueError(f"Y must be a 2-D (n_spots, n_genes) matrix with at least one gene, got shape {tuple(Y_shape)}")
    n = int(Y_shape[0])
    if n < 1:
        raise ValueError(f"Y must have at least one spot, got shape {tuple(Y_shape)}")
    if n > MAX_SPOTS:
        raise ValueError(f"marker genes are built for at most {MAX_SPOTS} spots, got {n}")
    labels, C = _check_labels(groups, n, n_groups)
    _check_pseudocount(pseudocount)
    _check_n_top(n_top)
    return labels, C


def _labels_on_device(labels, C, n, device):
    """(int32 device tensor (n,), C) - CUDA labels are checked here, the first thing the device does."""
    import torch
    if labels is None:
        return torch.zeros(max(n, 1), dtype=torch.int32, device=device), 1
    if _lib.is_cuda_tensor(labels):
        lab = labels.detach().to(device=device, dtype=torch.int64)
        lo, hi = (int(lab.min().item()), int(lab.max().item())) if n else (0, -1)
        if C is None:
            C = max(hi + 1, 1)
        if lo < -1 or hi >= C or C > MAX_GROUPS:
            raise ValueError(f"groups must lie in [-1, {C}) with at most {MAX_GROUPS} groups, got labels from {lo} to {hi}")
        return lab.to(torch.int32).contiguous(), C
    return torch.as_tensor(np.ascontiguousarray(labels, dtype=np.int32)).to(device), C


def _sums_device(Y, labels, C, n, G, max_sort_bytes):
    import torch
    _lib.require_gpu()
    lib = _lib.load()
    device = device_of(Y, labels)
    with torch.cuda.device(device):
        stream = _lib.current_stream(device)
        lab, C = _labels_on_device(labels, C, n, device)
        u = torch.empty((C, G), dtype=torch.float64, device=device)
        q = torch.empty((C, G), dtype=torch.float64, device=device)
        nnz = torch.empty((C, G), dtype=torch.int64, device=device)
        R2 = torch.empty((C, G), dtype=torch.int64, device=device)
        T = torch.empty(G, dtype=torch.int64, device=device)
        n_rows, n_used, info = np.zeros(C, dtype=np.int64), np.zeros(1, dtype=np.int64), np.zeros(3, dtype=np.int64)
        tail = (ctypes.c_void_p(lab.data_ptr()), C, max_sort_bytes, *(ctypes.c_void_p(t.data_ptr()) for t in (u, q, nnz, R2, T)),
                _lib.ptr_i64(n_rows), _lib.ptr_i64(n_used), _lib.ptr_i64(info), stream)
        with matrix_on_device(Y, device) as m:
            if m[0] == "csr":
                _lib.check(lib.fdx_gene_group_sums_csr_dev(ctypes.byref(m[1].view), *tail))
            else:
                _, ptr, code, ldy = m
                _lib.check(lib.fdx_gene_group_sums_dev(ptr, code, n, G, ldy, *tail))
        out = {name: _lib.tensor_to_host(t) for name, t in (("u", u), ("q", q), ("nnz", nnz), ("R2", R2), ("T", T))}
    out.update(n_rows=n_rows, n_used=int(n_used[0]), stripes=int(info[0]), stripe_entries=int(info[1]), workspace_bytes=int(info[2]))
    return out


def gene_group_sums(Y, groups, n_groups=None, max_sort_bytes=None):
    """The device half (module docstring): a dict of ``u``, ``q`` (C, G) float64, ``nnz``, ``R2`` (C, G) int64, ``T`` (G,) int64 -
    numpy - ``n_rows`` (C,) int64 and ``n_used``; beside them what the ranking took: ``stripes``, ``stripe_entries`` (the nonzeros
    of the largest) and ``workspace_bytes`` (its keys, payloads and sort workspace).  ``max_sort_bytes`` (None: about 1 GiB) bounds
    that workspace; it moves no bit of a result.  Everything checkable is checked before anything touches the GPU."""
    n, G = check_matrix(Y)
    labels, C = check_request((n, G), groups, n_groups)
    return _sums_device(Y, labels, C, n, G, _check_max_sort_bytes(max_sort_bytes))


def _ratio(a, b, ok):
    """``a / b`` where ``ok``, NaN elsewhere."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ok, a / np.where(ok, b, 1.0), np.nan)


def assemble_group_tests(n_rows, u, q, nnz, R2, T, pseudocount=1e-9):
    """The statistics of the module docstring from the sums of one call (pure host arithmetic, float64): a dict of ``mean``,
    ``mean_rest``, ``var``, ``var_rest``, ``pct``, ``pct_rest``, ``log2_fold_change``, ``t``, ``t_dof``, ``t_p_value``,
    ``t_q_value``, ``auc``, ``z_score``, ``p_value``, ``q_value`` (C, G) and ``order`` (C, G) int64."""
    from scipy.special import erfc, stdtr
    pseudocount = _check_pseudocount(pseudocount)
    n_rows = np.asarray(n_rows, dtype=np.int64)
    u, q = np.asarray(u, dtype=np.float64), np.asarray(q, dtype=np.float64)
    nnz, R2, T = np.asarray(nnz, dtype=np.int64), np.asarray(R2, dtype=np.int64), np.asarray(T, dtype=np.int64)
    if u.ndim != 2 or n_rows.shape != (u.shape[0],) or any(a.shape != u.shape for a in (q, nnz, R2)) or T.shape != (u.shape[1],):
        raise ValueError(f"n_rows (C,), u, q, nnz, R2 (C, G) and T (G,) are required, got shapes "
                         f"{[a.shape for a in (n_rows, u, q, nnz, R2, T)]}")
    C, G = u.shape
    N = int(n_rows.sum())
    u_tot, q_tot, nnz_tot = np.zeros(G), np.zeros(G), np.zeros(G, dtype=np.int64)
    for c in range(C):                                        # the totals: over c in ascending order
        u_tot, q_tot, nnz_tot = u_tot + u[c], q_tot + q[c], nnz_tot + nnz[c]
    nc = n_rows.astype(np.float64)[:, None] + np.zeros((1, G))
    nr = float(N) - nc
    u_r, q_r, nnz_r = u_tot[None, :] - u, q_tot[None, :] - q, nnz_tot[None, :] - nnz

    def moments(s1, s2, cnt):
        mean = _ratio(s1, cnt, cnt >= 1)
        var = _ratio(np.maximum(0.0, s2 - _ratio(s1 * s1, cnt, cnt >= 1)), cnt - 1.0, cnt >= 2)
        return mean, var
    mean, var = moments(u, q, nc)
    mean_r, var_r = moments(u_r, q_r, nr)
    both = (nc >= 1) & (nr >= 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        lfc = np.where(both, np.log2((mean + pseudocount) / (mean_r + pseudocount)), np.nan)
        a, b = var / nc, var_r / nr
        den = a + b
        t_ok = both & np.isfinite(den) & (den > 0)
        t = _ratio(mean - mean_r, np.sqrt(np.where(t_ok, den, 1.0)), t_ok)
        dof = _ratio(den * den, a * a / (nc - 1.0) + b * b / (nr - 1.0), t_ok)
        t_p = np.where(t_ok, 2.0 * stdtr(np.where(t_ok, dof, 1.0), -np.abs(np.where(t_ok, t, 0.0))), np.nan)
        # Wilcoxon: the tie term from the exact integer N^3 - N - T >= 0 (N <= 2 000 000: below 2^63)
        spread = np.array([N * N * N - N - int(v) for v in T.tolist()], dtype=np.float64)
        sigma2 = nc * nr / 12.0 * (spread[None, :] / (float(N) * float(N - 1)) if N >= 2 else np.zeros((1, G)))
        U = R2.astype(np.float64) / 2.0 - nc * (nc + 1.0) / 2.0
        auc = _ratio(U, nc * nr, both)
        z_ok = both & (sigma2 > 0)
        z = _ratio(U - nc * nr / 2.0, np.sqrt(np.where(z_ok, sigma2, 1.0)), z_ok)
        p = np.where(z_ok, erfc(np.abs(np.where(z_ok, z, 0.0)) / np.sqrt(2.0)), np.nan)
    return {"mean": mean, "mean_rest": mean_r, "var": var, "var_rest": var_r, "pct": _ratio(nnz.astype(np.float64), nc, nc >= 1),
            "pct_rest": _ratio(nnz_r.astype(np.float64), nr, nr >= 1), "log2_fold_change": lfc, "t": t, "t_dof": dof, "t_p_value": t_p,
            "t_q_value": np.stack([_benjamini_hochberg(t_p[c]) for c in range(C)]) if C else t_p.copy(), "auc": auc, "z_score": z,
            "p_value": p, "q_value": np.stack([_benjamini_hochberg(p[c]) for c in range(C)]) if C else p.copy(),
            "order": np.stack([_decreasing_order(z[c]) for c in range(C)]) if C else np.zeros((0, G), dtype=np.int64)}


def rank_genes_groups(Y, groups, n_groups=None, pseudocount=1e-9, n_top=None, output="numpy"):
    """Which genes mark each group of spots: per group and gene the Wilcoxon rank-sum test and the Welch t test of the group
    against all other used spots, with effect sizes, Benjamini-Hochberg q values and the ranking (module docstring).

    ``Y``: (n_spots, n_genes) - dense numpy / CUDA tensor, float32, float64 or integer counts, or CSR (scipy, CUDA
    ``torch.sparse_csr``); tested as it is passed (not normalised).  ``groups``: (n_spots,) integer labels in ``[-1, n_groups)``,
    ``-1`` = left out (``n_groups`` None: the largest label + 1; at most 256).  ``pseudocount``: added to both means of the fold
    change.  ``n_top``: also return ``top = order[:, :n_top]``.  ``output``: ``"numpy"``, or ``"torch"`` for CUDA tensors on the
    device of the call.  Arguments are checked before anything touches the GPU (``ValueError``).

    Returns a dict: ``z_score``, ``auc``, ``p_value``, ``q_value``, ``t``, ``t_dof``, ``t_p_value``, ``t_q_value``,
    ``log2_fold_change``, ``mean``, ``mean_rest``, ``var``, ``var_rest``, ``pct``, ``pct_rest`` (C, G) float64, ``order`` (C, G)
    int64, the sums ``u``, ``q``, ``nnz``, ``R2`` (C, G) and ``T`` (G,), ``n_rows`` (C,) int64 and ``n_used``."""
    if output not in ("numpy", "torch"):
        raise ValueError(f"Unknown output: {output}. Choose from 'numpy', 'torch'.")
    n, G = check_matrix(Y)
    labels, C = check_request((n, G), groups, n_groups, pseudocount, n_top)
    s = _sums_device(Y, labels, C, n, G, 0)
    out = assemble_group_tests(s["n_rows"], s["u"], s["q"], s["nnz"], s["R2"], s["T"], pseudocount)
    out.update({k: s[k] for k in ("u", "q", "nnz", "R2", "T", "n_rows")})
    if n_top is not None:
        out["top"] = out["order"][:, :n_top]
    if output == "torch":
        import torch
        device = device_of(Y, labels)
        out = {k: torch.as_tensor(np.ascontiguousarray(v)).to(device) for k, v in out.items()}
    out["n_used"] = s["n_used"]
    return out
