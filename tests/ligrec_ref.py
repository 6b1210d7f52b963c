"""NumPy reference of the ligand-receptor test between spot groups (utils.ligrec, csrc/label_gene_kernels.cpp), written
independently of the package's host code: the sums by ``Y[l^r == c].sum(0)`` on float64, the statistic with the same three
operations (one division per mean, one addition, one multiplication by 0.5), the accumulation permutation after permutation, and
the host statistics spelled out entry by entry."""
import numpy as np

from flashdeconv_amd.utils.spatial_stats import permutation_indices


def dense64(Y):
    """``Y`` (numpy, scipy sparse, torch dense or sparse CSR) as a host float64 array, every value converted from its storage."""
    if hasattr(Y, "toarray"):
        Y = Y.toarray()
    elif hasattr(Y, "to_dense"):
        import torch
        Y = (Y if Y.layout == torch.strided else Y.to_dense()).cpu().numpy()
    return np.asarray(Y).astype(np.float64)


def gene_list(pairs):
    return np.unique(np.asarray(pairs)).astype(np.int64)


def label_counts(labels, C):
    labels = np.asarray(labels)
    return np.array([(labels == c).sum() for c in range(C)], dtype=np.int64)


def group_sums(Yg, labels, C):
    """u (C, S): ``Yg[labels == c].sum(0)`` of the float64 columns ``Yg`` (n, S)."""
    return np.stack([Yg[labels == c].sum(axis=0) if (labels == c).any() else np.zeros(Yg.shape[1]) for c in range(C)])


def group_nnz(Yg, labels, C):
    return np.stack([(Yg[labels == c] != 0).sum(axis=0) for c in range(C)]).astype(np.int64)


def abs_sums(Yg, labels, C):
    """sum_{i in c} |y| per (c, s): the scale of the rounding bound of u."""
    return group_sums(np.abs(Yg), labels, C)


def null_sums(Yg, labels, C, seed, first, R):
    """(R, C, S): the sums of the labels ``labels[permutation_indices(seed, r, n)]``, r = first .. first + R - 1."""
    labels = np.asarray(labels)
    n = labels.shape[0]
    out = np.zeros((R, C, Yg.shape[1]))
    for k in range(R):
        out[k] = group_sums(Yg, labels[permutation_indices(seed, first + k, n)], C)
    return out


def statistic(u, counts, pairs, genes):
    """T (P, C, C) of sums u (C, S): (u[a, lig] / n_a + u[b, rec] / n_b) * 0.5; NaN where n_a or n_b is 0."""
    slot = {int(g): s for s, g in enumerate(genes)}
    P, C = len(pairs), u.shape[0]
    T = np.full((P, C, C), np.nan)
    for p, (lig, rec) in enumerate(np.asarray(pairs).tolist()):
        for a in range(C):
            for b in range(C):
                if counts[a] >= 1 and counts[b] >= 1:
                    ma = np.float64(u[a, slot[lig]]) / np.float64(counts[a])
                    mb = np.float64(u[b, slot[rec]]) / np.float64(counts[b])
                    T[p, a, b] = (ma + mb) * np.float64(0.5)
    return T


def statistic_fast(u, counts, pairs, genes):
    """``statistic`` vectorised for the large cases (the same three operations elementwise)."""
    slot = np.searchsorted(genes, np.asarray(pairs))
    nc = counts.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = u / nc[:, None]
        T = (m[:, slot[:, 0]].T[:, :, None] + m[:, slot[:, 1]].T[:, None, :]) * 0.5
    ok = (counts >= 1)[None, :, None] & (counts >= 1)[None, None, :]
    return np.where(ok, T, np.nan)


def accumulate(null_T, T):
    """(count_ge, count_le, sum_d, sumsq_d, sum_abs_d) over the permutations in order; nothing counted or added where T is NaN."""
    ge, le = np.zeros(T.shape, dtype=np.int64), np.zeros(T.shape, dtype=np.int64)
    sd, sq, sa = np.zeros(T.shape), np.zeros(T.shape), np.zeros(T.shape)
    live = ~np.isnan(T)
    for Tr in null_T:
        d = np.where(live, Tr - T, 0.0)
        ge += live & (Tr >= T)
        le += live & (Tr <= T)
        sd = sd + d
        sq = sq + d * d
        sa = sa + np.abs(d)
    return ge, le, sd, sq, sa


def bh(p):
    """Benjamini-Hochberg over the entries that are not NaN, by the textbook loop."""
    flat = p.ravel()
    q = np.full(flat.shape, np.nan)
    idx = [i for i in range(flat.size) if not np.isnan(flat[i])]
    idx.sort(key=lambda i: (flat[i], i))
    m = len(idx)
    running = 1.0
    for rank in range(m, 0, -1):
        i = idx[rank - 1]
        running = min(running, flat[i] * (float(m) / rank))
        q[i] = min(1.0, running)
    return q.reshape(p.shape)


def host_statistics(pairs, genes, u, nnz, counts, ge, le, sd, sq, R, threshold=0.01):
    """The keys of ``assemble_ligrec``, entry by entry."""
    pairs = np.asarray(pairs)
    slot = {int(g): s for s, g in enumerate(genes)}
    P, C = len(pairs), u.shape[0]
    T = statistic(u, counts, pairs, genes)
    pct = np.full(u.shape, np.nan)
    for c in range(C):
        if counts[c] >= 1:
            pct[c] = nnz[c].astype(np.float64) / np.float64(counts[c])
    expressed = np.zeros((P, C, C), dtype=bool)
    out = {k: np.full((P, C, C), np.nan) for k in ("p_greater", "p_less", "p_value", "null_mean", "null_std", "z_sim")}
    for p, (lig, rec) in enumerate(pairs.tolist()):
        for a in range(C):
            for b in range(C):
                if counts[a] < 1 or counts[b] < 1:
                    continue
                expressed[p, a, b] = pct[a, slot[lig]] >= threshold and pct[b, slot[rec]] >= threshold
                if not expressed[p, a, b] or R < 1:
                    continue
                g = (1.0 + ge[p, a, b]) / (R + 1.0)
                l = (1.0 + le[p, a, b]) / (R + 1.0)
                mean_d = sd[p, a, b] / np.float64(R)
                var = max(sq[p, a, b] / np.float64(R) - mean_d * mean_d, 0.0)
                std = np.sqrt(var)
                out["p_greater"][p, a, b], out["p_less"][p, a, b] = g, l
                out["p_value"][p, a, b] = min(1.0, 2.0 * min(g, l))
                out["null_mean"][p, a, b] = T[p, a, b] + mean_d
                out["null_std"][p, a, b] = std
                out["z_sim"][p, a, b] = -mean_d / std if std > 0 else np.nan
    flat_p = np.where(np.isnan(out["p_greater"]), np.inf, out["p_greater"]).ravel()
    flat_m = np.where(np.isnan(T), -np.inf, T).ravel()
    order = sorted(range(flat_p.size), key=lambda i: (flat_p[i], -flat_m[i], i))
    res = {"means": T, "pct": pct, "expressed": expressed,
           "order": np.array([np.unravel_index(i, (P, C, C)) for i in order], dtype=np.int64).reshape(-1, 3)}
    if R >= 1:
        res.update(out)
        res["q_value"] = bh(out["p_greater"])
        res["n_permutations"] = R
    return res
