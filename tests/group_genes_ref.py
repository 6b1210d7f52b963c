"""NumPy / scipy reference of the marker-gene sums and tests (flashdeconv_amd/utils/group_genes.py): twice-midranks from
``scipy.stats.rankdata(method="average")`` per column over the used rows, the tests from ``scipy.stats.mannwhitneyu(method=
"asymptotic", use_continuity=False)`` and ``scipy.stats.ttest_ind(equal_var=False)`` - group c against all other used rows."""
import numpy as np
from scipy import stats


def dense64(Y):
    """Y as a dense float64 array: every storage type converts exactly (float32, integer counts, scipy sparse)."""
    if hasattr(Y, "toarray"):
        Y = Y.toarray()
    return np.asarray(Y, dtype=np.float64)


def sums(Y, groups, C):
    """The integer planes and the counts as the device defines them: nnz, R2 (C, G) int64, T (G,) int64, n_rows (C,) int64, N.
    Sums of u and q are not made here: the device's are held bitwise to ``weighted_gene_sums``."""
    Y = dense64(Y)
    n, G = Y.shape
    groups = np.zeros(n, dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64)
    used = groups >= 0
    Yu, gu = Y[used], groups[used]
    N = int(used.sum())
    nnz, R2 = np.zeros((C, G), dtype=np.int64), np.zeros((C, G), dtype=np.int64)
    T = np.zeros(G, dtype=np.int64)
    n_rows = np.bincount(gu, minlength=C).astype(np.int64)
    for g in range(G):
        col = Yu[:, g]
        twice = np.rint(2.0 * stats.rankdata(col, method="average")).astype(np.int64) if N else np.zeros(0, dtype=np.int64)
        _, t = np.unique(col, return_counts=True)           # -0.0 == 0.0: one run
        T[g] = int(sum(int(v) ** 3 - int(v) for v in t))
        for c in range(C):
            mine = gu == c
            R2[c, g] = twice[mine].sum()
            nnz[c, g] = np.count_nonzero(col[mine])
    return {"nnz": nnz, "R2": R2, "T": T, "n_rows": n_rows, "n_used": N}


def float_sums(Y, groups, C):
    """u, q (C, G) float64 by plain NumPy sums (for the host tests, which need sums to assemble from, not bits)."""
    Y = dense64(Y)
    groups = np.zeros(Y.shape[0], dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64)
    u = np.stack([Y[groups == c].sum(axis=0) for c in range(C)])
    q = np.stack([(Y[groups == c] ** 2).sum(axis=0) for c in range(C)])
    return u, q


def scipy_tests(Y, groups, C):
    """p_value, z_sign (the sign of U - n_c n_r / 2), auc, t, t_dof, t_p_value (C, G) from scipy, group c against the other used
    rows; NaN where scipy cannot form a statistic (an empty side) or reports NaN (a constant gene).  scipy returns no z: the
    two-sided p value is a one-to-one function of |z|, the sign is held beside it."""
    Y = dense64(Y)
    n, G = Y.shape
    groups = np.zeros(n, dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64)
    out = {k: np.full((C, G), np.nan) for k in ("z_sign", "p_value", "auc", "t", "t_dof", "t_p_value")}
    for c in range(C):
        x, y = Y[groups == c], Y[(groups >= 0) & (groups != c)]
        n1, n2 = x.shape[0], y.shape[0]
        if n1 < 1 or n2 < 1:
            continue
        for g in range(G):
            with np.errstate(all="ignore"):
                r = stats.mannwhitneyu(x[:, g], y[:, g], method="asymptotic", use_continuity=False, alternative="two-sided")
            out["auc"][c, g] = r.statistic / (n1 * n2)
            if np.isfinite(r.pvalue) and np.ptp(np.concatenate([x[:, g], y[:, g]])) > 0:
                out["p_value"][c, g] = r.pvalue
                out["z_sign"][c, g] = np.sign(r.statistic - n1 * n2 / 2.0)
            if n1 >= 2 and n2 >= 2:
                with np.errstate(all="ignore"):
                    w = stats.ttest_ind(x[:, g], y[:, g], equal_var=False)
                if np.isfinite(w.statistic):
                    out["t"][c, g], out["t_p_value"][c, g], out["t_dof"][c, g] = w.statistic, w.pvalue, w.df
    return out


def expression_like(n, G, seed, density=0.1, dtype=np.float32):
    """A mostly-zero non-negative matrix with ties among the nonzeros (small counts), as expression matrices are."""
    rs = np.random.RandomState(seed)
    Y = rs.poisson(3.0, size=(n, G)).astype(np.float64) * (rs.random_sample((n, G)) < density)
    return Y.astype(dtype)
