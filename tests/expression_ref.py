"""NumPy definition of the cell-type expression statistics (flashdeconv_amd/utils/expression.py) and the cases its tests use.

**Inputs.**  ``Y`` is (n, G) dense or scipy CSR.  ``W`` is (n, K) float64, finite and non-negative, 1 <= K <= 272.  ``groups`` is
optional: (n,) integers in ``[-1, C)``; ``-1`` leaves a spot out; ``None`` means one group of all rows.  Scalars: ``ridge >= 0``,
``max_iter >= 1``, ``tol > 0``.

**Sums.**  For each group c, with its rows R_c taken in ascending row index, everything in float64::

    n_c    = |R_c|
    A_c    = sum_i w_i w_i'            (K, K)
    B_c    = sum_i w_i y_i'            (K, G)
    q_c[g] = sum_i y_ig^2      u_c[g] = sum_i y_ig

**Solve.**  For each (c, g), with ``D_k = A_c[k,k] + ridge * mean(diag A_c)`` (the diagonal added in ascending k, divided by K) and
``b = B_c[:, g]``, cyclic coordinate descent from ``s = 0``::

    for it = 1 .. max_iter:
        dmax = 0
        for k = 0 .. K-1:
            new  = max(0, (b_k - sum_{j != k} A_c[k,j] s_j) / D_k)   if D_k > 0 else 0
            dmax = max(dmax, |new - s_k|);  s_k = new
        if dmax <= tol * max_k s_k: converged, stop        (all-zero s: 0 <= 0, converged)

**Outputs.**  ``expression`` (C, K, G);  ``rss = max(0, q - 2 s.b + s' A_c s)`` with ``A_c`` without the ridge;
``tss = max(0, q - u^2 / n_c)`` (0 for an empty group);  ``r2 = 1 - rss / tss``, NaN where ``tss == 0``;  ``n_iter`` (C, G) int32;
``converged`` (C, G) bool;  ``gram`` (C, K, K), ``n_rows`` (C,);  ``estimable`` (C, K) = ``A_c[k,k] > 0``.  With ``groups=None``
the leading C axis is dropped.

The device may keep the running gradient ``A s - b``; its iterates then agree with these up to rounding (the GPU tests allow for
that), while the sums of the exact cases below are exactly representable in any order and must be EQUAL.
"""
import numpy as np

EPS = np.finfo(np.float64).eps


def _dense(Y):
    return np.asarray(Y.toarray() if hasattr(Y, "toarray") else Y, dtype=np.float64)


def sums(Y, W, groups=None, n_groups=None):
    """A (C, K, K), B (C, K, G), q, u (C, G), n_rows (C,) by the definition above (the C axis kept)."""
    Y, W = _dense(Y), np.asarray(W, dtype=np.float64)
    n, G = Y.shape
    K = W.shape[1]
    if groups is None:
        groups, C = np.zeros(n, dtype=np.int64), 1
    else:
        groups = np.asarray(groups).astype(np.int64)
        C = int(n_groups) if n_groups is not None else max(int(groups.max()) + 1, 1) if n else 1
    A, B, q, u = np.zeros((C, K, K)), np.zeros((C, K, G)), np.zeros((C, G)), np.zeros((C, G))
    n_rows = np.zeros(C, dtype=np.int64)
    for c in range(C):
        rows = np.flatnonzero(groups == c)
        n_rows[c] = rows.size
        Wc, Yc = W[rows], Y[rows]
        A[c], B[c], q[c], u[c] = Wc.T @ Wc, Wc.T @ Yc, (Yc * Yc).sum(axis=0), Yc.sum(axis=0)
    return A, B, q, u, n_rows


def ridge_diagonal(A, ridge):
    """D_k: the diagonal added in ascending k, divided by K, times ridge, added to A_kk."""
    K = A.shape[0]
    dsum = 0.0
    for k in range(K):
        dsum += A[k, k]
    return np.diag(A) + ridge * (dsum / K)


def coordinate_descent(A, B, ridge=0.0, max_iter=10000, tol=1e-10):
    """The solve of every column of B (K, G) against one A (K, K): S (K, G), n_iter (G,) int32, converged (G,) bool.  Columns
    that have converged are frozen; the others go on - each column sees exactly the loop of the definition."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    K, G = B.shape
    D = ridge_diagonal(A, ridge)
    Aoff = A.copy()
    np.fill_diagonal(Aoff, 0.0)                       # sum over j != k
    S = np.zeros((K, G))
    n_iter = np.full(G, max_iter, dtype=np.int32)
    conv = np.zeros(G, dtype=bool)
    act = np.arange(G)
    for it in range(1, max_iter + 1):
        Sa, Ba = S[:, act], B[:, act]
        dmax = np.zeros(act.size)
        for k in range(K):
            if D[k] > 0:
                new = np.maximum(0.0, (Ba[k] - Aoff[k] @ Sa) / D[k])
            else:
                new = np.zeros(act.size)
            dmax = np.maximum(dmax, np.abs(new - Sa[k]))
            Sa[k] = new
        S[:, act] = Sa
        done = dmax <= tol * Sa.max(axis=0)
        n_iter[act[done]] = it
        conv[act[done]] = True
        act = act[~done]
        if act.size == 0:
            break
    return S, n_iter, conv


def residuals(A, B, q, u, n_rows, S):
    """rss, tss, r2 (G,) of one group from its sums and S (K, G)."""
    sb = np.einsum("kg,kg->g", S, B)
    sas = np.einsum("kg,kg->g", S, A @ S)
    rss = np.maximum(0.0, q - 2.0 * sb + sas)
    tss = np.maximum(0.0, q - (u * u) / n_rows) if n_rows > 0 else np.zeros_like(q)
    with np.errstate(divide="ignore", invalid="ignore"):
        r2 = np.where(tss > 0, 1.0 - rss / np.where(tss > 0, tss, 1.0), np.nan)
    return rss, tss, r2


def rss_scale(A, B, q, S):
    """q + 2 |s|.|b| + |s|' |A| |s| per gene: what the rounding of rss is measured against."""
    aS = np.abs(S)
    return q + 2.0 * np.einsum("kg,kg->g", aS, np.abs(B)) + np.einsum("kg,kg->g", aS, np.abs(A) @ aS)


def celltype_expression(Y, W, groups=None, n_groups=None, ridge=0.0, max_iter=10000, tol=1e-10):
    """Everything the module returns, by the definition."""
    A, B, q, u, n_rows = sums(Y, W, groups, n_groups)
    C, K, G = B.shape
    out = {"expression": np.zeros((C, K, G)), "rss": np.zeros((C, G)), "tss": np.zeros((C, G)), "r2": np.zeros((C, G)),
           "n_iter": np.zeros((C, G), dtype=np.int32), "converged": np.zeros((C, G), dtype=bool), "gram": A, "n_rows": n_rows,
           "estimable": np.stack([np.diag(A[c]) > 0 for c in range(C)])}
    for c in range(C):
        S, n_it, cv = coordinate_descent(A[c], B[c], ridge, max_iter, tol)
        out["expression"][c], out["n_iter"][c], out["converged"][c] = S, n_it, cv
        out["rss"][c], out["tss"][c], out["r2"][c] = residuals(A[c], B[c], q[c], u[c], n_rows[c], S)
    if groups is None:
        out = {k: v[0] for k, v in out.items()}
    return out


def kkt(A, B, S, tol):
    """(gradient A s - b, bound) (K, G) each: the bound is sum_j |A_kj| tol max(s) + 4 K eps (|A| |s| + |b|)_k.  Where s_k > 0 the
    stopping rule leaves |gradient_k| <= bound (each later update of the last sweep moves s_j by at most tol max(s)); where
    s_k = 0, gradient_k >= -bound."""
    K = A.shape[0]
    grad = A @ S - B
    bound = np.abs(A).sum(axis=1)[:, None] * (tol * S.max(axis=0))[None, :] + 4 * K * EPS * (np.abs(A) @ np.abs(S) + np.abs(B))
    return grad, bound


def kkt_worst(A, B, S, tol):
    """The largest violation over the bound (<= 1 passes): |gradient| / bound where s > 0, -gradient / bound where s = 0."""
    grad, bound = kkt(A, B, S, tol)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(S > 0, np.abs(grad), np.maximum(-grad, 0.0)) / bound
    ratio = np.where(bound > 0, ratio, np.where(np.where(S > 0, np.abs(grad), np.maximum(-grad, 0.0)) > 0, np.inf, 0.0))
    return float(ratio.max())


# ------------------------------------------------------------------------------------------------------------------ cases
def dyadic_weights(n, K, seed, one_hot=False):
    """Weights in sixteenths, 0 .. 1, about a third of them zero (one_hot: one non-zero per row)."""
    rs = np.random.RandomState(seed)
    W = rs.randint(0, 17, size=(n, K)).astype(np.float64) / 16.0
    W[rs.rand(n, K) < 0.3] = 0.0
    if one_hot:
        keep = np.zeros((n, K), dtype=bool)
        keep[np.arange(n), rs.randint(0, K, size=n)] = True
        W = np.where(keep, np.maximum(W, 1.0 / 16.0), 0.0)
    return W


def integer_counts(n, G, seed, density=1.0, dtype=np.float32):
    """Small integers 0 .. 7 (density < 1: that share of the entries kept)."""
    rs = np.random.RandomState(seed + 1000)
    Y = rs.randint(0, 8, size=(n, G))
    if density < 1.0:
        Y = Y * (rs.rand(n, G) < density)
    return Y.astype(dtype)


def group_labels(n, kind, seed):
    """(labels or None, C): "none"; "three" (C = 3, about a fifth of the rows -1); "empty" (C = 4, group 2 has no row); "single"
    (C = 3, group 1 is one row)."""
    rs = np.random.RandomState(seed + 2000)
    if kind == "none":
        return None, None
    if kind == "three":
        g = rs.randint(0, 3, size=n)
        g[rs.rand(n) < 0.2] = -1
        return g.astype(np.int64), 3
    if kind == "empty":
        g = rs.choice([0, 1, 3], size=n)
        return g.astype(np.int64), 4
    if kind == "single":
        g = rs.choice([0, 2], size=n)
        g[n // 2] = 1
        return g.astype(np.int64), 3
    raise ValueError(kind)


def generic_case(n, G, K, seed, alpha=0.5, depth=20.0):
    """Dirichlet(alpha) weights and Poisson counts of a non-negative mixture: (Y float64, W)."""
    rs = np.random.RandomState(seed)
    W = rs.dirichlet(np.full(K, alpha), size=n)
    sig = rs.gamma(0.7, 1.0, size=(K, G)) * depth
    Y = rs.poisson(W @ sig).astype(np.float64)
    return Y, W


# (n, G, K, seed) of the generic solve cases of tests/test_gpu_expression.py; tests/test_expression_host.py asserts that every gene
# of every one converges in the reference within GENERIC_MAX_ITER at both tolerances
GENERIC_CASES = [(300, 40, 5, 1), (600, 48, 30, 2), (700, 40, 33, 3), (1200, 36, 65, 4), (2200, 36, 130, 5)]
GENERIC_TOLS = (1e-6, 1e-10)
GENERIC_MAX_ITER = 10000
GENERIC_GROUPS_CASE = (900, 40, 6, 7)           # solved per group with group_labels(n, "three", 7)
RIDGE_CASE = (400, 40, 12, 8, 0.05)             # ... and ridge
