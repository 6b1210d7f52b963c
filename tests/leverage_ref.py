"""Reference, yardstick and cases for the leverage-score tests (tests/test_leverage_host.py, tests/test_gpu_leverage.py).
numpy only; no GPU.

exact(X, reg)     utils/genes.py:238-290 in np.longdouble without an SVD: centre over the cell types, Householder QR of
                  [Xc^T ; sqrt(reg) I_K] (G + K rows, K columns), raw_g = squared norm of row g of Q, lev = raw / (sum raw + reg).
                  With Xc^T = U S V^T, row g of Q has squared norm sum_j U_gj^2 s_j^2 / (s_j^2 + reg): the reference's formula (a
                  centred gene has no component along the null direction that centring creates, so that direction adds nothing).
kappa(X, reg)     sqrt(s_1^2 + reg) / sqrt(s_r^2 + reg), s = float64 svd(Xc), r = min(K, G) - 1: the condition of the
                  ridge-augmented matrix once the centring null direction is removed - what the device factorises.
unit(lev, kappa)  u kappa sqrt(l_g l_max) + (u kappa)^2 l_max, u = 2^-53: the first-order change of a row's squared norm in Q under
                  a backward error of one unit roundoff (dl = 2 q dq + dq^2); the second term is the floor of a gene whose exact
                  score is 0.
bound(...)        M * L * unit per gene, never above the hard ceiling 2e-8 max(1, kappa / 1e4) |lev| + 1e-15 that the older tests
                  of tests/test_gpu_fit.py accept.  L is LAPACK's own largest error in units over the cases below
                  (test_leverage_host.py measures it and pins the constant); M = 8 is the margin of tests/test_gpu_leverage.py.

The cases are K x G matrices with prescribed singular values of the CENTRED matrix (right vectors orthogonal to the ones
vector), centred entries of r.m.s. 8 and a per-gene offset in [5, 35] that centring removes: values of order 1 - 50.
"""
import functools
from collections import namedtuple

import numpy as np

assert np.finfo(np.longdouble).eps < 1.1e-19, "the reference needs the x87 80-bit long double"

LD = np.longdouble
U53 = 2.0 ** -53
L_LAPACK = 48.0           # pinned by test_leverage_host.py::test_lapack_ratio_over_the_gpu_cases
M_DEVICE = 8.0
STRIPE = 64               # LEV_STRIPE of csrc/leverage_kernels.cpp
PIVOT_TOL = 1e-9          # LEV_PIVOT_TOL


# ---------------------------------------------------------------------------------------------------- reference
def exact(X, reg=1e-6):
    X = np.asarray(X, dtype=np.float64).astype(LD)
    K, G = X.shape
    if K == 1:
        return np.zeros(G, dtype=LD)
    A = np.empty((G + K, K), dtype=LD)
    A[:G] = (X - X.sum(axis=0) / LD(K)).T
    A[G:] = np.sqrt(LD(reg)) * np.eye(K, dtype=LD)
    vs = []
    for j in range(K):
        v = A[j:, j].copy()
        nx = np.sqrt(v @ v)
        v[0] += nx if v[0] >= 0 else -nx
        v /= np.sqrt(v @ v)                                      # (the ridge rows keep every column away from zero)
        A[j:, j:] -= np.outer(v + v, v @ A[j:, j:])
        vs.append(v)
    Q = np.zeros((G + K, K), dtype=LD)
    Q[:K] = np.eye(K, dtype=LD)
    for j in reversed(range(K)):
        v = vs[j]
        Q[j:, j:] -= np.outer(v + v, v @ Q[j:, j:])
    raw = (Q[:G] * Q[:G]).sum(axis=1)
    return raw / (raw.sum() + LD(reg))


def kappa(X, reg=1e-6):
    X = np.asarray(X, dtype=np.float64)
    r = min(X.shape) - 1
    if r < 1:
        return 1.0
    s = np.linalg.svd(X - X.mean(axis=0, keepdims=True), compute_uv=False)
    return float(np.sqrt(s[0] ** 2 + reg) / np.sqrt(s[r - 1] ** 2 + reg))


def unit(lev, kap):
    lev = np.abs(np.asarray(lev, dtype=np.float64))
    lmax = lev.max() if lev.size else 0.0
    return U53 * kap * np.sqrt(lev * lmax) + (U53 * kap) ** 2 * lmax


def ceiling(lev, kap):
    return 2e-8 * max(1.0, kap / 1e4) * np.abs(np.asarray(lev, dtype=np.float64)) + 1e-15


def bound(lev, kap, margin=M_DEVICE):
    return np.minimum(margin * L_LAPACK * unit(lev, kap), ceiling(lev, kap))


# ---------------------------------------------------------------------------------------------------- cases
# kind: "spread" (param = s_1 / s_last of the centred matrix), "kappa" (param = kappa() of the result), "twins" (rows 5 = 2,
# 7 = mean of 2 and 3), "zero_row", "all_equal", "const_gene", "tiny_gene", "huge_gene", "scaled" (param = factor on X),
# "wide" (spread 30 with centred r.m.s. = param instead of 8)
Case = namedtuple("Case", "K G kind param reg")
Case.__new__.__defaults__ = ("spread", 30.0, 1e-6)
Case.id = property(lambda c: f"{c.K}x{c.G}-{c.kind}{c.param:g}-reg{c.reg:g}")


def _base(K, G, spread, seed, reg=1e-6, as_kappa=False, rms=8.0):
    rs = np.random.RandomState(seed)
    r = min(K - 1, G)
    offset = 5.0 + 30.0 * rs.rand(1, G)
    if r < 1:
        return np.ascontiguousarray(np.repeat(offset, K, axis=0))
    U, _ = np.linalg.qr(rs.randn(G, r))
    B = rs.randn(K, r)
    B -= B.mean(axis=0, keepdims=True)                           # right vectors orthogonal to the ones vector
    V, _ = np.linalg.qr(B)
    s = np.geomspace(1.0, 1.0 / spread, r)
    s *= rms * np.sqrt(K * G / np.sum(s * s))
    if as_kappa and r > 1:                                       # (s_1^2 + reg) / (s_r'^2 + reg) = spread^2 at r' = min(K, G) - 1
        rr = min(min(K, G) - 1, r)
        last = np.sqrt(max((s[0] ** 2 + reg) / spread ** 2 - reg, 0.0))
        s[:rr] = np.geomspace(s[0], last, rr)
        s[rr:] = last
    return np.ascontiguousarray(((U * s) @ V.T).T + offset)


@functools.lru_cache(maxsize=None)
def matrix(case):
    K, G, kind, param = case.K, case.G, case.kind, case.param
    seed = 1000 * K + G
    if kind == "spread":
        X = _base(K, G, param, seed)
    elif kind == "kappa":
        X = _base(K, G, param, seed, case.reg, as_kappa=True)
    elif kind == "scaled":
        X = _base(K, G, 30.0, seed) * param
    elif kind == "wide":
        X = _base(K, G, 30.0, seed, rms=param)
    elif kind in ("twins", "zero_row"):
        X = np.random.RandomState(seed).gamma(2.0, 6.0, size=(K, G)) + 1.0
        if kind == "twins":
            X[5] = X[2]
            X[7] = 0.5 * (X[2] + X[3])
        else:
            X[3] = 0.0
    elif kind == "all_equal":                                    # dyadic values: K v / K == v exactly, every centred entry is 0
        X = np.repeat(np.random.RandomState(seed).randint(8, 400, size=(1, G)) / 8.0, K, axis=0)
    else:
        X = _base(K, G, 30.0, seed)
        g = G // 3
        if kind == "const_gene":
            X[:, g] = 13.625                                     # dyadic: centred to exactly 0 in any arithmetic
        elif kind == "tiny_gene":
            X[:, g] *= 1e-9
        elif kind == "huge_gene":
            X[:, g] *= 1e3
        else:
            raise ValueError(kind)
    X = np.ascontiguousarray(X, dtype=np.float64)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def evaluate(case):
    """dict(exact float64 (rounded once from the long double), kappa, unit) - computed once per case, read-only"""
    X = matrix(case)
    ex = np.asarray(exact(X, case.reg), dtype=np.float64)
    ex[ex < 1e-30] = 0.0            # the long double's own floor, (2^-64)^2 / reg: a gene that centres to exactly 0 scores exactly 0
    kap = kappa(X, case.reg)
    un = unit(ex, kap)
    for a in (ex, un):
        a.setflags(write=False)
    return dict(exact=ex, kappa=kap, unit=un)


def _grid(Ks, Gs, **kw):
    return [Case(K, G, **kw) for K in Ks for G in Gs]


# family -> [(case, routes)]; the expectations live in tests/test_gpu_leverage.py
QR64 = _grid((2, 3, 4, 17, 33, 63, 64), (64, 129)) + _grid((2, 17, 64), (1, 2, 63, 64, 65, 127, 128, 257, 1000))
QR128 = _grid((65, 66, 96, 127, 128), (130, 192, 321))
QRBIG = _grid((129, 130, 160, 161, 193, 257, 272), (320, 330))
# Fewer genes than K - 1: the Gram matrix has K - 1 - G pivots of ~reg, and the route refuses when they fall below 1e-9 x its
# largest diagonal entry, i.e. when some deflated row has a squared norm above ~reg 1e9 = 1e3.  At a centred r.m.s. of 8 and G = 1
# or 2 that is a toss-up (the float64 model: pivot / threshold 1.3 - 3.9: the route stands, and is accurate); these cases have a
# centred r.m.s. of 28, where the model refuses with pivot / threshold below 0.5.  The same shapes at r.m.s. 8 are in QR64, where
# the route may do either.
QR_WIDE = [Case(K, G, "wide", 28.0) for K, G in ((17, 1), (17, 2), (64, 1), (64, 2), (140, 64))]
STREAM = _grid((2, 3, 5, 16, 17, 32, 33, 63, 64), (65, 257)) + _grid((3, 33, 64), (1, 63, 64, 255, 256, 700))
ONE_WG = _grid((9,), (1, 511, 512, 513, 1024, 1025, 2048, 2049, 2600)) + _grid((1, 2, 7, 8, 16, 17, 64, 65, 100, 273), (130,))
COND_SHAPES = ((12, 300), (64, 257), (130, 320))
COND = [Case(K, G, "kappa", k) for K, G in COND_SHAPES for k in (1e1, 1e3, 1e4, 2e4)]
COND_STANDS = [Case(K, G, "kappa", 3e3) for K, G in COND_SHAPES]            # must not be refused
COND_REFUSED = [Case(K, G, "spread", 1e6) for K, G in COND_SHAPES]          # must be refused
RANK = [Case(K, 200, "twins", 0.0) for K in (12, 70, 129)] + [Case(12, 300, "zero_row", 0.0), Case(12, 300, "all_equal", 0.0)]
SPECIAL = [Case(12, 300, kind, 0.0) for kind in ("const_gene", "tiny_gene", "huge_gene")]
REG = [Case(K, G, "spread", 30.0, reg) for K, G in ((12, 300), (70, 200)) for reg in (1e-10, 1e-6, 1e-3, 1.0)]
SCALE = [Case(12, 300, "scaled", f) for f in (1e-6, 1e4)]


def routes_for(K):
    """the routes of fdx_leverage_scores_route that apply to K, route 0 apart"""
    return [r for r, ok in ((1, 2 <= K <= 272), (2, 2 <= K <= 64), (3, True)) if ok]


def _dedup(seq):
    seen, out = set(), []
    for c in seq:
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


ALL_CASES = _dedup(QR64 + QR128 + QRBIG + QR_WIDE + STREAM + ONE_WG + COND + COND_STANDS + COND_REFUSED + RANK + SPECIAL + REG
                   + SCALE)


# ---------------------------------------------------------------------------------------------------- float64 model
# The device algorithms restated in float64 numpy, with switches that break them one at a time: what test_leverage_host.py
# feeds to bound() to show that the bound has teeth, and what predicts a refusal of the Cholesky-QR route.
def _chol_watched(C):
    """lower factor with the device's pivot watch (lev_chol_lds): (L, refused, smallest pivot / threshold)"""
    C = C.copy()
    m = C.shape[0]
    mx = float(np.max(np.diag(C)))
    thr = mx * PIVOT_TOL
    bad = not (mx > 0.0) or not (mx < 1e300)
    piv = np.empty(m)
    worst = np.inf
    for j in range(m):
        d = C[j, j]
        worst = min(worst, d / thr if thr > 0 else 0.0)
        if not (d > thr):
            bad = True
            d = thr if thr > 0.0 else 1.0
        piv[j] = d
        C[j + 1:, j + 1:] -= np.outer(C[j + 1:, j], C[j + 1:, j]) / d
    Lf = np.tril(C, -1) / np.sqrt(piv) + np.diag(np.sqrt(piv))
    return Lf, bad, worst


def model_qr(X, reg=1e-6, passes=2, drop_stripe=None, ragged_raw=False):
    """CholeskyQR2 of the Householder-deflated, ridge-augmented matrix, Gram matrices summed by stripes of 64 genes.
    drop_stripe = (b, p, q): stripe b's share of entry (p, q) of the LAST Gram matrix is left out (the first one only steers: what it
    gets wrong the second factorisation puts right);  passes = 1: CholeskyQR once;
    ragged_raw: the last gene of a ragged last stripe is not normalised.  Returns (lev, refused, smallest pivot / threshold)."""
    from scipy.linalg import solve_triangular
    X = np.asarray(X, dtype=np.float64)
    K, G = X.shape
    m = K - 1
    Xc = X - X.sum(axis=0) / K
    rk = np.sqrt(float(K))
    Z = Xc[:m] - (Xc.sum(axis=0) / rk + Xc[m]) / (rk + 1.0)
    A = np.hstack([Z, np.sqrt(reg) * np.eye(m)])                 # m x (G + m): genes, then the ridge rows
    edges = list(range(0, G, STRIPE)) + [G] + list(range(G + STRIPE, G + m, STRIPE)) + [G + m]
    refused, worst = False, np.inf
    for it in range(passes):
        C = np.zeros((m, m))
        for b in range(len(edges) - 1):
            S = A[:, edges[b]:edges[b + 1]]
            P = S @ S.T
            if it == passes - 1 and drop_stripe is not None and drop_stripe[0] == b:
                P[drop_stripe[1], drop_stripe[2]] = P[drop_stripe[2], drop_stripe[1]] = 0.0
            C += P
        Lf, bad, w = _chol_watched(C)
        refused, worst = refused or bad, min(worst, w)
        A = solve_triangular(Lf, A, lower=True)
    raw = np.sum(A[:, :G] ** 2, axis=0)
    lev = raw / (raw.sum() + reg)
    if ragged_raw and G % STRIPE:
        lev[G - 1] = raw[G - 1]
    return lev, refused, worst


def model_jacobi(X, reg=1e-6, weights_reg=True, norm_reg=True, stale_sig2=False):
    """The Gram / eigen / rotate passes: A <- V^T A with V the eigenvectors of A A^T (here: LAPACK's left singular vectors of A - a
    float64 eigh of the Gram matrix has no relative accuracy, the device's Jacobi has), until the columns are orthogonal; then
    sig2_j = |a_j|^2 from the columns, lev_g = sum_j a_gj^2 / (sig2_j + reg), lev / (sum + reg).
    weights_reg = False: the weights without + reg;  norm_reg = False: normalised by the sum alone;  stale_sig2: one rotating pass
    whose sig2 is the Gram diagonal of the columns BEFORE that rotation."""
    X = np.asarray(X, dtype=np.float64)
    A = X - X.sum(axis=0) / X.shape[0]
    sig2 = None
    for _ in range(1 if stale_sig2 else 2):
        C = A @ A.T
        if stale_sig2:
            sig2 = np.diag(C).copy()
        A = np.linalg.svd(A, full_matrices=False)[0].T @ A
    if sig2 is None:
        sig2 = np.sum(A * A, axis=1)
    den = sig2 + reg if weights_reg else np.where(sig2 > 0.0, sig2, 1.0)
    raw = np.sum(A * A / den[:, None], axis=0)
    return raw / (raw.sum() + (reg if norm_reg else 0.0))
