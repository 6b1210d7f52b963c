"""NumPy definition of the gene-pair co-expression statistics (flashdeconv_amd/utils/gene_pairs.py) and the cases its tests use.

**Sums.**  ``Y`` is (n, G) dense, ``A`` a scipy adjacency (symmetric, binary, no diagonal), ``deg_i = sum_j A_ij``,
``lag_g = A y_g``, ``pairs`` (P, 2) of column indices (a, b).  Per pair, in float64::

    0 ua = sum y_a      1 ub = sum y_b      2 qa = sum y_a^2     3 qb = sum y_b^2     4 Da = sum deg y_a   5 Db = sum deg y_b
    6 S  = sum y_a y_b  7 Xab = sum y_a lag_b   8 Xba = sum y_b lag_a
    9 La = sum lag_a^2   10 Lb = sum lag_b^2      11 DLa = sum deg lag_a   12 DLb = sum deg lag_b
    13 amin  14 amax  15 bmin  16 bmax

**Statistics** (``assemble``)::

    m_a = ua/n            m2_a = qa - ua^2/n                                  (likewise b)
    C   = (Xab + Xba)/2 - m_a Db - m_b Da + m_a m_b W                        (= Z_a' A Z_b, Z = Y - mean)
    morans_r  = (n/W) C / sqrt(m2_a m2_b)                                    bivariate Moran's R
    pearson_r = (S - ua ub/n) / sqrt(m2_a m2_b)
    LLc_a = La - 2 m_a DLa + m_a^2 sum_deg_sq          s_a = Da - m_a W      (sum_i (A Z_a)_i^2, sum_i (A Z_a)_i)
    variance_b_moved = (n/W)^2 (LLc_a - s_a^2/n) / ((n - 1) m2_a)
    variance_a_moved = the same with a and b exchanged
    z_score = morans_r / sqrt(max(variance_b_moved, variance_a_moved))
    p_value = erfc(z_score / sqrt 2) / 2          q_value = Benjamini-Hochberg over the pairs whose p_value is not NaN
    order   = pairs by decreasing morans_r, NaN last, ties by ascending index

Everything of a pair is NaN where ``amin == amax`` or ``bmin == bmax``, ``m2 <= 0``, ``W == 0``, ``n < 2`` or where the variance is
not positive.  ``centred`` states R, Pearson's r and the local score on ``Z = Y - mean``; ``enumerate_moves`` the mean and the
variance of R over every reassignment of one gene's values, by brute force.
"""
import itertools
import math

import numpy as np
from scipy import sparse

import spatial_genes_ref as sr

EPS = sr.EPS
PLANES = ("ua", "ub", "qa", "qb", "Da", "Db", "S", "Xab", "Xba", "La", "Lb", "DLa", "DLb", "amin", "amax", "bmin", "bmax")
PAIR_TILE = 256                                    # pairs of a workgroup of the dense kernel
PAIR_COUNTS = (1, PAIR_TILE - 1, PAIR_TILE, PAIR_TILE + 1, 2 * PAIR_TILE + 1)          # 1, 255, 256, 257, 513


def _pattern(A):
    A = sparse.csr_matrix(A)
    return sparse.csr_matrix((np.ones(A.nnz), A.indices, A.indptr), shape=A.shape)


def planes(Y, A, pairs):
    """The 17 planes as a dict of (P,) float64 arrays, and n, W, sum_deg_sq."""
    Y = np.asarray(Y.toarray() if hasattr(Y, "toarray") else Y, dtype=np.float64)
    pairs = np.asarray(pairs, dtype=np.int64)
    n = Y.shape[0]
    deg = sr.degrees(A)
    d = deg.astype(np.float64)
    genes, inverse = np.unique(pairs.ravel(), return_inverse=True)
    Yg = Y[:, genes]
    lag = _pattern(A) @ Yg if sparse.csr_matrix(A).nnz else np.zeros_like(Yg)
    ia, ib = inverse.reshape(-1, 2).T
    ya, yb, la, lb = Yg[:, ia], Yg[:, ib], lag[:, ia], lag[:, ib]
    out = {"ua": ya.sum(0), "ub": yb.sum(0), "qa": (ya * ya).sum(0), "qb": (yb * yb).sum(0), "Da": d @ ya, "Db": d @ yb,
           "S": (ya * yb).sum(0), "Xab": (ya * lb).sum(0), "Xba": (yb * la).sum(0), "La": (la * la).sum(0), "Lb": (lb * lb).sum(0),
           "DLa": d @ la, "DLb": d @ lb, "amin": ya.min(0), "amax": ya.max(0), "bmin": yb.min(0), "bmax": yb.max(0)}
    out.update(n=n, W=int(deg.sum()), sum_deg_sq=int((deg * deg).sum()))
    return out


def assemble(n, W, sum_deg_sq, ua, ub, qa, qb, Da, Db, S, Xab, Xba, La, Lb, DLa, DLb, amin, amax, bmin, bmax):
    """The statistics pair by pair, in plain Python floats."""
    n, W, sum_deg_sq = int(n), int(W), int(sum_deg_sq)
    cols = [np.asarray(a, dtype=np.float64) for a in (ua, ub, qa, qb, Da, Db, S, Xab, Xba, La, Lb, DLa, DLb, amin, amax, bmin, bmax)]
    P = cols[0].size
    keys = ("mean_a", "mean_b", "m2_a", "m2_b", "morans_r", "pearson_r", "variance_b_moved", "variance_a_moved", "z_score", "p_value")
    out = {k: np.full(P, np.nan) for k in keys}
    for p in range(P):
        ua_, ub_, qa_, qb_, Da_, Db_, S_, Xab_, Xba_, La_, Lb_, DLa_, DLb_, amin_, amax_, bmin_, bmax_ = (float(c[p]) for c in cols)
        if n < 1:
            continue
        m_a, m_b = ua_ / n, ub_ / n
        m2_a, m2_b = qa_ - ua_ * ua_ / n, qb_ - ub_ * ub_ / n
        out["mean_a"][p], out["mean_b"][p], out["m2_a"][p], out["m2_b"][p] = m_a, m_b, m2_a, m2_b
        if amin_ == amax_ or bmin_ == bmax_ or not m2_a > 0 or not m2_b > 0 or W <= 0 or n < 2:
            continue
        scale = math.sqrt(m2_a * m2_b)
        C = 0.5 * (Xab_ + Xba_) - m_a * Db_ - m_b * Da_ + m_a * m_b * float(W)
        var = []
        for m, m2, L, DL, D in ((m_a, m2_a, La_, DLa_, Da_), (m_b, m2_b, Lb_, DLb_, Db_)):
            LLc = L - 2.0 * m * DL + m * m * float(sum_deg_sq)
            s = D - m * float(W)
            var.append((float(n) / W) ** 2 * (LLc - s * s / n) / ((n - 1.0) * m2))
        worst = max(var)
        if not (math.isfinite(worst) and worst > 0):
            continue
        R = (float(n) / W) * C / scale
        out["morans_r"][p], out["pearson_r"][p] = R, (S_ - ua_ * ub_ / n) / scale
        out["variance_b_moved"][p], out["variance_a_moved"][p] = var
        out["z_score"][p] = R / math.sqrt(worst)
        out["p_value"][p] = 0.5 * math.erfc(out["z_score"][p] / math.sqrt(2.0))
    out["q_value"] = sr.benjamini_hochberg(out["p_value"])
    out["order"] = sr.decreasing_order(out["morans_r"])
    return out


def centred(Y, A, pairs):
    """The textbook definitions on Z = Y - mean: (morans_r, pearson_r, local) with local (n, P) and
    local_i = (n / 2W) [z_a,i (A z_b)_i + z_b,i (A z_a)_i] / sqrt(sum z_a^2 sum z_b^2)."""
    Y = np.asarray(Y.toarray() if hasattr(Y, "toarray") else Y, dtype=np.float64)
    pairs = np.asarray(pairs, dtype=np.int64)
    n = Y.shape[0]
    W = float(sparse.csr_matrix(A).nnz)
    Z = Y - Y.mean(axis=0)
    AZ = _pattern(A) @ Z
    za, zb, la, lb = Z[:, pairs[:, 0]], Z[:, pairs[:, 1]], AZ[:, pairs[:, 0]], AZ[:, pairs[:, 1]]
    scale = np.sqrt((za * za).sum(0) * (zb * zb).sum(0))
    with np.errstate(divide="ignore", invalid="ignore"):        # a constant column: 0 / 0, the NaN the tests expect there
        local = (n / (2.0 * W)) * (za * lb + zb * la) / scale
        return (n / W) * (za * lb).sum(0) / scale, (za * zb).sum(0) / scale, local


def enumerate_moves(ya, yb, A):
    """(mean, variance) of R over ALL n! reassignments of yb's values to the spots, ya in place (population variance: the
    permutations are the whole population)."""
    ya, yb = np.asarray(ya, dtype=np.float64), np.asarray(yb, dtype=np.float64)
    n = ya.size
    W = float(sparse.csr_matrix(A).nnz)
    za, zb = ya - ya.mean(), yb - yb.mean()
    v = _pattern(A) @ za
    scale = math.sqrt((za * za).sum() * (zb * zb).sum())
    R = np.array([(n / W) * float(v @ zb[list(perm)]) / scale for perm in itertools.permutations(range(n))])
    return float(R.mean()), float(((R - R.mean()) ** 2).mean())


# ---------------------------------------------------------------- cases
def pair_list(G, P, seed):
    """P pairs over G >= 3 columns: a == b, a repeated pair, (a, b) beside (b, a) and the columns 0 and G - 1 come first (as many as
    P leaves room for), random pairs after them."""
    fixed = [(0, G - 1), (G - 1, 0), (1, 1), (2, 1), (2, 1), (G - 1, G - 1), (0, 0)]
    rs = np.random.RandomState(4000 + seed)
    rest = rs.randint(0, G, size=(max(0, P - len(fixed)), 2))
    return np.concatenate([np.array(fixed[:P], dtype=np.int64).reshape(-1, 2), rest]).astype(np.int64)


def planted_case():
    """The 25 x 24 grid of tests/gpu_graphs._grid (spot i at x = i % 24, y = i // 24): column 0 smooth (x + y), column 1 its partner
    ((x + 1) + y plus a Bernoulli(1/2) jitter), column 2 the smooth values shuffled, column 3 the constant 3, column 4
    50 - smooth; and the pairs (0, 1), (0, 2), (0, 3), (0, 4), (0, 0)."""
    i = np.arange(600)
    rs = np.random.RandomState(7)
    smooth = (i % 24 + i // 24).astype(np.float64)
    partner = (i % 24 + 1 + i // 24).astype(np.float64) + (rs.rand(600) < 0.5)
    shuffled = smooth[rs.permutation(600)]
    Y = np.stack([smooth, partner, shuffled, np.full(600, 3.0), 50.0 - smooth], axis=1)
    return Y, np.array([(0, 1), (0, 2), (0, 3), (0, 4), (0, 0)], dtype=np.int64)
