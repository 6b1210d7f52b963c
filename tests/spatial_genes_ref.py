"""NumPy definition of the spatially-variable-gene statistics (flashdeconv_amd/utils/spatial_genes.py) and the cases its tests use.

**Sums.**  ``Y`` is (n, G) dense, ``A`` a scipy adjacency (symmetric, binary, no diagonal), ``deg_i = sum_j A_ij``.  Per gene, in
float64::

    u = sum_i y_i       q = sum_i y_i^2       c3 = sum_i y_i^3       c4 = sum_i y_i^4
    D = sum_i deg_i y_i                       H = sum_i deg_i y_i^2
    P = sum_i y_i lag_i,   lag_i = sum_{j in N(i)} y_j
    ymin = min_i y_i      ymax = max_i y_i

**Statistics** (``assemble``)::

    m  = u / n                  m2 = q - u*u/n                 m4 = c4 - 4 m c3 + 6 m^2 q - 3 n m^4
    morans_i = (n / W) (P - 2 m D + m^2 W) / m2
    gearys_c = ((n - 1) / (2 W)) (2 H - 2 P) / m2
    E = -1 / (n - 1)      S1 = 2 W      S2 = 4 sum_i deg_i^2
    variance_i = (n^2 S1 - n S2 + 3 W^2) / ((n^2 - 1) W^2) - E^2                      z_score = (morans_i - E) / sqrt(variance_i)
    b2 = n m4 / m2^2
    E[I^2] = {n [(n^2 - 3n + 3) S1 - n S2 + 3 W^2] - b2 [(n^2 - n) S1 - 2n S2 + 6 W^2]} / [(n - 1)(n - 2)(n - 3) W^2]
    variance_i_rand = E[I^2] - 1 / (n - 1)^2                                          z_score_rand likewise
    p_value = erfc(z_score_rand / sqrt 2) / 2
    q_value = Benjamini-Hochberg over the genes whose p_value is not NaN
    order   = genes by decreasing morans_i, NaN last, ties by ascending index

NaN where ``ymin == ymax``, ``m2 <= 0``, ``W == 0``, ``n < 2`` (``n < 4`` for the randomisation variance) or where the variance is
not positive.  ``centred`` states Moran's I, Geary's C, m2 and m4 by their textbook definitions on ``Z = Y - mean``.

**Cases.**  The exact cases hold integers in [0, 7] (a negative column apart): every term of every plane is an integer below
7^4 n (1 + max deg) << 2^53, so every partial sum of every order is exactly representable and the device must return these
numbers, not close ones.  The generic cases hold non-negative lognormal values rounded to float32.
"""
import math

import numpy as np
from scipy import sparse

EPS = np.finfo(np.float64).eps
PLANES = ("u", "q", "c3", "c4", "D", "H", "P", "ymin", "ymax")
GENE_TILE = 512                                   # genes of a workgroup of the dense kernel
GENE_COUNTS = (1, GENE_TILE - 1, GENE_TILE, GENE_TILE + 1, 2 * GENE_TILE - 1, 2 * GENE_TILE, 2 * GENE_TILE + 1)


def degrees(A):
    return np.diff(sparse.csr_matrix(A).indptr).astype(np.int64)


def planes(Y, A):
    """The nine planes as a dict of (G,) float64 arrays, and n, W, sum_deg_sq."""
    Y = np.asarray(Y.toarray() if hasattr(Y, "toarray") else Y, dtype=np.float64)
    A = sparse.csr_matrix(A)
    n, G = Y.shape
    deg = degrees(A)
    pattern = sparse.csr_matrix((np.ones(A.nnz), A.indices, A.indptr), shape=A.shape)
    lag = pattern @ Y if A.nnz else np.zeros_like(Y)
    Y2 = Y * Y
    d = deg.astype(np.float64)
    out = {"u": Y.sum(axis=0), "q": Y2.sum(axis=0), "c3": (Y2 * Y).sum(axis=0), "c4": (Y2 * Y2).sum(axis=0), "D": d @ Y, "H": d @ Y2,
           "P": (Y * lag).sum(axis=0), "ymin": Y.min(axis=0), "ymax": Y.max(axis=0)}
    out.update(n=n, W=int(deg.sum()), sum_deg_sq=int((deg * deg).sum()))
    return out


def benjamini_hochberg(p):
    p = np.asarray(p, dtype=np.float64)
    q = np.full(p.shape, np.nan)
    keep = [i for i in range(p.size) if not math.isnan(p[i])]
    keep.sort(key=lambda i: (p[i], i))
    m, running = len(keep), math.inf
    for rank in range(m, 0, -1):
        i = keep[rank - 1]
        running = min(running, p[i] * (float(m) / rank))
        q[i] = min(1.0, running)
    return q


def decreasing_order(x):
    x = np.asarray(x, dtype=np.float64)
    return np.array(sorted(range(x.size), key=lambda i: (1, 0.0, i) if math.isnan(x[i]) else (0, -x[i], i)), dtype=np.int64)


def normal_moments(n, W, sum_deg_sq):
    """(expected_i, variance_i) under the normality assumption; NaN where undefined."""
    if n < 2:
        return np.float64(np.nan), np.float64(np.nan)
    expected = -1.0 / (n - 1.0)
    if W <= 0:
        return np.float64(expected), np.float64(np.nan)
    nf, Wf = float(n), float(W)
    S1, S2 = 2.0 * Wf, 4.0 * float(sum_deg_sq)
    return np.float64(expected), np.float64((nf * nf * S1 - nf * S2 + 3.0 * Wf * Wf) / ((nf * nf - 1.0) * Wf * Wf) - expected * expected)


def randomization_variance(n, W, sum_deg_sq, m2, m4):
    if n < 4 or W <= 0:
        return np.full(np.shape(m2), np.nan)
    nf, S0 = float(n), float(W)
    S1, S2 = 2.0 * S0, 4.0 * float(sum_deg_sq)
    with np.errstate(divide="ignore", invalid="ignore"):
        b2 = np.where(m2 > 0, nf * m4 / (m2 * m2), np.nan)
        e2 = (nf * ((nf * nf - 3.0 * nf + 3.0) * S1 - nf * S2 + 3.0 * S0 * S0)
              - b2 * ((nf * nf - nf) * S1 - 2.0 * nf * S2 + 6.0 * S0 * S0)) / ((nf - 1.0) * (nf - 2.0) * (nf - 3.0) * S0 * S0)
    return e2 - 1.0 / ((nf - 1.0) * (nf - 1.0))


def z_scores(stat, expected, variance):
    variance = np.broadcast_to(np.asarray(variance, dtype=np.float64), stat.shape)
    out = np.full(stat.shape, np.nan)
    for g in range(stat.size):
        v = variance[g]
        if np.isfinite(v) and v > 0:
            out[g] = (stat[g] - expected) / np.sqrt(v)
    return out


def morans_from_sums(n, W, u, q, D, P, dead):
    """(mean, m2, morans_i) from raw sums, NaN for the genes marked ``dead`` and those without variance."""
    with np.errstate(divide="ignore", invalid="ignore"):
        m = u / n
        m2 = q - u * u / n
        morans = np.full(u.shape, np.nan)
        if W > 0 and n >= 2:
            live = ~dead & (m2 > 0)
            val = (float(n) / float(W)) * (P - 2.0 * m * D + m * m * float(W)) / m2
            morans[live] = val[live]
    return m, m2, morans


def assemble(n, W, sum_deg_sq, u, q, c3, c4, D, H, P, ymin, ymax):
    n, W, sum_deg_sq = int(n), int(W), int(sum_deg_sq)
    u, q, c3, c4, D, H, P, ymin, ymax = (np.asarray(a, dtype=np.float64) for a in (u, q, c3, c4, D, H, P, ymin, ymax))
    m, m2, morans = morans_from_sums(n, W, u, q, D, P, ymin == ymax)
    dead = np.isnan(morans)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        m4 = c4 - 4.0 * m * c3 + 6.0 * (m * m) * q - 3.0 * n * (m * m) * (m * m)
        geary = np.full(u.shape, np.nan)
        if W > 0 and n >= 2:
            val = ((n - 1.0) / (2.0 * float(W))) * (2.0 * H - 2.0 * P) / m2
            geary[~dead] = val[~dead]
    expected, variance = normal_moments(n, W, sum_deg_sq)
    var_rand = randomization_variance(n, W, sum_deg_sq, np.where(dead, np.nan, m2), m4)
    var_rand = np.where(dead, np.nan, var_rand)
    z_rand = z_scores(morans, expected, var_rand)
    p = np.array([math.nan if math.isnan(v) else 0.5 * math.erfc(v / math.sqrt(2.0)) for v in z_rand.tolist()], dtype=np.float64)
    return {"mean": m, "m2": m2, "m4": m4, "morans_i": morans, "gearys_c": geary, "expected_i": expected, "variance_i": variance,
            "z_score": z_scores(morans, expected, variance), "variance_i_rand": var_rand, "z_score_rand": z_rand, "p_value": p,
            "q_value": benjamini_hochberg(p), "order": decreasing_order(morans)}


def centred(Y, A):
    """The textbook definitions on Z = Y - mean: (morans_i, gearys_c, m2, m4), Geary's C summed over the edges."""
    Y = np.asarray(Y, dtype=np.float64)
    A = sparse.coo_matrix(A)
    n = Y.shape[0]
    W = float(A.nnz)
    Z = Y - Y.mean(axis=0)
    pattern = sparse.csr_matrix((np.ones(A.nnz), (A.row, A.col)), shape=A.shape)
    m2 = (Z * Z).sum(axis=0)
    morans = (n / W) * (Z * (pattern @ Z)).sum(axis=0) / m2
    diff = Y[A.row] - Y[A.col]
    geary = ((n - 1.0) / (2.0 * W)) * (diff * diff).sum(axis=0) / m2
    return morans, geary, m2, (Z ** 4).sum(axis=0)


def residual_sums(Y, A, weights, E):
    """u, q, D, P of the dense residual R = Y - weights E, and per array the sum of the magnitudes of the terms of its expansion
    (all terms are non-negative for non-negative Y, weights and E: the magnitudes are the terms themselves)."""
    Y = np.asarray(Y.toarray() if hasattr(Y, "toarray") else Y, dtype=np.float64)
    A = sparse.csr_matrix(A)
    pattern = sparse.csr_matrix((np.ones(A.nnz), A.indices, A.indptr), shape=A.shape)
    w = np.asarray(weights, dtype=np.float64)
    deg = degrees(A).astype(np.float64)
    R = Y - w @ E
    got = {"u": R.sum(axis=0), "q": (R * R).sum(axis=0), "D": deg @ R, "P": (R * (pattern @ R)).sum(axis=0)}
    N = pattern @ w
    B, M, A_w, C_w = w.T @ Y, N.T @ Y, w.T @ w, w.T @ N
    s = planes(Y, A)
    mags = {"u": s["u"] + w.sum(axis=0) @ E,
            "q": s["q"] + 2.0 * (E * B).sum(axis=0) + np.einsum("kg,kl,lg->g", E, A_w, E),
            "D": s["D"] + (deg @ w) @ E,
            "P": s["P"] + 2.0 * (E * M).sum(axis=0) + np.einsum("kg,kl,lg->g", E, C_w, E)}
    return got, mags


# ---------------------------------------------------------------- cases
def exact_case(n, G, seed, density=1.0):
    """Integers in [0, 7] as float64; density < 1 zeroes entries at random (the CSR routes store what is left)."""
    rs = np.random.RandomState(1000 + seed)
    Y = rs.randint(0, 8, size=(n, G)).astype(np.float64)
    if density < 1.0:
        Y *= rs.rand(n, G) < density
    return Y


def generic_case(n, G, seed, constant=()):
    """Non-negative lognormal values rounded to float32 (as float64), the columns in ``constant`` set to one value each."""
    rs = np.random.RandomState(2000 + seed)
    Y = rs.lognormal(0.0, 1.5, size=(n, G)).astype(np.float32).astype(np.float64)
    for k, g in enumerate(constant):
        Y[:, g] = np.float64(np.float32(0.0 if k == 0 else 1.0 + 0.1 * k))
    return Y


def csr_contents_case(n, G, seed, variant):
    """A scipy CSR (float32 data, sorted rows) and its dense form for the structure cases; G >= 6, n >= 4.  Both variants: stored
    zeros, an empty column (1), and column 4 negative beside implicit zeros (its maximum is the implicit 0).
    ``"holes"``: rows 0 and n - 1 are empty.  ``"full"``: column 2 stores a positive and column 5 a negative value in every row
    (no implicit zero: the maximum of column 5 is negative), and row 3 stores all G columns (column 1 as a stored zero)."""
    rs = np.random.RandomState(3000 + seed)
    Y = exact_case(n, G, seed, density=0.35)
    Y[:, 4] = -Y[:, 4]
    Y[:, 1] = 0.0
    mask = Y != 0
    mask |= rs.rand(n, G) < 0.05                        # stored zeros
    mask[:, 1] = False
    if variant == "holes":
        mask[[0, n - 1]] = False
        Y[[0, n - 1]] = 0.0
    else:
        Y[:, 2] = 1.0 + rs.randint(0, 7, size=n)
        Y[:, 5] = -1.0 - rs.randint(0, 7, size=n)
        mask[:, [2, 5]] = True
        mask[3] = True
    rows, cols = np.nonzero(mask)
    indptr = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.int64)
    m = sparse.csr_matrix((Y[rows, cols].astype(np.float32), cols.astype(np.int32), indptr), shape=(n, G))
    assert m.nnz == int(mask.sum()) and np.array_equal(m.toarray(), Y) and (m.data == 0).any()
    return m, Y


def planted_case():
    """The 25 x 24 grid of tests/gpu_graphs._grid (spot i at x = i % 24, y = i // 24): gene 0 a smooth gradient, gene 1 the same
    values shuffled, gene 2 constant."""
    i = np.arange(600)
    smooth = (i % 24 + i // 24).astype(np.float64)
    shuffled = smooth[np.random.RandomState(7).permutation(600)]
    return np.stack([smooth, shuffled, np.full(600, 3.0)], axis=1)
