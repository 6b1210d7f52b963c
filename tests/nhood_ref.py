"""NumPy reference of the neighbourhood enrichment (utils.neighborhoods, csrc/label_pair_kernels.cpp), shared by
tests/test_nhood_host.py and tests/test_gpu_nhood.py.

    pair_counts(A, labels, C) = O' A O        O the one-hot matrix of the labels >= 0, int64
    the null                  = pair_counts of labels[permutation_indices(seed, r, n)], r = first .. first + R - 1
    the accumulation          = count_ge, count_le (int64), sum d, sum d^2 (float64) against the observed matrix in permutation order
    moments / moments_by_enumeration: the formulas of the module docstring, and the same moments over all n! permutations
"""
import itertools

import numpy as np
from scipy import sparse


def one_hot(labels, C):
    labels = np.asarray(labels)
    O = np.zeros((labels.shape[0], C), dtype=np.int64)
    ok = labels >= 0
    O[np.flatnonzero(ok), labels[ok]] = 1
    return O


def pair_counts(A, labels, C):
    A = sparse.csr_matrix(A).astype(bool).astype(np.int64)
    O = one_hot(labels, C)
    return np.asarray(O.T @ (A @ O), dtype=np.int64)


def label_counts(labels, C):
    labels = np.asarray(labels)
    return np.bincount(labels[labels >= 0], minlength=C).astype(np.int64)


def graph_counts(A):
    """(n, W, sum deg^2) as Python ints."""
    A = sparse.csr_matrix(A).astype(bool).astype(np.int64)
    deg = np.asarray(A.sum(axis=1)).ravel().astype(np.int64)
    return int(A.shape[0]), int(deg.sum()), int((deg * deg).sum())


def null_counts(A, labels, C, seed, first, R):
    """(R, C, C) int64: N^r for r = first .. first + R - 1."""
    from flashdeconv_amd.utils.spatial_stats import permutation_indices
    labels = np.asarray(labels)
    n = labels.shape[0]
    out = np.zeros((R, C, C), dtype=np.int64)
    for j in range(R):
        out[j] = pair_counts(A, labels[permutation_indices(seed, first + j, n)], C)
    return out


def accumulate(null, obs):
    """(count_ge, count_le, sum_d, sumsq_d) of a null against obs, added in permutation order."""
    C = obs.shape[0]
    ge, le = np.zeros((C, C), dtype=np.int64), np.zeros((C, C), dtype=np.int64)
    sd, sq = np.zeros((C, C)), np.zeros((C, C))
    for Nr in null:
        d = (Nr - obs).astype(np.float64)
        ge += Nr >= obs
        le += Nr <= obs
        sd = sd + d
        sq = sq + d * d
    return ge, le, sd, sq


def _falling(x, k):
    out = 1.0
    for j in range(k):
        out = out * (x - j)
    return out


def moments(n, W, sum_deg_sq, na):
    """(E, Var) (C, C) by the formulas, entry by entry in Python floats."""
    C = len(na)
    E, V = np.full((C, C), np.nan), np.full((C, C), np.nan)
    if n < 4 or W <= 0:
        return E, V
    S0, S1, S2 = float(W), 2.0 * W, 4.0 * sum_deg_sq
    d2, d3, d4 = _falling(float(n), 2), _falling(float(n), 3), _falling(float(n), 4)
    for a in range(C):
        for b in range(C):
            x, y = float(na[a]), float(na[b])
            if a == b:
                e = S0 * _falling(x, 2) / d2
                v = S1 * _falling(x, 2) / d2 + (S2 - 2 * S1) * _falling(x, 3) / d3 + (S0 * S0 + S1 - S2) * _falling(x, 4) / d4 - e * e
            else:
                e = S0 * x * y / d2
                v = 0.25 * (2 * S1 * x * y / d2 + (S2 - 2 * S1) * x * y * (x + y - 2) / d3
                            + 4 * (S0 * S0 + S1 - S2) * _falling(x, 2) * _falling(y, 2) / d4) - e * e
            E[a, b], V[a, b] = e, v
    return E, V


def moments_by_enumeration(A, labels, C):
    """(E, Var) over all n! reassignments of the labels to the spots (n <= 8)."""
    labels = np.asarray(labels)
    n = labels.shape[0]
    Ad = np.asarray(sparse.csr_matrix(A).astype(bool).astype(np.int64).todense())
    s1, s2, cnt = np.zeros((C, C)), np.zeros((C, C)), 0
    for p in itertools.permutations(range(n)):
        O = one_hot(labels[list(p)], C)
        N = (O.T @ Ad @ O).astype(np.float64)
        s1 += N
        s2 += N * N
        cnt += 1
    E = s1 / cnt
    return E, s2 / cnt - E * E


def random_graph(rs, n, p=0.4):
    """A symmetric binary adjacency without self loops and with at least one edge."""
    U = np.triu(rs.rand(n, n) < p, 1)
    U[0, 1] = True
    return sparse.csr_matrix((U | U.T).astype(np.int8))


def knn_graph(coords, k=6):
    """The symmetrised k-NN adjacency (cKDTree)."""
    from scipy.spatial import cKDTree
    n = coords.shape[0]
    _, idx = cKDTree(coords).query(coords, k=k + 1)
    rows = np.repeat(np.arange(n), k)
    A = sparse.csr_matrix((np.ones(n * k, dtype=np.int8), (rows, idx[:, 1:].ravel())), shape=(n, n))
    return ((A + A.T) > 0).astype(np.int8).tocsr()
