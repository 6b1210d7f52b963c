"""NumPy definition of the spatial gene modules (flashdeconv_amd/utils/gene_modules.py) and the cases its tests use.

**Sums.**  ``Y`` is (n, G) dense, ``A`` a scipy adjacency (symmetric, binary, no diagonal), ``deg_i = sum_j A_ij``,
``lag = A Y[:, genes]``.  In float64::

    per gene (S,):     u = sum y    D = sum deg y    L = sum lag^2    DL = sum deg lag    ymin    ymax
    matrices (S, S):   S = Yg' Yg        X = Yg' lag

**Statistics** (``assemble``): the formulas of tests/gene_pairs_ref.py pair by pair, (a, b) taking ``Xab = X[a, b]``,
``Xba = X[b, a]``; q values by Benjamini-Hochberg over the pairs a < b, mirrored, NaN on the diagonal.  ``centred`` states R and
Pearson's r on ``Z = Y - mean``.  ``modules`` is the clustering rule, ``scores`` the module scores.
"""
import numpy as np
from scipy import sparse
from scipy.cluster.hierarchy import fcluster, linkage
from scipy.spatial.distance import squareform

import gene_pairs_ref as gr
import spatial_genes_ref as sr

EPS = sr.EPS
GENE_PLANES = ("u", "D", "L", "DL", "ymin", "ymax")
GM_TILE = 64                                       # genes of a side of the contraction kernel's tile (GM_TILE, gene_module_kernels.cpp)
GENE_COUNTS = (1, 15, 16, 17, GM_TILE - 1, GM_TILE, GM_TILE + 1, 2 * GM_TILE + 1)        # 1, 15, 16, 17, 63, 64, 65, 129


def planes(Y, A, genes):
    """The six per-gene planes (S,), the matrices S and X (S, S), and n, W, sum_deg_sq."""
    Y = np.asarray(Y.toarray() if hasattr(Y, "toarray") else Y, dtype=np.float64)
    genes = np.asarray(genes, dtype=np.int64)
    deg = sr.degrees(A)
    d = deg.astype(np.float64)
    Yg = Y[:, genes]
    lag = gr._pattern(A) @ Yg if sparse.csr_matrix(A).nnz else np.zeros_like(Yg)
    out = {"u": Yg.sum(0), "D": d @ Yg, "L": (lag * lag).sum(0), "DL": d @ lag, "ymin": Yg.min(0), "ymax": Yg.max(0),
           "S": Yg.T @ Yg, "X": Yg.T @ lag}
    out.update(n=Y.shape[0], W=int(deg.sum()), sum_deg_sq=int((deg * deg).sum()))
    return out


def pair_planes(s, pairs):
    """The 17 planes of tests/gene_pairs_ref.py for the pairs (a, b) of PLACES in the gene list, from the sums ``s`` of planes()."""
    a, b = np.asarray(pairs, dtype=np.int64).reshape(-1, 2).T
    q = np.diagonal(s["S"])
    return {"ua": s["u"][a], "ub": s["u"][b], "qa": q[a], "qb": q[b], "Da": s["D"][a], "Db": s["D"][b], "S": s["S"][a, b],
            "Xab": s["X"][a, b], "Xba": s["X"][b, a], "La": s["L"][a], "Lb": s["L"][b], "DLa": s["DL"][a], "DLb": s["DL"][b],
            "amin": s["ymin"][a], "amax": s["ymax"][a], "bmin": s["ymin"][b], "bmax": s["ymax"][b]}


def assemble(n, W, sum_deg_sq, u, D, L, DL, ymin, ymax, S, X):
    """The statistics as (S, S) / (S,) arrays, every pair through gene_pairs_ref.assemble (plain Python floats)."""
    k = np.asarray(u).shape[0]
    s = {"u": np.asarray(u, dtype=np.float64), "D": np.asarray(D, dtype=np.float64), "L": np.asarray(L, dtype=np.float64),
         "DL": np.asarray(DL, dtype=np.float64), "ymin": np.asarray(ymin, dtype=np.float64), "ymax": np.asarray(ymax, dtype=np.float64),
         "S": np.asarray(S, dtype=np.float64), "X": np.asarray(X, dtype=np.float64)}
    pairs = np.array([(a, b) for a in range(k) for b in range(k)], dtype=np.int64).reshape(-1, 2)
    pp = pair_planes(s, pairs)
    flat = gr.assemble(n, W, sum_deg_sq, *(pp[name] for name in gr.PLANES))
    out = {key: flat[key].reshape(k, k) for key in ("morans_r", "pearson_r", "z_score", "p_value")}
    diag = np.arange(k) * (k + 1)
    out.update(mean=flat["mean_a"][diag], m2=flat["m2_a"][diag], variance_moved=flat["variance_b_moved"][diag])
    q = np.full((k, k), np.nan)
    ia, ib = np.triu_indices(k, 1)
    q[ia, ib] = sr.benjamini_hochberg(out["p_value"][ia, ib])
    q[ib, ia] = q[ia, ib]
    out["q_value"] = q
    return out


def centred(Y, A, genes):
    """The textbook definitions on Z = Y - mean: (morans_r, pearson_r), (S, S) each, morans_r = (n/W) Z_a' A Z_b / sqrt(m2_a m2_b)
    symmetrised as the pair statistics are ((Z_a' A Z_b + Z_b' A Z_a) / 2; A is symmetric, so the two agree up to rounding)."""
    Y = np.asarray(Y.toarray() if hasattr(Y, "toarray") else Y, dtype=np.float64)
    Z = Y[:, np.asarray(genes, dtype=np.int64)]
    Z = Z - Z.mean(axis=0)
    n, W = Y.shape[0], float(sparse.csr_matrix(A).nnz)
    ZAZ = Z.T @ (gr._pattern(A) @ Z)
    m2 = (Z * Z).sum(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.sqrt(m2[:, None] * m2[None, :])
        return (n / W) * 0.5 * (ZAZ + ZAZ.T) / scale, (Z.T @ Z) / scale


def modules(z, q, fdr=0.05, n_modules=None, min_module_size=3):
    """The clustering rule: labels (S,) int64, -1 for a dead, unassigned or too small gene."""
    z, q = np.asarray(z, dtype=np.float64), np.asarray(q, dtype=np.float64)
    k = z.shape[0]
    labels = np.full(k, -1, dtype=np.int64)
    alive = [a for a in range(k) if not np.isnan(z[a, a])]
    if len(alive) < 2:
        return labels
    m = len(alive)
    upper = [(i, j) for i in range(m) for j in range(i + 1, m)]
    zmax = max(max(z[alive[i], alive[j]], z[alive[j], alive[i]]) for i, j in upper)
    d = np.zeros((m, m))
    for i, j in upper:
        d[i, j] = d[j, i] = max(0.0, zmax - 0.5 * (z[alive[i], alive[j]] + z[alive[j], alive[i]]))
    tree = linkage(squareform(d, checks=False), "average")
    if n_modules is None:
        significant = [z[alive[i], alive[j]] for i, j in upper if q[alive[i], alive[j]] <= fdr]
        if not significant:
            return labels
        cluster = fcluster(tree, t=zmax - min(significant), criterion="distance")
    else:
        cluster = fcluster(tree, t=n_modules, criterion="maxclust")
    groups = {}
    for i, c in enumerate(cluster):
        groups.setdefault(int(c), []).append(alive[i])
    kept = sorted((g for g in groups.values() if len(g) >= min_module_size), key=lambda g: (-len(g), min(g)))
    for c, g in enumerate(kept):
        labels[g] = c
    return labels


def scores(Y, genes, labels, mean, m2):
    """score[i, c] = (1 / |M_c|) sum_{a in M_c} (y_a,i - mean_a) / sqrt(m2_a / n), (n, C)."""
    Y = np.asarray(Y.toarray() if hasattr(Y, "toarray") else Y, dtype=np.float64)
    genes, labels = np.asarray(genes, dtype=np.int64), np.asarray(labels, dtype=np.int64)
    n, C = Y.shape[0], int(labels.max()) + 1 if labels.size else 0
    out = np.zeros((n, C))
    for c in range(C):
        members = np.flatnonzero(labels == c)
        for a in members:
            out[:, c] += (Y[:, genes[a]] - mean[a]) / np.sqrt(m2[a] / n)
        if members.size:
            out[:, c] /= members.size
    return out


# ---------------------------------------------------------------- cases
def gene_list(G, S, seed):
    """S distinct columns of G >= S: the columns 0 and G - 1 first (as many as S leaves room for), the rest at random, unsorted."""
    rs = np.random.RandomState(5000 + seed)
    rest = rs.permutation(np.arange(1, G - 1))
    return np.concatenate([np.array([0, G - 1], dtype=np.int64)[:min(S, 2 if G > 1 else 1)], rest])[:S].astype(np.int64)


def lattice_adjacency(rows=25, cols=24):
    """The 4-neighbour adjacency of a rows x cols lattice, spot i at x = i % cols, y = i // cols."""
    i = np.arange(rows * cols)
    x, y = i % cols, i // cols
    right, down = i[x + 1 < cols], i[y + 1 < rows]
    r = np.concatenate([right, right + 1, down, down + cols])
    c = np.concatenate([right + 1, right, down + cols, down])
    return sparse.csr_matrix((np.ones(r.size), (r, c)), shape=(i.size, i.size))


def planted_case():
    """(Y, truth) on the 25 x 24 lattice (spot i at x = i % 24, y = i // 24): three spatial patterns - sin 2 pi x/24, cos 2 pi y/25,
    a central disc - with 12 genes each, ``floor(exp(1 + 0.8 pattern + 0.5 noise))``, and 20 noise genes
    ``floor(exp(1 + 0.7 noise))``; the 56 columns shuffled.  truth (56,): the pattern of a column, -1 for a noise gene."""
    rs = np.random.RandomState(3)
    i = np.arange(600)
    x, y = (i % 24) / 24.0, (i // 24) / 25.0
    disc = np.where((x - 0.5) ** 2 + (y - 0.5) ** 2 < 0.09, 1.0, -1.0)
    patterns = [np.sin(2 * np.pi * x), np.cos(2 * np.pi * y), disc]
    cols, truth = [], []
    for k, pattern in enumerate(patterns):
        for _ in range(12):
            cols.append(np.floor(np.exp(1.0 + 0.8 * pattern + 0.5 * rs.randn(600))))
            truth.append(k)
    for _ in range(20):
        cols.append(np.floor(np.exp(1.0 + 0.7 * rs.randn(600))))
        truth.append(-1)
    order = rs.permutation(len(cols))
    return np.stack(cols, axis=1)[:, order], np.array(truth, dtype=np.int64)[order]
