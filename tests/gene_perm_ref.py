"""NumPy definition of the permutation test per gene (flashdeconv_amd/utils/gene_permutations.py) and the cases its tests use.

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

**Cases** are those of tests/spatial_genes_ref.py (``exact_case``, ``generic_case``, ``csr_contents_case``, ``planted_case``): a
permutation only moves the values, so every term of ``P_r``, ``D_r``, ``H_r`` of an exact case is again an integer far below 2^53
and any summation order is exact.
"""
import math

import numpy as np
from scipy import sparse

import spatial_genes_ref as sr
from spatial_genes_ref import EPS, csr_contents_case, exact_case, generic_case, planted_case  # noqa: F401

OBS_PLANES = ("u", "q", "D", "H", "P", "ymin", "ymax")
NULL_PLANES = ("P", "D", "H")


def _dense(Y):
    return np.asarray(Y.toarray() if hasattr(Y, "toarray") else Y, dtype=np.float64)


def observed(Y, A, genes=None):
    """The seven observed planes of the listed columns as a dict of (S,) arrays, and n, W, sum_deg_sq."""
    Y = _dense(Y)
    s = sr.planes(Y if genes is None else Y[:, np.asarray(genes)], A)
    out = {name: s[name] for name in OBS_PLANES}
    out.update(n=s["n"], W=s["W"], sum_deg_sq=s["sum_deg_sq"])
    return out


def null_sums(Y, A, seed, first, R, genes=None):
    """(R, 3, S) float64: P_r, D_r, H_r of the permutations first .. first + R - 1 of ``seed``."""
    from flashdeconv_amd.utils.spatial_stats import permutation_indices
    Y = _dense(Y)
    if genes is not None:
        Y = Y[:, np.asarray(genes)]
    A = sparse.csr_matrix(A)
    n, S = Y.shape
    pattern = sparse.csr_matrix((np.ones(A.nnz), A.indices, A.indptr), shape=A.shape)
    d = sr.degrees(A).astype(np.float64)
    out = np.zeros((R, 3, S))
    for r in range(R):
        V = Y[permutation_indices(seed, first + r, n)]
        lag = pattern @ V if A.nnz else np.zeros_like(V)
        out[r, 0] = (V * lag).sum(axis=0)
        out[r, 1] = d @ V
        out[r, 2] = d @ (V * V)
    return out


def statistics(n, W, u, q, ymin, ymax, P, D, H):
    """(I, C, dead) of the sums P, D, H ((S,) or (R, S)); NaN for dead genes."""
    I, C = np.full(np.shape(P), np.nan), np.full(np.shape(P), np.nan)
    dead = np.ones(u.shape, dtype=bool)
    if n >= 2 and W > 0:
        with np.errstate(divide="ignore", invalid="ignore"):
            m = u / n
            m2 = q - u * u / n
            dead = (ymin == ymax) | ~(m2 > 0)
            vi = (float(n) / float(W)) * (P - 2.0 * m * D + m * m * float(W)) / m2
            vc = ((n - 1.0) / (2.0 * float(W))) * (2.0 * H - 2.0 * P) / m2
        I[..., ~dead] = vi[..., ~dead]
        C[..., ~dead] = vc[..., ~dead]
    return I, C, dead


def assemble(n, W, u, q, D, H, P, ymin, ymax, null):
    """The keys of the definition from the observed planes and the whole null (R, 3, S)."""
    n, W = int(n), int(W)
    u, q, D, H, P, ymin, ymax = (np.asarray(a, dtype=np.float64) for a in (u, q, D, H, P, ymin, ymax))
    null = np.asarray(null, dtype=np.float64)
    R, S = null.shape[0], u.shape[0]
    I, C, dead = statistics(n, W, u, q, ymin, ymax, P, D, H)
    out = {"morans_i": I, "gearys_c": C, "n_permutations": R}
    if R < 1:
        return out
    Ir, Cr, _ = statistics(n, W, u, q, ymin, ymax, null[:, 0], null[:, 1], null[:, 2])
    keys = ("p_sim", "p_sim_less", "gearys_p_sim", "z_sim", "null_mean", "null_std")
    out.update({k: np.full(S, np.nan) for k in keys})
    for g in range(S):
        if dead[g]:
            continue
        out["p_sim"][g] = (1.0 + sum(1 for r in range(R) if Ir[r, g] >= I[g])) / (R + 1.0)
        out["p_sim_less"][g] = (1.0 + sum(1 for r in range(R) if Ir[r, g] <= I[g])) / (R + 1.0)
        out["gearys_p_sim"][g] = (1.0 + sum(1 for r in range(R) if Cr[r, g] <= C[g])) / (R + 1.0)
        s = sq = np.float64(0.0)
        for r in range(R):
            s = s + Ir[r, g]
            sq = sq + Ir[r, g] * Ir[r, g]
        mean = s / R
        std = math.sqrt(max(sq / R - mean * mean, 0.0))
        out["null_mean"][g], out["null_std"][g] = mean, std
        if std > 0:
            out["z_sim"][g] = (I[g] - mean) / std
    out["q_sim"] = sr.benjamini_hochberg(out["p_sim"])
    return out
