"""Host reference of the fit tail: the four sums of the objective and the normalising export, term by term.

Inputs are in the CALLER's spot order throughout: a scipy adjacency A (structure only: every stored entry is a neighbour), beta (n, K),
H (K, n) and XtX (K, K).  With deg_i the number of stored entries of row i of A:

    cross = sum_ik beta_ik H_ki                                   <H, beta>
    quad  = sum_i  beta_i' XtX beta_i                             beta' XtX beta
    spat  = sum_ik beta_ik (deg_i beta_ik - sum_{j in N(i)} beta_jk)   tr(beta' L beta), L = D - A
    l1    = sum_ik |beta_ik|

Two evaluations:
  four_sums_exact       for integer-valued inputs, in int64 (checked against overflow by a bound computed first).  Every partial sum a
                        device kernel can form from such inputs is an integer far below 2^53, which float64 (FMA and MFMA included)
                        represents exactly - so the device must return these integers bit for bit, whatever its summation order, and
                        one dropped, doubled or misplaced term changes an integer.
  four_sums_longdouble  for real inputs, in np.longdouble, with the sum of the absolute values of the terms of each sum: the scale of
                        the rounding bound  |got - want| <= depth * 2^-53 * sum|terms|  (depth = additions and roundings a term
                        passes through on the device; read from the kernels, see tests/test_gpu_fit_tail.py).

export_ref is normalize_proportions of the reference (core/solver.py:431-452): a zero row sum gives 1/K, otherwise the row divided by
np.maximum(sum, 1e-10), which hands a NaN on.  Row sums are math.fsum (the correctly rounded sum): for rows whose partial sums are all
exact - the test rows - every summation order gives that number.

to_planes / h_to_planes go from the caller's order to what the solver holds: type-major planes (K, ld) in the graph's own spot order
(perm[p] = caller's id at solver position p, from fdx_graph_perm_dev), ld = round_up(n + 1, 64), column n the all-zero row the padded
neighbour lists point at.  padded_lists and four_sums_planes restate the device's traversal over those planes on the host - neighbour
lists padded with index n to a common width - so that the host tests can show what a wrong layout or a non-zero pad row does.
"""
import math

import numpy as np
from scipy import sparse

U = 2.0 ** -53
TERMS = ("cross <H,beta>", "quad beta'XtX beta", "spat tr(beta'L beta)", "l1 |beta|_1")


def round_up(a, m):
    return (int(a) + m - 1) // m * m


def _structure(A, n):
    A = sparse.csr_matrix(A)
    assert A.shape == (n, n), (A.shape, n)
    A.sort_indices()
    return A.indptr.astype(np.int64), A.indices.astype(np.int64)


def _as_int(a, name):
    a = np.asarray(a)
    ai = np.rint(a).astype(np.int64)
    assert np.array_equal(ai.astype(np.float64), np.asarray(a, dtype=np.float64)), f"{name} is not integer-valued"
    return ai


def four_sums_exact(A, beta, H, XtX, spots=None, count_twice=None, quad_upper_weight=2, quad_block=64):
    """(cross, quad, spat, l1) as Python ints.  The keyword arguments plant the faults the host tests use:
    spots: only these spots contribute (None: all); count_twice: this spot contributes a second time; quad_upper_weight: the weight
    of a quad_block x quad_block block of XtX above the block diagonal when the quadratic term is summed over the blocks on and above
    it (2: the block stands for its mirror image too - the right answer for a symmetric XtX)."""
    B, Hi, G = _as_int(beta, "beta"), _as_int(H, "H"), _as_int(XtX, "XtX")
    n, K = B.shape
    assert Hi.shape == (K, n) and G.shape == (K, K)
    assert np.array_equal(G, G.T), "XtX must be symmetric"
    indptr, indices = _structure(A, n)
    deg = np.diff(indptr)
    bmax, hmax, gmax = int(np.abs(B).max(initial=0)), int(np.abs(Hi).max(initial=0)), int(np.abs(G).max(initial=0))
    bound = n * K * max(bmax * hmax, K * gmax * bmax * bmax, 2 * int(deg.max(initial=0)) * bmax * bmax, bmax, 1)
    assert bound < 2 ** 52, "sums would leave the integers float64 holds exactly"
    Adj = sparse.csr_matrix((np.ones(len(indices), dtype=np.int64), indices, indptr), shape=(n, n))
    NB = np.asarray(Adj @ B)                                        # neighbour sums, int64
    per_cross = (B * Hi.T).sum(1)
    nb_ = (K + quad_block - 1) // quad_block
    per_quad = np.zeros(n, dtype=np.int64)
    for a in range(nb_):
        ra = slice(a * quad_block, min(K, (a + 1) * quad_block))
        for b in range(a, nb_):
            rb = slice(b * quad_block, min(K, (b + 1) * quad_block))
            w = 1 if a == b else quad_upper_weight
            per_quad += w * ((B[:, ra] @ G[ra, rb]) * B[:, rb]).sum(1)
    per_spat = (B * (deg[:, None] * B - NB)).sum(1)
    per_l1 = np.abs(B).sum(1)
    w = np.zeros(n, dtype=np.int64)
    if spots is None:
        w[:] = 1
    else:
        w[np.asarray(spots, dtype=np.int64)] = 1
    if count_twice is not None:
        w[count_twice] += 1
    return tuple(int((w * p).sum()) for p in (per_cross, per_quad, per_spat, per_l1))


def four_sums_longdouble(A, beta, H, XtX):
    """((cross, quad, spat, l1), (sum|terms| of each)) in np.longdouble.  The terms: beta_ik H_ki; XtX_kl beta_ik beta_il;
    deg_i beta_ik^2 and beta_ik beta_jk per neighbour j; |beta_ik|."""
    ld = np.longdouble
    B, Hl, G = np.asarray(beta, dtype=ld), np.asarray(H, dtype=ld), np.asarray(XtX, dtype=ld)
    n, K = B.shape
    assert Hl.shape == (K, n) and G.shape == (K, K)
    indptr, indices = _structure(A, n)
    deg = np.diff(indptr).astype(ld)
    aB = np.abs(B)
    NB, aNB = np.zeros((n, K), dtype=ld), np.zeros((n, K), dtype=ld)
    rows = np.repeat(np.arange(n), np.diff(indptr))
    np.add.at(NB, rows, B[indices])
    np.add.at(aNB, rows, aB[indices])
    sums = ((B * Hl.T).sum(), ((B @ G) * B).sum(), (B * (deg[:, None] * B - NB)).sum(), aB.sum())
    mags = ((aB * np.abs(Hl.T)).sum(), ((aB @ np.abs(G)) * aB).sum(), (aB * (deg[:, None] * aB + aNB)).sum(), aB.sum())
    return sums, mags


def objective_from_sums(sums, YtY, lambda_, rho):
    """compute_objective (core/solver.py:269-284) from the four sums."""
    c, q, s, l1 = sums
    return 0.5 * (YtY - 2.0 * c + q) + 0.5 * lambda_ * s + rho * l1


def assert_sums_exact(got4, want4, label=""):
    """The device's four float64 sums against the exact integers, bit for bit; names every term that is off."""
    bad = [f"{TERMS[t]}: got {float(got4[t])!r}, want {want4[t]} (off by {float(got4[t]) - want4[t]:+.17g})"
           for t in range(4) if not (float(got4[t]) == float(want4[t]) and int(got4[t]) == want4[t])]
    assert not bad, f"objective sums off [{label}]: " + "; ".join(bad)


def assert_sums_close(got4, want4, mags4, depth4, label=""):
    """|got - want| <= depth * 2^-53 * sum|terms| per sum, want and sum|terms| in longdouble."""
    bad = []
    for t in range(4):
        err = abs(np.longdouble(got4[t]) - want4[t])
        tol = np.longdouble(depth4[t]) * np.longdouble(U) * mags4[t]
        if not err <= tol:                               # (a NaN fails)
            bad.append(f"{TERMS[t]}: got {float(got4[t])!r}, want {float(want4[t])!r}, |diff| {float(err):.3e} > bound {float(tol):.3e} "
                       f"(depth {depth4[t]})")
    assert not bad, f"objective sums outside their rounding bound [{label}]: " + "; ".join(bad)


# ------------------------------------------------------------------------------------------------ export
def row_sums(beta):
    return np.array([math.fsum(r) for r in np.asarray(beta, dtype=np.float64)], dtype=np.float64).reshape(-1)


def export_ref(beta):
    """(beta_out, prop_out) of the reference for beta (n, K) in the caller's order."""
    beta = np.array(beta, dtype=np.float64, order="C")
    n, K = beta.shape
    s = row_sums(beta)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        prop = beta / np.maximum(s, 1e-10)[:, None]
    prop[s == 0] = 1.0 / K
    return beta, prop


def export_ref_longdouble(beta):
    ld = np.longdouble
    B = np.asarray(beta, dtype=ld)
    s = B.sum(1)
    prop = B / np.maximum(s, ld(1e-10))[:, None]
    prop[s == 0] = ld(1.0) / B.shape[1]
    return prop


def assert_same_bits(got, want, what, label=""):
    """Bit-for-bit equality of two float64 arrays (so -0.0 != 0.0), except that any NaN matches any NaN; names the first rows off."""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    same = (got.view(np.int64) == want.view(np.int64)) | (np.isnan(got) & np.isnan(want))
    if same.all():
        return
    rows = np.flatnonzero(~same.reshape(got.shape[0], -1).all(1))
    r = int(rows[0])
    c = int(np.flatnonzero(~same[r])[0])
    raise AssertionError(f"{what} off [{label}]: {len(rows)} rows, first row {r} (others {rows[1:6].tolist()}), column {c}: "
                         f"got {got[r, c]!r}, want {want[r, c]!r}")


# ------------------------------------------------------------------------------------------------ layout
def to_planes(M, perm, ld=None, pad_row=0.0):
    """M (n, K) in the caller's order -> (K, ld) float64 planes in solver order: planes[k, p] = M[perm[p], k] for p < n, the pad row
    (column n) = pad_row (0.0: what the solver keeps there), zeros behind it."""
    M = np.asarray(M, dtype=np.float64)
    n, K = M.shape
    perm = np.arange(n) if perm is None else np.asarray(perm, dtype=np.int64)
    assert sorted(perm.tolist()) == list(range(n)), "perm is not a permutation"
    ld = round_up(n + 1, 64) if ld is None else int(ld)
    assert ld >= n + 1
    P = np.zeros((K, ld), dtype=np.float64)
    P[:, :n] = M[perm].T
    P[:, n] = pad_row
    return P


def h_to_planes(H, perm, ldh=None, fill=np.nan):
    """H (K, n) in the caller's order -> (K, ldh) in solver order; the columns past n hold `fill` (NaN: a read of them shows)."""
    H = np.asarray(H, dtype=np.float64)
    K, n = H.shape
    perm = np.arange(n) if perm is None else np.asarray(perm, dtype=np.int64)
    ldh = round_up(n + 1, 64) if ldh is None else int(ldh)
    assert ldh >= n
    P = np.full((K, ldh), fill, dtype=np.float64)
    P[:, :n] = H[:, perm]
    return P


def padded_lists(A, perm):
    """The neighbour lists as the device keeps them: (n, w) solver positions of the neighbours of the spot at each solver position,
    padded to the common width w with index n (the all-zero row)."""
    A = sparse.csr_matrix(A)
    n = A.shape[0]
    perm = np.arange(n) if perm is None else np.asarray(perm, dtype=np.int64)
    rank = np.empty(n, dtype=np.int64)
    rank[perm] = np.arange(n)
    indptr, indices = _structure(A, n)
    deg = np.diff(indptr)
    w = int(deg.max(initial=0))
    L = np.full((n, max(w, 1)), n, dtype=np.int64)
    for p in range(n):
        i = perm[p]
        L[p, :deg[i]] = rank[indices[indptr[i]:indptr[i + 1]]]
    return L, deg[perm]


def four_sums_planes(planes, Hplanes, XtX, lists, deg, n):
    """The four sums as a device traversal forms them: from the planes, walking the padded lists at their full width (a pad entry adds
    whatever column n holds).  Exact Python ints; integer-valued inputs only."""
    P = _as_int(planes, "planes")
    G = _as_int(XtX, "XtX")
    Hp = _as_int(np.asarray(Hplanes)[:, :n], "H planes")
    K = P.shape[0]
    own = P[:, :n]                                                  # (K, n)
    nb = P[:, lists].sum(2)                                         # (K, n): over the full width
    cross = int((own * Hp).sum())
    quad = int(((G @ own) * own).sum())
    spat = int((own * (np.asarray(deg)[None, :] * own - nb)).sum())
    l1 = int(np.abs(own).sum())
    assert K == G.shape[0]
    return cross, quad, spat, l1


# ------------------------------------------------------------------------------------------------ inputs
def integer_problem(n, K, seed):
    """beta in {-2..3} (n, K), H in {-4..4} (K, n), XtX symmetric in {-3..3}: the inputs of the exact comparison."""
    rs = np.random.RandomState(seed)
    beta = rs.randint(-2, 4, size=(n, K)).astype(np.float64)
    H = rs.randint(-4, 5, size=(K, n)).astype(np.float64)
    T = rs.randint(-3, 4, size=(K, K))
    XtX = (np.triu(T) + np.triu(T, 1).T).astype(np.float64)
    return beta, H, XtX


def real_problem(n, K, seed):
    """Real-valued inputs of the rounding comparison: abundances with negative entries, a positive semi-definite XtX."""
    rs = np.random.RandomState(seed)
    beta = rs.randn(n, K) * rs.rand(n, 1)
    H = rs.randn(K, n)
    X = rs.randn(K, K + 3)
    return beta, H, X @ X.T / K


def tie_free_coords(n, dim, seed):
    """Random coordinates whose pairwise distances are all distinct with probability one (no k-NN choice to make)."""
    return np.random.RandomState(seed).rand(n, dim) * 100.0


def hub_and_spoke(n):
    """Spot 0 is everybody's neighbour, and a ring joins the others: one row of degree n - 1 next to rows of degree 3."""
    if n == 1:
        return sparse.csr_matrix((1, 1), dtype=np.float64)
    r, c = [], []
    for i in range(1, n):
        r += [0, i]
        c += [i, 0]
        j = 1 + (i % (n - 1))
        if j != i:
            r += [i, j]
            c += [j, i]
    A = sparse.csr_matrix((np.ones(len(r)), (r, c)), shape=(n, n))
    A.sum_duplicates()
    A.data[:] = 1.0
    A.sort_indices()
    return A


EXPORT_KINDS = ("zero", "negzero", "tiny", "negative", "cancel")


def export_rows(n, K, positions_kinds, seed):
    """beta (n, K), integer-valued with exact row sums, rows >= 0 with a positive sum except the special rows:
    zero: all 0.0; negzero: all -0.0; tiny: sum 5e-11 (below the 1e-10 floor); negative: mixed signs, sum < 0;
    cancel: non-zero entries that cancel to exactly 0.  positions_kinds: {row: kind}."""
    rs = np.random.RandomState(seed)
    B = rs.randint(0, 6, size=(n, K)).astype(np.float64)
    B[np.arange(n), rs.randint(0, K, size=n)] += 1.0                # no accidental zero row
    for r, kind in positions_kinds.items():
        row = np.zeros(K)
        if kind == "zero":
            pass
        elif kind == "negzero":
            row[:] = -0.0
        elif kind == "tiny":
            if K >= 2:
                row[[0, K - 1]] = 2.5e-11                           # 2.5e-11 + 2.5e-11 = 5e-11 exactly
            else:
                row[0] = 5e-11
        elif kind == "negative":
            row = rs.randint(-2, 2, size=K).astype(np.float64)
            if row.sum() >= 0:
                row[0] -= row.sum() + 1.0
        elif kind == "cancel":
            if K >= 2:
                row = rs.randint(-3, 4, size=K).astype(np.float64)
                row[0] = 2.0
                row[K - 1] = 0.0
                row[K - 1] = -row.sum()
        else:
            raise ValueError(kind)
        B[r] = row
    return B
