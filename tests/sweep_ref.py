"""Host reference of ONE block-coordinate-descent sweep, element by element - plain numpy, no GPU, no project import.

One sweep (flashdeconv/core/solver.py:29-184 of the reference, as summarised at the top of csrc/bcd_kernels.cpp).  Inputs are in the
CALLER's spot order: a scipy adjacency A (structure only: every stored entry is a neighbour), beta_in (n, K), H (K, n), XtX (K, K; not
required to be symmetric - the kernels read row k as stored), lambda and rho.  For spot i and k = 0..K-1 in order, b starting as
beta_in[i]:

    c_k = sum_{j in N(i)} beta_in[j, k]
    r_k = sum_j XtX[k, j] b_j                                  (b_j already replaced for j < k)
    res = H[k, i] - r_k + XtX[k, k] b_k + (deg_i > 0 ? lambda c_k : 0)
    den = XtX[k, k] + lambda deg_i
    b_k = den > 1e-10 ? max(0, soft(res, rho) / den) : 0

and the statistics max_diff = max |new - old|, max_abs_old = max |old|, rel_change = max_diff / (max_abs_old + 1e-10).

Two evaluations:
  sweep_exact       for the integer problems of integer_sweep_problem: XtX has nothing below its diagonal, so r_k meets only OLD,
                    integer abundances (the replaced b_j, j < k, are multiplied by an exact 0), every res and den is an integer -
                    evaluated in int64, an overflow bound asserted first - and the new value is the float64 quotient
                    float(st) / float(den): ONE correctly rounded division.  The project builds without fast-math, so a device kernel
                    must return that very number whatever its summation order, and one wrong operand changes an integer.
  sweep_longdouble  for real inputs, in np.longdouble, with a per-element bound E (n, K) that runs along with the coordinate steps.
                    With u = 2^-53, w the widest neighbour list and depth = K + w + 8:

                        T_k = |H_ki| + sum_j |XtX_kj| |b_j| + |XtX_kk| |b_k| + lambda sum_{j in N(i)} |beta_in[j, k]|
                        E_k = (depth u T_k + sum_{j<k} |XtX_kj| E_j) / den + 3 u |want_k|

                    depth bounds the roundings a term of res passes through in any of the four sweep kernels:
                      K   the row product.  bcd_sweep_kernel and bcd_sweep_tiled_kernel (csrc/bcd_sweep_inst.cpp): two chains of
                          K / 2 fmas (r0, r1) and their sum; bcd_sweep_generic_kernel (csrc/bcd_kernels.cpp): the same;
                          bcd_sweep_lds_kernel: per lane group two chains of KP / 8 fmas, their sum and two shuffle additions - all
                          at most K + 1, and a term of a chain of K / 2 passes through K / 2 of them
                      w   the neighbour sum: w additions in the register kernels (the tiled one adds its zero slot up to position 16:
                          an exact + 0.0) and in the generic kernel, w / 4 + 2 in the LDS kernel
                      8   `r0 + r1`, `h - r`, `gkk * old` and its addition, `lam_eff * c` and its addition, the subtraction of rho,
                          one spare
                    den = fl(XtX_kk + fl(lambda deg)) carries two roundings and the division one: 3 u |want_k|.  Soft threshold and
                    max(0, .) are 1-Lipschitz: the bound passes through them.  The error of the replaced b_j enters r_k with
                    |XtX_kj|.  The switch den > 1e-10 is kept far from the inputs by real_sweep_problem (XtX_kk >= 1).

sweep_planes restates the DEVICE's traversal - type-major planes in the graph's order (to_planes / h_to_planes of fit_tail_ref.py),
padded neighbour lists, chunks of KC types, tiles of 256 spots - with knobs that plant the faults a sweep kernel can plausibly have;
tests/test_sweep_host.py shows that each one trips the comparators below on the GPU tests' own base problem.
"""
import numpy as np
from scipy import sparse

from fit_tail_ref import U, _as_int, _structure

SENTINEL = -777.25
FULL_K = tuple(range(1, 65)) + (72, 80, 88, 96)          # every register-resident instantiation (csrc/Makefile: PARTS)
REAL_LAMBDA, REAL_RHO = 0.3, 0.2                         # of the real problems (not dyadic: lambda deg and res - rho round)


# ------------------------------------------------------------------------------------------------ statistics
def rel_change(beta_in, beta_out, spots=None):
    """max |new - old| / (max |old| + 1e-10) over `spots` (None: all), each operation in float64 as the kernels do it (max is exact
    and order-free)."""
    old, new = np.asarray(beta_in, dtype=np.float64), np.asarray(beta_out, dtype=np.float64)
    if spots is not None:
        old, new = old[np.asarray(spots, dtype=np.int64)], new[np.asarray(spots, dtype=np.int64)]
    return float(np.abs(new - old).max(initial=0.0) / (np.abs(old).max(initial=0.0) + 1e-10))


def _shares(res, rho, new, info):
    if info is None:
        return
    tot = float(res.size)
    info.update(res_above=float((res > rho).sum()) / tot, res_below=float((res < -rho).sum()) / tot,
                res_inside=float((np.abs(res) <= rho).sum()) / tot, clamped=float((new == 0).sum()) / tot,
                positive=float((new > 0).sum()) / tot)


def assert_branch_shares(info, rho, label="", least=0.05):
    """The conditions on the integer problems: every branch of the update in at least 5 % of the elements."""
    names = ["res_above", "res_below", "clamped", "positive"] + (["res_inside"] if rho > 0 else [])
    low = {k: round(info[k], 4) for k in names if not info[k] >= least}
    assert not low, f"branches too rare in the reference [{label}]: {low}"


# ------------------------------------------------------------------------------------------------ exact
def sweep_exact(A, beta_in, H, XtX, lam, rho, info=None):
    """(beta_out (n, K) float64, rel_change float64) of one sweep of an integer problem whose XtX is zero below the diagonal.
    info (a dict) receives the share of the elements on each branch."""
    B, Hi, G = _as_int(beta_in, "beta_in"), _as_int(H, "H"), _as_int(XtX, "XtX")
    lam_i, rho_i = int(lam), int(rho)
    assert lam_i == lam and rho_i == rho and lam_i >= 0 and rho_i >= 0, "lambda and rho must be non-negative integers"
    n, K = B.shape
    assert Hi.shape == (K, n) and G.shape == (K, K)
    assert not np.tril(G, -1).any(), "XtX must be zero below the diagonal: r_k may only meet old (integer) abundances"
    indptr, indices = _structure(A, n)
    deg = np.diff(indptr)
    bmax, hmax, gmax = int(np.abs(B).max(initial=0)), int(np.abs(Hi).max(initial=0)), int(np.abs(G).max(initial=0))
    bound = hmax + (K + 1) * gmax * bmax + lam_i * int(deg.max(initial=0)) * bmax + rho_i + gmax + lam_i * int(deg.max(initial=0))
    assert bound < 2 ** 52, "res would leave the integers float64 holds exactly"
    Adj = sparse.csr_matrix((np.ones(len(indices), dtype=np.int64), indices, indptr), shape=(n, n))
    NB = np.asarray(Adj @ B)                                         # c_k, int64
    d = np.diag(G).copy()
    R = B @ np.triu(G).T                                             # R[i, k] = sum_{j >= k} XtX[k, j] beta_in[i, j]
    res = Hi.T - R + d[None, :] * B + np.where(deg[:, None] > 0, lam_i * NB, 0)
    den = d[None, :] + lam_i * deg[:, None]
    st = np.where(res > rho_i, res - rho_i, np.where(res < -rho_i, res + rho_i, 0))
    new = np.zeros((n, K), dtype=np.float64)
    ok = den > 0                                                     # an integer: den > 1e-10 is den >= 1
    new[ok] = np.maximum(st[ok].astype(np.float64) / den[ok].astype(np.float64), 0.0)
    new += 0.0                                                       # no -0.0
    _shares(res, rho_i, new, info)
    return new, rel_change(B.astype(np.float64), new)


# ------------------------------------------------------------------------------------------------ long double
def sweep_longdouble(A, beta_in, H, XtX, lam, rho, info=None):
    """(want (n, K), E (n, K)) in np.longdouble: one sweep and its per-element rounding bound (module docstring)."""
    ld = np.longdouble
    B, Hl, G = np.asarray(beta_in, dtype=ld), np.asarray(H, dtype=ld), np.asarray(XtX, dtype=ld)
    lam, rho, u = ld(lam), ld(rho), ld(U)
    n, K = B.shape
    assert Hl.shape == (K, n) and G.shape == (K, K)
    indptr, indices = _structure(A, n)
    degi = np.diff(indptr)
    deg = degi.astype(ld)
    depth = ld(K + int(degi.max(initial=0)) + 8)
    rows = np.repeat(np.arange(n), degi)
    NB, aNB = np.zeros((n, K), dtype=ld), np.zeros((n, K), dtype=ld)
    np.add.at(NB, rows, B[indices])
    np.add.at(aNB, rows, np.abs(B)[indices])
    aG = np.abs(G)
    lam_eff = np.where(degi > 0, lam, ld(0))
    b = B.copy()
    E = np.zeros((n, K), dtype=ld)
    res_all = np.empty((n, K), dtype=ld)
    for k in range(K):
        old = b[:, k].copy()
        r = b @ G[k]
        T = np.abs(Hl[k]) + np.abs(b) @ aG[k] + aG[k, k] * np.abs(old) + lam * aNB[:, k]
        res = Hl[k] - r + G[k, k] * old + lam_eff * NB[:, k]
        den = G[k, k] + lam * deg
        st = np.where(res > rho, res - rho, np.where(res < -rho, res + rho, ld(0)))
        live = den > ld(1e-10)
        sden = np.where(live, den, ld(1))
        new = np.where(live, np.maximum(st / sden, ld(0)), ld(0))
        E[:, k] = np.where(live, (depth * u * T + E[:, :k] @ aG[k, :k]) / sden, ld(0)) + 3 * u * np.abs(new)
        b[:, k] = new
        res_all[:, k] = res
    _shares(res_all, rho, b, info)
    return b, E


# ------------------------------------------------------------------------------------------------ comparators
def _where(bad, got, want, n_show=4):
    idx = np.argwhere(bad)
    return f"{len(idx)} elements in {len(np.unique(idx[:, 0]))} spots, first " + "; ".join(
        f"(spot {i}, type {k}): got {got[i, k]!r}, want {float(want[i, k])!r}" for i, k in idx[:n_show].tolist())


def assert_sweep_exact(got, want, label=""):
    """Value for value (the sign of a zero is not compared; a NaN never equals)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    if not np.array_equal(got, want):
        raise AssertionError(f"sweep off [{label}]: " + _where(~(got == want), got, want))


def assert_sweep_close(got, want, E, label=""):
    """|got - want| <= E per element (a NaN fails); returns the largest err / E."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape == E.shape, (label, got.shape, want.shape, E.shape)
    err = np.abs(got.astype(np.longdouble) - want)
    bad = ~(err <= E)
    if bad.any():
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = float(np.nanmax(np.where(E > 0, err / np.where(E > 0, E, 1), np.where(err > 0, np.inf, 0))))
        raise AssertionError(f"sweep outside its rounding bound [{label}] (worst err / E {worst:.3g}): " + _where(bad, got, want))
    pos = E > 0
    return float((err[pos] / E[pos]).max()) if pos.any() else 0.0


# ------------------------------------------------------------------------------------------------ inputs
def integer_sweep_problem(n, K, seed, coupling):
    """beta_in in {-2..3} (n, K), H in {-40..40} (K, n), XtX: diagonal in {1..4}; coupling "none": nothing else, "upper": entries in
    {-3..3} strictly above the diagonal.  lambda in {1, 2} and rho in {0, 3} are the caller's."""
    assert coupling in ("none", "upper")
    rs = np.random.RandomState(seed)
    beta = rs.randint(-2, 4, size=(n, K)).astype(np.float64)
    H = rs.randint(-40, 41, size=(K, n)).astype(np.float64)
    XtX = np.diag(rs.randint(1, 5, size=K)).astype(np.float64)
    if coupling == "upper":
        XtX += np.triu(rs.randint(-3, 4, size=(K, K)), 1)
    return beta, H, XtX


def real_sweep_problem(n, K, seed):
    """Real inputs of the rounding comparison: XtX dense, XtX_kk in [1, 2], sum_{j != k} |XtX_kj| <= 0.5 XtX_kk (not symmetric);
    beta_in >= 0; H such that with REAL_LAMBDA and REAL_RHO all three branches of the soft threshold occur."""
    rs = np.random.RandomState(seed)
    beta = rs.rand(n, K) * rs.rand(n, 1)
    diag = 1.0 + rs.rand(K)
    off = rs.randn(K, K)
    np.fill_diagonal(off, 0.0)
    s = np.abs(off).sum(1)
    off *= (0.5 * diag * (0.5 + 0.5 * rs.rand(K)) / np.where(s > 0, s, 1.0))[:, None]
    XtX = off + np.diag(diag)
    assert (np.abs(off).sum(1) <= 0.5 * diag).all()
    H = 0.6 * rs.randn(K, n)
    return beta, H, XtX


# ------------------------------------------------------------------------------------------------ the device's traversal
def from_planes(planes, perm, n):
    """(K, >= n) planes in solver order -> (n, K) in the caller's order."""
    planes = np.asarray(planes)
    out = np.empty((n, planes.shape[0]), dtype=planes.dtype)
    out[np.arange(n) if perm is None else np.asarray(perm, dtype=np.int64)] = planes[:, :n].T
    return out


def sweep_planes(P, Hp, XtX, lists, deg, n, lam, rho, KC, dtype=np.float64, tile=256, slot_shift=None, halo_prev_chunk=False,
                 h_next_chunk=False, stale_b=None, deg_condition=True, skip_last=False):
    """One sweep as a device kernel walks it: planes P (K, ld) with the pad row at column n, H planes, neighbour lists (n, w) of solver
    positions padded with n, chunks of KC types, tiles of `tile` spots.  Returns the new planes (K, n); spots not written hold SENTINEL.
    dtype float64 for the integer problems (every operation exact but the one division), longdouble for real ones.  The faults:
      slot_shift=(p, m)       spot p's neighbour slot m reads the position one further
      halo_prev_chunk         from the second chunk on, a neighbour outside the spot's tile is read from type k - KC
      h_next_chunk            H of type k + KC is used for type k (where it exists)
      stale_b=(k, j)          the row product of type k takes the OLD b_j, j < k
      deg_condition=False     lambda c_k is added whatever the degree
      skip_last               the last spot is not swept
    (a non-zero pad row comes in through P itself: to_planes(..., pad_row=...))."""
    P, Hp, G = np.asarray(P, dtype=dtype), np.asarray(Hp, dtype=dtype), np.asarray(XtX, dtype=dtype)
    lam, rho = dtype(lam), dtype(rho)
    K = P.shape[0]
    lists = np.array(lists, dtype=np.int64)
    if slot_shift is not None:
        p, m = slot_shift
        assert lists[p, m] < n
        lists[p, m] += 1
    deg = np.asarray(deg)
    pos = np.arange(n)
    halo = (lists != n) & (lists // tile != (pos // tile)[:, None])
    b = P[:, :n].T.copy()
    old_all = b.copy()
    out = np.full((K, n), SENTINEL, dtype=dtype)
    lam_eff = np.where(deg > 0, lam, dtype(0)) if deg_condition else np.full(n, lam, dtype=dtype)
    for k in range(K):
        src = P[k][lists]
        if halo_prev_chunk and k >= KC:
            src = np.where(halo, P[k - KC][lists], src)
        c = src.sum(1)
        h = Hp[k + KC, :n] if (h_next_chunk and k + KC < K) else Hp[k, :n]
        bb = b
        if stale_b is not None and stale_b[0] == k:
            bb = b.copy()
            bb[:, stale_b[1]] = old_all[:, stale_b[1]]
        r = bb @ G[k]
        old = b[:, k].copy()
        res = h - r + G[k, k] * old + lam_eff * c
        den = G[k, k] + lam * deg.astype(dtype)
        st = np.where(res > rho, res - rho, np.where(res < -rho, res + rho, dtype(0)))
        live = den > dtype(1e-10)
        new = np.where(live, np.maximum(st / np.where(live, den, dtype(1)), dtype(0)), dtype(0))
        b[:, k] = new
        out[k] = new
    if skip_last:
        out[:, n - 1] = SENTINEL
    return out
