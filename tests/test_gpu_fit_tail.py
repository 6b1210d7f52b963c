"""-m gpu tests of the fit tail, term by term: the four sums of the objective on every route of solver_objective_partials
(csrc/solver.cpp) and the normalising export (normalize_export_kernel, csrc/finish_kernels.cpp) on both of its branches.

Seams:  fdx_objective_partials_dev returns (cross, quad, spat, l1) separately; FDX_NO_TILED=1 sends a tiled graph through the generic
kernel; fdx_graph_tile_info says which traversal a graph takes (every test asserts the route it means to take); fdx_export_dev is the
export of a fit (the graph's own perm), fdx_normalize_dev the export in the graph's own order.

Objective, exact.  beta in {-2..3}, H in {-4..4}, XtX symmetric in {-3..3}: every partial sum any kernel can form is an integer far
below 2^53, exact in float64 through FMA and MFMA alike, so the four device sums must EQUAL the integers of tests/fit_tail_ref.py,
whatever the summation order.  The graph's truth is the oracle's adjacency of the same coordinates (or the CSR handed in), never the
device graph's own export.  beta and H reach the device as the solver holds them (type-major planes in the graph's order, an all-zero
pad row at column n, ld = round_up(n + 1, 64)); the columns of H past n hold NaN, so a lane past n that read them would show.

Routes (solver_objective_partials):
    tiled traversal with the quadratic term          bcd_sweep_tiled_kernel<K, KC, true>           K = 1..64 on a tiled graph
    tiled traversal without it + beta_quad<5 | 6>    bcd_sweep_tiled_kernel<K, KC, true, false>    K = 72, 80, 88, 96 on a tiled graph
    generic kernel with the quadratic term           objective_partials_kernel, skip_quad = 0      K <= 64, FDX_NO_TILED or untiled graph
    generic kernel + beta_quad<5..7>                 skip_quad = 1                                 65 <= K <= 112 without a tiled instance
    generic kernel + beta_quad_block_kernel          skip_quad = 1, blocks of 64 types             K >= 113

Objective, rounding.  Real inputs, |got - want| <= depth * 2^-53 * sum|terms| per sum, want and sum|terms| in longdouble.  depth is
the number of roundings a term passes through, read from the kernels (w = widest neighbour list, S = slices of 64 spots one wave of
beta_quad walks = ceil(ceil(n / 64) / (4 * grid)), grid = min(256, rows, ceil(n / 256))):
    tail, all routes and sums: 6 shuffle levels + 3 additions of the 4-wave fold + 10 tree levels of sum_partials_kernel (at most 1024
          rows here: every thread's strided sum is one row) = 19
    cross, l1:    K  (one fma / one addition per type in the lane)                                              K + 19
    spat:         w additions of the neighbour sum, deg * b, the subtraction, K fmas                            w + 2 + K + 19
    quad, in the traversal (both kernels): at most K fmas of the row product (two chains of K / 2 and their sum in the tiled
                  kernel), K fmas over the types                                                                2 K + 19
    quad, beta_quad<TT>: the product, 64 S accumulations of a wave's spots, 4 fmas with XtX, TT (TT + 1) / 2 tile pairs,
                  6 shuffle levels, 2 additions of the wave fold, 10 tree levels                                64 S + TT (TT + 1) / 2 + 23
    quad, block kernel: the product, 64 S accumulations, 64 fmas with XtX (16 tiles x 4 registers), 6 + 2, one += per launch
                  (B (B + 1) / 2 launches, B = ceil(ceil(K / 16) / 4)), 10 tree levels                          64 S + B (B + 1) / 2 + 83

Export.  Integer-valued rows with exact sums (and the special rows: all zero, all -0.0, sum 5e-11, negative sum, cancelling to zero),
division correctly rounded (no fast-math in the build): beta_out and prop_out must equal the reference's bits; the outputs start as
a sentinel, so a row left out shows, and 64 doubles behind them must keep it.  K <= 63 takes the LDS branch (element f of a wave's
64 x K block advances (spot, type) by (64 / K, 64 % K) with a carry: K = 1, 2, 3, 5, 7, 32, 33, 63), K >= 64 the direct one.
"""
import ctypes

import numpy as np
import pytest
from scipy import sparse

import fdx_oracle as orc
import fit_tail_ref as ref
from gpu_graphs import _assert_tiled, _assert_untiled, _dev, _grid, _hub, _knn, _knn_untiled, _radius_isolated

pytestmark = pytest.mark.gpu

N_BASE = 600
N_LIST = (1, 63, 64, 65, 255, 256, 257, 600)
SENTINEL = -777.25


# ------------------------------------------------------------------------------------------------ device calls
def _device_sums(G, beta, H, XtX, ld=None, ldh=None):
    import torch
    from flashdeconv_amd import _lib
    K = beta.shape[1]
    P, Hp = ref.to_planes(beta, G.perm, ld), ref.h_to_planes(H, G.perm, ldh)
    dP, dH, dG = _dev(P), _dev(Hp), _dev(np.asarray(XtX, dtype=np.float64))
    out = (ctypes.c_double * 4)()
    _lib.check(_lib.load().fdx_objective_partials_dev(G.g.handle, ctypes.c_void_p(dP.data_ptr()), P.shape[1], ctypes.c_void_p(dH.data_ptr()),
                                                      Hp.shape[1], ctypes.c_void_p(dG.data_ptr()), K, out, None))
    torch.cuda.synchronize()
    return [out[0], out[1], out[2], out[3]]


_problems = {}


def _problem(n, K):
    if (n, K) not in _problems:
        beta, H, XtX = ref.integer_problem(n, K, 1000 * K + n)
        _problems[(n, K)] = (beta, H, XtX)
    return _problems[(n, K)]


_exact = {}


def _check_exact(G, K, label, ld=None, ldh=None, key=None):
    beta, H, XtX = _problem(G.n, K)
    ck = (key, G.n, K)
    if key is None or ck not in _exact:
        want = ref.four_sums_exact(G.A, beta, H, XtX)
        if key is not None:
            _exact[ck] = want
    else:
        want = _exact[ck]
    got = _device_sums(G, beta, H, XtX, ld, ldh)
    ref.assert_sums_exact(got, want, f"{label}, n={G.n}, K={K}")


# ------------------------------------------------------------------------------------------------ objective, exact
@pytest.mark.parametrize("K", list(range(1, 65)))
def test_tiled_objective_with_quadratic_term(K):
    G = _knn(N_BASE)
    _assert_tiled(G)
    _check_exact(G, K, "tiled traversal, quad inside", key="knn")


@pytest.mark.parametrize("K", [72, 80, 88, 96])
def test_tiled_objective_padded_sizes_with_beta_quad(K):
    G = _knn(N_BASE)
    _assert_tiled(G)
    _check_exact(G, K, "tiled traversal + beta_quad", key="knn")


@pytest.mark.parametrize("K", [1, 2, 7, 31, 63, 64])
def test_generic_objective_on_a_tiled_graph(K, monkeypatch):
    G = _knn(N_BASE)
    _assert_tiled(G)                                  # the same graph as above: only the switch selects the generic kernel
    monkeypatch.setenv("FDX_NO_TILED", "1")
    _check_exact(G, K, "generic kernel (FDX_NO_TILED), quad inside", key="knn")


@pytest.mark.parametrize("K", [1, 2, 7, 31, 63, 64])
def test_generic_objective_hub_and_spoke(K):
    G = _hub(N_BASE)
    _assert_untiled(G)
    assert G.max_deg == N_BASE - 1
    _check_exact(G, K, "generic kernel, hub and spoke")


@pytest.mark.parametrize("K", [65, 70, 81, 97, 112])
@pytest.mark.parametrize("tiled", [True, False])
def test_generic_objective_with_beta_quad(K, tiled):
    if tiled:                                         # no tiled instance at these K: the graph's tiles are not used
        G = _knn(N_BASE)
        _assert_tiled(G)
    else:
        G = _knn_untiled(N_BASE)
        _assert_untiled(G)
    _check_exact(G, K, f"generic kernel + beta_quad<{(K + 15) // 16}>", key="knn")


@pytest.mark.parametrize("K", [113, 128, 129, 200, 272, 300])     # 2, 2, 3, 4, 5, 5 blocks of 64 types; ragged and exact last tiles
def test_generic_objective_with_block_kernel(K):
    G = _knn_untiled(N_BASE)
    _assert_untiled(G)
    _check_exact(G, K, "generic kernel + beta_quad_block_kernel", key="knn")


@pytest.mark.parametrize("n", N_LIST)
@pytest.mark.parametrize("K", [31, 72, 130])
def test_objective_spot_counts(n, K):
    if K == 130:
        G = _knn_untiled(n)
        _assert_untiled(G)
    else:
        G = _knn(n)
        if n == 1:
            _assert_untiled(G)                        # no k-NN graph of one spot: the generic kernel takes it
        else:
            _assert_tiled(G)
    _check_exact(G, K, "spot counts")


@pytest.mark.parametrize("K", [31, 72])
def test_tiled_objective_rows_longer_than_16_slots(K):
    G = _knn(N_BASE, k=20, seed=12)
    _assert_tiled(G)
    assert G.max_deg > 16
    _check_exact(G, K, "k = 20: slots past 16 read from memory")


@pytest.mark.parametrize("K", [8, 31, 72])
def test_tiled_objective_halo_above_256(K):
    G = _knn(2000, k=48, seed=12)
    _assert_tiled(G, min_halo=256)                    # the second round of the halo staging loop (h = tid + 256)
    _check_exact(G, K, "halo above 256")


@pytest.mark.parametrize("K", [31, 72, 130])
def test_objective_radius_graph_with_isolated_spots(K):
    G = _radius_isolated()
    _assert_tiled(G)
    deg = np.diff(G.A.indptr)[G.perm]                 # in the graph's order
    assert (deg == 0).sum() >= 200
    widths = [deg[s:s + 64].max() for s in range(0, G.n, 64)]
    assert min(widths) == 0 and max(widths) > 0, widths
    _check_exact(G, K, "radius graph, isolated spots")


@pytest.mark.parametrize("K", [31, 72])
def test_objective_grid_graph(K):
    G = _grid()
    _assert_tiled(G)
    assert G.max_deg == 8
    _check_exact(G, K, "grid graph")


@pytest.mark.parametrize("K", [31, 72, 130])
def test_objective_leading_dimensions_above_the_minimum(K):
    G = _knn(N_BASE)
    _assert_tiled(G)
    ld, ldh = ref.round_up(N_BASE + 1, 64) + 64, N_BASE + 13
    assert ld != ldh and ld > ref.round_up(N_BASE + 1, 64) and ldh > N_BASE
    _check_exact(G, K, "ld and ldh above the minimum", ld=ld, ldh=ldh, key="knn")


@pytest.mark.parametrize("K", [72, 130])
def test_objective_70000_spots_beta_quad_second_step(K):
    """beta_quad's grid is capped at 256 workgroups of 4 waves = 1024 slices = 65 536 spots per step: the slice loop takes a second
    step here (K = 72: behind the tiled traversal; K = 130: the block kernel behind the generic one)."""
    n = 70000
    G = _knn(n)
    _assert_tiled(G)
    assert (n + 63) // 64 > 256 * 4 and min(256, G.tile[0], (n + 255) // 256) == 256
    _check_exact(G, K, "70000 spots")


# ------------------------------------------------------------------------------------------------ objective, rounding
def _tail_depth():
    return 6 + 3 + 10


def _quad_depth(route, n, K, rows):
    if route == "traversal":
        return 2 * K + _tail_depth()
    grid = min(256, rows, (n + 255) // 256)
    S = -(-((n + 63) // 64) // (4 * grid))
    TT = (K + 15) // 16
    if route == "beta_quad":
        assert TT <= 7
        return 64 * S + TT * (TT + 1) // 2 + 23
    assert route == "block" and TT > 7
    B = (TT + 3) // 4
    return 64 * S + B * (B + 1) // 2 + 83


@pytest.mark.parametrize("route,K,quad", [
    ("tiled", 31, "traversal"), ("tiled", 72, "beta_quad"), ("no_tiled", 31, "traversal"), ("hub", 64, "traversal"),
    ("untiled", 97, "beta_quad"), ("untiled", 200, "block")])
def test_objective_rounding(route, K, quad, monkeypatch):
    G = {"tiled": _knn, "no_tiled": _knn, "hub": _hub, "untiled": _knn_untiled}[route](N_BASE)
    if route in ("tiled", "no_tiled"):
        _assert_tiled(G)
        if route == "no_tiled":
            monkeypatch.setenv("FDX_NO_TILED", "1")
    else:
        _assert_untiled(G)
    beta, H, XtX = ref.real_problem(G.n, K, 77 + K)
    want, mags = ref.four_sums_longdouble(G.A, beta, H, XtX)
    w = G.max_deg
    rows = (G.n + 255) // 256                                           # tiles, or blocks of four slices: the same number
    depth = (K + _tail_depth(), _quad_depth(quad, G.n, K, rows), w + 2 + K + _tail_depth(), K + _tail_depth())
    got = _device_sums(G, beta, H, XtX)
    for t in range(4):
        print(f"{route} K={K} {ref.TERMS[t]}: |diff| {float(abs(np.longdouble(got[t]) - want[t])):.3e}, bound "
              f"{float(depth[t] * ref.U * mags[t]):.3e} (depth {depth[t]})")
    ref.assert_sums_close(got, want, mags, depth, f"{route}, K={K}")


# ------------------------------------------------------------------------------------------------ fdx_objective / compute_objective
@pytest.mark.parametrize("K", [7, 130])
def test_compute_objective_with_negative_abundances(K):
    """The scalar from the four exact sums; YtY an integer, lambda and rho dyadic: every operation of the assembly is exact, on both
    sides, so the objective is compared bit for bit."""
    from flashdeconv_amd.core.solver import compute_objective
    n = 300
    A = orc.knn_graph_kdtree(ref.tie_free_coords(n, 2, 21), 6)
    beta, H, XtX = ref.integer_problem(n, K, 5 + K)
    assert (beta < 0).any()
    L = (sparse.diags(np.asarray(A.sum(1)).ravel()) - A).tocsr()
    YtY, lam, rho = 4321.0, 0.25, 0.125
    want = ref.objective_from_sums(ref.four_sums_exact(A, beta, H, XtX), YtY, lam, rho)
    assert want == orc.objective(beta, H, XtX, YtY, A, lam, rho)
    got = compute_objective(beta, H, XtX, YtY, L, lam, rho)
    assert got == want, (got, want, got - want)


# ------------------------------------------------------------------------------------------------ export
def _special_positions(n):
    return sorted({p for p in (0, 1, 2, 62, 63, 64, 65, 126, 127, 128, 254, 255, 256, 257, n - 2, n - 1) if 0 <= p < n})


def _export_case(G, K, rotation, seed):
    """beta in the caller's order with the special rows at the graph's positions 0, 63 | 64, 255 | 256 (first and last spot of a slice
    and of a tile), n - 1, ... - the kinds dealt round-robin from `rotation`."""
    pos = _special_positions(G.n)
    perm = np.arange(G.n) if G.perm is None else G.perm
    kinds = {int(perm[p]): ref.EXPORT_KINDS[(j + rotation) % len(ref.EXPORT_KINDS)] for j, p in enumerate(pos)}
    return ref.export_rows(G.n, K, kinds, seed), kinds


def _device_export(G, B, route, want_beta=True, want_prop=True, ld=None):
    import torch
    from flashdeconv_amd import _lib
    n, K = B.shape
    P = ref.to_planes(B, G.perm if route == "export" else None, ld)
    dP = _dev(P)
    outs = [torch.full((n * K + 64,), SENTINEL, dtype=torch.float64, device="cuda:0") for _ in range(2)]
    pb = ctypes.c_void_p(outs[0].data_ptr()) if want_beta else None
    pp = ctypes.c_void_p(outs[1].data_ptr()) if want_prop else None
    lib = _lib.load()
    if route == "export":
        _lib.check(lib.fdx_export_dev(G.g.handle, ctypes.c_void_p(dP.data_ptr()), P.shape[1], K, pb, pp, None))
    else:
        _lib.check(lib.fdx_normalize_dev(ctypes.c_void_p(dP.data_ptr()), P.shape[1], n, K, pb, pp, None))
    torch.cuda.synchronize()
    res = []
    for o in outs:
        o = o.cpu().numpy()
        assert (o[n * K:] == SENTINEL).all(), "written behind the output"
        res.append(o[:n * K].reshape(n, K))
    return res


def _check_export(G, K, route, label):
    n = G.n
    for rotation in range(1 if len(_special_positions(n)) >= len(ref.EXPORT_KINDS) else len(ref.EXPORT_KINDS)):
        B, kinds = _export_case(G, K, rotation, 31 * K + n + rotation)
        if n >= len(ref.EXPORT_KINDS):
            assert set(kinds.values()) == set(ref.EXPORT_KINDS)
        want_beta, want_prop = ref.export_ref(B)
        got_beta, got_prop = _device_export(G, B, route)
        where = f"{label}, {route}, n={n}, K={K}, rotation {rotation}"
        assert not (got_beta == SENTINEL).any() and not (got_prop == SENTINEL).any(), f"rows left unwritten [{where}]"
        ref.assert_same_bits(got_beta, want_beta, "beta_out", where)
        ref.assert_same_bits(got_prop, want_prop, "prop_out", where)


EXPORT_K = [1, 2, 3, 5, 7, 32, 33, 63, 64, 65, 100, 300]


@pytest.mark.parametrize("K", EXPORT_K)
def test_export_in_the_callers_order(K):
    G = _knn(N_BASE)
    _assert_tiled(G)                                  # (also: the perm is not the identity)
    _check_export(G, K, "export", "device-built k-NN graph")


@pytest.mark.parametrize("K", EXPORT_K)
def test_normalize_in_the_graphs_order(K):
    _check_export(_knn_untiled(N_BASE), K, "normalize", "identity order")


@pytest.mark.parametrize("n", N_LIST)
@pytest.mark.parametrize("K", [5, 65])
def test_export_spot_counts(n, K):
    G = _knn(n)
    _check_export(G, K, "export", "spot counts")
    _check_export(G, K, "normalize", "spot counts")


@pytest.mark.parametrize("K", [7, 65])
def test_export_leading_dimension_above_the_minimum(K):
    G = _knn(N_BASE)
    B, _ = _export_case(G, K, 2, 9)
    want_beta, want_prop = ref.export_ref(B)
    got_beta, got_prop = _device_export(G, B, "export", ld=ref.round_up(N_BASE + 1, 64) + 192)
    ref.assert_same_bits(got_beta, want_beta, "beta_out", f"ld above the minimum, K={K}")
    ref.assert_same_bits(got_prop, want_prop, "prop_out", f"ld above the minimum, K={K}")


@pytest.mark.parametrize("route", ["export", "normalize"])
@pytest.mark.parametrize("K", [7, 65])
def test_export_null_outputs(K, route):
    G = _knn(N_BASE)
    B, _ = _export_case(G, K, 1, 4)
    want_beta, want_prop = ref.export_ref(B)
    got_beta, got_prop = _device_export(G, B, route, want_beta=False)
    assert (got_beta == SENTINEL).all()
    ref.assert_same_bits(got_prop, want_prop, "prop_out", f"beta_out null, {route}, K={K}")
    got_beta, got_prop = _device_export(G, B, route, want_prop=False)
    assert (got_prop == SENTINEL).all()
    ref.assert_same_bits(got_beta, want_beta, "beta_out", f"prop_out null, {route}, K={K}")
    got_beta, got_prop = _device_export(G, B, route, want_beta=False, want_prop=False)     # returns, nothing written
    assert (got_beta == SENTINEL).all() and (got_prop == SENTINEL).all()


@pytest.mark.parametrize("route", ["export", "normalize"])
@pytest.mark.parametrize("K", [1, 7, 63, 64, 65])
def test_export_row_with_a_nan_comes_out_all_nan(K, route):
    """np.maximum(row sum, 1e-10) hands a NaN on: the reference's row is all NaN (fmax would answer 1e-10 and export v / 1e-10)."""
    G = _knn(N_BASE)
    perm = G.perm
    B, kinds = _export_case(G, K, 3, 6)
    rows = [int(perm[p]) for p in (5, 70, 300, N_BASE - 1)]
    rows = [r for r in rows if r not in kinds] + [int(perm[N_BASE - 1])]
    rs = np.random.RandomState(K)
    for r in rows:
        B[r] = rs.randint(1, 5, size=K)
        B[r, rs.randint(K)] = np.nan
    want_beta, want_prop = ref.export_ref(B)
    assert np.isnan(want_prop[rows]).all() and np.isnan(want_prop).any(1).sum() == len(set(rows))
    got_beta, got_prop = _device_export(G, B, route)
    ref.assert_same_bits(got_beta, want_beta, "beta_out", f"NaN rows, {route}, K={K}")
    assert np.isnan(got_prop[rows]).all(), (f"a row that holds a NaN must come out all NaN [{route}, K={K}]", got_prop[rows[0]])
    ref.assert_same_bits(got_prop, want_prop, "prop_out", f"NaN rows, {route}, K={K}")


@pytest.mark.parametrize("K", [33, 100])
def test_export_rounding(K):
    """Real rows: the kernel's sequential row sum and any other order of the K positive terms differ by at most (K - 1) u relatively,
    the division adds one rounding: |prop - want| <= (K + 1) u |want| against the longdouble reference."""
    G = _knn(N_BASE)
    B = np.random.RandomState(K).rand(N_BASE, K) + 1e-3
    want = ref.export_ref_longdouble(B)
    got_beta, got_prop = _device_export(G, B, "export")
    ref.assert_same_bits(got_beta, B, "beta_out", f"real rows, K={K}")
    err = np.abs(got_prop.astype(np.longdouble) - want)
    bound = (K + 1) * np.longdouble(ref.U) * np.abs(want)
    print(f"K={K}: worst |prop - want| / ((K + 1) u |want|) = {float((err / bound).max()):.3f}")
    assert (err <= bound).all(), (K, float((err / bound).max()))
