"""-m gpu tests of ONE block-coordinate-descent sweep, element by element, on every kernel route and cell-type count.

Seams:  fdx_bcd_sweep_dev is one launch of launch_bcd_sweep; fdx_bcd_sweep_ex_dev adds the INIT form (first sweep from a constant
start) and the tile-list form of the tiled kernel; fdx_bcd_fold_dev evaluates rel_change of a sweep's statistics;
fdx_graph_tile_info says which traversal a graph takes, and every test asserts the route it means to take (_route restates
launch_bcd_sweep / launch_k of csrc/bcd_kernels.cpp and csrc/bcd_sweep_inst.cpp on those numbers).

Routes:
    tiled     bcd_sweep_tiled_kernel<K, KC, false>      K = 1..64, 72, 80, 88, 96 on a graph built from coordinates
    gather    bcd_sweep_kernel<K, KC>                   the same K on a graph from CSR (no tile tables)
    lds       bcd_sweep_lds_kernel                      every other K up to 272
    generic   bcd_sweep_generic_kernel                  beyond

Two tiers, as in tests/test_gpu_fit_tail.py (reference: tests/sweep_ref.py, truth of every graph: the oracle's adjacency):
  exact     integer problems whose XtX has nothing below the diagonal: res and den are integers, the new value one correctly rounded
            division - the device must return sweep_exact's float64, value for value, and rel_change[0] its float64.  Every test
            asserts from the reference alone that each branch of the update occurs in at least 5 % of the elements.
  rounding  real problems with a dense XtX (the replaced b_j enter the later row products): |got - want| <= E per element, want and
            E from sweep_longdouble; asserted from the reference alone: max E <= 1e-11 max |want|.  Each case prints its largest err / E.

Device buffers: beta_in holds NaN past column n (column n: the zero row), H holds NaN past n, beta_out and 64 doubles behind it start
as a sentinel - the real columns must all be written, everything else must keep the sentinel -, the statistics start as zeros.
"""
import ctypes

import numpy as np
import pytest

import fit_tail_ref as ref
import sweep_ref as sw
from gpu_graphs import _assert_tiled, _assert_untiled, _dev, _grid, _hub, _knn, _knn_untiled, _radius_isolated

pytestmark = pytest.mark.gpu

N_BASE = 600
N_LIST = (1, 63, 64, 65, 255, 256, 257, 600)
K_FULL = list(range(1, 65)) + [72, 80, 88, 96]
K_LDS = [97, 100, 112, 113, 128, 129, 200, 272]
K_EDGE = [8, 31, 50, 72]                  # chunks of 8, 7, 2 and a padded size (chunks of 6)
SENTINEL = sw.SENTINEL
PAIRS = [(1, 0), (2, 3)]                  # (lambda, rho) of the integer problems


# ------------------------------------------------------------------------------------------------ routes
def _route(G, K):
    n_tiles, halo_max, tiled = G.tile
    instantiated = 1 <= K <= 64 or K in (72, 80, 88, 96)
    if instantiated:
        fits = min(K, 8) * (256 + halo_max + 1) * 8 <= 64 * 1024
        return "tiled" if tiled and fits else "gather"
    KP = ref.round_up(K, 16)
    return "lds" if 4 * (KP * 17 + KP) * 8 <= 160 * 1024 else "generic"


def _assert_route(G, K, want):
    assert _route(G, K) == want, (f"this case was meant to take the {want} sweep", K, G.tile)
    if want == "tiled":
        _assert_tiled(G)


# ------------------------------------------------------------------------------------------------ device calls
def _planes_in(beta, G, ld=None, all_nan=False):
    P = ref.to_planes(beta, G.perm, ld)
    P[:, G.n + 1:] = np.nan
    if all_nan:
        P[:] = np.nan
    return P


def _sweep(G, P, Hp, XtX, lam, rho, it=0, tol=0.0, stats=None, rel=None, init=0.0, tiles=None, ex=False, fold=True):
    """One sweep through the C ABI.  Returns (beta_out (n, K) in the caller's order, the rest of the output buffer, rel_change array,
    stats tensor)."""
    import torch
    from flashdeconv_amd import _lib
    lib = _lib.load()
    K, ld = P.shape
    n = G.n
    dP, dH, dG = _dev(P), _dev(Hp), _dev(np.asarray(XtX, dtype=np.float64))
    out = torch.full((K * ld + 64,), SENTINEL, dtype=torch.float64, device="cuda:0")
    stats = torch.zeros((2, 128), dtype=torch.int64, device="cuda:0") if stats is None else stats
    rel = torch.full((2,), SENTINEL, dtype=torch.float64, device="cuda:0") if rel is None else rel
    args = [G.g.handle, ctypes.c_void_p(dH.data_ptr()), Hp.shape[1], ctypes.c_void_p(dG.data_ptr()), ctypes.c_void_p(dP.data_ptr()),
            ctypes.c_void_p(out.data_ptr()), ld, K, float(lam), float(rho), float(tol), int(it), ctypes.c_void_p(stats.data_ptr()),
            ctypes.c_void_p(rel.data_ptr())]
    if ex or init != 0.0 or tiles is not None:
        dT = None if tiles is None else _dev(np.asarray(tiles, dtype=np.int32))
        _lib.check(lib.fdx_bcd_sweep_ex_dev(*args, float(init), None if dT is None else ctypes.c_void_p(dT.data_ptr()),
                                            0 if tiles is None else len(tiles), None))
    else:
        _lib.check(lib.fdx_bcd_sweep_dev(*args, None))
    if fold:
        _lib.check(lib.fdx_bcd_fold_dev(ctypes.c_void_p(stats.data_ptr()), ctypes.c_void_p(rel.data_ptr()), int(it), None))
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    planes = o[:K * ld].reshape(K, ld)
    return sw.from_planes(planes, G.perm, n), (planes[:, n:], o[K * ld:]), rel.cpu().numpy(), stats


def _assert_rest_untouched(rest, label):
    pad, guard = rest
    assert (pad == SENTINEL).all(), f"written past column n of beta_out [{label}]"
    assert (guard == SENTINEL).all(), f"written behind beta_out [{label}]"


_problems, _exact = {}, {}


def _int_problem(n, K, coupling, zero_diag=None):
    key = (n, K, coupling, zero_diag)
    if key not in _problems:
        beta, H, XtX = sw.integer_sweep_problem(n, K, 1000 * K + n, coupling)
        if zero_diag is not None:
            XtX[zero_diag, zero_diag] = 0.0
        _problems[key] = (beta, H, XtX)
    return _problems[key]


def _exact_ref(G, gkey, K, coupling, lam, rho, zero_diag=None, check_shares=True):
    """sweep_exact of the problem on the graph's truth, cached per (graph, K, problem) and never modified."""
    key = (gkey, G.n, K, coupling, lam, rho, zero_diag)
    if key not in _exact:
        beta, H, XtX = _int_problem(G.n, K, coupling, zero_diag)
        info = {}
        want, rc = sw.sweep_exact(G.A, beta, H, XtX, lam, rho, info)
        want.setflags(write=False)
        _exact[key] = (want, rc, info)
    want, rc, info = _exact[key]
    if check_shares:
        sw.assert_branch_shares(info, rho, f"{gkey}, n={G.n}, K={K}, {coupling}, lambda={lam}, rho={rho}")
    return want, rc


def _check_exact(G, gkey, K, coupling, lam, rho, label, ld=None, ldh=None, zero_diag=None, check_shares=True):
    beta, H, XtX = _int_problem(G.n, K, coupling, zero_diag)
    want, want_rc = _exact_ref(G, gkey, K, coupling, lam, rho, zero_diag, check_shares)
    got, rest, rel, _ = _sweep(G, _planes_in(beta, G, ld), ref.h_to_planes(H, G.perm, ldh), XtX, lam, rho)
    where = f"{label}, n={G.n}, K={K}, {coupling}, lambda={lam}, rho={rho}"
    sw.assert_sweep_exact(got, want, where)
    _assert_rest_untouched(rest, where)
    assert rel[0] == want_rc, (where, rel[0], want_rc)
    return got


# ------------------------------------------------------------------------------------------------ exact, every route
@pytest.mark.parametrize("lam,rho", PAIRS)
@pytest.mark.parametrize("coupling", ["none", "upper"])
@pytest.mark.parametrize("K", K_FULL)
def test_tiled_register_sweep(K, coupling, lam, rho):
    G = _knn(N_BASE)
    _assert_route(G, K, "tiled")
    _check_exact(G, "knn", K, coupling, lam, rho, "tiled register kernel")


@pytest.mark.parametrize("lam,rho", PAIRS)
@pytest.mark.parametrize("K", K_FULL)
def test_global_gather_register_sweep(K, lam, rho):
    G = _knn_untiled(N_BASE)
    _assert_untiled(G)
    _assert_route(G, K, "gather")
    _check_exact(G, "knn", K, "upper", lam, rho, "global-gather register kernel")


@pytest.mark.parametrize("K", [1, 8, 31, 64])
def test_global_gather_sweep_hub_and_spoke(K):
    G = _hub(N_BASE)
    _assert_untiled(G)
    _assert_route(G, K, "gather")
    assert G.max_deg == N_BASE - 1
    _check_exact(G, "hub", K, "upper", 2, 3, "global-gather kernel, hub and spoke")


@pytest.mark.parametrize("tiled", [True, False])
@pytest.mark.parametrize("K", K_LDS)
def test_lds_resident_sweep(K, tiled):
    G = _knn(N_BASE) if tiled else _knn_untiled(N_BASE)
    (_assert_tiled if tiled else _assert_untiled)(G)              # a tiled graph's tiles are not used at these K
    _assert_route(G, K, "lds")
    _check_exact(G, "knn", K, "upper", 2, 3, "LDS-resident sweep")


def test_generic_sweep():
    G = _knn_untiled(N_BASE)
    _assert_untiled(G)
    _assert_route(G, 300, "generic")
    _check_exact(G, "knn", 300, "upper", 2, 3, "generic sweep")


@pytest.mark.parametrize("K", list(range(1, 65)))
def test_init_form_of_the_tiled_sweep(K):
    """The first sweep of a solve: every old abundance is the constant init_uniform, beta_in (all NaN here) is not read."""
    G = _knn(N_BASE)
    _assert_route(G, K, "tiled")
    _, H, XtX = _int_problem(G.n, K, "upper")
    start = np.full((G.n, K), 2.0)
    key = ("init", K)
    if key not in _exact:
        info = {}
        want, rc = sw.sweep_exact(G.A, start, H, XtX, 2, 3, info)
        _exact[key] = (want, rc, info)
    want, want_rc, info = _exact[key]
    sw.assert_branch_shares(info, 3, f"INIT, K={K}")
    got, rest, rel, _ = _sweep(G, _planes_in(start, G, all_nan=True), ref.h_to_planes(H, G.perm), XtX, 2, 3, init=2.0)
    sw.assert_sweep_exact(got, want, f"INIT form, K={K}")
    _assert_rest_untouched(rest, f"INIT form, K={K}")
    assert rel[0] == want_rc, (K, rel[0], want_rc)


# ------------------------------------------------------------------------------------------------ edges
@pytest.mark.parametrize("n", N_LIST)
@pytest.mark.parametrize("K", K_EDGE + [100])
def test_sweep_spot_counts(n, K):
    G = _knn(n)
    if K == 100:
        _assert_route(G, K, "lds")
    elif n == 1:
        _assert_untiled(G)                                        # no k-NN graph of one spot: the global-gather kernel takes it
        _assert_route(G, K, "gather")
    else:
        _assert_route(G, K, "tiled")
    # (one spot: K elements cannot promise 5 % on each of five branches)
    _check_exact(G, "knn", K, "upper", 2, 3, "spot counts", check_shares=n > 1)


@pytest.mark.parametrize("K", K_EDGE + [100])
def test_sweep_rows_longer_than_16_slots(K):
    G = _knn(N_BASE, k=20, seed=12)
    _assert_route(G, K, "lds" if K == 100 else "tiled")
    assert G.max_deg > 16
    _check_exact(G, "knn20", K, "upper", 2, 3, "k = 20: slots past 16 read from memory")


@pytest.mark.parametrize("K", K_EDGE + [100])
def test_sweep_halo_above_256(K):
    G = _knn(2000, k=48, seed=12)
    _assert_tiled(G, min_halo=256)                                # the second round of the halo staging loop (h = tid + 256)
    _assert_route(G, K, "lds" if K == 100 else "tiled")
    # lambda = 1: with some 55 neighbours per spot, lambda = 2 pushes res so far up that |res| <= rho falls below 5 % of the elements
    _check_exact(G, "knn48", K, "upper", 1, 3, "halo above 256")


@pytest.mark.parametrize("K", K_EDGE + [100])
def test_sweep_radius_graph_with_isolated_spots(K):
    """Degree 0 and slices of width 0; type 3 has XtX[3][3] = 0, so den = 0 on the isolated spots: the new value is 0, not the NaN
    or inf of the division."""
    G = _radius_isolated()
    _assert_route(G, K, "lds" if K == 100 else "tiled")
    deg = np.diff(G.A.indptr)
    assert (deg == 0).sum() >= 200
    widths = [deg[G.perm][s:s + 64].max() for s in range(0, G.n, 64)]
    assert min(widths) == 0 and max(widths) > 0, widths
    got = _check_exact(G, "radius", K, "upper", 2, 3, "radius graph, isolated spots", zero_diag=3)
    assert (got[deg == 0, 3] == 0).all() and np.isfinite(got).all()


@pytest.mark.parametrize("K", K_EDGE + [100])
def test_sweep_grid_graph(K):
    G = _grid()
    _assert_route(G, K, "lds" if K == 100 else "tiled")
    assert G.max_deg == 8
    _check_exact(G, "grid", K, "upper", 2, 3, "grid graph")


@pytest.mark.parametrize("K", K_EDGE + [100])
def test_sweep_leading_dimensions_above_the_minimum(K):
    G = _knn(N_BASE)
    _assert_route(G, K, "lds" if K == 100 else "tiled")
    ld, ldh = ref.round_up(N_BASE + 1, 64) + 64, N_BASE + 13
    assert ld != ldh and ld > ref.round_up(N_BASE + 1, 64) and ldh > N_BASE
    _check_exact(G, "knn", K, "upper", 2, 3, "ld and ldh above the minimum", ld=ld, ldh=ldh)


@pytest.mark.parametrize("K", K_EDGE)
def test_sweep_over_a_tile_list(K):
    """Tiles 4, 1, 2 of six: their spots equal the reference, every other spot keeps the sentinel, and the statistics are theirs."""
    n, tiles = 1500, [4, 1, 2]
    G = _knn(n)
    _assert_route(G, K, "tiled")
    assert G.tile[0] == 6
    beta, H, XtX = _int_problem(n, K, "upper")
    want, _ = _exact_ref(G, "knn", K, "upper", 2, 3)
    pos = np.concatenate([np.arange(256 * t, min(n, 256 * (t + 1))) for t in tiles])
    listed = np.zeros(n, dtype=bool)
    listed[G.perm[pos]] = True
    got, rest, rel, _ = _sweep(G, _planes_in(beta, G), ref.h_to_planes(H, G.perm), XtX, 2, 3, tiles=tiles)
    sw.assert_sweep_exact(got[listed], want[listed], f"tile list, K={K}")
    assert (got[~listed] == SENTINEL).all(), f"a tile outside the list was swept [K={K}]"
    _assert_rest_untouched(rest, f"tile list, K={K}")
    want_rc = sw.rel_change(beta, want, np.flatnonzero(listed))
    assert rel[0] == want_rc, (K, rel[0], want_rc)


def test_seam_refuses_what_the_launch_would_not_do():
    from flashdeconv_amd import _lib

    def refused(G, K, **extras):
        beta, H, XtX = _int_problem(G.n, K, "upper")
        with pytest.raises(_lib.FdxError, match=r"libfdx error -1:"):
            _sweep(G, _planes_in(beta, G), ref.h_to_planes(H, G.perm), XtX, 2, 3, ex=True, **extras)

    untiled, tiled = _knn_untiled(N_BASE), _knn(N_BASE)
    _assert_untiled(untiled)
    _assert_tiled(tiled)
    refused(untiled, 31, init=2.0)                                # no tiled sweep on this graph: the launch would read beta_in
    refused(untiled, 31, tiles=[0, 1])                            # ... or sweep every spot
    refused(tiled, 100, tiles=[0, 1])                             # the LDS-resident sweep knows no tile list
    refused(tiled, 72, init=2.0)                                  # no INIT instance above 64 types: nothing would run
    refused(tiled, 65)                                            # no sweep of 65 types at all (fdx_solver_padded_k: 72)
    refused(tiled, 31, init=2.0, tiles=[0])                       # the list would win and the start vector be read
    # and with no extras the seam is fdx_bcd_sweep_dev
    beta, H, XtX = _int_problem(N_BASE, 31, "upper")
    want, rc = _exact_ref(tiled, "knn", 31, "upper", 2, 3)
    got, rest, rel, _ = _sweep(tiled, _planes_in(beta, tiled), ref.h_to_planes(H, tiled.perm), XtX, 2, 3, ex=True)
    sw.assert_sweep_exact(got, want, "seam without extras")
    assert rel[0] == rc


# ------------------------------------------------------------------------------------------------ the stopping gate
@pytest.mark.parametrize("K", [8, 72, 100, 300])
def test_stopping_gate_at_the_top_of_the_sweep(K):
    """Sweep it = 1 folds sweep 0's statistics first: with tol above rel_change[0] it writes that number and nothing else, with tol
    below it runs - on sweep 0's (non-integer) output, so against the rounding bound."""
    import torch
    G = _knn(N_BASE) if K <= 96 else _knn_untiled(N_BASE)
    _assert_route(G, K, {8: "tiled", 72: "tiled", 100: "lds", 300: "generic"}[K])
    beta, H, XtX = _int_problem(G.n, K, "upper")
    want0, rc0 = _exact_ref(G, "knn", K, "upper", 2, 3)
    Hp = ref.h_to_planes(H, G.perm)
    stats = torch.zeros((2, 128), dtype=torch.int64, device="cuda:0")
    rel = torch.full((2,), SENTINEL, dtype=torch.float64, device="cuda:0")
    got0, _, _, _ = _sweep(G, _planes_in(beta, G), Hp, XtX, 2, 3, it=0, stats=stats, rel=rel, fold=False)
    sw.assert_sweep_exact(got0, want0, f"sweep 0, K={K}")
    assert rc0 > 0
    P1 = _planes_in(got0, G)
    # tol above: stops
    got1, rest, r, _ = _sweep(G, P1, Hp, XtX, 2, 3, it=1, tol=2.0 * rc0, stats=stats, rel=rel, fold=False)
    assert (got1 == SENTINEL).all(), f"a sweep behind the stopping rule wrote its output [K={K}]"
    _assert_rest_untouched(rest, f"stopped sweep, K={K}")
    assert r[0] == rc0 and r[1] == SENTINEL, (K, r, rc0)
    assert not stats[1].any().item(), "a stopped sweep left statistics"
    # tol below: runs
    rel.fill_(SENTINEL)
    got1, rest, r, _ = _sweep(G, P1, Hp, XtX, 2, 3, it=1, tol=0.5 * rc0, stats=stats, rel=rel, fold=True)
    want1, E1 = sw.sweep_longdouble(G.A, got0, H, XtX, 2, 3)
    worst = sw.assert_sweep_close(got1, want1, E1, f"sweep 1, K={K}")
    print(f"gate K={K}: second sweep, largest err / E = {worst:.3f}")
    _assert_rest_untouched(rest, f"sweep 1, K={K}")
    assert r[0] == rc0, (K, r, rc0)
    want_rc1 = sw.rel_change(got0, np.asarray(want1, dtype=np.float64))
    # max |new - old| is off by at most the largest E and one rounding, max |old| is exact, the sum and the division round once each
    assert abs(r[1] - want_rc1) <= float(E1.max()) / (np.abs(got0).max() + 1e-10) + 4 * ref.U * want_rc1, (K, r[1], want_rc1)


# ------------------------------------------------------------------------------------------------ rounding
_real = {}


def _check_rounding(G, gkey, K, route, init=0.0):
    _assert_route(G, K, route)
    key = (gkey, K, init)
    if key not in _real:
        beta, H, XtX = sw.real_sweep_problem(G.n, K, 77 + K)
        if init != 0.0:
            beta = np.full_like(beta, init)
        info = {}
        want, E = sw.sweep_longdouble(G.A, beta, H, XtX, sw.REAL_LAMBDA, sw.REAL_RHO, info)
        _real[key] = (beta, H, XtX, want, E, info)
    beta, H, XtX, want, E, info = _real[key]
    assert E.max() <= 1e-11 * np.abs(want).max(), (K, float(E.max()), float(np.abs(want).max()))
    got, rest, _, _ = _sweep(G, _planes_in(beta, G, all_nan=init != 0.0), ref.h_to_planes(H, G.perm), XtX, sw.REAL_LAMBDA, sw.REAL_RHO,
                             init=init)
    worst = sw.assert_sweep_close(got, want, E, f"{route}, K={K}")
    print(f"{route}{' INIT' if init else ''} K={K}: largest err / E = {worst:.4f} (largest E {float(E.max()):.2e}, largest |want| "
          f"{float(np.abs(want).max()):.3f})")
    _assert_rest_untouched(rest, f"{route}, K={K}")


@pytest.mark.parametrize("K", K_FULL)
def test_tiled_sweep_rounding(K):
    _check_rounding(_knn(N_BASE), "knn", K, "tiled")


@pytest.mark.parametrize("route,K", [("gather", 31), ("gather", 64), ("lds", 100), ("lds", 200), ("generic", 300)])
def test_other_sweeps_rounding(route, K):
    G = _knn_untiled(N_BASE)
    _assert_untiled(G)
    _check_rounding(G, "knn", K, route)


def test_init_form_rounding():
    _check_rounding(_knn(N_BASE), "knn", 31, "tiled", init=0.375)
