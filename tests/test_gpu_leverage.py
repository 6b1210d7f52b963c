"""Leverage scores PER GENE on every kernel route of csrc/leverage_kernels.cpp and at every size edge, through
fdx_leverage_scores_route (route 0 = the product path with its fallback, 1 = Cholesky-QR alone, 2 = the streaming Jacobi passes,
3 = the one-workgroup Jacobi kernel), against the long-double reference of tests/leverage_ref.py:

    |dev_g - exact_g| <= M * L * unit_g,      unit_g = u kappa sqrt(l_g l_max) + (u kappa)^2 l_max,   u = 2^-53

and never above the tolerance the older tests of tests/test_gpu_fit.py accept, 2e-8 max(1, kappa / 1e4) relative + 1e-15.
unit is the change of a row's squared norm in Q under a backward error of one unit roundoff; kappa is the condition of the
ridge-augmented matrix without the direction that centring annihilates (leverage_ref.kappa).  L = 48 is LAPACK's own largest
error in units over the cases of this file (float64 gesdd through the oracle: 31.0 measured, pinned by
tests/test_leverage_host.py; it is set by X * 1e-6, where every s^2 is below reg, and by the K = 2 shapes, where centring a
value of ~30 to ~8 costs two bits that unit does not know of - the device centres in float64 too).  M = 8 on every route: a
margin over the REFERENCE's error, three bits for a chain of roundings about three times LAPACK's (Householder deflation and two
factorisations, or two to four Gram / rotate passes) and sums over the genes in stripe order.  M is not derived from the device.

Sizes: stripes of 64 genes and blocks of 256 threads (G = 1, 2, 63 .. 65, 127 .. 129, 255 .. 257, 1000); K - 1 at 63 / 64 (LDS
factor of 64 or 128 rows), 128 / 129 (factor in global memory, blocked by 32: 128 = four whole blocks, 129 leaves one row, 271
leaves 15), 272 / 273 (no QR at all); the one-workgroup kernel's four forms by G (<= 512, <= 1024, <= 2048, streaming), its dummy
player at odd K and more pairs than waves above K = 16.

regularization = 0 is left out: the reference then gives the direction that centring annihilates (s ~ 1e-15) the weight
s^2 / s^2 = 1, so its own answer is rounding noise; the device drops that direction by construction.  For the same reason
X * 1e4 is measured against `exact` only and is no part of L (test_leverage_host.py::test_lapack_ratio_over_the_gpu_cases).

Fewer genes than K - 1: the Cholesky-QR route does not refuse every such matrix.  It refuses when
the K - 1 - G pivots of ~reg fall below 1e-9 x the largest diagonal entry of the Gram matrix, i.e. when a deflated row has a
squared norm above ~1e3; at G = 1 or 2 and a centred r.m.s. of 8 it stands (and is accurate: those shapes are in the plain
grid, where either answer is accepted and a standing route is held to the bound).  The cases that MUST refuse have a centred
r.m.s. of 28 (leverage_ref.QR_WIDE), where the float64 model refuses with a factor of two to spare.

Largest observed |dev - exact| / unit per route on an MI355X over the whole file, LAPACK's on the same cases (records, NOT limits;
the autouse fixture prints them):
    route                       cases   device      LAPACK      M
    0  product path               194   11.000      31.011      8      (64 x 2, r.m.s. 28: fell back to the streaming passes)
    1  Cholesky-QR                 97    4.635      31.011      8      (2 x 257)
    2  streaming Jacobi            56    9.759      31.011      8      (12 x 300, X * 1e-6)
    3  one-workgroup Jacobi        48    6.369      31.011      8      (12 x 300, X * 1e-6)
The file takes 6 s on that machine (403 tests).  Before the two fixes these cases forced in csrc/leverage_kernels.cpp
(LEV_NULL_TOL) the Jacobi routes were at 614 and 564 units on X * 1e4 - the weight of the direction that centring annihilates -
and reported "not converged" after all 4 passes / all 60 sweeps on every rank-deficient matrix.
"""
import functools
import time

import numpy as np
import pytest

import fdx_oracle as orc
import leverage_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e300
M = {0: R.M_DEVICE, 1: R.M_DEVICE, 2: R.M_DEVICE, 3: R.M_DEVICE}
NAMES = {0: "product path", 1: "Cholesky-QR", 2: "streaming Jacobi", 3: "one-workgroup Jacobi"}
_worst = {}
_t0 = [None]


@pytest.fixture(scope="module", autouse=True)
def _report_the_largest_ratios():
    _t0[0] = time.perf_counter()
    yield
    print(f"\n[test_gpu_leverage] largest |dev - exact| / unit per route (L = {R.L_LAPACK:g}; limit M * L):")
    for route in sorted(_worst):
        n, dev, where, lap = _worst[route]
        print(f"[test_gpu_leverage]   {route}  {NAMES[route]:<22s} {n:5d} cases   device {dev:9.3f} ({where})   LAPACK {lap:9.3f}   "
              f"M = {M[route]:g}")
    print(f"[test_gpu_leverage] {time.perf_counter() - _t0[0]:.1f} s")


@functools.lru_cache(maxsize=None)
def _lapack_ratio(case):
    e = R.evaluate(case)
    return _ratio(orc.leverage_scores(R.matrix(case), case.reg), e)


def _ratio(got, e):
    err = np.abs(got - e["exact"])
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(err == 0.0, 0.0, err / e["unit"])))


def run(case, route):
    """(scores, info) of one call; the 8 slots behind the scores keep their sentinel"""
    from flashdeconv_amd import _lib
    X = R.matrix(case)
    K, G = X.shape
    out = np.full(G + 8, SENTINEL)
    info = np.full(8, -1, dtype=np.int32)
    _lib.require_gpu()
    rc = _lib.load().fdx_leverage_scores_route(_lib.ptr_f64(X), K, G, float(case.reg), route, _lib.ptr_f64(out), _lib.ptr_i32(info))
    if rc == -2:                                            # FDX_ERR_HIP: nothing more is started on a device that has faulted
        pytest.exit(f"HIP error on {case.id} route {route}: {_lib.load().fdx_last_error()!r}", returncode=3)
    _lib.check(rc)
    assert np.all(out[G:] == SENTINEL), "wrote behind lev_out"
    assert np.all(info[5:] == 0) and info[0] in (1, 2, 3) and set(info[[1, 3, 4]].tolist()) <= {0, 1}, info
    return out[:G], info


def check(case, route, got):
    """the bound, per gene; the figures go to the record first"""
    e = R.evaluate(case)
    assert np.all(np.isfinite(got)), (case.id, route)
    r = _ratio(got, e)
    n, dev, where, lap = _worst.get(route, (0, 0.0, "", 0.0))
    lp = 0.0 if (case.kind == "scaled" and case.param > 1.0) else _lapack_ratio(case)
    _worst[route] = (n + 1, max(dev, r), case.id if r > dev else where, max(lap, lp))
    lim = R.bound(e["exact"], e["kappa"], M[route])
    bad = np.flatnonzero(np.abs(got - e["exact"]) > lim)
    assert bad.size == 0, (f"{case.id} route {route}: {bad.size} genes outside M L unit, worst {r:.1f} units (limit {M[route] * R.L_LAPACK:g}; "
                           f"kappa {e['kappa']:.3g}); gene {bad[0]}: {got[bad[0]]!r} vs {e['exact'][bad[0]]!r}")


def run_route(case, route, refuse=None):
    """One case on one route.  refuse (route 1): True = must refuse, False = must stand, None = may refuse above kappa 3e3."""
    got, info = run(case, route)
    K = case.K
    if route == 1:
        assert info[0] == 1 and info[4] == 0 and info[2] == 0
        refused = bool(info[1])
        assert refused == (info[3] == 0)
        if refuse is None:
            assert not refused or R.evaluate(case)["kappa"] > 3e3 or case.G < K - 1, (case.id, "refused")
        else:
            assert refused == refuse, (case.id, info)
        if refused:
            return info
    elif route == 2:
        assert info[0] == 2 and info[1] == 0 and info[4] == 0
        assert info[3] == 1 and info[2] <= 4, (case.id, "passes", info)
    elif route == 3:
        assert info[0] == 3 and info[1] == 0 and info[4] == 0
        assert info[3] == 1, (case.id, "sweeps", info)
    else:
        assert info[4] == info[1] and info[3] == 1, (case.id, info)
        assert info[0] == (1 if 2 <= K <= 272 and not info[4] else 2 if 2 <= K <= 64 else 3), (case.id, info)
        if refuse is not None:
            assert bool(info[4]) == refuse, (case.id, info)
    check(case, route, got)
    return info


def _ids(params):
    return [f"{c.id}-route{r}" for c, r, *_ in params]


# ---------------------------------------------------------------------------------------------- the routes at their size edges
_QR_PLAIN = [(c, 1, False if c.G >= c.K - 1 else None) for c in R._dedup(R.QR64 + R.QR128 + R.QRBIG)]


@pytest.mark.parametrize("case,route,refuse", _QR_PLAIN, ids=_ids(_QR_PLAIN))
def test_cholesky_qr_at_every_factor_size(case, route, refuse):
    run_route(case, route, refuse)


@pytest.mark.parametrize("case", R.QR_WIDE, ids=[c.id for c in R.QR_WIDE])
def test_cholesky_qr_refuses_fewer_genes_than_directions_and_the_fallback_is_accurate(case):
    run_route(case, 1, True)
    run_route(case, 0, True)


_STREAM = [(c, 2) for c in R._dedup(R.STREAM)]


@pytest.mark.parametrize("case,route", _STREAM, ids=_ids(_STREAM))
def test_streaming_jacobi_passes(case, route):
    run_route(case, route)


_ONE_WG = [(c, 3) for c in R._dedup(R.ONE_WG)]


@pytest.mark.parametrize("case,route", _ONE_WG, ids=_ids(_ONE_WG))
def test_one_workgroup_jacobi_in_its_four_forms(case, route):
    info = run_route(case, route)
    if case.K == 1:
        assert np.all(run(case, route)[0] == 0.0)
    if case.K == 273:                                       # no QR at that size: the product path is this kernel
        info = run_route(case, 0, False)
        assert info[0] == 3


# ---------------------------------------------------------------------------------------------- conditioning, rank, special genes
_COND = [(c, r) for c in R.COND for r in [0] + R.routes_for(c.K)]


@pytest.mark.parametrize("case,route", _COND, ids=_ids(_COND))
def test_conditioning_on_every_route(case, route):
    """kappa 1e1 .. 2e4.  Between kappa 3e3 and a spread of 1e6 nothing is asserted about the route Cholesky-QR takes: where it
    stands it is held to the bound, and route 0 is held to it either way."""
    run_route(case, route)


@pytest.mark.parametrize("case", R.COND_STANDS, ids=[c.id for c in R.COND_STANDS])
def test_kappa_3e3_is_not_refused(case):
    run_route(case, 1, False)
    run_route(case, 0, False)


@pytest.mark.parametrize("case", R.COND_REFUSED, ids=[c.id for c in R.COND_REFUSED])
def test_a_spread_of_1e6_is_refused_and_the_fallback_is_accurate(case):
    run_route(case, 1, True)
    run_route(case, 0, True)
    for r in R.routes_for(case.K)[1:]:
        run_route(case, r)


@pytest.mark.parametrize("case", R.RANK, ids=[c.id for c in R.RANK])
def test_rank_deficient_signatures_through_the_product_path(case):
    info = run_route(case, 0, True if case.kind == "twins" else False)
    if case.kind == "all_equal":
        assert np.all(R.evaluate(case)["exact"] == 0.0) and info[4] == 0
        for r in range(4):
            assert np.all(run(case, r)[0] == 0.0), r


_WIDE_ROUTES = [(c, r) for c in R.SPECIAL + R.REG + R.SCALE for r in [0] + R.routes_for(c.K)]


@pytest.mark.parametrize("case,route", _WIDE_ROUTES, ids=_ids(_WIDE_ROUTES))
def test_special_genes_regularization_and_scale_on_every_route(case, route):
    run_route(case, route)
    if case.kind == "const_gene":
        e = R.evaluate(case)
        g = case.G // 3
        assert e["exact"][g] == 0.0
        got, info = run(case, route)
        assert 0.0 <= got[g] <= M[route] * R.L_LAPACK * (R.U53 * e["kappa"]) ** 2 * e["exact"].max()


# ---------------------------------------------------------------------------------------------- cross-cutting
def test_a_route_that_does_not_apply_is_invalid():
    from flashdeconv_amd import _lib
    lib = _lib.load()
    _lib.require_gpu()
    for K, route in ((273, 1), (1, 1), (65, 2), (1, 2), (5, 4), (5, -1)):
        X = np.ones((K, 10))
        out, info = np.zeros(10), np.zeros(8, dtype=np.int32)
        rc = lib.fdx_leverage_scores_route(_lib.ptr_f64(X), K, 10, 1e-6, route, _lib.ptr_f64(out), _lib.ptr_i32(info))
        assert rc == -1, (K, route, rc)                     # FDX_ERR_INVALID


_REPEAT = [(R.Case(272, 330), 1), (R.Case(96, 192), 1), (R.Case(17, 129), 1), (R.Case(33, 257), 2), (R.Case(9, 513), 3),
           (R.Case(9, 2600), 3), (R.Case(65, 130), 3), (R.Case(12, 200, "twins", 0.0), 0), (R.Case(129, 200, "twins", 0.0), 0)]


@pytest.mark.parametrize("case,route", _REPEAT, ids=_ids(_REPEAT))
def test_two_runs_give_the_same_bits(case, route):
    a, ia = run(case, route)
    b, ib = run(case, route)
    assert np.array_equal(a, b) and np.array_equal(ia, ib)


@pytest.mark.parametrize("case", R.ALL_CASES, ids=[c.id for c in R.ALL_CASES])
def test_route_0_is_compute_leverage_scores_bit_for_bit(case):
    from flashdeconv_amd.utils.genes import compute_leverage_scores
    got, _ = run(case, 0)
    assert np.array_equal(got, compute_leverage_scores(R.matrix(case), case.reg))
    check(case, 0, got)


_JOBS = [R.Case(12, 300), R.Case(70, 200), R.Case(130, 320), R.Case(12, 200, "twins", 0.0), R.Case(3, 1)]


@pytest.mark.parametrize("no_cache", [False, True])
@pytest.mark.parametrize("case", _JOBS, ids=[c.id for c in _JOBS])
def test_route_0_is_the_leverage_job_bit_for_bit(case, no_cache, monkeypatch):
    from flashdeconv_amd.utils.genes import LeverageJob
    if no_cache:
        monkeypatch.setenv("FDX_NO_PLAN_CACHE", "1")
    got, _ = run(case, 0)
    for queue_async in (True, False):
        assert np.array_equal(got, LeverageJob(R.matrix(case), case.reg, queue_async=queue_async).result()), queue_async


def test_the_one_workgroup_switch_maps_onto_route_3(monkeypatch):
    from flashdeconv_amd.utils.genes import compute_leverage_scores
    case = R.Case(17, 129)
    want, _ = run(case, 3)
    monkeypatch.setenv("FDX_LEV_ONE_WG", "1")
    monkeypatch.setenv("FDX_NO_PLAN_CACHE", "1")
    assert np.array_equal(compute_leverage_scores(R.matrix(case), case.reg), want)
    got, info = run(case, 0)
    assert np.array_equal(got, want) and info[0] == 3 and info[4] == 0


def test_nothing_of_a_large_case_reaches_a_small_one():
    """(272, 330) on route 1 and then (3, 65) on every route in the same process: the pooled scratch, the arrival counters and
    the status word of the big case must not reach the small one."""
    run_route(R.Case(272, 330), 1, False)
    small = R.Case(3, 65)
    first = {}
    for route in range(4):
        run_route(small, route, False if route < 2 else None)
        first[route] = run(small, route)[0]
    run_route(R.COND_REFUSED[2], 1, True)                   # a refusal's status word, then the small case again
    for route in range(4):
        assert np.array_equal(run(small, route)[0], first[route]), route
