"""-m gpu tests of the local spatial statistics (fdx_local_stats_dev, fdx_conditional_indices_dev, utils.local_stats,
FlashDeconv.get_local_spatial_statistics, tl.deconvolve(local_stats=)).

Reference: tests/local_stats_ref.py - the draw restated in plain Python integers and a loop-level NumPy reference of S, S_r, the
counts and the sums, on the graph's truth adjacency (tests/gpu_graphs.py) in the caller's spot order.

Exact cases use dyadic inputs: integers in [0, 16) over 16 with about 60 % zeros.  A sum of at most 600 of them is a multiple of
1/16 below 2^10, d = S_r - S likewise, d^2 a multiple of 1/256 below 2^20 and a sum of 130 of those below 2^27: every one is exact
in float64 in any order, so count_ge, count_le, sum_d, sumsq_d and neighbor_sum must EQUAL the reference - no tolerance, no share
of cases left out.  On generic float64 data neighbor_sum is held to 4 deg_i 2^-53 sum_j |V_ja| (deg_i terms added in any order on
both sides) and local_i / gi_star to rtol 1e-11 (no absolute term) of assemble_local fed the reference sums; counts are not
compared there.
"""
import ctypes
import math

import numpy as np
import pytest
from scipy import sparse

import datagen
import local_stats_ref as ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
PERM_ARRAYS = ("count_ge", "count_le", "sum_d", "sumsq_d")
BASE_KEYS = {"local_i", "gi_star", "quadrant", "neighbor_sum", "degree", "mean", "m2", "n", "n_edges"}
PERM_KEYS = {"n_permutations", "p_greater", "p_less", "p_value", "z_sim", "local_i_p_greater"}


# ---------------------------------------------------------------- helpers
def _dyadic(n, K, seed):
    rs = np.random.RandomState(seed)
    return np.where(rs.rand(n, K) < 0.6, 0.0, rs.randint(0, 16, (n, K)) / 16.0)


def _generic(n, K, seed):
    rs = np.random.RandomState(seed)
    return rs.dirichlet(np.full(K, 0.3), n) if K > 1 else rs.rand(n, 1)


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


_refs = {}


def _reference(name, V, A, seed, first, R):
    """The loop reference, computed once per case and shared (read-only)."""
    key = (name, V.shape, seed, first, R)
    if key not in _refs:
        out = ref.local_reference(V, A, seed, first, R)
        for v in out.values():
            v.setflags(write=False)
        _refs[key] = out
    return _refs[key]


def _check_exact(name, G, K, R, seed=5, first=0, vseed=None):
    from flashdeconv_amd.utils.local_stats import local_sums
    from flashdeconv_amd.utils.spatial_stats import spatial_sums
    V = _dyadic(G.n, K, 1000 + K if vseed is None else vseed)
    got = local_sums(V, G.g, seed=seed, first_perm=first, n_permutations=R)
    want = _reference(name, V, G.A, seed, first, R)
    assert got["neighbor_sum"].dtype == np.float64 and got["degree"].dtype == np.int32 and got["n_permutations"] == R
    assert np.array_equal(got["neighbor_sum"], want["S"]), name
    assert np.array_equal(got["degree"], want["deg"]), name
    if R:
        assert got["count_ge"].dtype == np.int32 and got["count_le"].dtype == np.int32 and got["sum_d"].dtype == np.float64
        assert np.array_equal(got["count_ge"], want["count_ge"]), name
        assert np.array_equal(got["count_le"], want["count_le"]), name
        assert np.array_equal(got["sum_d"], want["sum_d"]), name
        assert np.array_equal(got["sumsq_d"], want["sumsq_d"]), name
        assert np.all(got["count_ge"] + got["count_le"] >= R)
    else:
        assert not set(PERM_ARRAYS) & set(got)
    base = spatial_sums(V, G.g)
    for key in ("mean", "m2"):
        assert np.array_equal(got[key], base[key]), (name, key)
    assert (got["n"], got["W"], got["sum_deg_sq"]) == (base["n"], base["W"], base["sum_deg_sq"])
    assert got["W"] == int(want["deg"].sum()) and got["sum_deg_sq"] == int((want["deg"] ** 2).sum())
    return V, got, want


def _small_graph(n):
    import gpu_graphs as gg
    if n <= 2:
        return gg._csr(sparse.csr_matrix(np.ones((n, n)) - np.eye(n)), ("complete", n))
    return gg._knn(n)


# ---------------------------------------------------------------- 1. the draw on the device
@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 65, 257, 4097, 65537])
def test_device_draw_equals_the_definition(n):
    import torch
    from flashdeconv_amd import _lib
    from flashdeconv_amd.utils.local_stats import conditional_indices
    lib = _lib.load()
    top = min(n - 1, 300)
    for seed, r in ((0, 0), (2 ** 64 - 1, 998)):
        for spot in sorted({0, n // 3, n - 1}):
            for count in sorted({0, min(1, top), min(6, top), top}):
                out = torch.full((count + 1,), -7, dtype=torch.int32, device="cuda:0")
                _lib.check(lib.fdx_conditional_indices_dev(ctypes.c_uint64(seed), r, spot, n, count, ctypes.c_void_p(out.data_ptr()),
                                                           None))
                torch.cuda.synchronize()
                got = out.cpu().numpy()
                assert got[count] == -7                                             # nothing past count
                assert np.array_equal(got[:count].astype(np.int64), conditional_indices(seed, r, spot, n, count)), (seed, r, spot, count)
                assert list(got[:count]) == list(ref.conditional_indices(seed, r, spot, n, count))


def test_device_draw_argument_checks():
    from flashdeconv_amd import _lib
    lib = _lib.load()
    for args, msg in (((0, 0, 5, 2, None), "null argument"), ((-1, 0, 5, 2, None), "r must not be negative"),
                      ((0, 0, 0, 0, None), "n must be"), ((0, 5, 5, 2, None), "spot must be"), ((0, -1, 5, 2, None), "spot must be"),
                      ((0, 0, 5, 5, None), "count must be"), ((0, 0, 5, -1, None), "count must be")):
        with pytest.raises(_lib.FdxError, match=msg):
            _lib.check(lib.fdx_conditional_indices_dev(ctypes.c_uint64(0), *args, None))
    _lib.check(lib.fdx_conditional_indices_dev(ctypes.c_uint64(0), 0, 0, 1, 0, None, None))


# ---------------------------------------------------------------- 2. exact counts and sums
def test_exact_on_a_knn_graph_in_morton_order():
    import gpu_graphs as gg
    G = gg._knn(130)
    assert G.perm is not None and not np.array_equal(G.perm, np.arange(130)), "Morton order is the identity: nothing permuted"
    _check_exact("knn130", G, 9, 65)


def test_exact_on_a_radius_graph_with_isolated_spots():
    import gpu_graphs as gg
    G = gg._radius_isolated()
    _, got, want = _check_exact("radius", G, 3, 33)
    iso = want["deg"] == 0
    assert iso.sum() >= 200
    assert np.all(got["count_ge"][iso] == 33) and np.all(got["count_le"][iso] == 33) and not got["sum_d"][iso].any()


def test_exact_on_a_hub_whose_centre_draws_everybody():
    import gpu_graphs as gg
    G = gg._hub(130)
    _, got, want = _check_exact("hub130", G, 9, 65)
    hub = int(np.argmax(want["deg"]))
    assert want["deg"][hub] == 129 and np.all(np.delete(want["deg"], hub) == 3)      # the hub, and a ring joins the others
    assert np.all(got["count_ge"][hub] == 65) and np.all(got["count_le"][hub] == 65)       # the null of the hub does not vary
    assert not got["sum_d"][hub].any() and not got["sumsq_d"][hub].any()


def test_exact_on_an_identity_order_graph_from_csr():
    import gpu_graphs as gg
    G = gg._knn_untiled(130)
    gg._assert_untiled(G)
    _check_exact("csr130", G, 9, 65)


@pytest.mark.parametrize("n", [1, 2, 37, 64, 65, 257])
def test_exact_slice_tails(n):
    _check_exact(f"n={n}", _small_graph(n), 5, 65 if n <= 65 else 33)


@pytest.mark.parametrize("K", [1, 8, 9, 17, 33])
def test_exact_k_coverage(K):
    import gpu_graphs as gg
    _check_exact("knn130", gg._knn(130), K, 64)


@pytest.mark.parametrize("R", [1, 63, 64, 65, 130])
def test_exact_r_coverage(R):
    import gpu_graphs as gg
    _check_exact("knn130", gg._knn(130), 9, R, first=3)


def test_split_calls_add_up_and_two_calls_return_the_same_bits():
    import gpu_graphs as gg
    from flashdeconv_amd.utils.local_stats import local_sums
    G = gg._knn(130)
    V = _dyadic(130, 9, 77)
    whole = local_sums(V, G.g, seed=5, n_permutations=65)
    a = local_sums(V, G.g, seed=5, first_perm=0, n_permutations=30)
    b = local_sums(V, G.g, seed=5, first_perm=30, n_permutations=35)
    for key in PERM_ARRAYS:
        assert np.array_equal(a[key] + b[key], whole[key]), key
    for K in (5, 33):
        Vg = _generic(130, K, 300 + K)
        one, two = local_sums(Vg, G.g, seed=9, n_permutations=65), local_sums(Vg, G.g, seed=9, n_permutations=65)
        for key in ("neighbor_sum", "degree", "mean", "m2") + PERM_ARRAYS:
            assert np.array_equal(one[key], two[key]), (K, key)
        # split calls on generic data: the counts are integers of the same comparisons, the sums differ by rounding at the most
        a = local_sums(Vg, G.g, seed=9, first_perm=0, n_permutations=30)
        b = local_sums(Vg, G.g, seed=9, first_perm=30, n_permutations=35)
        assert np.array_equal(a["count_ge"] + b["count_ge"], one["count_ge"])
        assert np.array_equal(a["count_le"] + b["count_le"], one["count_le"])
        np.testing.assert_allclose(a["sum_d"] + b["sum_d"], one["sum_d"], rtol=0, atol=65 * 11 * 8 * U)


# ---------------------------------------------------------------- 3. generic data
@pytest.mark.parametrize("which", ["knn", "radius", "hub"])
def test_generic_data_within_the_rounding_bounds(which):
    """neighbor_sum within 4 deg u sum |V| and local_i / gi_star within rtol 1e-11, no absolute term, of assemble_local fed the
    reference sums.  Measured worst relative errors (local_i / gi_star): k-NN 6.8e-13 / 7.3e-13, hub 5.3e-12 / 1.1e-13, radius
    8.1e-12 / 3.1e-13.  The radius figure is one element, (307, 1): S = 1.3102 against deg mean = 10 x 0.13101 leaves
    lag = 2.75e-5, a cancellation of 47,640, so ONE ulp of the mean is 1.0e-11 of local_i; the device's mean of that column is one
    ulp from the correctly rounded mean."""
    import gpu_graphs as gg
    from flashdeconv_amd.utils.local_stats import assemble_local, local_spatial_statistics
    G = {"knn": gg._knn, "hub": gg._hub}[which](130) if which != "radius" else gg._radius_isolated()
    V = _generic(G.n, 7, 41)
    got = local_spatial_statistics(V, G.g)
    assert set(got) == BASE_KEYS
    S, deg = ref.neighbor_sums(V, G.A)
    bound = 4 * deg[:, None] * U * (G.A @ np.abs(V))
    err = np.abs(got["neighbor_sum"] - S)
    print(f"{which}: max |S - ref| {err.max():.3e}, worst err / bound {np.max(err[bound > 0] / bound[bound > 0]):.3e}")
    assert np.all(err <= bound) and np.array_equal(got["degree"], deg)
    n = G.n
    # the reference mean is the correctly rounded one (math.fsum): where lag = S - deg mean cancels, an ulp of the mean is far
    # more than an ulp of the statistic, and V.sum(0) / n is itself up to 6 ulps off on this data
    mean = np.array([math.fsum(V[:, a]) / n for a in range(V.shape[1])])
    m2 = np.array([math.fsum((V[:, a] - mean[a]) ** 2) for a in range(V.shape[1])])
    print(f"{which}: device mean - reference mean in ulps {((got['mean'] - mean) / np.spacing(mean)).tolist()}")
    want = assemble_local(V, S, deg, mean, m2, n, int(deg.sum()))
    np.testing.assert_allclose(got["mean"], mean, rtol=1e-13)
    np.testing.assert_allclose(got["m2"], m2, rtol=1e-12)
    for key in ("local_i", "gi_star"):
        assert np.array_equal(np.isnan(got[key]), np.isnan(want[key])), key
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(want[key] != 0, np.abs(got[key] - want[key]) / np.abs(want[key]), np.abs(got[key]))
        print(f"{which}: {key} worst relative error {np.nanmax(rel):.3e} at {np.unravel_index(np.nanargmax(rel), rel.shape)}")
        np.testing.assert_allclose(got[key], want[key], rtol=1e-11, atol=0, equal_nan=True)
    assert got["n"] == n and got["n_edges"] == int(deg.sum()) // 2
    np.testing.assert_allclose(got["local_i"].mean(0), _morans(V, G), rtol=1e-10)     # isolated spots contribute exact zeros


def _morans(V, G):
    from flashdeconv_amd.utils.spatial_stats import spatial_autocorrelation
    return spatial_autocorrelation(V, G.g)["morans_i"]


# ---------------------------------------------------------------- 4. a planted pattern
def test_planted_block_is_a_hot_spot_and_noise_is_not():
    """25 x 24 lattice with 8 neighbours: column 0 is 1 inside the 6 x 6 block of rows 8 .. 13, columns 9 .. 14 and 0 elsewhere,
    column 1 is RandomState(17).rand noise; R = 199, seed 2.  An interior spot of the block (its 8 neighbours inside) has S = 8,
    and a draw reaches 8 only from 8 of the 35 other block spots among 599: p_greater = 1 / 200.  On the CPU reference
    (tests/local_stats_ref.py) with this seed the noise column's share of p_value <= 0.05 is 0.0750."""
    import gpu_graphs as gg
    from flashdeconv_amd.utils.local_stats import local_spatial_statistics
    G = gg._grid()
    V, inner = _planted()
    got = local_spatial_statistics(V, G.g, n_permutations=199, random_state=2)
    assert set(got) == BASE_KEYS | PERM_KEYS and got["n_permutations"] == 199
    assert inner.sum() == 16
    assert np.all(got["quadrant"][inner, 0] == 1) and np.all(got["gi_star"][inner, 0] > 3)
    assert np.all(got["p_greater"][inner, 0] == 1.0 / 200) and np.all(got["local_i_p_greater"][inner, 0] == 1.0 / 200)
    share = float(np.mean(got["p_value"][:, 1] <= 0.05))
    print(f"noise column: share of p_value <= 0.05 = {share:.4f}")
    assert share < 0.15


def _planted():
    yy, xx = np.mgrid[0:25, 0:24]
    yy, xx = yy.ravel(), xx.ravel()
    block = (yy >= 8) & (yy <= 13) & (xx >= 9) & (xx <= 14)
    inner = (yy >= 9) & (yy <= 12) & (xx >= 10) & (xx <= 13)
    V = np.stack([block.astype(np.float64), np.random.RandomState(17).rand(600)], 1)
    return V, inner


# ---------------------------------------------------------------- 5. input kinds and refusals
def test_input_kinds():
    import torch
    import gpu_graphs as gg
    from flashdeconv_amd.utils.local_stats import local_spatial_statistics, local_sums
    G = gg._knn(130)
    V = _generic(130, 5, 8)
    V32 = V.astype(np.float32)
    kw = dict(n_permutations=33, random_state=2)
    want, want32 = local_spatial_statistics(V, G.g, **kw), local_spatial_statistics(V32.astype(np.float64), G.g, **kw)

    def same(out, expect, cuda):
        assert set(out) == set(expect) == BASE_KEYS | PERM_KEYS
        for key in expect:
            v = out[key]
            if key in ("mean", "m2", "n", "n_edges", "n_permutations"):
                assert not isinstance(v, torch.Tensor)
                assert np.array_equal(v, expect[key]), key
                continue
            assert (isinstance(v, torch.Tensor) and v.is_cuda) if cuda else isinstance(v, np.ndarray), key
            v = _host(v)
            assert v.dtype == expect[key].dtype and v.shape == expect[key].shape, key
            if not np.array_equal(v, expect[key], equal_nan=True):
                print(f"{key}: {int(np.sum(~((v == expect[key]) | (np.isnan(v) & np.isnan(expect[key])))))} entries differ, worst "
                      f"{np.nanmax(np.abs(v - expect[key]) / np.abs(expect[key])):.3e} relative")
            assert np.array_equal(v, expect[key], equal_nan=True), key      # torch on the device forms the same IEEE operations

    same(local_spatial_statistics(V32, G.g, **kw), want32, False)
    same(local_spatial_statistics(torch.as_tensor(V, device="cuda:0"), G.g, **kw), want, True)
    same(local_spatial_statistics(torch.as_tensor(V32, device="cuda:0"), G.g, **kw), want32, True)
    wide = torch.full((130, 11), float("nan"), dtype=torch.float64, device="cuda:0")
    wide[:, :5] = torch.as_tensor(V, device="cuda:0")
    same(local_spatial_statistics(wide[:, :5], G.g, **kw), want, True)                 # row stride 11, read in place
    sums = local_sums(torch.as_tensor(V, device="cuda:0"), G.g, seed=2, n_permutations=33)
    assert all(isinstance(sums[k], torch.Tensor) and sums[k].is_cuda for k in ("neighbor_sum", "degree") + PERM_ARRAYS)
    # the same graph uploaded for the call keeps the caller's order
    up = local_spatial_statistics(V, G.A, **kw)
    _same_on_both_graphs(up, want)
    # no permutations: the permutation keys are left out
    plain = local_spatial_statistics(V, G.g)
    assert set(plain) == BASE_KEYS
    for key in plain:
        assert np.array_equal(plain[key], want[key], equal_nan=True), key


def _same_on_both_graphs(got, want):
    """A device-built graph (solver order) against the same adjacency uploaded from CSR (caller's order).  The ELL keeps a row's
    entries in ascending caller's index, so the neighbour sums add in the same order on both and, with them, the counts, the sums
    and everything formed from them alone are the same bits; the mean too (column sums in the caller's order).  m2 is summed in
    position order, which differs between the two graphs (and must: it is the m2 of fdx_spatial_autocorr_dev on that graph, bit
    for bit), so m2 and the two statistics that divide by it or by its root, local_i and gi_star, cannot be the same bits.  They
    are held to the bound of a sum of n non-negative terms added in two orders, 2 n u each way, and two more roundings of the
    division: rtol 4 (n + 2) u (1.8e-13 at n = 200) - Z, lag and every other factor are the same bits, so nothing cancels."""
    assert set(got) == set(want)
    rtol = 4 * (int(want["n"]) + 2) * U
    for key in want:
        g, w = np.asarray(_host(got[key])), np.asarray(_host(want[key]))
        if key in ("m2", "local_i", "gi_star"):
            with np.errstate(divide="ignore", invalid="ignore"):
                print(f"{key}: worst relative difference {np.nanmax(np.where(w != 0, np.abs(g - w) / np.abs(w), 0.0)):.3e} (bound {rtol:.3e})")
            np.testing.assert_allclose(g, w, rtol=rtol, atol=0, equal_nan=True)
        else:
            assert np.array_equal(g, w, equal_nan=g.dtype.kind == "f"), key


def test_stage_level_entry_refusals():
    import torch
    import gpu_graphs as gg
    from flashdeconv_amd import _lib
    lib = _lib.load()
    G = gg._knn(130)
    n, K = 130, 4
    Vd = torch.as_tensor(_dyadic(n, K, 10), device="cuda:0")
    S = torch.empty((n, K), dtype=torch.float64, device="cuda:0")
    deg = torch.empty(n, dtype=torch.int32, device="cuda:0")
    ge, le = (torch.empty((n, K), dtype=torch.int32, device="cuda:0") for _ in range(2))
    sd, sq = (torch.empty((n, K), dtype=torch.float64, device="cuda:0") for _ in range(2))
    mean, m2, counts = np.zeros(K), np.zeros(K), np.zeros(3, dtype=np.int64)

    def call(gh=G.g.handle, vp=Vd.data_ptr(), ld=K, k=K, first=0, cnt=2, drop=()):
        dev = [None if i in drop else ctypes.c_void_p(t.data_ptr()) for i, t in enumerate((S, deg, ge, le, sd, sq))]
        host = [None if 6 + i in drop else p for i, p in enumerate((_lib.ptr_f64(mean), _lib.ptr_f64(m2), _lib.ptr_i64(counts)))]
        return lib.fdx_local_stats_dev(gh, None if vp is None else ctypes.c_void_p(vp), ld, k, ctypes.c_uint64(1), first, cnt, *dev,
                                       *host, None)

    _lib.check(call())
    torch.cuda.synchronize()
    assert counts[0] == n and bool(torch.all(ge + le >= 2))
    _lib.check(call(cnt=0, drop=(2, 3, 4, 5)))                                          # R = 0 accepts null permutation outputs
    for bad, msg in ([(dict(drop=(i,)), "null argument") for i in range(9)] +
                     [(dict(vp=None), "null argument"), (dict(gh=None), "null argument"), (dict(ld=K - 1), "ldv at least K"),
                      (dict(k=0), "K must be positive"), (dict(first=-1), "must not be negative"),
                      (dict(cnt=-1), "must not be negative"), (dict(cnt=2 ** 31), "below 2\\^31")]):
        with pytest.raises(_lib.FdxError, match=msg):
            _lib.check(call(**bad))
    # "a graph without device tables" is refused too (capi_dev.cpp), but no such graph can be made from Python: every builder
    # (from_csr, the k-NN and radius builds, localize) allocates the ELL, slice offsets and degrees of a graph with n >= 1, and a
    # graph with n = 0 returns before the tables are looked at
    local = ctypes.c_void_p()
    bounds = np.array([0, 256, 600], dtype=np.int64)                                   # (range starts are multiples of 256)
    _lib.check(lib.fdx_graph_localize(gg._knn(600).g.handle, 2, _lib.ptr_i64(bounds), 0, None, ctypes.byref(local)))
    shard = _lib.Graph(local.value)
    try:
        with pytest.raises(_lib.FdxError, match="shard"):
            _lib.check(call(gh=shard.handle))
    finally:
        shard.close()


# ---------------------------------------------------------------- 6. model and AnnData surface
@pytest.mark.parametrize("output", ["numpy", "torch"])
def test_model_method(output):
    from flashdeconv_amd import FlashDeconv
    from flashdeconv_amd.utils.local_stats import local_spatial_statistics
    Y, X, coords, _ = datagen.count_like(200, 300, 5, 0.1, seed=9)
    m = FlashDeconv(sketch_dim=64, max_iter=20, random_state=3).fit(Y, X, coords, output=output)
    with pytest.raises(ValueError, match="n_permutations must be an int >= 0"):
        m.get_local_spatial_statistics(n_permutations=-1)
    with pytest.raises(ValueError, match="Unknown what"):
        m.get_local_spatial_statistics(what="counts")
    got = m.get_local_spatial_statistics(n_permutations=33)
    want = local_spatial_statistics(m.proportions_, m.adjacency_, n_permutations=33, random_state=3)
    assert set(got) == set(want) == BASE_KEYS | PERM_KEYS and got["n_permutations"] == 33
    _same_on_both_graphs(got, want)
    assert isinstance(got["local_i"], np.ndarray) == (output == "numpy")
    same = m.get_local_spatial_statistics(n_permutations=33, random_state=3)
    other = m.get_local_spatial_statistics(n_permutations=33, random_state=4)
    assert np.array_equal(_host(same["p_value"]), _host(got["p_value"]))
    assert not np.array_equal(_host(other["p_value"]), _host(got["p_value"]))
    assert np.array_equal(_host(other["local_i"]), _host(got["local_i"]))
    plain = m.get_local_spatial_statistics(what="abundances")
    assert set(plain) == BASE_KEYS
    p = _host(got["p_value"])
    assert np.all((p >= 2.0 / 34) & (p <= 1)) and np.isfinite(_host(got["gi_star"])).all()
    np.testing.assert_allclose(_host(got["local_i"]).mean(0), m.get_spatial_autocorrelation()["morans_i"], rtol=1e-10)


def test_deconvolve_writes_the_local_tables_on_request_only():
    import flashdeconv_amd as fd
    from flashdeconv_amd.io import prepare_data
    case = datagen.anndata_case()
    kw = dict(cell_type_key="celltype", sketch_dim=64, k_neighbors=4, n_hvg=300, n_markers_per_type=20)
    st0, ref0 = datagen.anndata_objects(case)
    assert fd.tl.deconvolve(st0, ref0, **kw) is None
    st, ref1 = datagen.anndata_objects(case)
    assert fd.tl.deconvolve(st, ref1, local_stats=True, **kw) is None
    assert set(st.obsm) == set(st0.obsm) | {"flashdeconv_local_moran", "flashdeconv_hotspot"}
    assert set(st.uns) == set(st0.uns) and set(st.obs.columns) == set(st0.obs.columns)
    assert set(st.uns["flashdeconv_params"]) == set(st0.uns["flashdeconv_params"]) | {"local_stats"}
    assert st.uns["flashdeconv_params"]["local_stats"] is True

    st2, ref2 = datagen.anndata_objects(case)
    assert fd.tl.deconvolve(st2, ref2, local_stats=True, spatial_permutations=29, **kw) is None
    assert set(st2.obsm) == set(st.obsm) | {"flashdeconv_hotspot_pvalue"}
    assert st2.uns["flashdeconv_params"]["spatial_permutations"] == 29
    Y, X, coords, names, _ = prepare_data(st2, ref2, cell_type_key="celltype")
    m = fd.FlashDeconv(sketch_dim=64, k_neighbors=4, n_hvg=300, n_markers_per_type=20).fit(Y, X, coords)
    want = m.get_local_spatial_statistics(n_permutations=29)
    types = [str(t) for t in names]
    for key, field in (("flashdeconv_local_moran", "local_i"), ("flashdeconv_hotspot", "gi_star"),
                       ("flashdeconv_hotspot_pvalue", "p_value")):
        df = st2.obsm[key]
        assert list(df.index) == list(st2.obs_names) and list(df.columns) == types
        np.testing.assert_array_equal(df.values, want[field])
    np.testing.assert_array_equal(st.obsm["flashdeconv_hotspot"].values, st2.obsm["flashdeconv_hotspot"].values)
    pv = st2.obsm["flashdeconv_hotspot_pvalue"].values
    assert np.all((pv[~np.isnan(pv)] >= 2.0 / 30) & (pv[~np.isnan(pv)] <= 1.0))
