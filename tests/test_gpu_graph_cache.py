"""The cache of whole spatial graphs by content of the coordinates (csrc/graph_cache.h, graph_cache.cpp; fdx_graph_build_dev looks a
build up there first).  A hit hands out the graph the first build produced, so every comparison here is BITWISE: every array a
graph exports - CSR, spot order, counts, tie count, tile information - against the same call under FDX_NO_PLAN_CACHE=1, which
bypasses the cache; fdx_graph_cache_stats tells a hit from a miss."""
import ctypes
import warnings

import numpy as np
import pytest

import datagen

pytestmark = pytest.mark.gpu

KNN, RADIUS = 0, 1   # FDX_GRAPH_KNN, FDX_GRAPH_RADIUS (include/fdx.h)
SWITCHES = ("FDX_GRAPH_SORT", "FDX_GRAPH_SYNC", "FDX_GRAPH_WCAP", "FDX_GRAPH_WCAP_RANK", "FDX_GRAPH_TWO_ELL_KERNELS", "FDX_NO_TILED")


def _lib():
    from flashdeconv_amd import _lib as L
    return L


def _stats():
    """{hits, misses, entries, bytes held}; hits and misses since the library was loaded."""
    out = (ctypes.c_int64 * 4)()
    _lib().check(_lib().load().fdx_graph_cache_stats(out))
    return np.array(list(out), dtype=np.int64)


def _trim():
    _lib().check(_lib().load().fdx_trim())


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _build(t, method=KNN, k=6, radius=0.0, stream=None, shape=None):
    """fdx_graph_build_dev on a device tensor (its bytes read as `shape`, by default its own)."""
    L = _lib()
    n, dim = shape if shape is not None else tuple(t.shape)
    h = ctypes.c_void_p()
    L.check(L.load().fdx_graph_build_dev(ctypes.c_void_p(t.data_ptr()), n, dim, method, k, float(radius), stream, ctypes.byref(h)))
    return L.Graph(h.value)


def _arrays(g):
    """Everything a graph exports (asking for it also completes a queued build, which publishes it)."""
    import torch
    L = _lib()
    info = g.info()
    indptr, indices = g.to_csr_arrays()
    perm = torch.empty(max(info[0], 1), dtype=torch.int32, device="cuda")
    L.check(L.load().fdx_graph_perm_dev(g.handle, ctypes.c_void_p(perm.data_ptr()), None))
    torch.cuda.synchronize()
    return dict(indptr=indptr, indices=indices, perm=perm.cpu().numpy()[:info[0]], info=np.array(info), ties=np.array(g.knn_ties()),
                tiles=np.array(g.tile_info(), dtype=np.int64))


def _same(a, b):
    assert a.keys() == b.keys()
    for key in a:
        assert np.array_equal(a[key], b[key]), key


def _uncached(monkeypatch, fn):
    """fn() with the cache bypassed; the bypassed call counts as neither a hit nor a miss and leaves no entry."""
    monkeypatch.setenv("FDX_NO_PLAN_CACHE", "1")
    s0 = _stats()
    out = fn()
    assert np.array_equal(_stats(), s0)
    monkeypatch.delenv("FDX_NO_PLAN_CACHE")
    return out


def _points(n, dim, seed=0):
    return np.random.RandomState(1000 * dim + seed).rand(n, dim) * np.sqrt(n)


def _lattice():
    j, i = np.meshgrid(np.arange(32.0), np.arange(32.0))
    return np.stack([i.ravel(), j.ravel()], axis=1)


def _hit_equals_uncached(monkeypatch, pts, **kw):
    """Build (miss), consume, build again from an equal tensor in ANOTHER allocation (hit): the hit's graph, still there after the
    first handle and the first tensor are gone, is the graph of an uncached build."""
    t1 = _dev(pts)
    s0 = _stats()
    g1 = _build(t1, **kw)
    first = _arrays(g1)
    s1 = _stats()
    assert np.array_equal((s1 - s0)[:2], [0, 1]) and s1[2] >= 1, (s0, s1)
    t2 = _dev(pts)
    assert t2.data_ptr() != t1.data_ptr()
    g1.close()
    t1.fill_(-7.0)                                                    # the entry owns its copy
    del t1
    g2 = _build(t2, **kw)
    assert np.array_equal((_stats() - s1)[:2], [1, 0])
    hit = _arrays(g2)
    cold = _uncached(monkeypatch, lambda: _arrays(_build(t2, **kw)))
    _same(hit, cold)
    _same(first, cold)
    return g2, t2, cold


@pytest.mark.parametrize("dim", [1, 2, 3])
@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 257, 1000, 5000])
def test_knn_hit_is_the_graph_of_an_uncached_build(monkeypatch, n, dim):
    """Uniform points; n * dim odd in a third of the cases (the tail of the compare kernel), one block and many."""
    _trim()
    for k in (1, 6):
        _hit_equals_uncached(monkeypatch, _points(n, dim), k=k)


def test_radius_grid_and_lattice_graphs_hit_with_the_same_bits(monkeypatch):
    from flashdeconv_amd import FlashDeconv
    _trim()
    pts = _points(1000, 2)
    _hit_equals_uncached(monkeypatch, pts, method=RADIUS, k=0, radius=1.7)
    _hit_equals_uncached(monkeypatch, _points(1000, 3), method=RADIUS, k=0, radius=2.5)
    for coords in (pts, _lattice()):                                  # "grid": radius from the median nearest distance
        gm, gk, gr = FlashDeconv(spatial_method="grid")._graph_request(coords, coords)
        assert gm == RADIUS
        _hit_equals_uncached(monkeypatch, coords, method=gm, k=gk, radius=gr)
    g, _, cold = _hit_equals_uncached(monkeypatch, _lattice(), k=6)   # k-NN on a lattice: ties, and their count with the entry
    assert cold["ties"] > 0 and g.knn_ties() == cold["ties"]


def test_any_changed_word_is_a_miss(monkeypatch):
    """One word at the first, a middle and the last position; one ulp; 0.0 -> -0.0; the SAME tensor modified in place."""
    _trim()
    n, dim = 1001, 3                                                  # 3003 words: not a multiple of anything the kernel strides by
    pts = _points(n, dim)
    pts[500, 1] = 0.0
    base = _dev(pts)
    _arrays(_build(base))
    flat = pts.ravel()
    changes = [(0, flat[0] + 1.0), (1234, flat[1234] + 1.0), (flat.size - 1, flat[-1] + 1.0), (flat.size - 1, np.nextafter(flat[-1], np.inf)),
               (0, np.nextafter(flat[0], -np.inf)), (500 * dim + 1, -0.0)]
    for at, value in changes:
        other = pts.copy()
        other.ravel()[at] = value
        t = _dev(other)
        s0 = _stats()
        g = _build(t)
        got = _arrays(g)
        assert np.array_equal((_stats() - s0)[:2], [0, 1]), (at, value)
        _same(got, _uncached(monkeypatch, lambda: _arrays(_build(t))))
    s0 = _stats()
    again = _dev(pts)
    g = _build(again)                                                 # (the six misses evicted it: two entries)
    _arrays(g)
    assert np.array_equal((_stats() - s0)[:2], [0, 1])
    s0 = _stats()
    _build(again)
    assert np.array_equal((_stats() - s0)[:2], [1, 0])
    again[n - 1, dim - 1] += 0.5                                      # pointer equal, content not
    s0 = _stats()
    moved = _arrays(_build(again))
    assert np.array_equal((_stats() - s0)[:2], [0, 1])
    _same(moved, _uncached(monkeypatch, lambda: _arrays(_build(again))))


def test_same_bytes_under_another_k_method_radius_or_shape_is_a_miss(monkeypatch):
    _trim()
    t = _dev(_points(1500, 2))
    base = dict(method=KNN, k=6, radius=0.0, shape=(1500, 2))
    _arrays(_build(t, **base))
    for change in (dict(k=5), dict(method=RADIUS, radius=1.5), dict(method=RADIUS, radius=1.75), dict(shape=(1000, 3)), dict(shape=(3000, 1))):
        kw = {**base, **change}
        s0 = _stats()
        _build(t, **base)                                             # (most recently used again: the next miss evicts the other entry)
        got = _arrays(_build(t, **kw))
        assert np.array_equal((_stats() - s0)[:2], [1, 1]), change
        _same(got, _uncached(monkeypatch, lambda: _arrays(_build(t, **kw))))


@pytest.mark.parametrize("switch", SWITCHES)
def test_a_graph_switch_with_another_value_is_a_miss(monkeypatch, switch):
    """The tests of the build routes compare one coordinate set under different switches: with a key that ignored them they would
    compare a graph with itself."""
    _trim()
    t = _dev(_points(3000, 2))
    plain = _arrays(_build(t))
    monkeypatch.setenv(switch, "1")
    s0 = _stats()
    routed = _arrays(_build(t))
    assert np.array_equal((_stats() - s0)[:2], [0, 1])
    s0 = _stats()
    again = _arrays(_build(t))
    assert np.array_equal((_stats() - s0)[:2], [1, 0])
    cold = _uncached(monkeypatch, lambda: _arrays(_build(t)))
    _same(routed, cold)
    _same(again, cold)
    monkeypatch.delenv(switch)
    s0 = _stats()
    back = _arrays(_build(t))
    assert np.array_equal((_stats() - s0)[:2], [1, 0])
    _same(back, plain)


@pytest.mark.parametrize("first_goes_first", [True, False])
def test_two_handles_of_one_entry_outlive_each_other(monkeypatch, first_goes_first):
    _trim()
    t = _dev(_points(2000, 2))
    a = _build(t)
    want = _arrays(a)
    b = _build(t)
    assert a.handle.value == b.handle.value                           # one graph, counted
    (a if first_goes_first else b).close()
    _trim()                                                           # ... and without the cache's own reference
    _same(_arrays(b if first_goes_first else a), want)
    _same(want, _uncached(monkeypatch, lambda: _arrays(_build(t))))


def test_two_entries_least_recently_used_out_and_trim(monkeypatch):
    _trim()
    ts = [_dev(_points(1200, 2, seed)) for seed in (1, 2, 3)]
    want = []
    for t in ts:                                                      # three coordinate sets, room for two: the first is gone
        want.append(_arrays(_build(t)))
    for i, delta in ((1, [1, 0]), (2, [1, 0]), (0, [0, 1])):
        s0 = _stats()
        got = _arrays(_build(ts[i]))
        assert np.array_equal((_stats() - s0)[:2], delta), i
        _same(got, want[i])
    held = _build(ts[0])
    assert _stats()[2] == 2 and _stats()[3] > 2 * 1200 * 2 * 8
    _trim()
    assert np.array_equal(_stats()[2:], [0, 0])
    _same(_arrays(held), want[0])                                     # a held handle stays valid
    s0 = _stats()
    _same(_arrays(_build(ts[0])), want[0])
    assert np.array_equal((_stats() - s0)[:2], [0, 1])


@pytest.mark.parametrize("build_on_side", [True, False])
def test_built_on_one_stream_and_hit_on_another(monkeypatch, build_on_side):
    import torch
    L = _lib()
    side = ctypes.c_void_p()
    L.check(L.load().fdx_side_stream(ctypes.byref(side)))
    _trim()
    t = _dev(_points(4000, 2))
    torch.cuda.synchronize()
    streams = (side, None) if build_on_side else (None, side)
    s0 = _stats()
    a = _build(t, stream=streams[0])
    want = _arrays(a)
    t2 = t.clone()
    torch.cuda.synchronize()
    b = _build(t2, stream=streams[1])
    assert np.array_equal((_stats() - s0)[:2], [1, 1])
    _same(_arrays(b), want)
    _same(want, _uncached(monkeypatch, lambda: _arrays(_build(t))))


def test_a_failed_or_unconsumed_build_is_not_published():
    _trim()
    pts = _points(500, 2)
    bad = pts.copy()
    bad[17, 0] = np.inf
    with pytest.raises(_lib().FdxError):
        _build(_dev(bad))
    assert _stats()[2] == 0
    t = _dev(pts)
    _build(t).close()                                                 # destroyed before anything asked for it
    assert _stats()[2] == 0
    s0 = _stats()
    _arrays(_build(t))
    assert np.array_equal((_stats() - s0)[:3], [0, 1, 1])


# ---------------------------------------------------------------------------------------------------------------- fit level
def _fit(Y, X, coords, **kw):
    from flashdeconv_amd import FlashDeconv
    kw = {**dict(sketch_dim=64, k_neighbors=6, max_iter=20, random_state=0), **kw}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)                  # (k-NN ties under knn_ties="index")
        return FlashDeconv(**kw).fit(Y, X, coords)


def _same_fit(a, b):
    assert np.array_equal(a.beta_, b.beta_) and np.array_equal(a.proportions_, b.proportions_)
    assert a.info_ == b.info_ and a.lambda_used_ == b.lambda_used_
    A, B = a.adjacency_, b.adjacency_
    assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)


@pytest.fixture(scope="module")
def slides():
    """Two slides of 5000 spots x 200 genes, each with a 4-type and a 9-type reference (float64 counts)."""
    out = []
    for seed in (21, 22):
        Y4, X4, coords, _ = datagen.count_like(5000, 200, 4, 0.1, seed)
        Y9, X9, _, _ = datagen.count_like(5000, 200, 9, 0.1, seed + 10)
        out.append(dict(coords=coords, fits=[(Y4.astype(np.float64), X4, dict(random_state=0)), (Y9.astype(np.float64), X9, dict(random_state=3))]))
    return out


def test_fits_of_one_slide_share_the_graph_and_keep_their_bits(monkeypatch, slides):
    """Another X, K and random_state on the same coordinates: one miss, then hits; outputs as without the cache."""
    _trim()
    s = slides[0]
    s0 = _stats()
    got = [_fit(Y, X, s["coords"], **kw) for Y, X, kw in s["fits"]]
    got.append(_fit(*s["fits"][0][:2], s["coords"].copy(), random_state=5))
    assert np.array_equal((_stats() - s0)[:3], [2, 1, 1])
    cold = _uncached(monkeypatch, lambda: [_fit(Y, X, s["coords"], **kw) for Y, X, kw in s["fits"]] + [_fit(*s["fits"][0][:2], s["coords"], random_state=5)])
    for a, b in zip(got, cold):
        _same_fit(a, b)
    assert not np.array_equal(got[0].beta_, got[2].beta_)


def test_two_models_alternating_on_two_slides(monkeypatch, slides):
    from flashdeconv_amd import FlashDeconv
    _trim()
    models = [FlashDeconv(sketch_dim=64, max_iter=20), FlashDeconv(sketch_dim=64, max_iter=20, random_state=2)]
    s0 = _stats()
    for rnd in range(2):
        for m, s in zip(models, slides):
            Y, X, _ = s["fits"][rnd]
            m.fit(Y, X, s["coords"])
    assert np.array_equal((_stats() - s0)[:3], [2, 2, 2])
    for m, s in zip(models, slides):
        Y, X, _ = s["fits"][1]
        cold = _uncached(monkeypatch, lambda: FlashDeconv(sketch_dim=64, max_iter=20, random_state=m.random_state).fit(Y, X, s["coords"]))
        _same_fit(m, cold)


def test_lattice_fits_share_the_device_build_and_keep_their_tie_remedy(monkeypatch):
    """knn_ties="auto" on a 32 x 32 lattice: the second fit takes the device's build - tie count with it - from the cache, stops on
    the ties like the first and rebuilds on the reference's tie order; knn_ties="index" solves on the cached build itself."""
    coords = _lattice()
    Y, X, _, _ = datagen.count_like(coords.shape[0], 200, 4, 0.1, 31)
    Y = Y.astype(np.float64)
    _trim()
    s0 = _stats()
    a = _fit(Y, X, coords, knn_ties="auto")
    s1 = _stats()
    assert np.array_equal((s1 - s0)[:3], [0, 1, 1])
    b = _fit(Y, X, coords.copy(), knn_ties="auto", random_state=4)
    by_index = _fit(Y, X, coords, knn_ties="index")
    assert np.array_equal((_stats() - s1)[:3], [2, 0, 0])
    assert a.info_["knn_ties"] > 0 and b.info_["knn_ties"] == a.info_["knn_ties"] == by_index.info_["knn_ties"]
    assert a.timings_["ties_remedy_ms"] > 0.0 and b.timings_["ties_remedy_ms"] > 0.0
    cold = _uncached(monkeypatch, lambda: [_fit(Y, X, coords, knn_ties="auto"), _fit(Y, X, coords, knn_ties="auto", random_state=4),
                                           _fit(Y, X, coords, knn_ties="index")])
    for got, want in zip((a, b, by_index), cold):
        _same_fit(got, want)
    _trim()
