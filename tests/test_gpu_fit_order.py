"""The order in which a repeated fit queues its work (csrc/fit.cpp, solver.cpp, graph_cache.cpp) changes no bit of any output.

A fit whose sketch plan and X side come from their caches launches the sketch ahead of the side-stream preamble (the abundance
buffers and their pad fills are queued behind it and reach the sweeps through the same event), and a hit of the graph cache
computes no bounding box.  Everything here is compared BITWISE between the first fit of a model (every cache misses: the old
order), its repeats (every cache hits: the new order), a fit under FDX_NO_PLAN_CACHE=1 and one under FDX_NO_SIDE_STREAM=1 (no
second stream anywhere); the solve loop's rel_change trace and iteration count likewise, at every chunk edge.  Shapes: n in {1, 63, 257, 600} spots (one spot; less than a slice; more than a tile; several
tiles and blocks), 64 genes, 7 types, sketch_dim 32, k = 6, uniform random coordinates."""
import ctypes

import numpy as np
import pytest

import datagen

pytestmark = pytest.mark.gpu

NS = (1, 63, 257, 600)
G, K, D, KNN_K = 64, 7, 32, 6
KNN, RADIUS, GIVEN = 0, 1, 2   # FDX_GRAPH_KNN, FDX_GRAPH_RADIUS, FDX_GRAPH_GIVEN (include/fdx.h)


def _lib():
    from flashdeconv_amd import _lib as L
    return L


def _graph_stats():
    out = (ctypes.c_int64 * 4)()
    _lib().check(_lib().load().fdx_graph_cache_stats(out))
    return np.array(list(out), dtype=np.int64)


def _x_stats():
    """leverage hits, misses, X-side hits, misses."""
    out = (ctypes.c_int64 * 4)()
    _lib().check(_lib().load().fdx_x_cache_stats(out))
    return np.array(list(out), dtype=np.int64)


def _trim():
    _lib().check(_lib().load().fdx_trim())


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _uniform(n, dim=2, seed=0):
    return np.random.RandomState(7000 + 10 * n + seed).rand(n, dim) * np.sqrt(n)


# ------------------------------------------------------------------------------------------------ same bits on every path
def _outputs(m):
    return dict(beta=m.beta_.copy(), proportions=m.proportions_.copy(), n_iterations=m.info_["n_iterations"],
                final_change=m.info_["final_change"], final_objective=m.info_["final_objective"], lambda_used=m.lambda_used_)


def _same_outputs(a, b, what):
    for key in a:
        assert np.array_equal(a[key], b[key]), (what, key)


@pytest.mark.parametrize("n", NS)
def test_first_fit_repeats_uncached_and_one_stream_give_the_same_bits(monkeypatch, n):
    from flashdeconv_amd import FlashDeconv
    Y, X, _, _ = datagen.count_like(n, G, K, 0.1, 300 + n)
    Y = Y.astype(np.float64)
    coords = _uniform(n)
    kw = dict(sketch_dim=D, k_neighbors=KNN_K, max_iter=30, random_state=n)
    _trim()
    m = FlashDeconv(**kw)
    g0, x0 = _graph_stats(), _x_stats()
    first = _outputs(m.fit(Y, X, coords))
    g1, x1 = _graph_stats(), _x_stats()
    assert np.array_equal((x1 - x0), [0, 1, 0, 1]), "the first fit misses the leverage and the X-side cache"
    assert np.array_equal((g1 - g0)[:2], [0, 1])
    for rep in (2, 3):
        _same_outputs(_outputs(m.fit(Y, X, coords)), first, f"fit {rep} of the model")
    assert np.array_equal((_x_stats() - x1), [2, 0, 2, 0]), "the repeats hit both"
    if n > 1:                                                  # (a graph of one spot is never published)
        assert np.array_equal((_graph_stats() - g1)[:2], [2, 0])
    monkeypatch.setenv("FDX_NO_PLAN_CACHE", "1")
    _same_outputs(_outputs(FlashDeconv(**kw).fit(Y, X, coords)), first, "FDX_NO_PLAN_CACHE")
    monkeypatch.delenv("FDX_NO_PLAN_CACHE")
    monkeypatch.setenv("FDX_NO_SIDE_STREAM", "1")
    _same_outputs(_outputs(FlashDeconv(**kw).fit(Y, X, coords)), first, "FDX_NO_SIDE_STREAM")
    monkeypatch.delenv("FDX_NO_SIDE_STREAM")
    _same_outputs(_outputs(m.fit(Y, X, coords)), first, "and back")


# ------------------------------------------------------------------------------------------------ lookup
def _build(t, method=KNN, k=KNN_K, radius=0.0):
    L = _lib()
    n, dim = tuple(t.shape)
    h = ctypes.c_void_p()
    L.check(L.load().fdx_graph_build_dev(ctypes.c_void_p(t.data_ptr()), n, dim, method, k, float(radius), None, ctypes.byref(h)))
    return L.Graph(h.value)


def _adjacency(g):
    """The exported CSR arrays (asking for them also completes a queued build, which publishes it)."""
    indptr, indices = g.to_csr_arrays()
    return np.asarray(indptr).copy(), np.asarray(indices).copy()


def _same_adjacency(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _uncached_adjacency(monkeypatch, t, **kw):
    monkeypatch.setenv("FDX_NO_PLAN_CACHE", "1")
    s0 = _graph_stats()
    out = _adjacency(_build(t, **kw))
    assert np.array_equal(_graph_stats(), s0)
    monkeypatch.delenv("FDX_NO_PLAN_CACHE")
    return out


def _last_word_changed(pts):
    other = pts.copy()
    other.ravel()[-1] = np.nextafter(other.ravel()[-1], np.inf)
    return other


def _delta(s0):
    return (_graph_stats() - s0)[:2]


@pytest.mark.parametrize("dim", [2, 4])
@pytest.mark.parametrize("n", NS[1:])
def test_lookup_without_a_box_hits_and_misses_as_before(monkeypatch, n, dim):
    """A candidate that differs in its last 64-bit word is a miss whose build (own box, second round trip) gives the graph of an
    uncached build; the cached slide is a hit afterwards; with two cached slides of one size the second one is found.  dim = 4:
    the k-NN build bins the first three coordinates and searches in all four - the compare kernel sees all of them."""
    _trim()
    a = _uniform(n, dim)
    ta, tb = _dev(a), _dev(_last_word_changed(a))
    s0 = _graph_stats()
    want_a = _adjacency(_build(ta))
    assert np.array_equal(_delta(s0), [0, 1])                 # no candidate
    s0 = _graph_stats()
    got_b = _adjacency(_build(tb))
    assert np.array_equal(_delta(s0), [0, 1])                 # a candidate, compared, different
    _same_adjacency(got_b, _uncached_adjacency(monkeypatch, tb))
    for t, want in ((ta, want_a), (tb, got_b), (ta, want_a)):  # two entries of this n: the older one is the second candidate
        s0 = _graph_stats()
        _same_adjacency(_adjacency(_build(_dev(t.cpu().numpy()))), want)
        assert np.array_equal(_delta(s0), [1, 0])
    _same_adjacency(want_a, _uncached_adjacency(monkeypatch, ta))
    tc = _dev(_last_word_changed(_last_word_changed(a)))       # a third slide: compared with both entries, a miss, evicts one
    s0 = _graph_stats()
    _same_adjacency(_adjacency(_build(tc)), _uncached_adjacency(monkeypatch, tc))
    assert np.array_equal(_delta(s0), [0, 1]) and _graph_stats()[2] == 2


@pytest.mark.parametrize("n", NS[1:])
def test_radius_lookup_hits_and_misses_and_four_coordinates_are_refused_as_before(monkeypatch, n):
    """The radius method: same rules.  With dim = 4 it takes no coordinates at all (1 to 3 only) - the call fails behind a counted
    miss as it always did, leaves no entry and does not disturb the entries that are there."""
    L = _lib()
    _trim()
    a = _uniform(n, 3)
    ta, tb = _dev(a), _dev(_last_word_changed(a))
    kw = dict(method=RADIUS, k=0, radius=1.5)
    want_a = _adjacency(_build(ta, **kw))
    s0 = _graph_stats()
    _same_adjacency(_adjacency(_build(tb, **kw)), _uncached_adjacency(monkeypatch, tb, **kw))
    assert np.array_equal(_delta(s0), [0, 1])
    t4 = _dev(_uniform(n, 4))
    for _ in range(2):
        s0 = _graph_stats()
        with pytest.raises(L.FdxError):
            _build(t4, **kw)
        assert np.array_equal((_graph_stats() - s0)[:3], [0, 1, 0])
    s0 = _graph_stats()
    _same_adjacency(_adjacency(_build(ta, **kw)), want_a)
    assert np.array_equal(_delta(s0), [1, 0])
    _same_adjacency(want_a, _uncached_adjacency(monkeypatch, ta, **kw))


def test_one_spot_is_never_cached_and_every_build_of_it_counts_as_a_miss():
    """n = 1: the empty graph is not built from the coordinates and is not published (unchanged); nothing is compared."""
    _trim()
    t = _dev(_uniform(1))
    for _ in range(2):
        s0 = _graph_stats()
        g = _build(t)
        assert g.info()[0] == 1
        assert np.array_equal((_graph_stats() - s0)[:3], [0, 1, 0])


def test_fits_of_a_changed_and_of_the_cached_slide(monkeypatch):
    """Fit level, n = 600: a slide that differs in its last word misses and gets the adjacency of an uncached build; the cached
    slide fitted again afterwards hits."""
    from flashdeconv_amd import FlashDeconv
    n = NS[-1]
    Y, X, _, _ = datagen.count_like(n, G, K, 0.1, 41)
    Y = Y.astype(np.float64)
    a = _uniform(n, 2, seed=3)
    b = _last_word_changed(a)
    kw = dict(sketch_dim=D, k_neighbors=KNN_K, max_iter=10, random_state=1)
    _trim()
    s0 = _graph_stats()
    ma = FlashDeconv(**kw).fit(Y, X, a)
    mb = FlashDeconv(**kw).fit(Y, X, b)
    assert np.array_equal(_delta(s0), [0, 2])
    s0 = _graph_stats()
    ma2 = FlashDeconv(**kw).fit(Y, X, a.copy())
    assert np.array_equal(_delta(s0), [1, 0])
    monkeypatch.setenv("FDX_NO_PLAN_CACHE", "1")
    cold_a, cold_b = FlashDeconv(**kw).fit(Y, X, a), FlashDeconv(**kw).fit(Y, X, b)
    monkeypatch.delenv("FDX_NO_PLAN_CACHE")
    for got, want in ((ma, cold_a), (mb, cold_b), (ma2, cold_a)):
        A, B = got.adjacency_, want.adjacency_
        assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
        assert np.array_equal(got.beta_, want.beta_) and np.array_equal(got.proportions_, want.proportions_)


# ------------------------------------------------------------------------------------------------ solve loop
class _Problem:
    """One gaussian/raw problem resident on the device, fitted through fdx_fit_dev itself: FlashDeconv does not hand out the
    rel_change trace."""

    def __init__(self, n, seed):
        import torch
        from flashdeconv_amd.core.sketching import sketch_tables
        L = _lib()
        Y, X, coords, _ = datagen.gaussian_raw(n, G, K, seed=seed)
        self.n = n
        self.Y, self.coords = _dev(Y), _dev(coords)
        self.X = np.ascontiguousarray(X, dtype=np.float64)
        self.bucket, self.wy, self.wx, self.mode_y, self.mode_x = sketch_tables(G, D, None, 5, "raw", self.X)
        self.graph = _build(self.coords)
        torch.cuda.synchronize()

    def fit(self, max_iter, tol):
        """(n_iterations, converged, rel_change trace, beta) of one fit."""
        import torch
        L = _lib()
        prm = L.FitParams()
        prm.sketch_dim, prm.mode_y, prm.mode_x = D, self.mode_y, self.mode_x
        prm.graph_method, prm.k_neighbors = GIVEN, KNN_K
        prm.lambda_auto, prm.max_iter, prm.verbose = 1, int(max_iter), 0
        prm.rho_sparsity, prm.tol = 0.01, float(tol)
        beta = torch.empty((self.n, K), dtype=torch.float64, device="cuda")
        prop = torch.empty((self.n, K), dtype=torch.float64, device="cuda")
        objs = np.zeros(max(max_iter, 1))
        rels = np.full(max(max_iter, 1), -1.0)
        info = L.FitInfo()
        gh = ctypes.c_void_p(self.graph.handle.value)
        torch.cuda.synchronize()
        L.check(L.load().fdx_fit_dev(ctypes.c_void_p(self.Y.data_ptr()), L.FDX_F64, self.n, G, G, L.ptr_f64(self.X), K,
                                     L.ptr_i32(self.bucket), L.ptr_f64(self.wy), L.ptr_f64(self.wx),
                                     ctypes.c_void_p(self.coords.data_ptr()), 2, ctypes.byref(prm), ctypes.byref(gh),
                                     ctypes.c_void_p(beta.data_ptr()), ctypes.c_void_p(prop.data_ptr()), L.ptr_f64(objs),
                                     L.ptr_f64(rels), ctypes.byref(info), None))
        n_it = int(info.solve.n_iterations)
        return n_it, bool(info.solve.converged), rels[:n_it].copy(), beta.cpu().numpy()


@pytest.fixture(scope="module")
def problems():
    return {n: _Problem(n, seed=90 + n) for n in NS}


def _one_stream(monkeypatch, p, max_iter, tol):
    monkeypatch.setenv("FDX_NO_SIDE_STREAM", "1")
    out = p.fit(max_iter, tol)
    monkeypatch.delenv("FDX_NO_SIDE_STREAM")
    return out


def _two_streams_equal_one(monkeypatch, p, max_iter, tol):
    """The fit without a side stream against two fits with it: whatever the caches held before, the second of them finds the
    X side cached (the sketch launched first, the abundance buffers prepared behind it)."""
    want = _one_stream(monkeypatch, p, max_iter, tol)
    for rep in range(2):
        x0 = _x_stats()
        got = p.fit(max_iter, tol)
        if rep == 1:
            assert np.array_equal((_x_stats() - x0)[2:], [1, 0])
        assert got[0] == want[0] and got[1] == want[1], (rep, got[:2], want[:2])
        assert np.array_equal(got[2], want[2]), rep
        assert np.array_equal(got[3], want[3]), rep
    return want


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("max_iter", [0, 1, 3, 4, 5, 9])
def test_trace_at_the_chunk_edges_and_with_the_sweeps_queued_ahead(monkeypatch, problems, n, max_iter):
    """tol = 0 never stops (a rel_change is not negative): max_iter sweeps, all real.  0: no sweep; 1, 3: inside the first chunk
    of four; 4: exactly one chunk, nothing queued ahead; 5: the one sweep queued ahead is the second chunk; 9: two sweeps queued
    ahead of each read-back, three chunks."""
    n_it, converged, trace, _ = _two_streams_equal_one(monkeypatch, problems[n], max_iter, 0.0)
    assert n_it == max_iter and not converged and trace.shape == (max_iter,)
    assert np.all(trace >= 0.0)


@pytest.mark.parametrize("n", NS)
def test_trace_when_the_first_sweep_converges(monkeypatch, problems, n):
    """tol above any rel_change: one iteration, the three sweeps behind it in the chunk and the two queued ahead are no-ops."""
    n_it, converged, trace, _ = _two_streams_equal_one(monkeypatch, problems[n], 30, 1e300)
    assert n_it == 1 and converged and trace.shape == (1,)


@pytest.mark.parametrize("n", NS)
def test_trace_when_the_solve_converges_inside_the_second_chunk(monkeypatch, problems, n):
    """The headline's pattern (gaussian/raw: converges behind the first read-back): the tolerance is put between two values of the
    one-stream fit's own tol = 0 trace so that the stopping rule first holds at an iteration of the second chunk (4 .. 7)."""
    p = problems[n]
    _, _, free, _ = _one_stream(monkeypatch, p, 9, 0.0)
    at = next((j for j in range(4, 8) if free[j] < free[:j].min()), None)
    assert at is not None, free                                # (a trace that keeps falling that far)
    tol = 0.5 * (free[at] + free[:at].min())
    n_it, converged, trace, _ = _two_streams_equal_one(monkeypatch, p, 30, tol)
    assert n_it == at + 1 and converged
    assert np.array_equal(trace, free[:at + 1])
