"""The two content-keyed caches of what depends on the signature matrix X alone (csrc/x_cache.h): the leverage scores
(csrc/fit.cpp) and the X side of a fit - X_sketch, XtX (csrc/prepare.cpp).  A hit returns what the first computation produced, so
every result here is compared BITWISE with the same call under FDX_NO_PLAN_CACHE=1, which bypasses both; fdx_x_cache_stats tells a
hit from a miss."""
import ctypes
import threading

import numpy as np
import pytest

import datagen
from conftest import load_golden

pytestmark = pytest.mark.gpu


def _stats():
    """{leverage hits, leverage misses, X-side hits, X-side misses} since the library was loaded."""
    from flashdeconv_amd import _lib
    out = (ctypes.c_int64 * 4)()
    _lib.check(_lib.load().fdx_x_cache_stats(out))
    return np.array(list(out), dtype=np.int64)


def _trim():
    from flashdeconv_amd import _lib
    _lib.check(_lib.load().fdx_trim())


def _fit(Y, X, coords, **kw):
    from flashdeconv_amd import FlashDeconv
    kw = {**dict(sketch_dim=64, k_neighbors=6, max_iter=20, random_state=0), **kw}
    return FlashDeconv(**kw).fit(Y, X, coords)


def _same_fit(a, b):
    assert np.array_equal(a.beta_, b.beta_) and np.array_equal(a.proportions_, b.proportions_)
    assert a.info_ == b.info_ and a.lambda_used_ == b.lambda_used_


def _uncached(monkeypatch, fn):
    """fn() with both caches bypassed; the bypassed call counts as neither a hit nor a miss."""
    monkeypatch.setenv("FDX_NO_PLAN_CACHE", "1")
    s0 = _stats()
    out = fn()
    assert np.array_equal(_stats(), s0)
    monkeypatch.delenv("FDX_NO_PLAN_CACHE")
    return out


def _problem(seed, n=600, G=300, K=5):
    Y, X, coords, _ = datagen.count_like(n, G, K, 0.1, seed)
    return Y.astype(np.float64), X, coords


def test_leverage_scores_of_a_repeated_matrix_are_a_hit_with_the_same_bits(monkeypatch):
    """Every matrix of tests/golden/leverage.npz (the rank-deficient one settles on the SVD fallback: that route is cached too)."""
    from flashdeconv_amd.utils.genes import compute_leverage_scores
    g = load_golden("leverage.npz")
    _trim()
    for name in g["names"]:
        X = np.ascontiguousarray(g[f"{name}_X"], dtype=np.float64)
        s0 = _stats()
        first = compute_leverage_scores(X)
        s1 = _stats()
        again = compute_leverage_scores(X.copy())                    # by content: another address
        s2 = _stats()
        assert np.array_equal(s1 - s0, [0, 1, 0, 0]) and np.array_equal(s2 - s1, [1, 0, 0, 0]), (name, s0, s1, s2)
        cold = _uncached(monkeypatch, lambda: compute_leverage_scores(X))
        assert np.array_equal(first, again) and np.array_equal(first, cold), name
        np.testing.assert_allclose(first, g[f"{name}_lev"], rtol=1e-9, atol=1e-14, err_msg=str(name))


def test_leverage_cache_misses_on_one_ulp_another_regularization_and_a_transposed_shape(monkeypatch):
    from flashdeconv_amd.utils.genes import compute_leverage_scores
    rs = np.random.RandomState(5)
    X = rs.gamma(2.0, 3.0, size=(5, 300))
    _trim()
    compute_leverage_scores(X)
    ulp = X.copy()
    ulp[3, 117] = np.nextafter(ulp[3, 117], np.inf)
    cases = [(ulp, 1e-6), (X, 1e-4), (np.ascontiguousarray(X.reshape(300, 5)), 1e-6)]   # (300, 5): the same bytes
    for Xc, reg in cases:
        s0 = _stats()
        got = compute_leverage_scores(Xc, reg)
        assert np.array_equal(_stats() - s0, [0, 1, 0, 0]), (Xc.shape, reg)
        cold = _uncached(monkeypatch, lambda: compute_leverage_scores(Xc, reg))
        assert np.array_equal(got, cold), (Xc.shape, reg)
    s0 = _stats()
    compute_leverage_scores(X)                                       # the four entries are all still there
    assert np.array_equal(_stats() - s0, [1, 0, 0, 0])


def test_second_fit_with_the_same_signatures_hits_both_caches(monkeypatch):
    """The real-use case: one reference X, another slide (Y and coordinates) per fit."""
    Y1, X, c1 = _problem(3)
    Y2, _, c2 = _problem(4)
    Y2, c2 = Y2[:555], c2[:555] * 1.5
    _trim()
    s0 = _stats()
    _fit(Y1, X, c1)
    s1 = _stats()
    assert np.array_equal(s1 - s0, [0, 1, 0, 1])
    hit = _fit(Y2, X.copy(), c2)
    assert np.array_equal(_stats() - s1, [1, 0, 1, 0])
    cold = _uncached(monkeypatch, lambda: _fit(Y2, X, c2))
    _same_fit(hit, cold)


def test_x_side_entries_of_one_matrix_do_not_alias_across_preprocessing_and_sketch_dimension(monkeypatch):
    Y, X, coords = _problem(6)
    _trim()
    variants = [dict(preprocess="raw"), dict(preprocess="log_cpm"), dict(preprocess="pearson"), dict(preprocess="log_cpm", sketch_dim=96)]
    s0 = _stats()
    first = [_fit(Y, X, coords, **kw) for kw in variants]
    s1 = _stats()
    assert (s1 - s0)[2] == 0 and (s1 - s0)[3] == len(variants)       # four X sides of one X: a miss each
    again = [_fit(Y, X, coords, **kw) for kw in variants]
    assert np.array_equal(_stats() - s1, [len(variants), 0, len(variants), 0])
    for kw, a, b in zip(variants, first, again):
        cold = _uncached(monkeypatch, lambda: _fit(Y, X, coords, **kw))
        _same_fit(a, cold)
        _same_fit(b, cold)
    for i in range(len(variants)):
        for j in range(i):
            assert not np.array_equal(again[i].beta_, again[j].beta_)


def test_bordered_xtx_of_70_cell_types_hit_equals_miss(monkeypatch):
    Y, X, coords = _problem(70, n=600, G=300, K=70)
    kw = dict(sketch_dim=128, max_iter=10)
    _trim()
    miss = _fit(Y, X, coords, **kw)
    s1 = _stats()
    hit = _fit(Y, X, coords, **kw)
    assert np.array_equal(_stats() - s1, [1, 0, 1, 0])
    _same_fit(miss, hit)
    _same_fit(hit, _uncached(monkeypatch, lambda: _fit(Y, X, coords, **kw)))


def test_eviction_past_four_entries_and_trim_are_misses_and_correct(monkeypatch):
    Y, X0, coords = _problem(8)
    rs = np.random.RandomState(9)
    Xs = [X0] + [X0 * (1.0 + 0.2 * rs.rand(*X0.shape)) for _ in range(5)]
    _trim()
    first = _fit(Y, Xs[0], coords)
    for X in Xs[1:]:
        _fit(Y, X, coords)
    s0 = _stats()
    back = _fit(Y, Xs[0], coords)                                    # six distinct X, four entries: the first is long gone
    assert np.array_equal(_stats() - s0, [0, 1, 0, 1])
    _same_fit(first, back)
    s0 = _stats()
    _fit(Y, Xs[0], coords)
    assert np.array_equal(_stats() - s0, [1, 0, 1, 0])
    _trim()
    s0 = _stats()
    after = _fit(Y, Xs[0], coords)
    assert np.array_equal(_stats() - s0, [0, 1, 0, 1])
    _same_fit(first, after)
    _same_fit(first, _uncached(monkeypatch, lambda: _fit(Y, Xs[0], coords)))


def test_lattice_fit_that_stops_on_ties_shares_the_x_side_with_its_carry(monkeypatch):
    """knn_ties="auto" on a square lattice: the first native call stops on ties and hands its running sketch -> H stage (which reads
    X_sketch) to the second call as a carry; with a published X side the carry and the cache share it."""
    g = load_golden("lattice.npz")
    coords = g["square_k6_coords"]
    Y, X, _, _ = datagen.count_like(coords.shape[0], 400, 5, 0.1, int(g["square_k6_seed"]))
    kw = dict(preprocess="log_cpm", max_iter=30)
    _trim()
    s0 = _stats()
    a = _fit(Y, X, coords, **kw)
    s1 = _stats()
    assert np.array_equal(s1 - s0, [0, 1, 1, 1])                     # the stopped call publishes, the call with the carry hits
    b = _fit(Y, X, coords, **kw)
    assert np.array_equal(_stats() - s1, [1, 0, 2, 0])
    assert a.info_["knn_ties"] > 0
    cold = _uncached(monkeypatch, lambda: _fit(Y, X, coords, **kw))
    _same_fit(a, cold)
    _same_fit(b, cold)
    _trim()                                                          # (drops the entry the fits above left)


def test_four_threads_fitting_two_signature_matrices_concurrently():
    probs = [_problem(11, n=300, G=200, K=4), _problem(12, n=300, G=200, K=4)]
    kw = dict(sketch_dim=32, max_iter=10)
    want = [_fit(*p, **kw) for p in probs]
    _trim()
    got, errors = [None] * 4, []

    def run(t):
        try:
            for _ in range(3):
                got[t] = _fit(*probs[t % 2], **kw)
        except Exception as e:                                       # noqa: BLE001 (reported by the assertion below)
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=run, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t in range(4):
        _same_fit(got[t], want[t % 2])


def test_leverage_job_keep_x_on_a_hit_hands_out_a_fresh_device_copy():
    from flashdeconv_amd import _lib
    from flashdeconv_amd.utils.genes import LeverageJob, compute_leverage_scores
    rs = np.random.RandomState(13)
    X = rs.gamma(2.0, 3.0, size=(5, 300))
    _trim()
    want = compute_leverage_scores(X)
    s0 = _stats()
    job = LeverageJob(X)
    lev = job.result(keep_x=True)
    assert np.array_equal(_stats() - s0, [1, 0, 0, 0]) and np.array_equal(lev, want)
    assert job.x_dev is not None
    back = np.empty_like(X)
    _lib.check(_lib.load().fdx_memcpy_d2h(back.ctypes.data_as(ctypes.c_void_p), job.x_dev, X.nbytes, None))
    assert np.array_equal(back, X)
    job.release_x()
    assert job.x_dev is None
    assert np.array_equal(compute_leverage_scores(X), want)          # the entry is untouched by the hand-over
