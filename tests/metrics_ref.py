"""Reference, yardstick and inputs for the metrics tests (tests/test_metrics_host.py, tests/test_gpu_metrics_fields.py,
tests/test_gpu_metrics.py).  numpy and scipy only; no GPU, no torch.

Written from the formulas of the reference's ``utils/metrics.py`` (the line numbers are in the header of
``csrc/metrics_kernels.cpp``), per field of the ``(K + 1) x 18`` stats block of ``fdx_metrics_*_dev`` (include/fdx.h FDX_MX_*):

fields(p, t, thr)       (K + 1, 14) float64: SSE, SAE, sum p, sum t, min / max of p and of t ignoring NaN, the NaN flags and
                        n_rare / tp / fp / fn per column; row K is all n K entries.  Sums in np.longdouble where it is wider than
                        float64 (math.fsum per column otherwise), rounded once at the end; counts are Python ints.
                        rare = 0 < t < thr, present = p > thr / 2, tp = present and rare, fp = present and t == 0,
                        fn = not present and rare.
centred(p, t)           (K + 1, 3) float64: sum (p - mp)(t - mt), sum (p - mp)^2, sum (t - mt)^2 about the column means, row K
                        about the overall means; two passes in the same wide arithmetic.
twice_ranks(x, seg)     int64, 2 x the 1-based average rank inside consecutive segments of ``seg`` entries, from
                        scipy.stats.rankdata(method="average"), checked to be integral.  -0.0 ties with +0.0; NaN is refused.
rank_sums(rp, rt, N)    exact Python ints: sum (2 r_p - (N + 1))(2 r_t - (N + 1)) and the two squares.
rho_from_sums(...)      corr_from_sums of the kernels' host side restated in float64: (cpt / den) / sqrt(cpp / den) / sqrt(ctt / den)
                        with den = N - 1, clipped to [-1, 1].
jsd(p, t, eps)          per spot in wide arithmetic, and S = 1/2 sum_c (|a log(a / m)| + |b log(b / m)|) per spot.

The comparators (check_stats, check_rho, check_jsd) hold the bounds that tests/test_gpu_metrics_fields.py derives in its
docstring; test_metrics_host.py shows on the CPU that each of them fails on a reference that is wrong in one place.  Every
comparison prints its largest error as a fraction of its bound (pytest -s shows them).
"""
import functools
import math

import numpy as np

LD = np.longdouble
WIDE = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
U = 2.0 ** -53

# fields of a stats row (include/fdx.h FDX_MX_*)
SSE, SAE, SUM_P, SUM_T, MIN_P, MAX_P, MIN_T, MAX_T, NAN_P, NAN_T, N_RARE, TP, FP, FN, JSD_SUM, C_PT, C_PP, C_TT = range(18)
FIELDS = 18
FIELD_NAMES = ["sse", "sae", "sum_p", "sum_t", "min_p", "max_p", "min_t", "max_t", "nan_p", "nan_t", "n_rare", "tp", "fp", "fn",
               "jsd_sum", "c_pt", "c_pp", "c_tt"]
SPEARMAN_OVERALL, SPEARMAN_PER_TYPE = 1, 2
EXACT_N = 208063            # the largest N with N^3 < 2^53: integer rank sums are exact in float64 in every order up to here
assert EXACT_N ** 3 < 2 ** 53 <= (EXACT_N + 1) ** 3


# ---------------------------------------------------------------------------------------------------- wide sums
def _wide(a):
    a = np.asarray(a, dtype=np.float64)
    return a.astype(LD) if WIDE else a


def _col_sums(A):
    """Sums down the rows of a 2-D array, one per column."""
    if WIDE:
        return np.asarray(A, dtype=LD).sum(axis=0)
    return np.array([math.fsum(c) if not np.isnan(c).any() else np.nan for c in np.asarray(A, dtype=np.float64).T])


def _total(v):
    """Sum of a vector of column sums."""
    if WIDE:
        return np.asarray(v, dtype=LD).sum()
    v = np.asarray(v, dtype=np.float64)
    return np.nan if np.isnan(v).any() else math.fsum(v)


def _row_sums(A):
    return _col_sums(np.asarray(A).T)


# ---------------------------------------------------------------------------------------------------- reference
def fields(p, t, threshold=0.05):
    p = np.asarray(p, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    n, K = p.shape
    P, T = _wide(p), _wide(t)
    out = np.zeros((K + 1, 14))
    with np.errstate(invalid="ignore"):
        d = P - T
        for f, A in ((SSE, d * d), (SAE, np.abs(d)), (SUM_P, P), (SUM_T, T)):
            s = _col_sums(A)
            out[:K, f] = np.asarray(s, dtype=np.float64)
            out[K, f] = np.float64(_total(s))
        for f, A, red in ((MIN_P, p, np.fmin), (MAX_P, p, np.fmax), (MIN_T, t, np.fmin), (MAX_T, t, np.fmax)):
            out[:K, f] = red.reduce(A, axis=0)                       # fmin / fmax: a NaN entry is passed over
            out[K, f] = red.reduce(A, axis=None)
        for f, A in ((NAN_P, p), (NAN_T, t)):
            out[:K, f] = np.isnan(A).any(axis=0)
            out[K, f] = np.isnan(A).any()
        half = threshold / 2
        rare = (t > 0) & (t < threshold)
        present = p > half
        for f, M in ((N_RARE, rare), (TP, present & rare), (FP, present & (t == 0)), (FN, ~present & rare)):
            counts = [int(np.count_nonzero(M[:, c])) for c in range(K)]
            out[:K, f] = counts
            out[K, f] = sum(counts)
    return out


def centred(p, t):
    p = np.asarray(p, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    n, K = p.shape
    P, T = _wide(p), _wide(t)
    out = np.zeros((K + 1, 3))
    with np.errstate(invalid="ignore"):
        sp, st = _col_sums(P), _col_sums(T)
        dp, dt = P - sp / n, T - st / n
        ep, et = P - _total(sp) / (n * K), T - _total(st) / (n * K)
        for f, (A, B) in enumerate(((dp, dt), (dp, dp), (dt, dt))):
            out[:K, f] = np.asarray(_col_sums(A * B), dtype=np.float64)
        for f, (A, B) in enumerate(((ep, et), (ep, ep), (et, et))):
            out[K, f] = np.float64(_total(_col_sums(A * B)))
    return out


def twice_ranks(x, seg):
    from scipy.stats import rankdata
    x = np.asarray(x).ravel()
    assert x.size % seg == 0, "whole segments only"
    assert not np.isnan(x).any(), "NaN has no rank here"
    r2 = 2.0 * rankdata(x.reshape(-1, seg), method="average", axis=1)
    out = np.rint(r2).astype(np.int64)
    assert np.array_equal(out, r2), "twice an average rank is an integer"
    return out.ravel()


def rank_sums(rp, rt, N):
    """(cpt, cpp, ctt) of twice-ranks about their exact mean N + 1, as Python ints (int64 chunks that cannot overflow)."""
    a = np.asarray(rp, dtype=np.int64) - (N + 1)
    b = np.asarray(rt, dtype=np.int64) - (N + 1)
    assert a.shape == b.shape == (N,)
    step = max(1, (2 ** 62) // (N * N))
    out = [0, 0, 0]
    for lo in range(0, N, step):
        x, y = a[lo:lo + step], b[lo:lo + step]
        out[0] += int(np.dot(x, y))
        out[1] += int(np.dot(x, x))
        out[2] += int(np.dot(y, y))
    return tuple(out)


def rho_from_sums(cpt, cpp, ctt, N):
    den = np.float64(N) - np.float64(1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = (np.float64(cpt) / den) / np.sqrt(np.float64(cpp) / den) / np.sqrt(np.float64(ctt) / den)
    return np.float64(min(max(r, -1.0), 1.0)) if not np.isnan(r) else np.float64(np.nan)


def column_twice_ranks(x):
    """(n, K) twice-ranks of every column among its own n values."""
    x = np.asarray(x)
    n, K = x.shape
    return np.ascontiguousarray(twice_ranks(np.ascontiguousarray(x.T).ravel(), n).reshape(K, n).T)


def rho_from_ranks(rcol_p, rcol_t, rall_p, rall_t, flags):
    """(K + 1) rho as the C entries return it: column k where flags has PER_TYPE, row K where it has OVERALL, NaN elsewhere;
    raw, a constant column gives 0 / 0 = NaN."""
    n, K = rcol_p.shape if rcol_p is not None else rall_p.shape
    rho = np.full(K + 1, np.nan)
    if flags & SPEARMAN_PER_TYPE:
        for k in range(K):
            rho[k] = rho_from_sums(*rank_sums(rcol_p[:, k], rcol_t[:, k], n), n)
    if flags & SPEARMAN_OVERALL:
        rho[K] = rho_from_sums(*rank_sums(rall_p.ravel(), rall_t.ravel(), n * K), n * K)
    return rho


def spearman_raw(p, t, flags=3):
    p, t = np.asarray(p), np.asarray(t)
    n, K = p.shape
    per, ov = flags & SPEARMAN_PER_TYPE, flags & SPEARMAN_OVERALL
    return rho_from_ranks(column_twice_ranks(p) if per else None, column_twice_ranks(t) if per else None,
                          twice_ranks(p.ravel(), n * K).reshape(n, K) if ov else None,
                          twice_ranks(t.ravel(), n * K).reshape(n, K) if ov else None, flags)


def jsd(p, t, eps=1e-10):
    """(jsd, S) per spot, float64 rounded once from the wide values."""
    lo, hi = np.float64(eps), np.float64(1.0) - np.float64(eps)
    a = np.clip(_wide(p), lo, hi)
    b = np.clip(_wide(t), lo, hi)
    a = a / _row_sums(a)[:, None]
    b = b / _row_sums(b)[:, None]
    m = (a + b) / 2
    x, y = a * np.log(a / m), b * np.log(b / m)
    j = (_row_sums(x) + _row_sums(y)) / 2
    S = (_row_sums(np.abs(x)) + _row_sums(np.abs(y))) / 2
    return np.asarray(j, dtype=np.float64), np.asarray(S, dtype=np.float64)


def rankdata_spearman(a, b):
    """Spearman's rho the plain way: Pearson of scipy's average ranks."""
    from scipy.stats import rankdata
    return np.corrcoef(rankdata(a), rankdata(b))[0, 1]


# ---------------------------------------------------------------------------------------------------- the public results
def safe(row, value):
    """_safe_corr (metrics.py:98-103) on a fields row: 0.0 when either ptp is 0, NaN when an entry is NaN."""
    if row[NAN_P] or row[NAN_T]:
        return np.nan                              # ptp is NaN: not 0, and the correlation of a NaN is NaN
    if row[MAX_P] - row[MIN_P] == 0 or row[MAX_T] - row[MIN_T] == 0:
        return 0.0
    return value


def pearson_from_centred(c, N):
    return rho_from_sums(c[0], c[1], c[2], N)


def results(p, t):
    """What the reference's functions return for (p, t), built from the pieces above: a dict keyed as golden/metrics.npz is."""
    p = np.asarray(p, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    n, K = p.shape
    N = n * K
    F, C = fields(p, t), centred(p, t)
    out = {"rmse": np.sqrt(F[K, SSE] / N), "rmse_per": np.sqrt(F[:K, SSE] / n), "mae": F[K, SAE] / N, "mae_per": F[:K, SAE] / n}
    out["pearson_per"] = np.array([safe(F[k], pearson_from_centred(C[k], n)) for k in range(K)])
    out["pearson"] = safe(F[K], pearson_from_centred(C[K], N))
    clean = [not (F[k, NAN_P] or F[k, NAN_T]) for k in range(K + 1)]
    out["spearman_per"] = np.array([safe(F[k], rho_from_sums(*rank_sums(twice_ranks(p[:, k], n), twice_ranks(t[:, k], n), n), n)
                                         if clean[k] else np.nan) for k in range(K)])
    out["spearman"] = safe(F[K], rho_from_sums(*rank_sums(twice_ranks(p.ravel(), N), twice_ranks(t.ravel(), N), N), N)
                           if clean[K] else np.nan)
    out["jsd"], out["jsd_e3"] = jsd(p, t, 1e-10)[0], jsd(p, t, 1e-3)[0]
    for key, thr in (("rare_t05", 0.05), ("rare_t20", 0.2)):
        n_rare, tp, fp, fn = (int(v) for v in fields(p, t, thr)[K, N_RARE:FN + 1])
        if n_rare == 0:
            out[key] = np.full(3, np.nan)
        else:
            prec, rec = tp / (tp + fp + 1e-10), tp / (tp + fn + 1e-10)
            out[key] = np.array([prec, rec, 2 * prec * rec / (prec + rec + 1e-10)])
    out["mean_proportion_true"], out["mean_proportion_pred"] = F[:K, SUM_T] / n, F[:K, SUM_P] / n
    return out


# ---------------------------------------------------------------------------------------------------- inputs
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def pair(n, K, dtype="float64", seed=0):
    """Seeded (pred, true): proportion-like, non-negative, about 60 % exact zeros, the rest quantised to 3 decimals (ties
    everywhere); pred's column 1 is constant where K >= 3.  Read-only."""
    rng = np.random.default_rng(1000003 * K + 7 * n + seed)
    t = np.round(rng.beta(0.6, 4.0, size=(n, K)), 3) * (rng.random((n, K)) < 0.4)
    p = np.round(np.clip(t + rng.normal(0, 0.03, size=(n, K)), 0, None), 3)
    p = p * np.where(t > 0, rng.random((n, K)) < 0.8, rng.random((n, K)) < 0.3)
    if K >= 3:
        p[:, 1] = 0.125
    return _frozen(np.ascontiguousarray(p.astype(dtype)), np.ascontiguousarray(t.astype(dtype)))


@functools.lru_cache(maxsize=None)
def jsd_pair(n, K, dtype="float64"):
    """pair() with all-zero rows: pred's first, true's last and, where there is room, row 1 of both."""
    p, t = (a.copy() for a in pair(n, K, dtype, seed=1))
    p[0] = 0
    t[n - 1] = 0
    if n >= 4:
        p[1] = 0
        t[1] = 0
    return _frozen(p, t)


@functools.lru_cache(maxsize=None)
def tie_pair(dtype="float64"):
    """(64, 4) with the tie structure the rank kernels' segment arithmetic has to get right, in pred and (shifted by one column)
    in true: column 0 all distinct; column 1 is 95 % zeros and its maximum 0.5 (four times) is also column 2's minimum (five
    times), so that in the column-ordered keys a run ends segment 1 and an equal-valued run starts segment 2; column 2's maximum
    0.75 (three times) is column 3's minimum (twice); column 3 of pred mixes -0.0 and +0.0 below that.  true's column 0 is
    constant."""
    rng = np.random.default_rng(64004)
    n = 64
    p = np.zeros((n, 4))
    p[:, 0] = rng.permutation(n) / 128.0 + 0.0078125
    p[rng.permutation(n)[:4], 1] = 0.5                                     # 60 of 64 zeros: 94 %, the nearest to 95 % n = 64 has
    c2 = np.concatenate([np.full(5, 0.5), np.full(3, 0.75), 0.5 + np.round(rng.random(n - 8) * 0.2, 2) + 0.01])
    p[:, 2] = rng.permutation(c2)
    c3 = np.concatenate([np.full(2, 0.75), np.full(2, 1.0), 0.75 + np.round(rng.random(n - 4) * 0.2, 2) + 0.01])
    p[:, 3] = rng.permutation(c3)
    t = np.roll(p, 1, axis=1)[rng.permutation(n)]
    t[:, 0] = 0.25                                                         # the constant column
    z = p.copy()
    z[:, 3] = np.where(rng.random(n) < 0.5, -0.0, 0.0) * 1.0
    z[rng.permutation(n)[:20], 3] = np.round(rng.random(20), 1)
    assert p[:, 1].max() == p[:, 2].min() == 0.5 and p[:, 2].max() == p[:, 3].min() == 0.75
    assert np.signbit(z[:, 3]).any() and (~np.signbit(z[:, 3]) & (z[:, 3] == 0)).any()
    return _frozen(np.ascontiguousarray(p.astype(dtype)), np.ascontiguousarray(t.astype(dtype)),
                   np.ascontiguousarray(z.astype(dtype)))


# ---------------------------------------------------------------------------------------------------- comparators
def note(what, name, err, bound):
    err, bound = np.atleast_1d(np.asarray(err, dtype=np.float64)), np.atleast_1d(np.asarray(bound, dtype=np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    print(f"[metrics] {what}: {name} error at most {float(np.max(frac, initial=0.0)):.3g} of its bound")


def reference(p, t, threshold=0.05):
    """Everything check_stats needs of a pair, computed once: pass it on unchanged."""
    p64, t64 = np.asarray(p, dtype=np.float64), np.asarray(t, dtype=np.float64)
    n, K = p64.shape
    with np.errstate(invalid="ignore"):
        mabs = np.stack([np.concatenate([np.abs(a).mean(axis=0), [np.abs(a).mean()]]) for a in (p64, t64)])
    return dict(n=n, K=K, fields=fields(p64, t64, threshold), centred=centred(p64, t64), mabs=mabs)


def block_of(ref, jsd_sum=0.0):
    """The (K + 1, 18) stats block a faultless device would return for the reference."""
    K = ref["K"]
    b = np.zeros((K + 1, FIELDS))
    b[:, :14] = ref["fields"]
    b[K, JSD_SUM] = jsd_sum
    b[:, C_PT:] = ref["centred"]
    return b


def _within(what, name, got, want, bound):
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: {name} is NaN in other rows than the reference's"
    ok = ~np.isnan(want)
    err = np.abs(got - want)[ok]
    note(what, name, err, bound[ok])
    bad = err > bound[ok]
    assert not bad.any(), (f"{what}: {name} off by {err[bad].max():.3g} where the bound is {bound[ok][bad].max():.3g} "
                           f"(row {np.flatnonzero(ok)[np.argmax(bad)]})")


def check_stats(stats, ref, what="", jsd_sum_checked=False):
    """All 18 fields of every row of a device stats block against reference(): counts, flags, min and max exact, sums and centred
    sums within the derived bounds.  Row K's JSD sum is check_jsd's; it must be 0 here unless jsd_sum_checked."""
    n, K = ref["n"], ref["K"]
    F, C = ref["fields"], ref["centred"]
    stats = np.asarray(stats, dtype=np.float64)
    assert stats.shape == (K + 1, FIELDS)
    cnt = np.concatenate([np.full(K, float(n)), [float(n) * K]])
    for f in (N_RARE, TP, FP, FN, NAN_P, NAN_T):
        bad = np.flatnonzero(stats[:, f] != F[:, f])
        assert bad.size == 0, f"{what}: {FIELD_NAMES[f]} of row {bad[0]} is {stats[bad[0], f]}, the reference has {F[bad[0], f]}"
    for f in (MIN_P, MAX_P, MIN_T, MAX_T):
        bad = np.flatnonzero(~(stats[:, f] == F[:, f]))                    # by value: -0.0 == 0.0
        assert bad.size == 0, f"{what}: {FIELD_NAMES[f]} of row {bad[0]} is {stats[bad[0], f]!r}, the reference has {F[bad[0], f]!r}"
    note(what, "counts, NaN flags, min and max (exact)", 0.0, 1.0)
    for f in (SSE, SAE, SUM_P, SUM_T):
        _within(what, FIELD_NAMES[f], stats[:, f], F[:, f], (cnt + 4) * U * np.abs(F[:, f]))
    assert np.all(stats[:K, JSD_SUM] == 0), f"{what}: a column row carries a JSD sum"
    if not jsd_sum_checked:
        assert stats[K, JSD_SUM] == 0, f"{what}: a JSD sum without a JSD"
    dp, dt = (cnt + 1) * U * ref["mabs"][0], (cnt + 1) * U * ref["mabs"][1]
    with np.errstate(invalid="ignore"):
        _within(what, "c_pp", stats[:, C_PP], C[:, 1], (cnt + 4) * U * C[:, 1] + cnt * dp * dp)
        _within(what, "c_tt", stats[:, C_TT], C[:, 2], (cnt + 4) * U * C[:, 2] + cnt * dt * dt)
        _within(what, "c_pt", stats[:, C_PT], C[:, 0], (cnt + 4) * U * np.sqrt(C[:, 1] * C[:, 2]) + cnt * dp * dt)


def check_rho(rho, want, what="", atol_rows=()):
    """Bit for bit (a NaN matches a NaN) in every row but ``atol_rows``, where |rho - want| <= 1e-12."""
    rho, want = np.asarray(rho, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert rho.shape == want.shape
    assert np.array_equal(np.isnan(rho), np.isnan(want)), f"{what}: rho is NaN in other rows than the reference's: {rho} / {want}"
    ok = ~np.isnan(want)
    loose = np.zeros(len(want), dtype=bool)
    loose[list(atol_rows)] = True
    err = np.abs(rho - want)
    note(what, "rho (bit for bit: any difference is beyond the bound)", err[ok & ~loose], np.zeros(int((ok & ~loose).sum())))
    bad = np.flatnonzero(ok & ~loose & (rho.view(np.uint64) != want.view(np.uint64)) & ~((rho == 0) & (want == 0)))
    assert bad.size == 0, f"{what}: rho of row {bad[0]} is {rho[bad[0]]!r}, the exact rank sums give {want[bad[0]]!r}"
    if loose.any():
        note(what, "rho beyond exact sums", err[ok & loose], np.full(int((ok & loose).sum()), 1e-12))
        assert np.all(err[ok & loose] <= 1e-12), f"{what}: rho off by {err[ok & loose].max():.3g}"


def jsd_bound(S, K):
    return (K + 8) * U * (np.asarray(S, dtype=np.float64) + 1.0)


def check_jsd(got, got_sum, ref_j, ref_S, K, what=""):
    """Every spot within (K + 8) u (S + 1); the sum within the sum of those plus (n + 1) u sum |jsd|."""
    got = np.asarray(got, dtype=np.float64)
    n = len(ref_j)
    assert got.shape == (n,)
    assert not np.isnan(got).any(), f"{what}: a NaN JSD (spot {np.flatnonzero(np.isnan(got))[:1]})"
    b = jsd_bound(ref_S, K)
    err = np.abs(got - ref_j)
    note(what, "jsd per spot", err, b)
    bad = np.flatnonzero(err > b)
    assert bad.size == 0, f"{what}: jsd of spot {bad[0]} is {got[bad[0]]!r}, the reference has {ref_j[bad[0]]!r} (bound {b[bad[0]]:.3g})"
    if got_sum is not None:
        want = float(_total(_wide(ref_j)))
        bs = float(b.sum() + (n + 1) * U * np.abs(ref_j).sum())
        note(what, "jsd sum", abs(got_sum - want), bs)
        assert abs(got_sum - want) <= bs, f"{what}: jsd sum {got_sum!r}, the reference has {want!r}"
