"""-m gpu tests of the spatial niches (csrc/niche_kernels.cpp, fdx_kmeans_assign_dev / fdx_label_sums_dev / fdx_kmeans_seed_dist_dev /
fdx_kmeans_dev, utils.niches, FlashDeconv.get_spatial_niches, tl.deconvolve(n_niches=...)).

Reference, in NumPy float64: d = ((F[:, None, :] - M[None]) ** 2).sum(-1), argmin (the smallest index on ties), and Lloyd's loop
    labels = -1;  for it = 1 .. max_iter:  assign;  changed == 0: converged, stop;  it == max_iter: stop;
                                           centres[c] = sum of its members / their count where the count is positive.

Label parity is EXACT and nobody is left out.  In every iteration the reference computes each spot's margin, the second-best minus
the best d2; a spot whose margin is <= 1e-9 (best + second) could be left out of the comparison, the cap on such spots is zero and
every case asserts that the reference leaves out none (the rounding of a d2 is bounded by 8 (D + 2) u (best + second), seven
orders of magnitude below that margin, so the device cannot pick another centre).  Then, with u = 2^-53:
    labels, counts, n_iter, converged     equal to the reference
    centers    |centers - ref| <= 4 (count_c + 2) u max|F_.k|   elementwise (a mean of count_c values, summed in any order, on both
               sides); an empty niche's centre is bit-equal to its initial row
    inertia    |inertia - ref| <= 4 (n + D + 2) u ref           (n sums of D products, in any order, on both sides)
    min_d2     |min_d2 - ref|  <= 4 (D + 2) u d2
    label sums |sums - ref|    <= 4 (count_c + 2) u max|F_.k|,  counts exact

Paths of the launcher crossed by the shapes: 256-row workgroups and their 64-row slices (n = 1, 2, 64, 65, 130, 256, 257, 300, 1000,
2000), the distance kernel's 32-column chunks (D = 32 | 33, 64 | 65, 100, 272, 544), its 8 / 16 accumulators and further walks of the
columns (C = 8 | 9, 16 | 17, 32 | 33, 64), the label sums' second column block (D = 272 > 256), its LDS above 64 KB (C > 32) and
more than one of its row blocks (n > 1024), the seed distance's blocks of 256 rows (n = 140: one, n = 700: three).
"""
import ctypes
import functools

import numpy as np
import pytest

import datagen

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
MARGIN = 1e-9

# (n, K, C, seed): the issue's nine, then slice tails with one centre and C = n, column-chunk edges, centre-walk edges
CASES = [(130, 5, 4, 1), (257, 30, 12, 2), (300, 8, 7, 3), (1000, 30, 12, 4), (130, 1, 3, 5), (300, 64, 33, 6), (300, 65, 64, 7),
         (200, 100, 5, 8), (2000, 30, 12, 9),
         (1, 3, 1, 11), (2, 3, 1, 12), (2, 3, 2, 13), (64, 3, 1, 14), (65, 3, 1, 15), (256, 4, 3, 16),
         (130, 32, 5, 17), (130, 33, 5, 18), (70, 272, 3, 19), (70, 544, 3, 20),
         (130, 5, 1, 21), (200, 8, 32, 22), (200, 6, 8, 23), (200, 6, 9, 24), (200, 6, 16, 25), (200, 6, 17, 26)]


# ---------------------------------------------------------------- reference
def _data(n, K, seed):
    rs = np.random.RandomState(seed)
    return rs.dirichlet(np.full(K, 0.3), n) if K > 1 else rs.rand(n, 1)


def _init(F, C, seed):
    return F[np.random.RandomState(100 + seed).choice(F.shape[0], C, replace=False)].copy()


def _d2(F, M):
    return ((F[:, None, :] - M[None]) ** 2).sum(-1)


def _assign(F, M):
    """(labels, best d2, spots whose margin is within MARGIN (best + second): the ones that may be left out)."""
    d = _d2(F, M)
    labels = d.argmin(1)
    best = d[np.arange(F.shape[0]), labels]
    if M.shape[0] == 1:
        return labels, best, 0
    second = np.partition(d, 1, axis=1)[:, 1]
    return labels, best, int(np.count_nonzero(second - best <= MARGIN * (best + second)))


def _label_sums(F, labels, C):
    sums = np.zeros((C, F.shape[1]))
    ok = (labels >= 0) & (labels < C)
    np.add.at(sums, labels[ok], F[ok])
    return sums, np.bincount(labels[ok], minlength=C).astype(np.int64)


def _lloyd(F, init, max_iter=100):
    centres = np.array(init, dtype=np.float64)
    C = centres.shape[0]
    labels = np.full(F.shape[0], -1)
    left_out, it, converged = 0, 0, False
    while True:
        it += 1
        new, best, tight = _assign(F, centres)
        left_out += tight
        changed = int(np.count_nonzero(new != labels))
        labels, inertia = new, float(best.sum())
        if changed == 0:
            converged = True
            break
        if it == max_iter:
            break
        sums, counts = _label_sums(F, labels, C)
        centres = np.where(counts[:, None] > 0, sums / np.maximum(counts, 1)[:, None], centres)
    return {"labels": labels.astype(np.int32), "centers": centres, "counts": _label_sums(F, labels, C)[1], "inertia": inertia,
            "n_iter": it, "converged": converged, "left_out": left_out}


@functools.lru_cache(maxsize=None)
def _case(n, K, C, seed, max_iter=100):
    F = _data(n, K, seed)
    init = _init(F, C, seed)
    for a in (F, init):
        a.setflags(write=False)
    return F, init, _lloyd(F, init, max_iter)


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _check_result(got, ref, F, label=""):
    n, D = F.shape
    assert ref["left_out"] == 0, (label, "the reference would leave spots out: change the seed", ref["left_out"])
    labels = _host(got["labels"])
    assert labels.dtype == np.int32 and labels.shape == (n,)
    cerr = np.abs(got["centers"] - ref["centers"])
    ctol = 4 * (ref["counts"][:, None] + 2) * U * np.abs(F).max(0)[None, :]
    ierr, itol = abs(got["inertia"] - ref["inertia"]), 4 * (n + D + 2) * U * ref["inertia"]
    print(f"{label} n_iter {got['n_iter']} (ref {ref['n_iter']}), labels differing {int(np.count_nonzero(labels != ref['labels']))}, "
          f"centres worst err / bound {float((cerr / ctol).max()):.3e}, inertia err {ierr:.3e} bound {itol:.3e}")
    assert np.array_equal(labels, ref["labels"]), label
    assert got["counts"].dtype == np.int64 and np.array_equal(got["counts"], ref["counts"]), label
    assert got["n_iter"] == ref["n_iter"] and got["converged"] is ref["converged"], label
    assert got["centers"].shape == ref["centers"].shape and np.all(cerr <= ctol), label
    assert ierr <= itol, label


# ---------------------------------------------------------------- 1. label parity
@pytest.mark.parametrize("n,K,C,seed", CASES)
def test_label_parity(n, K, C, seed):
    from flashdeconv_amd.utils.niches import kmeans
    F, init, ref = _case(n, K, C, seed)
    assert ref["converged"]
    got = kmeans(F, init)
    assert set(got) == {"labels", "centers", "counts", "inertia", "n_iter", "converged"} and isinstance(got["labels"], np.ndarray)
    _check_result(got, ref, F, f"n={n} K={K} C={C}")
    # on convergence the centres are the means of their members and the labels their arg-min
    sums, counts = _label_sums(F, ref["labels"], C)
    assert np.all(np.abs(got["centers"] * counts[:, None] - sums)[counts > 0] <=
                  (4 * (counts[:, None] + 2) * U * np.abs(F).max(0)[None, :] * counts[:, None])[counts > 0])


@pytest.mark.parametrize("max_iter", [1, 2])
def test_max_iter_reached(max_iter):
    from flashdeconv_amd.utils.niches import kmeans
    n, K, C, seed = 2000, 30, 12, 9
    F, init, ref = _case(n, K, C, seed, max_iter)
    assert not ref["converged"] and ref["n_iter"] == max_iter
    got = kmeans(F, init, max_iter=max_iter)
    _check_result(got, ref, F, f"max_iter={max_iter}")
    assert got["converged"] is False and got["n_iter"] == max_iter
    labels, _, tight = _assign(F, got["centers"])              # the labels returned are the arg-min of the centres returned
    assert tight == 0 and np.array_equal(got["labels"], labels)


# ---------------------------------------------------------------- 2. stage entries
def _dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device="cuda:0")


def _padded(F, ldf):
    wide = np.full((F.shape[0], ldf), np.nan)
    wide[:, :F.shape[1]] = F
    return wide


def _assign_dev(Fd, ldf, n, D, Md, C, labels_d, min_d2_d=None):
    from flashdeconv_amd import _lib
    changed, inertia = np.zeros(1, dtype=np.int64), np.zeros(1)
    _lib.check(_lib.load().fdx_kmeans_assign_dev(
        ctypes.c_void_p(Fd.data_ptr()), ldf, n, D, ctypes.c_void_p(Md.data_ptr()), C, ctypes.c_void_p(labels_d.data_ptr()),
        ctypes.c_void_p(min_d2_d.data_ptr()) if min_d2_d is not None else None, _lib.ptr_i64(changed), _lib.ptr_f64(inertia), None))
    return int(changed[0]), float(inertia[0])


@pytest.mark.parametrize("n,D,C,ldf", [(300, 7, 5, 11), (700, 40, 20, 41)])
def test_assign_entry(n, D, C, ldf):
    import torch
    rs = np.random.RandomState(n)
    F = _data(n, D, 30 + n)
    M = F[rs.choice(n, C, replace=False)] * 0.5 + 0.5 / D
    want, best, tight = _assign(F, M)
    assert tight == 0
    prefill = rs.randint(-1, C, n).astype(np.int32)
    Fd, Md = _dev(_padded(F, ldf)), _dev(M)
    labels_d, min_d = _dev(prefill), torch.full((n,), np.nan, dtype=torch.float64, device="cuda:0")
    changed, inertia = _assign_dev(Fd, ldf, n, D, Md, C, labels_d, min_d)
    assert np.array_equal(labels_d.cpu().numpy(), want)
    assert changed == int(np.count_nonzero(prefill != want)) and 0 < changed < n
    err = np.abs(min_d.cpu().numpy() - best)
    print(f"min_d2 worst err / bound {float((err / (4 * (D + 2) * U * best)).max()):.3e}")
    assert np.all(err <= 4 * (D + 2) * U * best)
    assert abs(inertia - best.sum()) <= 4 * (n + D + 2) * U * best.sum()
    # a second pass over its own labels changes nothing, without min_d2
    assert _assign_dev(Fd, ldf, n, D, Md, C, labels_d) == (0, inertia)
    # d2 depends on the row alone: shuffled rows give exactly the shuffled labels and distances
    sh = rs.permutation(n)
    lab2, min2 = _dev(np.full(n, -1, dtype=np.int32)), torch.empty(n, dtype=torch.float64, device="cuda:0")
    changed2, _ = _assign_dev(_dev(_padded(F[sh], ldf)), ldf, n, D, Md, C, lab2, min2)
    assert changed2 == n and np.array_equal(lab2.cpu().numpy(), want[sh])
    assert np.array_equal(min2.cpu().numpy(), min_d.cpu().numpy()[sh])


@pytest.mark.parametrize("n,D,C", [(1, 3, 2), (300, 7, 12), (300, 1, 1), (130, 272, 3), (2500, 30, 12), (1100, 5, 64), (300, 6, 33)])
def test_label_sums_entry(n, D, C):
    from flashdeconv_amd import _lib
    rs = np.random.RandomState(n + D + C)
    ldf = D + 3
    F = _data(n, D, 40 + n) - (0.5 if D == 7 else 0.0)          # (signed values once)
    labels = rs.randint(0, C, n).astype(np.int32)
    never = C - 2 if C > 2 else None
    if never is not None:
        labels[labels == never] = C - 1                         # a label that never occurs
    if n > 10:
        labels[rs.choice(n, 5, replace=False)] = [-1, -7, C, C + 1, 2 ** 30]     # outside 0 .. C - 1: skipped
    want, counts = _label_sums(F, labels.astype(np.int64), C)
    sums, got_counts = np.full((C, D), np.nan), np.full(C, -1, dtype=np.int64)
    Fd, ld = _dev(_padded(F, ldf)), _dev(labels)
    _lib.check(_lib.load().fdx_label_sums_dev(ctypes.c_void_p(Fd.data_ptr()), ldf, n, D, ctypes.c_void_p(ld.data_ptr()), C,
                                              _lib.ptr_f64(sums), _lib.ptr_i64(got_counts), None))
    assert np.array_equal(got_counts, counts)
    tol = 4 * (counts[:, None] + 2) * U * np.abs(F).max(0)[None, :]
    print(f"label sums worst err / bound {float((np.abs(sums - want) / tol).max()):.3e}")
    assert np.all(np.abs(sums - want) <= tol)
    if never is not None:
        assert counts[never] == 0 and got_counts[never] == 0 and np.all(sums[never] == 0.0)


def test_seed_distance_entry():
    import torch
    from flashdeconv_amd import _lib
    lib = _lib.load()
    n, D, ldf = 700, 5, 8
    F = _data(n, D, 50)
    Fd = _dev(_padded(F, ldf))
    d2 = torch.full((n,), float("inf"), dtype=torch.float64, device="cuda:0")
    sums = np.full(1024, np.nan)
    R, nb = ctypes.c_int64(0), ctypes.c_int32(0)
    want = np.full(n, np.inf)
    for row in (17, 600, 17):
        _lib.check(lib.fdx_kmeans_seed_dist_dev(ctypes.c_void_p(Fd.data_ptr()), ldf, n, D, ctypes.c_void_p(Fd.data_ptr() + row * ldf * 8),
                                                ctypes.c_void_p(d2.data_ptr()), _lib.ptr_f64(sums), ctypes.byref(R), ctypes.byref(nb),
                                                None))
        new = _d2(F, F[row:row + 1])[:, 0]
        want = np.minimum(want, new)
        got = d2.cpu().numpy()
        assert np.all(np.abs(got - want) <= 4 * (D + 2) * U * want) and got[row] == 0.0
        assert R.value == 256 and nb.value == 3
        for b in range(3):
            blk = got[b * 256:(b + 1) * 256]
            assert abs(sums[b] - blk.sum()) <= 4 * (256 + 2) * U * blk.sum()
    assert got[17] == 0.0 and got[600] == 0.0


def test_refusals():
    import torch
    from flashdeconv_amd import _lib
    lib = _lib.load()
    n, D, C = 10, 3, 2
    Fd = _dev(_data(n, D, 60))
    Md = _dev(_data(C, D, 61))
    lab = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    d2 = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    i64, f64, i32a, i32b = np.zeros(64, dtype=np.int64), np.zeros(1024), ctypes.c_int32(0), ctypes.c_int32(0)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None     # noqa: E731

    def assign(F=Fd, ldf=D, n=n, D=D, M=Md, C=C, L=lab, ch=_lib.ptr_i64(i64), ine=_lib.ptr_f64(f64)):
        return lib.fdx_kmeans_assign_dev(p(F), ldf, n, D, p(M), C, p(L), None, ch, ine, None)

    def sums(F=Fd, ldf=D, n=n, D=D, L=lab, C=C, so=_lib.ptr_f64(f64), co=_lib.ptr_i64(i64)):
        return lib.fdx_label_sums_dev(p(F), ldf, n, D, p(L), C, so, co, None)

    def seed(F=Fd, ldf=D, n=n, D=D, M=Md, d=d2, so=_lib.ptr_f64(f64), ro=ctypes.byref(ctypes.c_int64(0)), no=ctypes.byref(i32a)):
        return lib.fdx_kmeans_seed_dist_dev(p(F), ldf, n, D, p(M), p(d), so, ro, no, None)

    def lloyd(F=Fd, ldf=D, n=n, D=D, C=C, mi=5, M=Md, L=lab, co=_lib.ptr_i64(i64), ine=_lib.ptr_f64(f64), ni=ctypes.byref(i32a),
              cv=ctypes.byref(i32b)):
        return lib.fdx_kmeans_dev(p(F), ldf, n, D, C, mi, p(M), p(L), co, ine, ni, cv, None)

    for fn in (assign, sums, seed, lloyd):
        _lib.check(fn())                                        # the good call passes
    shape = [(dict(D=0, ldf=0), "D must be positive"), (dict(ldf=D - 1), "ldf must be at least D"),
             (dict(n=2 ** 31 - 128), "too many rows")]
    centres = [(dict(C=0), "C must be between 1 and 64"), (dict(C=65, n=100), "C must be between 1 and 64")]
    cases = {
        assign: shape + centres + [(dict(C=n + 1), "C must not exceed n")] +
        [({k: None}, "null argument") for k in ("F", "M", "L", "ch", "ine")],
        sums: shape + centres + [({k: None}, "null argument") for k in ("F", "L", "so", "co")],
        seed: shape + [(dict(n=0), "C must not exceed n")] +
        [({k: None}, "null argument") for k in ("F", "M", "d", "so", "ro", "no")],
        lloyd: shape + centres + [(dict(C=n + 1), "C must not exceed n"), (dict(mi=0), "max_iter must be positive")] +
        [({k: None}, "null argument") for k in ("F", "M", "L", "co", "ine", "ni", "cv")],
    }
    names = {assign: "fdx_kmeans_assign_dev", sums: "fdx_label_sums_dev", seed: "fdx_kmeans_seed_dist_dev", lloyd: "fdx_kmeans_dev"}
    for fn, bads in cases.items():
        for bad, msg in bads:
            with pytest.raises(_lib.FdxError, match=names[fn] + ": " + msg):
                _lib.check(fn(**bad))


# ---------------------------------------------------------------- 3. rules
def test_identical_initial_centres():
    """Centres 1 and 3 start identical: every tie goes to the lower index, so niche 3 wins nothing, keeps its centre bit for bit and
    has no composition.  After one pass that holds for any twins (here a row of F).  Over a whole run an empty niche's stale centre
    can win spots back once its twin has moved to the mean of what both won, so the run to convergence starts the twins at
    1.5 e_3, outside the simplex the rows lie in: every row is nearer to the mean of the rows the twins won than to that point."""
    from flashdeconv_amd.utils.niches import spatial_niches
    n, K, C = 300, 5, 4
    F = _data(n, K, 70)
    outside = np.zeros(K)
    outside[3] = 1.5
    for twin, max_iter in ((_init(F, C, 70)[1], 1), (outside, 100)):
        init = _init(F, C, 70)
        init[1] = init[3] = twin
        ref = _lloyd(F, init, max_iter)
        # the margin of the reference is 0 between the twins by construction: it is measured with the upper twin taken out
        assert _lloyd(F, init[:3], max_iter)["left_out"] == 0
        assert ref["counts"][3] == 0 and ref["counts"][1] > 0 and np.array_equal(ref["centers"][3], twin)
        assert ref["converged"] == (max_iter > 1)
        ref["left_out"] = 0
        got = spatial_niches(F, C, init=init, max_iter=max_iter)
        _check_result(got, ref, F, f"twins, max_iter={max_iter}")
        assert got["counts"][3] == 0 and got["counts"][1] > 0 and not np.any(_host(got["labels"]) == 3)
        assert np.array_equal(got["centers"][3], twin)
        assert np.isnan(got["composition"][3]).all() and np.isfinite(got["composition"][:3]).all()


# ---------------------------------------------------------------- 4. seeding
@pytest.mark.parametrize("m", [20, 100])
def test_kmeans_plusplus_draws_every_distinct_row_once(m):
    from flashdeconv_amd.utils.niches import kmeans_plusplus
    C, K = 7, 6
    rows = _data(C, K, 80)
    rs = np.random.RandomState(m)
    F = np.repeat(rows, m, axis=0)[rs.permutation(C * m)]
    orders = []
    for seed in (0, 0, 1, 2):
        got = kmeans_plusplus(F, C, random_state=seed)
        assert got.shape == (C, K) and got.dtype == np.float64
        which = [int(np.flatnonzero((rows == g).all(1))[0]) for g in got]          # bit-equal to a row of F, or IndexError
        assert sorted(which) == list(range(C)), (seed, which)
        orders.append(which)
    assert orders[0] == orders[1]
    # fewer centres than distinct rows: still distinct ones; float32 input: the float32 rows, widened
    got = kmeans_plusplus(F.astype(np.float32), 3, random_state=5)
    r32 = rows.astype(np.float32).astype(np.float64)
    assert len({int(np.flatnonzero((r32 == g).all(1))[0]) for g in got}) == 3


def test_kmeans_plusplus_on_identical_rows():
    from flashdeconv_amd.utils.niches import kmeans_plusplus
    F = np.tile(_data(1, 4, 81), (300, 1))
    got = kmeans_plusplus(F, 5, random_state=3)
    assert got.shape == (5, 4) and np.array_equal(got, F[:5])
    assert np.array_equal(kmeans_plusplus(F[:1], 1), F[:1])


# ---------------------------------------------------------------- 5. determinism, inputs, feature modes
def _device_graph(coords, k=6):
    import torch
    from flashdeconv_amd import _lib
    coords = np.ascontiguousarray(coords, dtype=np.float64)
    cd = torch.as_tensor(coords, device="cuda:0")
    h = ctypes.c_void_p()
    _lib.check(_lib.load().fdx_graph_build_dev(ctypes.c_void_p(cd.data_ptr()), coords.shape[0], coords.shape[1], _lib.GRAPH_KNN, int(k),
                                               0.0, None, ctypes.byref(h)))
    g = _lib.Graph(h.value)
    g.info()
    torch.cuda.synchronize()
    return g


@pytest.fixture(scope="module")
def knn300():
    rs = np.random.RandomState(300)
    g = _device_graph(rs.rand(300, 2) * np.sqrt(300.0))
    yield g
    g.close()


def _same(a, b):
    assert set(a) == set(b)
    for key in a:
        assert np.array_equal(_host(a[key]), _host(b[key]), equal_nan=True), key


def test_two_calls_return_the_same_bits(knn300):
    from flashdeconv_amd.utils.niches import spatial_niches
    V = _data(300, 8, 90)
    a, b = (spatial_niches(V, 6, knn300, features="both", random_state=4) for _ in range(2))
    assert set(a) == {"labels", "centers", "counts", "inertia", "n_iter", "converged", "composition"}
    _same(a, b)
    assert a["centers"].shape == (6, 16) and a["composition"].shape == (6, 8) and a["counts"].sum() == 300


def test_input_kinds():
    import torch
    from flashdeconv_amd.utils.niches import kmeans
    n, K, C = 130, 5, 4
    V = _data(n, K, 91)
    V32 = V.astype(np.float32)
    init = _init(V, C, 91)
    want = kmeans(V, init)
    want32 = kmeans(V32.astype(np.float64), init)
    _check_result(kmeans(V32, init), _lloyd(V32.astype(np.float64), init), V32.astype(np.float64), "numpy float32")

    def same(out, ref, cuda):
        lab = out["labels"]
        assert (isinstance(lab, torch.Tensor) and lab.is_cuda and lab.dtype == torch.int32) if cuda else isinstance(lab, np.ndarray)
        _same(out, ref)

    same(kmeans(V32, init), want32, False)
    same(kmeans(V, init.astype(np.float32).astype(np.float64)), kmeans(V, init.astype(np.float32)), False)
    same(kmeans(torch.as_tensor(V, device="cuda:0"), init), want, True)
    same(kmeans(torch.as_tensor(V32, device="cuda:0"), init), want32, True)
    init_d = torch.as_tensor(init, device="cuda:0")
    same(kmeans(torch.as_tensor(V, device="cuda:0"), init_d), want, True)
    assert np.array_equal(init_d.cpu().numpy(), init)                      # the caller's centres are not written
    wide = torch.full((n, 2 * K + 1), float("nan"), dtype=torch.float64, device="cuda:0")
    wide[:, :K] = torch.as_tensor(V, device="cuda:0")
    same(kmeans(wide[:, :K], init), want, True)                            # row stride 2 K + 1, read in place
    wide[:, 0:2 * K:2] = torch.as_tensor(V, device="cuda:0")
    view = wide[:, 0:2 * K:2]
    assert not view.is_contiguous() and view.stride(1) == 2
    same(kmeans(view, init), want, True)


def test_feature_modes(knn300):
    import torch
    from flashdeconv_amd.utils.niches import kmeans, kmeans_plusplus, spatial_niches
    from flashdeconv_amd.utils.spatial_stats import spatial_sums
    n, K, C, w = 300, 8, 5, 0.5
    V = _data(n, K, 92)
    nm = spatial_sums(V, knn300, neighbor_mean=True)["neighbor_mean"]
    for mode, F in (("composition", V), ("neighborhood", nm), ("both", np.concatenate([V, w * nm], axis=1))):
        got = spatial_niches(V, C, knn300, features=mode, neighbor_weight=w, random_state=7)
        want = kmeans(F, kmeans_plusplus(F, C, random_state=7))
        for key in want:
            assert np.array_equal(got[key], want[key]), (mode, key)
        sums, counts = _label_sums(V, got["labels"].astype(np.int64), C)
        assert np.array_equal(counts, got["counts"])
        full = counts > 0
        assert np.isnan(got["composition"][~full]).all()
        assert np.all(np.abs(got["composition"] - sums / np.maximum(counts, 1)[:, None])[full] <=
                      (4 * (counts[:, None] + 2) * U * V.max(0)[None, :])[full]), mode
        # CUDA values: the labels stay on the device, everything else is the same
        dev = spatial_niches(torch.as_tensor(V, device="cuda:0"), C, knn300, features=mode, neighbor_weight=w, random_state=7)
        assert isinstance(dev["labels"], torch.Tensor) and dev["labels"].is_cuda
        _same(dev, got)
    explicit = spatial_niches(V, C, knn300, features="both", init=np.concatenate([V[:C], nm[:C]], axis=1))
    _same(explicit, {**kmeans(np.concatenate([V, nm], axis=1), np.concatenate([V[:C], nm[:C]], axis=1)),
                     "composition": explicit["composition"]})
    for mode in ("neighborhood", "both"):
        with pytest.raises(ValueError, match="needs a graph"):
            spatial_niches(V, C, features=mode)


# ---------------------------------------------------------------- 6. model and AnnData surface
def test_model_method():
    from flashdeconv_amd import FlashDeconv
    from flashdeconv_amd.utils.niches import spatial_niches
    Y, X, coords, _ = datagen.count_like(200, 300, 5, 0.1, seed=9)
    with pytest.raises(RuntimeError, match=r"Model has not been fitted\. Call fit\(\) first\."):
        FlashDeconv().get_spatial_niches(3)
    results = {}
    for output in ("numpy", "torch"):
        m = FlashDeconv(sketch_dim=64, max_iter=20).fit(Y, X, coords, output=output)
        with pytest.raises(ValueError, match="Unknown what"):
            m.get_spatial_niches(3, what="nope")
        with pytest.raises(ValueError, match="Unknown features"):
            m.get_spatial_niches(3, features="nope")
        for what, values in (("proportions", m.proportions_), ("abundances", m.beta_)):
            got = m.get_spatial_niches(4, what=what, random_state=1)
            assert isinstance(got["labels"], np.ndarray) == (output == "numpy")
            _same(got, spatial_niches(values, 4, graph=m, features="both", random_state=1))
            assert got["centers"].shape == (4, 10) and got["composition"].shape == (4, 5) and got["counts"].sum() == 200
            results[output, what] = got
        comp = m.get_spatial_niches(3, features="composition", max_iter=1)
        assert comp["centers"].shape == (3, 5) and comp["n_iter"] == 1 and not comp["converged"]
        res = results[output, "proportions"]
        np.testing.assert_allclose(res["composition"][res["counts"] > 0].sum(1), 1.0, rtol=1e-12)
    for what in ("proportions", "abundances"):
        _same(results["numpy", what], results["torch", what])


def test_deconvolve_writes_the_niches_on_request_only():
    import pandas as pd
    import flashdeconv_amd as fd
    from flashdeconv_amd.io import prepare_data
    case = datagen.anndata_case()
    kw = dict(cell_type_key="celltype", sketch_dim=64, k_neighbors=4, n_hvg=300, n_markers_per_type=20)
    st, ref = datagen.anndata_objects(case)
    assert fd.tl.deconvolve(st, ref, **kw) is None
    st2, ref2 = datagen.anndata_objects(case)
    assert fd.tl.deconvolve(st2, ref2, n_niches=3, **kw) is None
    assert set(st2.obs.columns) - set(st.obs.columns) == {"flashdeconv_niche"} and set(st.obs.columns) <= set(st2.obs.columns)
    assert set(st2.obsm) == set(st.obsm)
    assert set(st2.uns) - set(st.uns) == {"flashdeconv_niche_composition"} and set(st.uns) <= set(st2.uns)
    assert set(st2.uns["flashdeconv_params"]) - set(st.uns["flashdeconv_params"]) == {"n_niches"}
    assert set(st.uns["flashdeconv_params"]) <= set(st2.uns["flashdeconv_params"]) and st2.uns["flashdeconv_params"]["n_niches"] == 3
    assert np.array_equal(st2.obsm["flashdeconv"].values, st.obsm["flashdeconv"].values)
    Y, X, coords, names, _ = prepare_data(st2, ref2, cell_type_key="celltype")
    m = fd.FlashDeconv(sketch_dim=64, k_neighbors=4, n_hvg=300, n_markers_per_type=20).fit(Y, X, coords)
    want = m.get_spatial_niches(3)
    niche, comp = st2.obs["flashdeconv_niche"], st2.uns["flashdeconv_niche_composition"]
    assert isinstance(niche.dtype, pd.CategoricalDtype) and list(niche.cat.categories) == [0, 1, 2]
    assert np.array_equal(np.asarray(niche), want["labels"])
    assert list(comp.index) == [0, 1, 2] and list(comp.columns) == [str(t) for t in names]
    np.testing.assert_array_equal(comp.values, want["composition"])
