"""Per-gene tests of the gene-statistics kernels: dense and CSR moments of log1p(CPM-10k), column sums, the column gather
and the per-type sums, each against plain NumPy in extended precision at the shapes where the launchers fork.

The reference is written from the formulas of the reference's ``utils/genes.py:52-102``:
    lib = max(rowsum, 1),  z = log1p(y / lib * 1e4),  mean = sum z / n,  var = sum (z - mean)^2 / (n - 1)   (two passes)
with every sum in ``np.longdouble`` where that is wider than float64 (``math.fsum`` per column otherwise).  float32 inputs
are the same float32 values widened.

Tolerances (u = 2^-53; none is measured on the code under test):
    a recursive sum of n non-negative terms, in any order, is within (n - 1) u relative; the row scale carries up to G u from
    the row sum; the device log1p is within 1 ulp (csrc/device_math.h).  With B = (n + G + 16) u
        |mean - ref| <= B ref
        |var - ref|  <= 4 B n/(n-1) E_ref[z^2]      absolute, scaled by the second moment: all the one-pass form
                                                    (sum z^2 / n - mean^2) n/(n-1) of the kernels can promise
    column and type sums of integers are exact (below 2^53 in every order); of non-negative fractions within (n + 4) u;
    a type mean is one more rounding (2 u); a gather is exact on the bits.
Every comparison prints its largest error as a fraction of its bound (pytest -s shows them).
"""
import ctypes
import functools
import math

import numpy as np
import pytest
from scipy import sparse

gpu = pytest.mark.gpu
U = 2.0 ** -53
WIDE = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
DTYPES = [np.float32, np.float64]


# ------------------------------------------------------------------------------------------------ reference and comparator
def _col_sums(A):
    if WIDE:
        return np.asarray(A, dtype=np.longdouble).sum(axis=0)
    return np.array([math.fsum(c) for c in np.asarray(A, dtype=np.float64).T])


def _ref_z(Y):
    """z per entry, in the widest float there is.  NaN goes where NumPy puts it: np.maximum keeps a NaN row sum."""
    Y = np.asarray(Y, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        if WIDE:
            Yw = Y.astype(np.longdouble)
            lib = np.maximum(Yw.sum(axis=1, keepdims=True), 1)
            return np.log1p(Yw / lib * np.longdouble(1e4))
        lib = np.maximum(np.array([math.fsum(r) for r in Y])[:, None], 1.0)
        return np.log1p(Y / lib * 1e4)


def _ref_from_z(Z):
    """(mean, two-pass ddof-1 variance, E[z^2]) per column, rounded to float64 at the end."""
    n = Z.shape[0]
    with np.errstate(invalid="ignore"):
        mean = _col_sums(Z) / n
        var = _col_sums((Z - mean) ** 2) / (n - 1) if n >= 2 else np.zeros(Z.shape[1])
        ez2 = _col_sums(Z * Z) / n
    return tuple(np.asarray(a, dtype=np.float64) for a in (mean, var, ez2))


def _ref_moments(Y):
    return _ref_from_z(_ref_z(Y))


def _note(what, name, err, bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = np.where(bound > 0, err / bound, 0.0)
    print(f"[gene-stats] {what}: {name} error at most {float(np.max(frac, initial=0.0)):.3g} of its bound")


def _check_moments(mean, var, ref, n, G, what=""):
    """The derived bounds of the module docstring; NaN exactly where the reference has NaN."""
    rmean, rvar, ez2 = ref
    B = (n + G + 16) * U
    assert mean.shape == rmean.shape and var.shape == rvar.shape
    assert np.array_equal(np.isnan(mean), np.isnan(rmean)), "mean: NaN in other genes than the reference's"
    assert np.array_equal(np.isnan(var), np.isnan(rvar)), "var: NaN in other genes than the reference's"
    ok = ~np.isnan(rmean)
    em, bm = np.abs(mean - rmean)[ok], B * np.abs(rmean)[ok]
    _note(what, "mean", em, bm)
    assert np.all(em <= bm), f"mean off by up to {np.max(em - bm):.3g} beyond the bound (gene {np.flatnonzero(ok)[np.argmax(em - bm)]})"
    ok = ~np.isnan(rvar)
    ev = np.abs(var - rvar)[ok]
    bv = (4 * B * (n / (n - 1.0)) * ez2[ok]) if n >= 2 else np.zeros(int(ok.sum()))
    _note(what, "var", ev, bv)
    assert np.all(ev <= bv), f"var off by up to {np.max(ev - bv):.3g} beyond the bound (gene {np.flatnonzero(ok)[np.argmax(ev - bv)]})"
    assert np.all(var[ok] >= 0)
    zero = ok & (ez2 == 0)
    assert np.all(var[zero] == 0) and np.all(mean[zero] == 0)


def _check_sums(got, Y, what="", exact_cols=None):
    """Column sums: exact where every term is an integer, (n + 4) u relative elsewhere (non-negative terms)."""
    Y = np.asarray(Y, dtype=np.float64)
    n = Y.shape[0]
    want = _col_sums(Y)
    if exact_cols is None:
        exact_cols = np.all(Y == np.rint(Y), axis=0)
    assert np.array_equal(got[exact_cols], want[exact_cols].astype(np.float64))
    err = np.abs(got - want).astype(np.float64)
    bound = ((n + 4) * U * np.abs(want)).astype(np.float64)
    _note(what, "column sum", err, bound)
    assert np.all(err <= bound)


def _counts(seed, n, G):
    """Poisson counts thinned to ~35 % density, 1 % of the entries in 64..5000 (rows with and without the kernels' log1p table),
    one all-zero row and one all-zero column where the shape has room for them."""
    rs = np.random.RandomState(seed)
    Y = (1 + rs.poisson(1.0, size=(n, G))) * (rs.random_sample((n, G)) < 0.35)
    big = rs.random_sample((n, G)) < 0.01
    Y = np.where(big, rs.randint(64, 5001, size=(n, G)), Y).astype(np.float64)
    if n >= 3:
        Y[n // 2] = 0
    if G >= 2:
        Y[:, G // 3] = 0
    return Y


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


# ------------------------------------------------------------------------------------------------ the comparator bites (CPU)
def _self_test_case():
    Y = _counts(5, 300, 50)
    Z = _ref_z(Y)
    ref = _ref_from_z(Z)
    _check_moments(ref[0], ref[1], ref, 300, 50, "self-test, reference against itself")
    return Y, Z, ref


def test_comparator_fails_on_one_dropped_entry():
    Y, Z, ref = _self_test_case()
    g = 7
    r = int(np.flatnonzero(Y[:, g] == 1)[0])          # the smallest entry a gene can lose
    Z2 = Z.copy()
    Z2[r, g] = 0
    mean, var, _ = _ref_from_z(Z2)
    assert abs(mean[g] - ref[0][g]) > 1e-7 * ref[0][g]
    with pytest.raises(AssertionError, match="mean off"):
        _check_moments(mean, var, ref, 300, 50, "self-test, dropped entry")
    with pytest.raises(AssertionError, match="var off"):
        _check_moments(ref[0], var, ref, 300, 50, "self-test, dropped entry (variance alone)")


def test_comparator_fails_on_a_neighbours_sum():
    _, _, ref = _self_test_case()
    mean = ref[0].copy()
    g = 7
    assert mean[g] != mean[g + 1]
    mean[g] = ref[0][g + 1]                           # the z-sum of the gene next door
    with pytest.raises(AssertionError, match="mean off"):
        _check_moments(mean, ref[1], ref, 300, 50, "self-test, neighbour's sum")


# ------------------------------------------------------------------------------------------------ device helpers
def _to_device(Y, pad=0):
    """The matrix in HBM (row stride G + pad, NaN in the pad so that any read of it shows)."""
    import torch
    t = torch.from_numpy(np.array(Y, order="C")).cuda()
    if pad:
        buf = torch.full((Y.shape[0], Y.shape[1] + pad), float("nan"), dtype=t.dtype, device="cuda")
        buf[:, :Y.shape[1]] = t
        t = buf
    torch.cuda.synchronize()
    return t


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


# ------------------------------------------------------------------------------------------------ 1. dense moments
# (n, G).  Row stripes: min(512, ceil(n / 256)) of ceil(n / stripes) rows each - one with n = 1, 2, 256; two (129 + 128 rows) at
# 257; three at 513 with G = 1; four of 250 at 1000, with G past one 512-gene step of the row sum; 131373 rows put the count at
# its cap (512 stripes of 257 rows, the last with 46) and so do 131073, where 511 stripes hold every row and the last owns none
DENSE_SHAPES = [(1, 40), (2, 40), (256, 257), (257, 513), (513, 1), (1000, 1025), (131073 + 300, 8), (131073, 8)]


@functools.lru_cache(maxsize=None)
def _dense_case(n, G, dtype):
    Y = _counts(100 + n + G, n, G).astype(dtype)
    return _frozen(Y, *_ref_moments(Y))


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("n,G", DENSE_SHAPES)
def test_dense_moments(n, G, dtype):
    from flashdeconv_amd import _lib
    from flashdeconv_amd.utils import genes
    Y, *ref = _dense_case(n, G, dtype)
    t = _to_device(Y)
    code = _lib.dtype_code(Y)
    mean, var = genes.gene_moments_device(t.data_ptr(), code, n, G, G)
    mean2, var2 = genes.gene_moments_device(t.data_ptr(), code, n, G, G)
    assert _bits_equal(mean, mean2) and _bits_equal(var, var2)            # stripes folded in stripe order
    _check_moments(mean, var, ref, n, G, f"dense {n}x{G} {Y.dtype} (device pointer)")
    mean_h, var_h = genes._gene_moments(Y)                                # the same kernels behind an upload
    assert _bits_equal(mean_h, mean) and _bits_equal(var_h, var)
    _check_moments(mean_h, var_h, ref, n, G, f"dense {n}x{G} {Y.dtype} (host array)")


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_dense_moments_row_stride(dtype):
    from flashdeconv_amd import _lib
    from flashdeconv_amd.utils import genes
    n, G = 257, 513
    Y, *ref = _dense_case(n, G, dtype)
    t = _to_device(Y, pad=13)
    mean, var = genes.gene_moments_device(t.data_ptr(), _lib.dtype_code(Y), n, G, G + 13)
    _check_moments(mean, var, ref, n, G, f"dense {n}x{G} {Y.dtype}, ldy = G + 13")
    tight = genes.gene_moments_device(_to_device(Y).data_ptr(), _lib.dtype_code(Y), n, G, G)
    assert _bits_equal(mean, tight[0]) and _bits_equal(var, tight[1])     # the stride changes no arithmetic


# ------------------------------------------------------------------------------------------------ 2. dense moments, value edges
def _dense_moments_f64(Y):
    from flashdeconv_amd import _lib
    from flashdeconv_amd.utils import genes
    t = _to_device(Y)
    return genes.gene_moments_device(t.data_ptr(), _lib.FDX_F64, Y.shape[0], Y.shape[1], Y.shape[1])


@gpu
def test_dense_moments_small_library_sizes():
    """Fractional rows scaled by 1e-6 .. 1e4: many row sums are below 1 and take lib = 1."""
    rs = np.random.RandomState(21)
    n, G = 300, 70
    Y = rs.random_sample((n, G)) * (rs.random_sample((n, G)) < 0.4) * 10.0 ** rs.uniform(-6, 4, size=(n, 1))
    assert 50 < np.sum(Y.sum(axis=1) < 1) < 250
    mean, var = _dense_moments_f64(Y)
    _check_moments(mean, var, _ref_moments(Y), n, G, "dense, library sizes on both sides of 1")


@gpu
def test_dense_moments_cancellation():
    """A column that is the same z = 9 in every row (true variance 0: the one-pass form is all rounding there), and one that
    is constant but for a single entry.  Every row is a permutation of the same integers, so every library size is equal."""
    rs = np.random.RandomState(22)
    n, G = 300, 64
    base = 1 + rs.poisson(3.0, size=G - 2)
    Y = np.empty((n, G))
    for r in range(n):
        Y[r, 2:] = rs.permutation(base)
    Y[:, 0] = np.rint(base.sum() * 0.81 / 0.19)                           # y / lib * 1e4 ~ 8100: z ~ 9.0
    Y[:, 1] = 5
    Y[17, 1] += 1
    Y[17, 2] -= 1                                                         # (row 17 keeps its library size)
    assert len(set(Y.sum(axis=1))) == 1 and np.all(Y >= 0)
    ref = _ref_moments(Y)
    assert abs(ref[0][0] - 9.0) < 0.01 and ref[1][0] < 1e-30 and ref[1][1] > 1e-6
    mean, var = _dense_moments_f64(Y)
    _check_moments(mean, var, ref, n, G, "dense, constant column at z = 9")


def _nan_case(value):
    Y = _counts(23, 300, 64)
    Y[5, 7] = value
    return Y


@gpu
def test_dense_moments_entry_below_minus_one():
    """log1p of less than -1 is NaN: the gene's mean and variance are NaN as NumPy's are, every other gene is untouched, and the
    ranking sees what the reference's ranking sees.  (The variance clamp was fmax(v, 0) = 0 for a NaN v: the gene then counted
    as a real, constant member of the top mean bin - where np.digitize puts a NaN mean - and gave the whole bin finite
    dispersions where the reference's are NaN.)"""
    from flashdeconv_amd.utils import genes
    Y = _nan_case(-3.0)
    assert Y[5].sum() > 1
    ref = _ref_moments(Y)
    assert np.flatnonzero(np.isnan(ref[0])).tolist() == [7] and np.isnan(ref[1][7])
    mean, var = _dense_moments_f64(Y)
    assert np.isnan(mean[7]) and np.isnan(var[7])
    _check_moments(mean, var, ref, 300, 64, "dense, one entry below -1")
    for n_top in (5, 20):
        assert np.array_equal(genes._hvg_from_moments(mean, var, n_top, 0.0125, 3.0, 0.5),
                              genes._hvg_from_moments(ref[0], ref[1], n_top, 0.0125, 3.0, 0.5))


@gpu
def test_dense_moments_nan_entry():
    """A NaN entry makes its row's library size NaN (np.maximum keeps it), so the whole row and with it every gene is NaN in
    NumPy; the device's row scale does the same."""
    from flashdeconv_amd.utils import genes
    Y = _nan_case(np.nan)
    ref = _ref_moments(Y)
    assert np.all(np.isnan(ref[0])) and np.all(np.isnan(ref[1]))
    mean, var = _dense_moments_f64(Y)
    assert np.isnan(mean[7]) and np.isnan(var[7])
    _check_moments(mean, var, ref, 300, 64, "dense, one NaN entry")
    assert np.array_equal(genes._hvg_from_moments(mean, var, 10, 0.0125, 3.0, 0.5),
                          genes._hvg_from_moments(ref[0], ref[1], 10, 0.0125, 3.0, 0.5))


# ------------------------------------------------------------------------------------------------ 3. dense column sums
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("n,G", DENSE_SHAPES)
def test_dense_column_sums(n, G, dtype):
    from flashdeconv_amd import _lib
    lib = _lib.load()
    Y = _dense_case(n, G, dtype)[0]
    rs = np.random.RandomState(n + G)
    code = _lib.dtype_code(Y)
    for kind, M in (("counts", Y), ("fractions", (Y * rs.random_sample(Y.shape)).astype(dtype))):
        out = np.full(G, -1.0)
        _lib.check(lib.fdx_column_sums(M.ctypes.data_as(ctypes.c_void_p), code, n, G, _lib.ptr_f64(out)))
        _check_sums(out, M, f"column sums {n}x{G} {Y.dtype} {kind} (host array)")
        for pad in (0, 13):
            t = _to_device(M, pad=pad)
            dev = np.full(G, -1.0)
            _lib.check(lib.fdx_column_sums_dev(t.data_ptr(), code, n, G, G + pad, _lib.ptr_f64(dev), None))
            assert _bits_equal(dev, out)                                  # same kernels, stripes folded in order
    assert np.all(Y == np.rint(Y))                                        # (the counts went through the exact branch)


# ------------------------------------------------------------------------------------------------ 4. column gather
# dtype, G_all, n, pad of the row stride.  Staged rows: 4 waves while 4 rows fit in 64 KB of LDS, else 2, else 1 (then up to
# 160 KB: the launch raises the dynamic-LDS limit); at most 2048 workgroups, so more than 2048 x waves rows make every wave
# come round to a second row.  Rows above 160 KB are gathered straight from memory.
GATHER = [(np.float32, 600, 8192 + 5, 0), (np.float64, 3000, 4096 + 3, 3), (np.float64, 9000, 2048 + 3, 0),
          (np.float32, 41000, 70, 5), (np.float64, 20481, 70, 0)]


@gpu
@pytest.mark.parametrize("dtype,G_all,n,pad", GATHER, ids=["f32-4waves", "f64-2waves", "f64-1wave-72KB", "f32-direct", "f64-direct"])
def test_gather_columns(dtype, G_all, n, pad):
    import torch
    from flashdeconv_amd import _lib
    lib = _lib.load()
    rs = np.random.RandomState(G_all)
    ld = G_all + pad
    Y = rs.standard_normal((n, ld)).astype(dtype)
    Y[0, 0], Y[n - 1, G_all - 1], Y[n // 2, 1] = -0.0, np.nan, np.inf       # bits, not values
    bits = np.uint32 if dtype == np.float32 else np.uint64
    t = _to_device(Y)
    guard, mark = 64, 12345.0
    for Gs in (1, 63, 64, 65, G_all):
        idx = np.sort(rs.choice(G_all, Gs, replace=False)).astype(np.int32)
        idx[-1] = G_all - 1
        if Gs > 1:
            idx[0] = 0
        assert np.all(np.diff(idx) > 0)
        out = torch.full((guard + n * Gs + guard,), mark, dtype=t.dtype, device="cuda")
        torch.cuda.synchronize()
        _lib.check(lib.fdx_gather_columns_dev(t.data_ptr(), _lib.dtype_code(Y), n, G_all, ld, _lib.ptr_i32(idx), Gs,
                                              out.data_ptr() + guard * Y.itemsize, None))
        got = out.cpu().numpy()
        assert np.array_equal(got[guard:-guard].reshape(n, Gs).view(bits), np.ascontiguousarray(Y[:, idx]).view(bits)), Gs
        assert np.all(got[:guard] == mark) and np.all(got[-guard:] == mark), Gs


# ------------------------------------------------------------------------------------------------ 5. CSR moments, sorted rows
def _tile_width(G, ns):
    """Genes per LDS tile of the sorted-row kernel, as csr_kernels.cpp documents it: 136 KB of sums per tile (ns arrays of doubles:
    sum z, sum z^2 and, with column sums, sum y), the gene axis in even shares rounded up to whole 64s, never above what fits.
    Only places the entries that sit on a tile's edge; nothing is asserted about it."""
    tmax = 136 * 1024 // (ns * 8)
    tiles = -(-G // tmax)
    return min(G, tmax, (-(-G // tiles) + 63) & ~63)


@functools.lru_cache(maxsize=None)
def _csr_case(n, G, last, dtype):
    """(scipy CSR matrix with sorted rows, reference moments of its dense form, mask of columns holding a non-integer)."""
    rs = np.random.RandomState(7 * n + G)
    base = _counts(3 * n + G, n, G)
    zc = G // 3                                                           # the all-zero column
    widths = [_tile_width(G, ns) for ns in (2, 3)]
    bounds = sorted({b for w in widths for b in range(w, G, w)})          # first columns of the tiles after the first, either layout
    first_end = bounds[0] if bounds else G                                # columns below it are in the first tile either way
    next_beg = max(widths) if max(widths) < G else None                   # columns from it on are past the first tile either way
    last_beg = bounds[-1] if bounds else 0

    def pick(lo, hi, k):
        pool = np.setdiff1d(np.arange(lo, hi), [zc])
        return np.sort(rs.choice(pool, min(k, len(pool)), replace=False))

    def small(k):
        return rs.randint(1, 40, size=k).astype(np.float64)

    rows = []
    for r in range(n):
        c = np.flatnonzero(base[r])
        rows.append((c, base[r, c]))
    three = pick(0, G, 3)
    if n >= 257:
        rows[0] = (np.empty(0, dtype=np.int64), np.empty(0))              # empty first row
        c = pick(last_beg, G, 200)
        rows[1] = (c, small(len(c)))                                      # every entry in the last tile
        c = pick(0, first_end, 200)
        rows[2] = (c, small(len(c)))                                      # every entry in the first tile
        v = small(G)
        v[zc] = 0.0
        rows[3] = (np.arange(G), v)                                       # every column stored (an explicit zero in the zero column)
        for r, m in ((4, 1), (5, 8)):                                     # exactly 64 m entries in the first tile, then the next tile
            c = pick(0, first_end, 64 * m)
            assert len(c) == 64 * m
            if next_beg is not None:
                c = np.concatenate([c, pick(next_beg, G, 5)])
            rows[r] = (c, small(len(c)))
        c = np.unique([0, G - 1] + [x for b in bounds for x in (b - 1, b)])
        c = c[c != zc]
        rows[6] = (c, small(len(c)))                                      # a tile's last column, then the next tile's first
        c = pick(0, G, 100)
        v = small(len(c))
        v[::2] = 0.0
        rows[7] = (c, v)                                                  # explicitly stored zeros
        c = pick(0, G, 150)
        v = small(len(c))
        v[::2] = rs.random_sample(len(v[::2])) * 50 + 0.25                # a table row whose every other entry misses the table
        rows[8] = (c, v)
        c = pick(0, G, 150)
        v = small(len(c))
        v[::3] = rs.random_sample(len(v[::3])) * 50 + 0.25                # counts, fractions and one value past the table: no table
        v[1] = 777.0
        rows[9] = (c, v)
        rows[n - 1] = (three, small(3)) if last == "three" else (np.empty(0, dtype=np.int64), np.empty(0))
    elif n == 2:
        rows = [(np.empty(0, dtype=np.int64), np.empty(0)), (three, small(3))]
    else:
        rows = [(three, small(3))]
    indptr = np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])]).astype(np.int64)
    indices = np.concatenate([c for c, _ in rows]).astype(np.int32)
    data = np.concatenate([v for _, v in rows]).astype(dtype)
    A = sparse.csr_matrix((data, indices, indptr), shape=(n, G))
    assert A.has_sorted_indices and A.nnz == len(data)
    D = A.toarray().astype(np.float64)
    frac = np.any(D != np.rint(D), axis=0)
    return (A,) + _frozen(*_ref_moments(D), np.asarray(_col_sums(D), dtype=np.float64), frac)


# n, G, column sums, last row.  Tiles: 700 genes fit in one; 5803 with column sums (136 KB / 24 B = 5802) and 8705 without
# (8704) take two; 18000 takes three without and four with; 11600 with column sums is two tiles of the full 5802.
CSR_SORTED = [(300, 700, False, "empty"), (300, 700, True, "three"), (300, 5803, True, "three"), (300, 8705, False, "empty"),
              (257, 18000, False, "three"), (257, 18000, True, "empty"), (300, 11600, True, "three"),
              (1, 700, False, "three"), (1, 700, True, "three"), (2, 700, False, "three"), (2, 700, True, "three")]


def _check_csr(csr, colsum, ref, n, G, what):
    rmean, rvar, ez2, rsum, frac = ref
    mean, var, cs = csr.gene_moments(want_colsum=colsum)
    _check_moments(mean, var, (rmean, rvar, ez2), n, G, what)
    if not colsum:
        assert cs is None
        return
    assert np.array_equal(cs[~frac], rsum[~frac])
    err, bound = np.abs(cs - rsum), (n + 4) * U * np.abs(rsum)
    _note(what, "column sum", err, bound)
    assert np.all(err <= bound)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("n,G,colsum,last", CSR_SORTED)
def test_csr_moments_sorted_rows(n, G, colsum, last, dtype):
    from flashdeconv_amd import _lib
    A, *ref = _csr_case(n, G, last, dtype)
    csr = _lib.CsrOnDevice.from_scipy(A)
    try:
        assert csr.view.sorted_rows == 1 and csr.view.nnz == A.nnz and csr.view.dtype == _lib.dtype_code(A.data)
        _check_csr(csr, colsum, ref, n, G, f"CSR sorted {n}x{G} {A.dtype} colsum={colsum}")
    finally:
        csr.free()


# ------------------------------------------------------------------------------------------------ 6. CSR moments, unsorted rows
def _reverse_every_third_row(A):
    A = A.copy()
    for r in range(0, A.shape[0], 3):
        a, b = A.indptr[r], A.indptr[r + 1]
        A.indices[a:b] = A.indices[a:b][::-1].copy()
        A.data[a:b] = A.data[a:b][::-1].copy()
    A.has_sorted_indices = False
    return A


# 64 KB of sums per tile: 2730 genes with column sums, 4096 without
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("G,colsum", [(700, True), (700, False), (2731, True), (4097, False)])
def test_csr_moments_unsorted_rows(G, colsum, dtype):
    from flashdeconv_amd import _lib
    n = 300
    A, *ref = _csr_case(n, G, "three", dtype)
    un = _lib.CsrOnDevice.from_scipy(_reverse_every_third_row(A), sort=False)
    try:
        assert un.view.sorted_rows == 0 and un.view.nnz == A.nnz
        _check_csr(un, colsum, ref, n, G, f"CSR unsorted {n}x{G} {A.dtype} colsum={colsum}")
    finally:
        un.free()


@gpu
@pytest.mark.parametrize("colsum", [False, True])
def test_csr_moments_no_stored_entry(colsum):
    from flashdeconv_amd import _lib
    csr = _lib.CsrOnDevice.from_scipy(sparse.csr_matrix((300, 700), dtype=np.float64))
    try:
        assert csr.view.nnz == 0
        mean, var, cs = csr.gene_moments(want_colsum=colsum)
    finally:
        csr.free()
    assert np.all(mean == 0) and np.all(var == 0) and mean.shape == var.shape == (700,)
    assert cs is None if not colsum else np.all(cs == 0)


@gpu
@pytest.mark.parametrize("value", [-3.0, np.nan], ids=["below-minus-one", "nan"])
def test_csr_moments_nan_propagates(value):
    """The sparse branch of the reference: zeros that are not stored contribute nothing, np.maximum keeps a NaN library size
    (every STORED entry of that row is then NaN) and np.maximum(var, 0) keeps a NaN variance.  Both CSR kernels."""
    from flashdeconv_amd import _lib
    n, G = 300, 700
    A = _csr_case(n, G, "three", np.float64)[0].copy()
    q = int(A.indptr[40]) + 2
    A.data[q] = value
    D = A.toarray()
    stored = np.zeros((n, G), dtype=bool)
    stored[np.repeat(np.arange(n), np.diff(A.indptr)), A.indices] = True
    Z = np.where(stored, _ref_z(D), 0)
    ref = _ref_from_z(Z)
    want_nan = stored[40] if np.isnan(value) else np.arange(G) == A.indices[q]
    assert np.array_equal(np.isnan(ref[0]), want_nan)
    for form in (A, _reverse_every_third_row(A)):
        csr = _lib.CsrOnDevice.from_scipy(form, sort=False)
        try:
            assert csr.view.sorted_rows == (1 if form is A else 0)
            mean, var, _ = csr.gene_moments()
        finally:
            csr.free()
        _check_moments(mean, var, ref, n, G, f"CSR with one entry {value}, sorted_rows={form is A}")


# ------------------------------------------------------------------------------------------------ 7. CSR against dense
def _dispersion(mean, var):
    """Variance z-scored inside 20 percentile bins of the positive means (what the ranking sorts by)."""
    disp = np.zeros(len(mean))
    edges = np.unique(np.percentile(mean[mean > 0], np.linspace(0, 100, 21)))
    which = np.clip(np.digitize(mean, edges) - 1, 0, len(edges) - 2)
    for b in range(len(edges) - 1):
        m = which == b
        if m.sum() > 1:
            disp[m] = (var[m] - var[m].mean()) / (var[m].std() + 1e-10)
    return disp


@gpu
def test_csr_and_dense_moments_agree_through_the_reference():
    from flashdeconv_amd import _lib
    from flashdeconv_amd.utils import genes
    n, G = 300, 5803
    A, rmean, rvar, ez2, _, _ = _csr_case(n, G, "three", np.float64)
    D = A.toarray()
    md, vd = genes._gene_moments(D)
    ms, vs = genes._gene_moments(A)
    _check_moments(md, vd, (rmean, rvar, ez2), n, G, "dense form of the CSR case")
    _check_moments(ms, vs, (rmean, rvar, ez2), n, G, "CSR form")
    # (no bit equality between the two: a gene's terms are added in another order)
    disp = _dispersion(rmean, rvar)
    valid = np.sort(disp[(rmean >= 0.0125) & (rmean <= 3.0) & (disp >= 0.5)])[::-1]
    gaps = valid[:-1] - valid[1:]
    n_top = next(k for k in range(20, len(valid) // 2) if gaps[k - 1] > 1e-6)   # the cut between two clearly different genes
    hs, hd = genes.select_hvg(A, n_top), genes.select_hvg(D, n_top)
    assert len(hs) == n_top and np.array_equal(hs, hd)


# ------------------------------------------------------------------------------------------------ 8. type sums
TYPE_SIZES = (1, 0, 7, 64, 3, 200)


def _check_types(got, S, cnt, mean, terms_rtol, what):
    """S: exact (K, G) sums; terms_rtol: 0 for counts, (cells + 4) u per type for fractions."""
    with np.errstate(invalid="ignore", divide="ignore"):
        want = np.asarray(S / cnt[:, None] if mean else S, dtype=np.float64)
    if mean:
        assert np.all(np.isnan(got[cnt == 0])) and np.array_equal(np.isnan(got), np.isnan(want))
    else:
        assert np.all(got[cnt == 0] == 0)
        if not np.any(terms_rtol):
            assert np.array_equal(got, want)
    ok = ~np.isnan(want)
    bound = ((terms_rtol + (2 * U if mean else 0.0))[:, None] * np.abs(want))
    err = np.abs(got - want)
    _note(what, "type mean" if mean else "type sum", err[ok], bound[ok])
    assert np.all(err[ok] <= bound[ok])


def _type_layout(rs, sizes):
    K, n = len(sizes), int(sum(sizes))
    labels = np.repeat(np.arange(K), sizes)
    rs.shuffle(labels)
    order = np.argsort(labels, kind="stable").astype(np.int32)            # by type, ascending row inside a type
    off = np.concatenate([[0], np.cumsum(np.bincount(labels, minlength=K))]).astype(np.int32)
    return K, n, labels, order, off


def _type_sums(view_or_tensor, code, n, G, ld, order, off, K, mean):
    import torch
    from flashdeconv_amd import _lib
    lib = _lib.load()
    rows_d, off_d = torch.from_numpy(order).cuda(), torch.from_numpy(off).cuda()
    X = torch.full((K, G), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    if isinstance(view_or_tensor, _lib.CsrOnDevice):
        _lib.check(lib.fdx_type_sums_csr_dev(ctypes.byref(view_or_tensor.view), rows_d.data_ptr(), off_d.data_ptr(), K, mean,
                                             X.data_ptr(), None))
    else:
        _lib.check(lib.fdx_type_sums_dev(view_or_tensor.data_ptr(), code, n, G, ld, rows_d.data_ptr(), off_d.data_ptr(), K, mean,
                                         X.data_ptr(), None))
    torch.cuda.synchronize()
    return X.cpu().numpy()


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("G", [1, 256, 257, 700])
def test_type_sums(G, dtype):
    from flashdeconv_amd import _lib
    rs = np.random.RandomState(G)
    for sizes in ((275,), TYPE_SIZES):
        K, n, labels, order, off = _type_layout(rs, sizes)
        Y = _counts(G + K, n, G).astype(dtype)
        if G == 1:
            Y[::2, 0] = 3                                                 # (one column: not the all-zero one)
        cnt = np.asarray(sizes, dtype=np.float64)
        S = np.stack([Y[labels == k].astype(np.float64).sum(axis=0) for k in range(K)])
        code = _lib.dtype_code(Y)
        csr = _lib.CsrOnDevice.from_scipy(sparse.csr_matrix(Y))
        try:
            assert csr.view.dtype == code
            for mean in (0, 1):
                for pad in ((0, 5) if G == 257 else (0,)):
                    got = _type_sums(_to_device(Y, pad=pad), code, n, G, G + pad, order, off, K, mean)
                    _check_types(got, S, cnt, mean, np.zeros(K), f"type sums dense {n}x{G} K={K} {Y.dtype} ldy=G+{pad}")
                got = _type_sums(csr, code, n, G, G, order, off, K, mean)
                _check_types(got, S, cnt, mean, np.zeros(K), f"type sums CSR {n}x{G} K={K} {Y.dtype}")
        finally:
            csr.free()


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_type_sums_csr_fractions(dtype):
    from flashdeconv_amd import _lib
    rs = np.random.RandomState(9)
    G = 257
    K, n, labels, order, off = _type_layout(rs, TYPE_SIZES)
    Y = (_counts(9, n, G) * rs.random_sample((n, G))).astype(dtype)
    cnt = np.asarray(TYPE_SIZES, dtype=np.float64)
    S = np.stack([_col_sums(Y[labels == k].astype(np.float64)) for k in range(K)])
    csr = _lib.CsrOnDevice.from_scipy(sparse.csr_matrix(Y))
    try:
        for mean in (0, 1):
            got = _type_sums(csr, _lib.dtype_code(Y), n, G, G, order, off, K, mean)
            _check_types(got, S, cnt, mean, (cnt + 4) * U, f"type sums CSR fractions {Y.dtype}")
    finally:
        csr.free()
