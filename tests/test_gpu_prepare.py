"""The sketch -> H stage on its own output: fdx_prepare_dev / fdx_prepare_csr_dev (preprocess, CountSketch, contraction with
X_sketch -> H, XtX, YtY) against a plain float64 numpy evaluation of the same formulas, PER ELEMENT, on every kernel path
the dispatch can take.  Every dense case first asks fdx_sketch_path which kernels the library will run (0 = two-kernel path,
1 = narrow, 2 = wide tile form) and asserts the answer it was written for; every tile-path case runs once more under
FDX_NO_FUSED=1 (the two-kernel path) against the same reference.  The CSR cases at the end ask fdx_sketch_csr_path in the same
way; the CSR kernels' own file is test_gpu_prepare_csr.py.

The bound.  With T = f(Y) (the mode's rule), S = T Omega, H = S_x S_y^T and M = (|f(X)| |Omega_x|) (|f(Y)| |Omega_y|)^T:

    |H - H_ref| <= (c64 * 2^-53 + c32 * 2^-23) * M          element by element

c64 (float64 chains; 2^-53 = unit roundoff) is the worst-case count of roundings on the way to one entry of H, each at most
one unit roundoff of the running magnitude (first-order error analysis of a dot product, Higham 3.1):
    occ_y + occ_x   a bucket sum is a dot product over the genes of the bucket: one rounding per gene (product, or fused
                    multiply-add) - the largest bucket occupancy on each side;
    d               the contraction over the sketch dimension, one rounding per bucket whatever the order or the split;
    3 + 4 + G       log modes, per side: the device log1p is within 3 ulp (csrc/tile_device.h, tile_sketch_kernel.h header), the
                    argument y * scale carries the roundings of (sum + 1e-10), 1 / ., . * 1e4 and the product (4), and the
                    row sum of G non-negative addends at most G roundings; d log1p(x) / log1p(x) <= dx / x, so a relative
                    error of the argument is at most that of the value;
    4               the float64 numpy reference itself (it stays within 3.2 units of an 80-bit evaluation on shapes like these);
    1               everything of second order (c64 * 2^-53 is below 1e-11).
c32 (float32 rows in the log modes on the tile path, whose log1p is float32-class by design; 2^-23 = one float32 ulp) is
4 + 1 + 1: the 4 ulp of test_float32_log1p_of_the_tile_kernel_is_float32_accurate, one rounding of the scale to float32 and
one of the product y * scale.  XtX and YtY take the same form against their own magnitude sums: twice the per-side terms
(every entry is a product of two sketched values), d, and for YtY the n addends of the final sum.
None of this is fitted to the output.  A gene that is dropped, counted twice or taken with a wrong weight changes an entry by
about its share of M, i.e. by 1e3 (float32-class) to 1e12 (float64) times these bounds.

Largest observed err / (eps * M) per path family over the whole file on an MI355X (recorded here, NOT used as a limit;
eps = 2^-53, for the float32-class rows 2^-23), the range of the derived c over the family's cases, and the largest share of
its own c that any case used:
    family                              H: observed   c               share  | YtY: observed   c              share
    tile narrow, float64 chain             3.673      15 .. 3307      0.109  |    2.475        65 .. 12378    0.038
    tile wide, float64 chain               5.861      79 .. 3455      0.044  |    3.786        80 .. 12640    0.012
    tile narrow, float32-class             0.798      6               0.133  |    0.649        12             0.054
    tile wide, float32-class               0.712      6               0.119  |    0.644        12             0.054
    two-kernel path                        9.995      15 .. 83513     0.052  |    3.786        65 .. 83550    0.038
    CSR, fused kernel                      5.119      273 .. 2295     0.018  |    1.355        475 .. 2495    0.002
    CSR, scatter + contraction             4.175      273 .. 1539     0.008  |    1.199        473 .. 1739    0.002
    XtX (every case)                      11.567      15 .. 83513     0.044
(the c above 80000: the rows of 41003 genes that are streamed, whose row sum has that many addends.)
The file takes 5 s on that machine (273 cases).
"""
import ctypes

import numpy as np
import pytest
from scipy import sparse

pytestmark = pytest.mark.gpu

E64, E32 = 2.0 ** -53, 2.0 ** -23
C32 = 4 + 1 + 1
SENTINEL = 1.2345e300
MODES = ("raw", "log_cpm", "log_cpm_sparse")
LOG_MODES = ("log_cpm", "log_cpm_sparse")
DTYPES = (np.float32, np.float64)
_worst = {}


@pytest.fixture(scope="module", autouse=True)
def _report_the_largest_ratios():
    yield
    if _worst:
        print("\n[test_gpu_prepare] largest err / (eps * M) per path family (derived c: min .. max; largest share of a case's own c):")
        for fam in sorted(_worst):
            r, lo, hi, part = _worst[fam]
            print(f"[test_gpu_prepare]   {fam:<34s} {r:10.3f}   c = {lo:g} .. {hi:g}   {part:.4f}")


def _note(family, ratio, c):
    r, lo, hi, part = _worst.get(family, (0.0, c, c, 0.0))
    _worst[family] = (max(r, float(ratio)), min(lo, c), max(hi, c), max(part, float(ratio) / c))


# ---------------------------------------------------------------------------------------------- reference (float64 numpy)
def transform(A, mode):
    A = np.asarray(A, dtype=np.float64)
    if mode == "raw":
        return A
    s = A.sum(axis=1, keepdims=True)
    with np.errstate(all="ignore"):
        if mode == "log_cpm":
            return np.log1p(A / (s + 1e-10) * 1e4)
        s = np.where(s == 0.0, 1.0, s)
        return np.log1p(A / s * 1e4)


def sketch(T, bucket, w, d):
    S = np.zeros((T.shape[0], d))
    with np.errstate(all="ignore"):
        np.add.at(S, (slice(None), bucket), T * w)
    return S


def reference(Y, X, bucket, wy, wx, d, mode_y, mode_x):
    Ty, Tx = transform(Y, mode_y), transform(X, mode_x)
    Sy, Sx = sketch(Ty, bucket, wy, d), sketch(Tx, bucket, wx, d)
    Ay, Ax = sketch(np.abs(Ty), bucket, np.abs(wy), d), sketch(np.abs(Tx), bucket, np.abs(wx), d)
    occ = int(np.bincount(bucket, minlength=d).max())
    with np.errstate(all="ignore"):
        return dict(H=Sx @ Sy.T, M=Ax @ Ay.T, XtX=Sx @ Sx.T, Mxx=Ax @ Ax.T, YtY=float((Sy * Sy).sum()),
                    Myy=float((Ay * Ay).sum()), occ=occ)


def c_transform(mode, addends):
    """relative error of one transformed value on a float64 chain, in units of 2^-53 (module docstring)"""
    return 0 if mode == "raw" else 3 + 4 + addends


def bounds(ref, n, G, d, mode_y, mode_x, f32_class):
    """(c64 of H, c64 of XtX, c64 of YtY, relative float32-class term of H, of YtY).  A reference over stored entries
    (prepare_csr_ref.py) states the spot side's two data terms itself: occ_y, the most stored selected entries of one row in one
    bucket, and addends_y, the longest selected row; without them both are the dense ones (bucket occupancy, G)."""
    occ_y = ref.get("occ_y", ref["occ"])
    ty, tx = c_transform(mode_y, ref.get("addends_y", G)), c_transform(mode_x, G)   # (float32-class rows too: their row sum is a float64 one)
    c_h = occ_y + ref["occ"] + d + ty + tx + 4 + 1
    c_xx = 2 * (ref["occ"] + tx) + d + 4 + 1
    c_yy = 2 * (occ_y + ty) + d + n + 4 + 1
    e32 = C32 * E32 if f32_class else 0.0
    return c_h, c_xx, c_yy, e32, (1.0 + e32) ** 2 - 1.0


# ---------------------------------------------------------------------------------------------- running the stage
def _codes():
    from flashdeconv_amd import _lib
    return {"raw": _lib.PRE_RAW, "log_cpm": _lib.PRE_LOG_CPM, "log_cpm_sparse": _lib.PRE_LOG_CPM_SPARSE}


class _DeviceArrays:
    """fdx_malloc'ed copies of host arrays, returned on exit"""

    def __init__(self):
        from flashdeconv_amd import _lib
        self._lib, self.lib, self.ptrs = _lib, _lib.load(), []

    def put(self, arr, offset=0):
        p = ctypes.c_void_p()
        self._lib.check(self.lib.fdx_malloc(ctypes.byref(p), max(arr.nbytes + offset, 16)))
        self.ptrs.append(p)
        q = ctypes.c_void_p(p.value + offset)
        self._lib.upload_bytes(q, arr)
        return q

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.lib.fdx_free(p)


def sketch_path(dtype, ptr, ldy, G, d, K, mode, bucket, wy, flags=0):
    """(path, {NWC, NWL, JW, TT, GB, NBLK}) of fdx_sketch_path"""
    from flashdeconv_amd import _lib
    path = ctypes.c_int32(-1)
    dims = np.zeros(6, dtype=np.int32)
    _lib.check(_lib.load().fdx_sketch_path(_lib.dtype_code(np.dtype(dtype)), ptr, ldy, G, d, K, _codes()[mode] | flags, _lib.ptr_i32(bucket),
                                           _lib.ptr_f64(wy), ctypes.byref(path), _lib.ptr_i32(dims)))
    return path.value, dict(zip(("NWC", "NWL", "JW", "TT", "GB", "NBLK"), (int(v) for v in dims)))


def csr_sketch_path(dtype, G_all, n_sel, d, K, mode):
    """(path, the eight dims) of fdx_sketch_csr_path: 0 = scatter kernel + contraction, 1 = the fused kernel; no device needed"""
    from flashdeconv_amd import _lib
    path = ctypes.c_int32(-1)
    dims = np.zeros(8, dtype=np.int32)
    _lib.check(_lib.load().fdx_sketch_csr_path(_lib.dtype_code(np.dtype(dtype)), G_all, n_sel, d, K, _codes().get(mode, mode),
                                               ctypes.byref(path), _lib.ptr_i32(dims)))
    return path.value, [int(v) for v in dims]


def run_dense(Ybuf, n, G, X, bucket, wy, wx, d, mode_y, mode_x, row_map=None, ldh=None, flags=0, offset=0, query=True):
    """fdx_prepare_dev on rows of Ybuf (row stride = its second dimension).  H comes back whole, (K, ldh), prefilled with
    SENTINEL; `path` is what fdx_sketch_path says for exactly this call."""
    from flashdeconv_amd import _lib
    lib = _lib.load()
    _lib.require_gpu()
    K, ldy = X.shape[0], Ybuf.shape[1]
    ldh = n + 3 if ldh is None else ldh
    H = np.full((K, ldh), SENTINEL)
    XtX, XtX_h, yty = np.zeros((K, K)), np.zeros((K, K)), ctypes.c_double(0.0)
    assert Ybuf.flags.c_contiguous and X.flags.c_contiguous and X.dtype == np.float64 and bucket.dtype == np.int32
    with _DeviceArrays() as dev:
        dY, dH, dG = dev.put(Ybuf, offset), dev.put(H), dev.put(XtX)
        dmap = dev.put(np.ascontiguousarray(row_map, dtype=np.int32)) if row_map is not None else None
        path, dims = sketch_path(Ybuf.dtype, dY, ldy, G, d, K, mode_y, bucket, wy, flags) if query else (None, None)
        _lib.check(lib.fdx_prepare_dev(dY, _lib.dtype_code(Ybuf.dtype), n, G, ldy, dmap, _lib.ptr_f64(X), K, _lib.ptr_i32(bucket),
                                       _lib.ptr_f64(wy), _lib.ptr_f64(wx), d, _codes()[mode_y] | flags, _codes()[mode_x], dH, ldh,
                                       dG, _lib.ptr_f64(XtX_h), ctypes.byref(yty), None))
        _lib.download_bytes(H, dH)
        _lib.download_bytes(XtX, dG)
    return dict(H=H, XtX=XtX, XtX_host=XtX_h, YtY=yty.value, path=path, dims=dims)


def compare(got, ref, n, G, d, mode_y, mode_x, f32_class, family, bad_spots=()):
    """H, XtX, YtY of one run against the reference, element by element; the sentinel columns of H untouched."""
    c_h, c_xx, c_yy, e32, e32_yy = bounds(ref, n, G, d, mode_y, mode_x, f32_class)
    H = got["H"]
    assert np.all(H[:, n:] == SENTINEL), "columns [n, ldh) of H were written"
    H = H[:, :n]
    fin = np.isfinite(ref["H"])
    assert np.array_equal(np.isfinite(H), fin), "non-finite entries of H are not where the reference has them"
    bad = np.flatnonzero(~fin.all(axis=0))
    assert set(bad) <= set(bad_spots), f"non-finite reference columns {bad} in a case that expects {bad_spots}"
    err = np.where(fin, np.abs(np.where(fin, H, 0.0) - np.where(fin, ref["H"], 0.0)), 0.0)
    M = np.where(fin, ref["M"], 0.0)
    eps = E32 if f32_class else E64
    pos = M > 0
    ratio = float((err[pos] / (eps * M[pos])).max()) if pos.any() else 0.0
    c_show = C32 + c_h * E64 / E32 if f32_class else c_h
    print(f"[{family}] H: err/(eps M) = {ratio:.3f} (c = {c_show:g}); n={n} G={G} d={d} K={H.shape[0]} {mode_y}")
    assert np.all(err[~pos] == 0.0), "entries whose magnitude sum is zero must be exact zeros"
    assert np.all(err <= (c_h * E64 + e32) * M), (family, ratio, c_show, np.argwhere(err > (c_h * E64 + e32) * M)[:5])
    _note(family + " H", ratio, c_show)
    # XtX: always a float64 chain (the signatures are float64), the device copy and the host copy are the same bits
    assert np.array_equal(got["XtX"], got["XtX_host"])
    ex = np.abs(got["XtX"] - ref["XtX"])
    rx = float((ex / (E64 * ref["Mxx"])).max())
    print(f"[{family}] XtX: err/(eps M) = {rx:.3f} (c = {c_xx})")
    assert np.all(ex <= c_xx * E64 * ref["Mxx"]), (family, rx, c_xx)
    _note("XtX", rx, c_xx)
    if np.isfinite(ref["YtY"]):
        ey = abs(got["YtY"] - ref["YtY"])
        ry = ey / (eps * ref["Myy"]) if ref["Myy"] > 0 else 0.0
        c_show_y = 2 * C32 + c_yy * E64 / E32 if f32_class else c_yy
        print(f"[{family}] YtY: err/(eps M) = {ry:.3f} (c = {c_show_y:g})")
        assert ey <= (c_yy * E64 + e32_yy) * ref["Myy"], (family, ry, c_show_y)
        _note(family + " YtY", ry, c_show_y)
    else:
        assert not np.isfinite(got["YtY"])


def problem(n, G, K, d, mode, dtype, seed, pearson=False):
    """Rows as the mode meets them: signed reals for raw; for the log modes counts (rows that take log1p from the table of
    small counts), a count above 63, and rows of non-integers."""
    rs = np.random.RandomState(seed)
    if mode == "raw":
        Y = rs.randn(n, G) * np.exp(rs.randn(1, G))
    else:
        Y = rs.poisson(0.8, size=(n, G)).astype(np.float64)
        Y[1::3] *= rs.uniform(0.3, 2.5, size=Y[1::3].shape)
        Y[0, G // 2] = 70.0
    X = np.ascontiguousarray(np.exp(rs.randn(K, G) * 0.5))
    bucket = rs.randint(0, d, size=G).astype(np.int32)
    sign = rs.choice([-1.0, 1.0], size=G)
    wy = sign * rs.uniform(0.5, 2.0, size=G)
    wx = sign * rs.uniform(0.5, 2.0, size=G) if pearson else wy
    return np.ascontiguousarray(Y.astype(dtype)), X, bucket, wy, wx


def family_of(path, f32_class):
    return ("two-kernel", "tile narrow", "tile wide")[path] + (" float32-class" if f32_class else " float64")


def check_case(monkeypatch, Y, X, bucket, wy, wx, d, mode, want_path, flags=0, pad=0, offset=0, row_map=None, bad_spots=(),
               mode_x=None):
    """One case: path asserted, result compared, and a tile-path case once more on the two-kernel path.  `pad` extra columns
    (filled with a large value nobody may read) make ldy > G; row_map selects and orders the rows."""
    from flashdeconv_amd import _lib
    mode_x = mode if mode_x is None else mode_x
    G = Y.shape[1]
    Ybuf = Y
    if pad:
        Ybuf = np.full((Y.shape[0], G + pad), 3.0e30, dtype=Y.dtype)
        Ybuf[:, :G] = Y
    rows = Y if row_map is None else Y[np.asarray(row_map)]
    n = rows.shape[0]
    ref = reference(rows, X, bucket, wy, wx, d, mode, mode_x)
    got = run_dense(Ybuf, n, G, X, bucket, wy, wx, d, mode, mode_x, row_map=row_map, flags=flags, offset=offset)
    if want_path == "tile":
        assert got["path"] >= 1, got
    else:
        assert got["path"] == want_path, got
    f32_class = Y.dtype == np.float32 and mode != "raw" and got["path"] >= 1 and not (flags & _lib.PRE_F64_MATH)
    compare(got, ref, n, G, d, mode, mode_x, f32_class, family_of(got["path"], f32_class), bad_spots)
    if got["path"] >= 1:
        monkeypatch.setenv("FDX_NO_FUSED", "1")
        two = run_dense(Ybuf, n, G, X, bucket, wy, wx, d, mode, mode_x, row_map=row_map, flags=flags, offset=offset)
        monkeypatch.delenv("FDX_NO_FUSED")
        assert two["path"] == 0, two                              # the query follows the switch, like the dispatch
        compare(two, ref, n, G, d, mode, mode_x, False, family_of(0, False), bad_spots)
    return got


# ---------------------------------------------------------------------------------------------- the dispatch matrix
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K", [1, 16, 17, 32, 33, 48, 49, 64])
def test_type_tiles_narrow_and_wide(K, mode, dtype, monkeypatch):
    """1..16 types: one type tile; 17..32: two; 33..64: the wide form with four.  300 spots: 18 whole tiles and one of 12.
    The wave split (consumer waves, loader waves, groups per consumer wave) is that of the mode and the form."""
    n, G, d = 300, 600, 128
    Y, X, bucket, wy, wx = problem(n, G, K, d, mode, dtype, seed=1000 + K)
    got = check_case(monkeypatch, Y, X, bucket, wy, wx, d, mode, 1 if K <= 32 else 2)
    assert got["dims"]["TT"] == ((K + 15) // 16 if K <= 32 else 4)
    split = {("raw", False): (12, 4, 11), ("raw", True): (12, 4, 22), ("log", False): (16, 0, 8), ("log", True): (8, 0, 32)}
    assert tuple(got["dims"][k] for k in ("NWC", "NWL", "JW")) == split["raw" if mode == "raw" else "log", K > 32], got["dims"]


@pytest.mark.parametrize("mode", LOG_MODES)
@pytest.mark.parametrize("K", [1, 16, 17, 32, 49])
def test_float32_rows_on_the_float64_chain(K, mode, monkeypatch):
    """FDX_PRE_F64_MATH (integer counts stored as float32): the float64 log chain, held to the float64 bound - its own kernels
    for one type tile, two, and the wide form."""
    from flashdeconv_amd import _lib
    n, G, d = 300, 600, 128
    Y, X, bucket, wy, wx = problem(n, G, K, d, mode, np.float32, seed=1100 + K)
    Y = np.ascontiguousarray(np.round(Y))
    check_case(monkeypatch, Y, X, bucket, wy, wx, d, mode, 1 if K <= 32 else 2, flags=_lib.PRE_F64_MATH)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode,d,path", [("raw", 528, 1), ("raw", 529, 2), ("raw", 1056, 2), ("raw", 1057, 0),
                                         ("log_cpm", 512, 1), ("log_cpm", 513, 2), ("log_cpm", 1024, 2), ("log_cpm", 1025, 0),
                                         ("log_cpm_sparse", 512, 1), ("log_cpm_sparse", 513, 2), ("log_cpm_sparse", 1024, 2),
                                         ("log_cpm_sparse", 1025, 0)])
def test_sketch_dim_narrow_wide_and_past_the_limit(mode, d, path, dtype, monkeypatch):
    """The narrow split owns 4 x 12 x 11 = 528 buckets (raw) or 4 x 16 x 8 = 512 (log), the wide one 1056 or 1024; one more
    bucket than that and the two-kernel path takes the shape."""
    n, G, K = 200, 1200, 8
    Y, X, bucket, wy, wx = problem(n, G, K, d, mode, dtype, seed=1200 + d)
    check_case(monkeypatch, Y, X, bucket, wy, wx, d, mode, path)


@pytest.mark.parametrize("mode,dtype", [("raw", np.float32), ("log_cpm", np.float64), ("log_cpm_sparse", np.float32)])
def test_sixty_five_types_take_the_two_kernel_path(mode, dtype, monkeypatch):
    n, G, K, d = 200, 600, 65, 128
    Y, X, bucket, wy, wx = problem(n, G, K, d, mode, dtype, seed=1300)
    check_case(monkeypatch, Y, X, bucket, wy, wx, d, mode, 0)


# ---------------------------------------------------------------------------------------------- rows and genes
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype,G,K,d", [(np.float64, 1500, 7, 256), (np.float32, 3000, 40, 700), (np.float64, 1100, 20, 1024)])
def test_several_column_blocks(dtype, G, K, d, mode, monkeypatch):
    """Rows longer than a stage buffer are cut into column blocks; the last block is a partial one."""
    Y, X, bucket, wy, wx = problem(150, G, K, d, mode, dtype, seed=1400 + G)
    got = check_case(monkeypatch, Y, X, bucket, wy, wx, d, mode, "tile")
    assert got["dims"]["NBLK"] >= 2 and G % got["dims"]["GB"] != 0, got["dims"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype,G,K", [(np.float32, 256, 5), (np.float64, 128, 40)])
def test_a_single_column_block(dtype, G, K, mode, monkeypatch):
    Y, X, bucket, wy, wx = problem(150, G, K, 64, mode, dtype, seed=1500 + G)
    got = check_case(monkeypatch, Y, X, bucket, wy, wx, 64, mode, "tile")
    assert got["dims"]["NBLK"] == 1, got["dims"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype,G", [(np.float32, 4), (np.float64, 2)])
def test_smallest_rows_the_tile_kernel_takes(dtype, G, mode, monkeypatch):
    """One 16-byte vector per row."""
    Y, X, bucket, wy, wx = problem(50, G, 3, 8, mode, dtype, seed=1600 + G)
    check_case(monkeypatch, Y, X, bucket, wy, wx, 8, mode, "tile")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype,G,pad,offset", [(np.float32, 602, 0, 0), (np.float32, 601, 0, 0), (np.float64, 601, 0, 0),   # rows not whole vectors
                                                (np.float32, 600, 1, 0), (np.float32, 600, 2, 0), (np.float64, 600, 1, 0),  # row stride not
                                                (np.float64, 600, 0, 8)])                                                  # first row not
def test_rows_that_are_not_whole_aligned_vectors_take_the_two_kernel_path(dtype, G, pad, offset, mode, monkeypatch):
    Y, X, bucket, wy, wx = problem(150, G, 6, 128, mode, dtype, seed=1700 + G + pad)
    check_case(monkeypatch, Y, X, bucket, wy, wx, 128, mode, 0, pad=pad, offset=offset)


# ---------------------------------------------------------------------------------------------- spot counts
@pytest.mark.parametrize("form", ["narrow", "wide"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [1, 15, 16, 17, 4096, 4097, 8192 + 15, 3 * 4096 + 1])
def test_spot_counts_around_a_tile_and_around_a_full_grid(n, mode, form, monkeypatch):
    """Tiles are 16 spots, a launch has at most 256 workgroups: above 4096 spots a workgroup takes a second and a third tile
    (the next tile's rows, row sums and stage buffer parity), with a whole or a partial last tile."""
    dtype, G, K, d = (np.float32, 256, 5, 64) if form == "narrow" else (np.float64, 128, 40, 64)
    Y, X, bucket, wy, wx = problem(n, G, K, d, mode, dtype, seed=1800 + n % 1000)
    check_case(monkeypatch, Y, X, bucket, wy, wx, d, mode, 1 if form == "narrow" else 2)


@pytest.mark.parametrize("mode,dtype,G,K,d", [("log_cpm", np.float64, 1500, 7, 256), ("raw", np.float32, 3000, 40, 700),
                                              ("log_cpm_sparse", np.float32, 3000, 12, 512)])
def test_second_tile_of_a_workgroup_with_several_column_blocks(mode, dtype, G, K, d, monkeypatch):
    """The next tile's first column block is requested while the last block of this tile is consumed."""
    Y, X, bucket, wy, wx = problem(4096 + 16 + 5, G, K, d, mode, dtype, seed=1900 + G)
    got = check_case(monkeypatch, Y, X, bucket, wy, wx, d, mode, "tile")
    assert got["dims"]["NBLK"] >= 2, got["dims"]


# ---------------------------------------------------------------------------------------------- Omega edges
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode,d,path", [("raw", 512, 1), ("log_cpm", 512, 1), ("raw", 1024, 2), ("log_cpm_sparse", 1024, 2)])
def test_fewer_genes_than_buckets(mode, d, path, dtype, monkeypatch):
    Y, X, bucket, wy, wx = problem(100, 64, 4, d, mode, dtype, seed=2000 + d)
    check_case(monkeypatch, Y, X, bucket, wy, wx, d, mode, path)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", MODES)
def test_genes_outside_omega(mode, dtype, monkeypatch):
    """A gene outside Omega is a gene of weight 0.0 at this seam (the log modes' library size still counts it, as the
    reference's does when Omega has an empty row); bucket -1, the schedule builder's own mark for such genes, is refused
    by the entry points, not read as an index."""
    from flashdeconv_amd import _lib
    n, G, K, d = 120, 600, 9, 128
    Y, X, bucket, wy, wx = problem(n, G, K, d, mode, dtype, seed=2100)
    wy = wy.copy()
    wy[::7] = 0.0
    wy[G - 1] = 0.0
    check_case(monkeypatch, Y, X, bucket, wy, wy, d, mode, 1)
    b2 = bucket.copy()
    b2[5] = -1
    with pytest.raises(_lib.FdxError, match="bucket index out of range"):
        sketch_path(dtype, None, G, G, d, K, mode, b2, wy)
    with pytest.raises(_lib.FdxError, match="bucket index out of range"):
        run_dense(Y, n, G, X, b2, wy, wy, d, mode, mode, query=False)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,d", [(9, 128), (40, 600)])
def test_pearson_style_weights_differ_between_the_two_sides(K, d, dtype, monkeypatch):
    """"pearson" is raw mode with sign / sigma_g on the spot side and other weights on the signature side."""
    Y, X, bucket, wy, wx = problem(130, 600, K, d, "raw", dtype, seed=2200 + K, pearson=True)
    wy = wy / (0.05 + np.abs(Y).mean(axis=0))
    check_case(monkeypatch, Y, X, bucket, wy, wx, d, "raw", 1 if K <= 32 else 2)


@pytest.mark.parametrize("mode", ["raw", "log_cpm"])
def test_plans_are_cached_by_content_not_by_bucket_alone(mode, monkeypatch):
    """Two calls of one process with the same buckets and other spot-side weights: each its own reference."""
    Y, X, bucket, wy, wx = problem(100, 600, 9, 128, mode, np.float32, seed=2300)
    check_case(monkeypatch, Y, X, bucket, wy, wy, 128, mode, 1)
    wy2 = wy * np.where(np.arange(600) % 5 == 0, -3.0, 0.5)
    check_case(monkeypatch, Y, X, bucket, wy2, wy, 128, mode, 1)
    check_case(monkeypatch, Y, X, bucket, wy, wy, 128, mode, 1)


@pytest.mark.parametrize("dtype,d", [(np.float32, 4), (np.float32, 2), (np.float64, 1)])
@pytest.mark.parametrize("mode", MODES)
def test_an_omega_the_tile_schedule_refuses(mode, dtype, d, monkeypatch):
    """2000 genes in four, two or one bucket: more than 255 genes of a bucket inside one column block (1024 float32 genes, or a
    few hundred float64 ones), which the schedule's byte per group length cannot hold (test_host.py:
    test_tile_schedule_refuses_...).  No tile schedule, so the two-kernel path - and the same numbers."""
    Y, X, bucket, wy, wx = problem(100, 2000, 6, d, mode, dtype, seed=2400)
    check_case(monkeypatch, Y, X, bucket, wy, wx, d, mode, 0)


@pytest.mark.parametrize("dtype,G", [(np.float64, 21001), (np.float32, 41003)])
@pytest.mark.parametrize("mode", MODES)
def test_rows_that_do_not_fit_in_lds_are_streamed(mode, dtype, G, monkeypatch):
    """More genes than LDS holds as a staged row (160 KB: 20480 float64 or 40960 float32 values) or as the scatter kernel's
    table: sketch_rows_stream_kernel reads weight and bucket per gene from global memory.  The signatures are float64, so the
    X side takes it for both shapes; under FDX_NO_FUSED the spot side does too (10 workgroups of 4 rows, the last with one).
    Not covered: a wave's second row, which takes more than 8192 rows of 168 KB each."""
    Y, X, bucket, wy, wx = problem(37, G, 5, 64, mode, dtype, seed=2450 + G % 100)
    monkeypatch.setenv("FDX_NO_FUSED", "1")
    check_case(monkeypatch, Y, X, bucket, wy, wx, 64, mode, 0)


# ---------------------------------------------------------------------------------------------- row contents
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", LOG_MODES)
def test_an_all_zero_row(mode, dtype, monkeypatch):
    """log_cpm divides by (0 + 1e-10), log_cpm_sparse by 1: either way the row's column of H is exactly zero (the bound is 0)."""
    Y, X, bucket, wy, wx = problem(70, 600, 6, 128, mode, dtype, seed=2500)
    Y[3] = 0.0
    Y[37] = 0.0
    Y[38, 1:] = 0.0                                           # and a row with one entry
    got = check_case(monkeypatch, Y, X, bucket, wy, wx, 128, mode, 1)
    assert np.all(got["H"][:, 3] == 0.0) and np.all(got["H"][:, 37] == 0.0)


@pytest.mark.parametrize("mode,K,d", [("raw", 6, 128), ("log_cpm", 6, 128), ("log_cpm_sparse", 6, 128), ("log_cpm", 40, 600)])
def test_values_over_eighteen_decades(mode, K, d, monkeypatch):
    """float64 rows from 1e-12 to 1e6: library sizes where log_cpm's 1e-10 matters and where it does not."""
    rs = np.random.RandomState(26)
    Y, X, bucket, wy, wx = problem(96, 600, K, d, mode, np.float64, seed=2600)
    Y[:48] = 10.0 ** rs.uniform(-12, 6, size=(48, 600))
    Y[48:64] = 10.0 ** rs.uniform(-12, -9, size=(16, 600))    # library size near log_cpm's 1e-10
    Y[64:80] = rs.rand(16, 600) * 1e-3
    check_case(monkeypatch, Y, X, bucket, wy, wx, d, mode, 1 if K <= 32 else 2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode,K,d", [("raw", 6, 128), ("log_cpm", 6, 128), ("log_cpm_sparse", 6, 128), ("raw", 40, 600),
                                      ("log_cpm", 40, 600)])
def test_negative_nan_and_inf_entries_stay_in_their_spots(mode, K, d, dtype, monkeypatch):
    """A negative entry, a NaN and an Inf in three spots of three tiles: non-finite output in exactly the columns where the
    reference has it, every other column - the 15 other spots of those tiles too - within the bound."""
    n, G = 100, 600
    Y, X, bucket, wy, wx = problem(n, G, K, d, mode, dtype, seed=2700)
    Y[5, 17] = -2.0                                            # log modes: 1 + y * scale is far below zero, the reference's NaN
    Y[40, G - 1] = np.nan
    Y[77, 300] = np.inf
    bad = (40, 77) if mode == "raw" else (5, 40, 77)
    check_case(monkeypatch, Y, X, bucket, wy, wx, d, mode, 1 if K <= 32 else 2, bad_spots=bad)


# ---------------------------------------------------------------------------------------------- layout invariants, bit for bit
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode,K,d", [("raw", 12, 128), ("log_cpm", 12, 128), ("log_cpm_sparse", 12, 128), ("raw", 40, 600),
                                      ("log_cpm", 40, 600)])
def test_layout_does_not_change_a_bit(mode, K, d, dtype, fused, monkeypatch):
    """csrc/prepare.cpp: shards keep the same bits.  On finite non-negative rows H is identical with a padded row stride,
    through a row map, for a leading part of the rows that ends on a multiple of 256, and from run to run."""
    n, G = 1000, 600
    Y, X, bucket, wy, wx = problem(n, G, K, d, mode, dtype, seed=2800)
    Y = np.abs(Y)
    if not fused:
        monkeypatch.setenv("FDX_NO_FUSED", "1")
    want_path = (1 if K <= 32 else 2) if fused else 0
    base = run_dense(Y, n, G, X, bucket, wy, wx, d, mode, mode)
    assert base["path"] == want_path
    again = run_dense(Y, n, G, X, bucket, wy, wx, d, mode, mode)
    assert np.array_equal(again["H"], base["H"]) and np.array_equal(again["XtX"], base["XtX"])
    pad = 16 // Y.dtype.itemsize                               # rows stay whole 16-byte vectors
    Ypad = np.full((n, G + pad), 3.0e30, dtype=dtype)
    Ypad[:, :G] = Y
    padded = run_dense(Ypad, n, G, X, bucket, wy, wx, d, mode, mode)
    assert padded["path"] == want_path and np.array_equal(padded["H"], base["H"])
    perm = np.random.RandomState(3).permutation(n).astype(np.int32)
    mapped = run_dense(Y, n, G, X, bucket, wy, wx, d, mode, mode, row_map=perm)
    assert mapped["path"] == want_path and np.array_equal(mapped["H"][:, :n], base["H"][:, perm])
    both = run_dense(Ypad, 700, G, X, bucket, wy, wx, d, mode, mode, row_map=perm[:700])
    assert np.array_equal(both["H"][:, :700], base["H"][:, perm[:700]]) and np.all(both["H"][:, 700:] == SENTINEL)
    for n_cut in (256, 768):
        cut = run_dense(Y, n_cut, G, X, bucket, wy, wx, d, mode, mode)
        assert np.array_equal(cut["H"][:, :n_cut], base["H"][:, :n_cut])


# ---------------------------------------------------------------------------------------------- the CSR seam
def run_csr(Ycsr, gene_idx, G, X, bucket, wy, wx, d, mode, ldh, ex=None, sort=True):
    """fdx_prepare_csr_dev, or with ex = (row_map or None, n_rows) fdx_prepare_csr_ex_dev; sort=False uploads the rows as stored"""
    from flashdeconv_amd import _lib
    lib = _lib.load()
    _lib.require_gpu()
    K, n = X.shape[0], Ycsr.shape[0]
    H = np.full((K, ldh), SENTINEL)
    XtX, XtX_h, yty = np.zeros((K, K)), np.zeros((K, K)), ctypes.c_double(0.0)
    csr = _lib.CsrOnDevice.from_scipy(Ycsr, sort=sort)
    try:
        assert csr.view.dtype == _lib.dtype_code(Ycsr.data)
        with _DeviceArrays() as dev:
            dH, dG = dev.put(H), dev.put(XtX)
            gi = _lib.ptr_i32(gene_idx) if gene_idx is not None else None
            args = (ctypes.byref(csr.view), gi, G, _lib.ptr_f64(X), K, _lib.ptr_i32(bucket), _lib.ptr_f64(wy), _lib.ptr_f64(wx), d,
                    _codes().get(mode, mode), _codes().get(mode, mode), dH, ldh, dG, _lib.ptr_f64(XtX_h), ctypes.byref(yty))
            if ex is None:
                _lib.check(lib.fdx_prepare_csr_dev(*args, None))
            else:
                dmap = dev.put(np.ascontiguousarray(ex[0], dtype=np.int32)) if ex[0] is not None else None
                _lib.check(lib.fdx_prepare_csr_ex_dev(*args, dmap, ex[1], None))
            _lib.download_bytes(H, dH)
            _lib.download_bytes(XtX, dG)
    finally:
        csr.free()
    return dict(H=H, XtX=XtX, XtX_host=XtX_h, YtY=yty.value, n=n)


def csr_problem(n, G_all, G, K, d, dtype, seed, dense_rows=0.5):
    rs = np.random.RandomState(seed)
    dens = np.where(np.arange(n) % 2 == 0, dense_rows, 0.05)[:, None]
    Y = rs.poisson(2.0, size=(n, G_all)) * (rs.rand(n, G_all) < dens)
    Y = Y.astype(np.float64)
    Y[2::5] *= rs.uniform(0.3, 2.5, size=Y[2::5].shape)
    Y[0, 0] = 70.0
    Y[4] = 0.0                                                 # empty rows, one of them the last
    Y[n - 1] = 0.0
    gene_idx = None if G == G_all else np.sort(rs.choice(G_all, size=G, replace=False)).astype(np.int32)
    if gene_idx is not None:
        Y[9] = 0.0
        Y[9, np.setdiff1d(np.arange(G_all), gene_idx)[:20]] = 3.0   # a row whose entries are all outside the selection
    X = np.ascontiguousarray(np.exp(rs.randn(K, G) * 0.5))
    bucket = rs.randint(0, d, size=G).astype(np.int32)
    wy = rs.choice([-1.0, 1.0], size=G) * rs.uniform(0.5, 2.0, size=G)
    return Y.astype(dtype), gene_idx, X, bucket, wy


def check_csr(Y, gene_idx, X, bucket, wy, d, mode, family):
    n, G = Y.shape[0], X.shape[1]
    path, _ = csr_sketch_path(Y.dtype, Y.shape[1], G, d, X.shape[0], mode)
    assert path == {"CSR fused": 1, "CSR two-kernel": 0}[family], (family, path)
    rows = Y if gene_idx is None else Y[:, gene_idx]           # the subset first, then the library size over it
    ref = reference(rows, X, bucket, wy, wy, d, mode, mode)
    got = run_csr(sparse.csr_matrix(Y), gene_idx, G, X, bucket, wy, wy, d, mode, n + 5)
    compare(got, ref, n, G, d, mode, mode, False, family)      # float32 values too: the CSR kernels have one, float64, chain
    return got


@pytest.mark.parametrize("subset", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["raw", "log_cpm_sparse"])
def test_csr_rows(mode, dtype, subset, monkeypatch):
    """fdx_prepare_csr_dev, shapes the fused CSR kernel takes (csr_contract_ok: d % 4 == 0, blocks of 256 buckets x type tiles
    <= 4): all columns or a selected subset, empty rows, a row with nothing selected.  check_csr asserts the path by
    fdx_sketch_csr_path."""
    Y, gene_idx, X, bucket, wy = csr_problem(300, 900, 500 if subset else 900, 8, 256, dtype, seed=3000 + subset)
    check_csr(Y, gene_idx, X, bucket, wy, 256, mode, "CSR fused")


@pytest.mark.parametrize("mode,dtype", [("raw", np.float64), ("log_cpm_sparse", np.float32)])
@pytest.mark.parametrize("K,d,fused", [(32, 512, True), (33, 512, False), (64, 256, True), (65, 256, False), (8, 254, False),
                                       (8, 1024, True)])
def test_csr_on_both_sides_of_what_the_fused_kernel_takes(K, d, fused, mode, dtype, monkeypatch):
    """Two blocks of buckets x two type tiles is the most the fused CSR kernel holds: 33 types at d = 512, 65 types anywhere
    and a sketch dimension that is no multiple of 4 go through the CSR scatter kernel and the contraction."""
    Y, gene_idx, X, bucket, wy = csr_problem(200, 900, 500, K, d, dtype, seed=3100 + K)
    check_csr(Y, gene_idx, X, bucket, wy, d, mode, "CSR fused" if fused else "CSR two-kernel")


@pytest.mark.parametrize("dtype", DTYPES)
def test_csr_rows_longer_than_the_keep_buffer(dtype, monkeypatch):
    """FDX_CSR_KEEP_CAP=64: every row with more than 64 selected entries overflows the wave's keep buffer and is walked again."""
    Y, gene_idx, X, bucket, wy = csr_problem(200, 1200, 1000, 8, 256, dtype, seed=3200)
    assert ((Y[:, gene_idx] != 0).sum(axis=1) > 300).sum() > 50 and ((Y[:, gene_idx] != 0).sum(axis=1) < 64).sum() > 50
    a = check_csr(Y, gene_idx, X, bucket, wy, 256, "log_cpm_sparse", "CSR fused")
    monkeypatch.setenv("FDX_CSR_KEEP_CAP", "64")
    b = check_csr(Y, gene_idx, X, bucket, wy, 256, "log_cpm_sparse", "CSR fused")
    assert np.array_equal(np.isfinite(a["H"]), np.isfinite(b["H"]))
