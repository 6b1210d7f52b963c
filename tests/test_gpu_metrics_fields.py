"""The metrics kernels (csrc/metrics_kernels.cpp) per field, per rank and at every geometry edge, against the plain reference of
tests/metrics_ref.py (which tests/test_metrics_host.py checks against the recorded outputs of the real reference, and whose
comparators it shows to fail on a reference that is wrong in one place).

The C entries are called through ctypes, so the row strides, the flags and the raw (K + 1) x 18 stats block are in the test's
hands; a handful of cases go through the Python API for its routing.  Inputs (metrics_ref.pair) are seeded, proportion-like and
non-negative, about 60 % exact zeros and the rest quantised to 3 decimals, with one constant column where K >= 3.

What is covered
    column passes   all 18 fields of every row at K = 1 (256 lanes), 3 (85 lanes, one idle thread), 100 (56 idle threads),
                    128 / 129 (2 lanes -> 1), 255 / 256 / 257 / 513 (column groups 1 -> 2 -> 3, a last group of one column), slab
                    depths 2, 65, 129 and the cap of 1024 with empty trailing blocks; a NaN in pred only and one in true only
    JSD             every spot and the sum at epsilon 1e-10 and 1e-3: tile heights 256, 227, 2, 1, short, full and ragged tiles,
                    more tiles than blocks, the untiled kernel with one and two blocks, all-zero rows in either matrix
    ranks           rho of flags 1, 2, 3 and of fdx_metrics_spearman_dev alone at every width of the column sort's key, tie runs
                    that end one column's segment and start the next, constant / 95 % zero / all-distinct / signed-zero columns,
                    float32 denormals, n K = 150 000 and 40 961 x 129
    row stride      ld = K, K + 3, 2 K with NaN and huge values in the padding; column slices, row-strided and transposed
                    views, mixed dtypes and mixed host / device inputs through Python
    refusals        every argument check of the three C entries
Left out: the grid stride of the untiled JSD kernel (K >= 2049) needs n > 262 144 rows of more than 2048 columns, several GB.

Bounds (u = 2^-53; derived, none measured on the code under test)
    counts and NaN flags are exact integers; min and max are equal by value (-0.0 == 0.0)
    SSE, SAE, sum p, sum t: a sum of n non-negative terms, each from at most two roundings, in any order:
        |err| <= (n + 4) u ref, with N = n K terms in row K (n + K <= N + 4 roundings the column-then-row order makes);
        a NaN exactly where the reference has one
    centred sums, with d_p = (n + 1) u mean|p| the error of the device mean (d_t likewise; N for n in row K): about a mean that is
    off by d the sum of squares grows by exactly n d^2 (the cross term vanishes), the rest is the rounding of a sum:
        |C_PP - ref| <= (n + 4) u ref + n d_p^2
        |C_PT - ref| <= (n + 4) u sqrt(C_PP C_TT) + n d_p d_t              (Cauchy-Schwarz on sum |dp dt|)
    rank sums: twice-ranks and their mean N + 1 are integers and every partial sum is an integer of magnitude <= N^3, so for
        N^3 < 2^53 (N <= 208 063; per column N = n) the three device sums are exact in every order and with every contraction.
        rho is then made on the host by corr_from_sums from correctly rounded divisions and square roots, with nothing to
        contract: rho_host equals metrics_ref.rho_from_sums of the exact integer sums BIT FOR BIT.  Above that size (the overall
        rho of 40 961 x 129): atol 1e-12, as tests/test_gpu_metrics.py uses
    JSD per spot: the row sums carry (K - 1) u, each quotient 2 u, log is within 1 ulp (csrc/device_math.h / ocml):
        |err| <= (K + 8) u (S + 1),  S = 1/2 sum_c (|a log(a / m)| + |b log(b / m)|) from metrics_ref.jsd
        the sum: within the sum of the per-spot bounds plus (n + 1) u sum |jsd|
Every comparison prints its largest error as a fraction of its bound (pytest -s shows them).
"""
import ctypes
import functools

import numpy as np
import pytest

import metrics_ref as R

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "float64"]
THR = 0.05
MARK = -7.0                    # what the outputs hold before a call: a refused call leaves it there


# ------------------------------------------------------------------------------------------------ device helpers
def _on_device(a, ld=None):
    """The matrix in HBM with row stride ld; pad cells alternate NaN and the largest finite value, so that any read of them shows."""
    import torch
    a = np.ascontiguousarray(a)
    n, K = a.shape
    if ld is None or ld == K:
        return torch.from_numpy(a.copy()).cuda()
    buf = np.full((n, ld), np.nan, dtype=a.dtype)
    buf[:, K + 1::2] = np.finfo(a.dtype).max
    buf[:, :K] = a
    return torch.from_numpy(buf).cuda()


def _code(a):
    from flashdeconv_amd import _lib
    return _lib.FDX_F32 if str(a.dtype).endswith("float32") else _lib.FDX_F64


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _outputs(n, K, want_jsd):
    import torch
    stats = np.full((K + 1, R.FIELDS), MARK)
    rare = np.full(4, int(MARK), dtype=np.int64)
    rho = np.full(K + 1, MARK)
    jsd = torch.full((n,), MARK, dtype=torch.float64, device="cuda") if want_jsd else None
    torch.cuda.synchronize()
    return stats, rare, rho, jsd


def _evaluate(P, T, n, K, ldp=None, ldq=None, thr=THR, eps=1e-10, flags=0, want_jsd=False, entry="evaluate"):
    """(stats, rare, rho, jsd on the host or None) of fdx_metrics_evaluate_dev, or of fdx_metrics_moments_dev (no rho)."""
    from flashdeconv_amd import _lib
    lib = _lib.load()
    stats, rare, rho, jsd = _outputs(n, K, want_jsd)
    jp = ctypes.c_void_p(jsd.data_ptr()) if want_jsd else None
    args = (ctypes.c_void_p(P.data_ptr()), ctypes.c_void_p(T.data_ptr()), _code(P), n, K, ldp or K, ldq or K, thr, eps)
    if entry == "evaluate":
        _lib.check(lib.fdx_metrics_evaluate_dev(*args, flags, jp, _lib.ptr_f64(stats), _lib.ptr_i64(rare), _lib.ptr_f64(rho), _stream()))
    else:
        _lib.check(lib.fdx_metrics_moments_dev(*args, jp, _lib.ptr_f64(stats), _lib.ptr_i64(rare), _stream()))
    return stats, rare, rho, (jsd.cpu().numpy() if want_jsd else None)


def _spearman(P, T, n, K, flags, ldp=None, ldq=None):
    from flashdeconv_amd import _lib
    rho = np.full(K + 1, MARK)
    _lib.check(_lib.load().fdx_metrics_spearman_dev(ctypes.c_void_p(P.data_ptr()), ctypes.c_void_p(T.data_ptr()), _code(P), n, K,
                                                    ldp or K, ldq or K, flags, _lib.ptr_f64(rho), _stream()))
    return rho


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def _reference(n, K, dtype):
    return R.reference(*R.pair(n, K, dtype), THR)


@functools.lru_cache(maxsize=None)
def _rho3(n, K, dtype):
    rho = R.spearman_raw(*R.pair(n, K, dtype), 3)
    rho.setflags(write=False)
    return rho


def _masked(rho3, flags):
    """What the C entries return for `flags` of the rho of flags 3: NaN in the rows that were not asked for."""
    out = rho3.copy()
    if not flags & R.SPEARMAN_PER_TYPE:
        out[:-1] = np.nan
    if not flags & R.SPEARMAN_OVERALL:
        out[-1] = np.nan
    return out


# ------------------------------------------------------------------------------------------------ 1. column passes
# (K, n): col_geom gives cw = min(K, 256) columns and 256 // cw row lanes per block, ceil(K / cw) column groups and
# nbx = min(1024, ceil(n / (32 lanes))) row chunks, the depth of the slab that mx_slab_reduce folds 64 blocks at a time
COLUMN_SHAPES = [(1, 1), (1, 255), (1, 256), (1, 257), (1, 8193),      # 256 lanes of one column; nbx = 2 at 8193
                 (3, 37), (3, 2721),                                   # 85 lanes, one idle thread; a second row chunk
                 (100, 65),                                            # 2 lanes, 56 idle threads
                 (128, 65), (129, 65),                                 # 2 lanes -> 1
                 (255, 33), (256, 33), (257, 33), (513, 33),           # column groups 1 -> 2 -> 3, the last of one column
                 (129, 2049), (129, 4097),                             # slab depth 65 and 129
                 (129, 40961)]                                         # nbx at its cap: chunks of 41 rows, blocks 1000 .. 1023 empty


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,n", COLUMN_SHAPES)
def test_column_passes_every_field(K, n, dtype):
    p, t = R.pair(n, K, dtype)
    ref = _reference(n, K, dtype)
    P, T = _on_device(p), _on_device(t)
    what = f"columns {n}x{K} {dtype}"
    stats, rare, rho, _ = _evaluate(P, T, n, K)
    R.check_stats(stats, ref, what)
    assert rare.tolist() == [int(v) for v in ref["fields"][K, R.N_RARE:R.FN + 1]]
    assert np.all(rho == MARK)                                            # flags 0: rho is not written
    stats2, rare2, _, _ = _evaluate(P, T, n, K, entry="moments")
    assert _same_bits(stats, stats2) and rare.tolist() == rare2.tolist()  # one device sequence behind both entries, fixed order
    other, _, _, _ = _evaluate(P, T, n, K, thr=0.2)                       # another threshold moves the counts and nothing else
    R.check_stats(other, dict(ref, fields=R.fields(p, t, 0.2)), what + ", threshold 0.2")


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_in_one_matrix_flags_its_column_and_row_k_only(dtype):
    """A NaN in pred (column 0, in the second row chunk) and one in true (column 2): the flag is set in that column and in row K,
    min and max pass the NaN over, the sums that touch it are NaN and no other."""
    K, n = 3, 2721
    p, t = (a.copy() for a in R.pair(n, K, dtype))
    p[n - 1, 0] = np.nan
    t[5, 2] = np.nan
    ref = R.reference(p, t, THR)
    F = ref["fields"]
    assert F[:, R.NAN_P].tolist() == [1, 0, 0, 1] and F[:, R.NAN_T].tolist() == [0, 0, 1, 1]
    assert not np.isnan(F[:, R.MIN_P:R.MAX_T + 1]).any()
    assert np.isnan(F[:, R.SSE]).tolist() == [True, False, True, True] and np.isnan(F[:, R.SUM_T]).tolist() == [False, False, True, True]
    stats, rare, _, _ = _evaluate(_on_device(p), _on_device(t), n, K)
    R.check_stats(stats, ref, f"NaN entries {n}x{K} {dtype}")
    assert rare.tolist() == [int(v) for v in F[K, R.N_RARE:R.FN + 1]]


# ------------------------------------------------------------------------------------------------ 2. JSD
# (K, n): rows are staged in LDS in tiles of R = min(2048 // K, 256) spots, tiles grid-strided over at most 1024 blocks
JSD_SHAPES = [(1, 5),                                  # the JSD of a one-type row is 0
              (2, 257),                                # the smallest real row
              (8, 255), (8, 256), (8, 257),            # R = 256: a short tile, a full tile, a ragged second tile
              (9, 228),                                # R = 227: a ragged second tile
              (1024, 2051),                            # R = 2: 1026 tiles on 1024 blocks, blocks 0 and 1 take a second tile
              (2047, 3), (2048, 3),                    # R = 1
              (2048, 1030),                            # R = 1 and the grid stride
              (2049, 3), (2049, 300)]                  # the untiled kernel, one and two blocks


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,n", JSD_SHAPES)
def test_jsd_every_spot_and_the_sum(K, n, dtype):
    p, t = R.jsd_pair(n, K, dtype)
    P, T = _on_device(p), _on_device(t)
    for eps, entry in ((1e-10, "evaluate"), (1e-3, "moments")):
        j, S = R.jsd(p, t, eps)
        stats, _, _, got = _evaluate(P, T, n, K, eps=eps, want_jsd=True, entry=entry)
        R.check_jsd(got, stats[K, R.JSD_SUM], j, S, K, f"jsd {n}x{K} {dtype} eps {eps:g}")
        assert np.all(stats[:K, R.JSD_SUM] == 0)
        if K == 1:
            assert np.all(got == 0)
    if n * K <= 20000:                                                    # the other 17 fields do not move when the JSD runs
        R.check_stats(stats, R.reference(p, t, THR), f"jsd {n}x{K} {dtype}, the stats beside it", jsd_sum_checked=True)


# ------------------------------------------------------------------------------------------------ 3. ranks and Spearman
def _check_all_flags(p, t, want3, what, atol_overall=False):
    """flags 1, 2 and 3 through fdx_metrics_evaluate_dev, then fdx_metrics_spearman_dev alone, against the rho of the exact sums."""
    n, K = p.shape
    P, T = _on_device(p), _on_device(t)
    loose = (K,) if atol_overall else ()
    got = {}
    for flags in (1, 2, 3):
        got[flags] = _evaluate(P, T, n, K, flags=flags)[2]
        R.check_rho(got[flags], _masked(want3, flags), f"{what} flags {flags}", atol_rows=loose if flags & 1 else ())
    alone = _spearman(P, T, n, K, 3)
    R.check_rho(alone, want3, f"{what} spearman entry", atol_rows=loose)
    assert _same_bits(alone, got[3]) and _same_bits(got[3][:K], got[2][:K]) and _same_bits(got[3][K], got[1][K])
    return got[3]


# ceil(log2 K) bits of the stable column sort: 1, 1, 2, 2, 3, 4, 5, 5, 6, 8, 9
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 16, 17, 32, 33, 256, 257])
def test_spearman_at_every_width_of_the_column_key(K, dtype):
    n = 37
    p, t = R.pair(n, K, dtype)
    want = _rho3(n, K, dtype)
    if K >= 3:
        assert np.isnan(want[1])                                          # the constant column: raw 0 / 0 in the C entry
    _check_all_flags(p, t, want, f"ranks {n}x{K} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_spearman_tie_runs_at_the_column_boundaries(dtype):
    """metrics_ref.tie_pair: a run that ends one column's sorted segment and an equal-valued run that starts the next, in both
    matrices; a constant, a 95 % zero and an all-distinct column; then the same with signed zeros mixed in."""
    from flashdeconv_amd.utils import metrics as M
    p, t, z = R.tie_pair(dtype)
    n, K = p.shape
    for a, b, name in ((p, t, "ties"), (t, p, "ties swapped"), (z, t, "signed zeros")):
        want = R.spearman_raw(a, b, 3)
        const = [k for k in range(K) if np.ptp(a[:, k]) == 0 or np.ptp(b[:, k]) == 0]
        assert const == [0] and np.flatnonzero(np.isnan(want)).tolist() == const
        _check_all_flags(a, b, want, f"{name} {n}x{K} {dtype}")
        per = M.compute_correlation(a, b, method="spearman", per_cell_type=True)      # through _safe: 0.0 for the constant column
        assert per[0] == 0.0 and _same_bits(per[1:], want[1:K])
        assert _same_bits(M.compute_correlation(a, b, method="spearman"), want[K])
    unsigned = np.abs(z)
    assert not _same_bits(unsigned, z) and np.array_equal(unsigned, z)
    assert _same_bits(R.spearman_raw(unsigned, t, 3), R.spearman_raw(z, t, 3))          # -0.0 ties with +0.0


def test_float32_denormals_rank_as_distinct_values():
    """0, 1e-45, 2e-45, 3e-45, 1e-40 and 1e-38 as float32: 1e-45 and 2e-45 both round to 2^-149, so these are five values, four
    of them denormal.  The radix sort keeps them apart and the run heads' compare must too: a flushed compare would see one
    run, a constant column and rho = NaN."""
    n, K = 42, 2
    rng = np.random.default_rng(45)
    vals = np.array([0, 1e-45, 2e-45, 3e-45, 1e-40, 1e-38], dtype=np.float32)
    assert len(np.unique(vals)) == 5 and np.all(vals[1:] < np.finfo(np.float32).tiny) and np.all(vals[1:] > 0)
    p, t = (a.copy() for a in R.pair(n, K, "float32"))
    p[:, 0] = rng.permutation(np.tile(vals, n // 6))
    t[:, 0] = p[rng.permutation(n), 0]
    t[:8, 0] = p[:8, 0]
    want = R.spearman_raw(p, t, 3)
    assert not np.isnan(want).any()
    flushed = [np.where(np.abs(a) < np.finfo(np.float32).tiny, np.float32(0), a) for a in (p, t)]
    assert np.isnan(R.spearman_raw(*flushed, 3)[0])
    _check_all_flags(p, t, want, "float32 denormals")
    stats = _evaluate(_on_device(p), _on_device(t), n, K)[0]
    R.check_stats(stats, R.reference(p, t, THR), "float32 denormals")
    assert stats[0, R.MAX_P] == float(vals[5]) and stats[0, R.SUM_P] > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_spearman_at_the_largest_exact_size(dtype):
    """n K = 150 000: N^3 = 3.4e15 < 2^53 = 9.0e15, the overall rank sums are still exact and rho bit for bit."""
    n, K = 3000, 50
    assert n * K == 150000 <= R.EXACT_N
    _check_all_flags(*R.pair(n, K, dtype), _rho3(n, K, dtype), f"ranks {n}x{K} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_spearman_with_the_row_chunks_at_their_cap(dtype):
    """40 961 x 129: the twice-ranks go through mx_centred at nbx = 1024 with empty trailing blocks.  Per column (N = 40 961) the
    sums are exact; the overall sums (N = 5.3e6, N^3 > 2^53) are not: atol 1e-12."""
    n, K = 40961, 129
    p, t = R.pair(n, K, dtype)
    assert n <= R.EXACT_N < n * K
    got = _spearman(_on_device(p), _on_device(t), n, K, 3)
    R.check_rho(got, _rho3(n, K, dtype), f"ranks {n}x{K} {dtype}", atol_rows=(K,))


# ------------------------------------------------------------------------------------------------ 4. row stride and routing
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,n", [(5, 300), (257, 33), (9, 228)])
def test_row_stride_changes_no_bit(K, n, dtype):
    p, t = R.jsd_pair(n, K, dtype)
    tight = None
    for ldp, ldq in ((K, K), (K + 3, K), (2 * K, 2 * K)):
        P, T = _on_device(p, ldp), _on_device(t, ldq)
        stats, rare, rho, jsd = _evaluate(P, T, n, K, ldp, ldq, flags=3, want_jsd=True)
        alone = _spearman(P, T, n, K, 3, ldp, ldq)
        if tight is None:
            tight = (stats, rare, rho, jsd)
            what = f"stride {n}x{K} {dtype}"
            R.check_stats(stats, R.reference(p, t, THR), what, jsd_sum_checked=True)
            R.check_rho(rho, R.spearman_raw(p, t, 3), what)
            R.check_jsd(jsd, stats[K, R.JSD_SUM], *R.jsd(p, t, 1e-10), K, what)
        assert _same_bits(stats, tight[0]), (ldp, ldq)
        assert rare.tolist() == tight[1].tolist()
        assert _same_bits(rho, tight[2]) and _same_bits(alone, tight[2]), (ldp, ldq)
        assert _same_bits(jsd, tight[3]), (ldp, ldq)


def _everything(M, p, t):
    """Every number the Python API makes of a pair, flat."""
    ev = M.evaluate_deconvolution(p, t)
    out = list(ev["overall"].values())
    for d in ev["per_cell_type"].values():
        out += list(d.values())
    for per in (False, True):
        out += list(np.atleast_1d(M.compute_rmse(p, t, per_cell_type=per))) + list(np.atleast_1d(M.compute_mae(p, t, per_cell_type=per)))
        for meth in ("pearson", "spearman"):
            out += list(np.atleast_1d(M.compute_correlation(p, t, method=meth, per_cell_type=per)))
    out += list(M.compute_rare_cell_detection(p, t))
    j = M.compute_jsd(p, t)
    out += list(j.cpu().numpy() if type(j).__module__.split(".")[0] == "torch" else j)
    return np.array(out, dtype=np.float64)


def test_python_routing_of_views_and_mixed_inputs():
    """Column slices and row-strided views go to the kernels where they lie (ld = stride(0)), a transposed view is copied, float32
    with float64 runs as float64, a host array is uploaded beside a device tensor: each equals the bits of the plain contiguous
    float64 host call on the same values."""
    import torch
    from flashdeconv_amd.utils import metrics as M
    n, K = 200, 6
    p, t = R.pair(n, K)
    base = _everything(M, p, t)
    assert not np.isnan(base).any()
    dev = lambda a: torch.from_numpy(np.array(a, order="C")).cuda()

    wide_p, wide_t = _on_device(p, K + 5), _on_device(t, 2 * K)
    sl = (wide_p[:, :K], wide_t[:, :K])
    assert sl[0].stride() == (K + 5, 1) and not sl[0].is_contiguous()
    assert _same_bits(_everything(M, *sl), base), "W[:, :K]"

    def every_other(a):
        buf = np.full((2 * n, K), np.nan)
        buf[::2] = a
        return dev(buf)[::2]
    eo = (every_other(p), every_other(t))
    assert eo[0].stride() == (2 * K, 1) and tuple(eo[0].shape) == (n, K)
    assert _same_bits(_everything(M, *eo), base), "X[::2]"

    tr = (dev(p.T).T, dev(t.T).T)
    assert tr[0].stride() == (1, n) and tuple(tr[0].shape) == (n, K)
    assert _same_bits(_everything(M, *tr), base), "transposed view"
    assert _same_bits(_everything(M, sl[0], tr[1]), base), "a slice beside a transposed view"

    assert _same_bits(_everything(M, p, dev(t)), base), "host pred, device true"
    assert _same_bits(_everything(M, dev(p), t), base), "device pred, host true"

    p32 = R.pair(n, K, "float32")[0]
    base32 = _everything(M, p32.astype(np.float64), t)
    assert not _same_bits(base32, base)
    assert _same_bits(_everything(M, p32, t), base32), "float32 host pred, float64 host true"
    assert _same_bits(_everything(M, dev(p32), dev(t)), base32), "float32 device pred, float64 device true"
    assert _same_bits(_everything(M, p32, dev(t)), base32), "float32 host pred, float64 device true"


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_argument_checks_refuse_before_anything_runs():
    """Every refusal is a non-zero code with a message, and leaves the outputs as they were."""
    import torch
    from flashdeconv_amd import _lib
    lib = _lib.load()
    n, K = 8, 4
    p, t = R.pair(n, K)
    P, T = _on_device(p), _on_device(t)
    pp, tp = ctypes.c_void_p(P.data_ptr()), ctypes.c_void_p(T.data_ptr())
    stats, rare, rho, jsd = _outputs(n, K, True)
    sp, rp, hp, jp = _lib.ptr_f64(stats), _lib.ptr_i64(rare), _lib.ptr_f64(rho), ctypes.c_void_p(jsd.data_ptr())
    F64 = _lib.FDX_F64

    def evaluate(n=n, K=K, ldp=K, ldq=K, code=F64, flags=3, P=pp, T=tp, sp=sp, hp=hp):
        return lib.fdx_metrics_evaluate_dev(P, T, code, n, K, ldp, ldq, THR, 1e-10, flags, jp, sp, rp, hp, _stream())

    def moments(n=n, K=K, ldp=K, ldq=K, code=F64, sp=sp):
        return lib.fdx_metrics_moments_dev(pp, tp, code, n, K, ldp, ldq, THR, 1e-10, jp, sp, rp, _stream())

    def spearman(n=n, K=K, ldp=K, ldq=K, code=F64, flags=3, hp=hp):
        return lib.fdx_metrics_spearman_dev(pp, tp, code, n, K, ldp, ldq, flags, hp, _stream())

    refused = []
    for entry in (evaluate, moments, spearman):
        refused += [(entry, dict(n=0), "bad shape"), (entry, dict(K=0), "bad shape"), (entry, dict(ldp=K - 1), "bad shape"),
                    (entry, dict(ldq=K - 1), "bad shape"), (entry, dict(code=2), "dtype"), (entry, dict(code=-1), "dtype"),
                    (entry, dict(n=2 ** 31, K=1, ldp=1, ldq=1), "2^31 - 1"), (entry, dict(n=2 ** 29, ldp=K, ldq=K), "2^31 - 1")]
    refused += [(evaluate, dict(flags=4), "unknown Spearman flags"), (evaluate, dict(flags=7), "unknown Spearman flags"),
                (spearman, dict(flags=4), "unknown Spearman flags"), (spearman, dict(flags=0), "select nothing"),
                (moments, dict(sp=None), "null stats_host"), (evaluate, dict(sp=None), "null output"),
                (evaluate, dict(hp=None), "null output"), (spearman, dict(hp=None), "null rho_host"),
                (evaluate, dict(P=None), "null matrix"), (evaluate, dict(T=None), "null matrix")]
    for entry, kw, text in refused:
        rc = entry(**kw)
        msg = (lib.fdx_last_error() or b"").decode()
        assert rc != 0, f"{entry.__name__}({kw}) was accepted"
        assert text in msg and f"fdx_metrics_{entry.__name__}_dev" in msg, f"{entry.__name__}({kw}): {msg!r}"
    torch.cuda.synchronize()
    assert np.all(stats == MARK) and np.all(rare == int(MARK)) and np.all(rho == MARK) and bool((jsd == MARK).all())
    assert evaluate(flags=0, hp=None) == 0                                # no Spearman asked for: rho_host may be null
    assert evaluate() == 0 and moments() == 0 and spearman() == 0          # and the entries still serve a good call
    R.check_stats(stats, R.reference(p, t, THR), "after the refusals", jsd_sum_checked=True)
    R.check_rho(rho, R.spearman_raw(p, t, 3), "after the refusals")
