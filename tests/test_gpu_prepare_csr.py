"""The two CSR sketch -> H kernels (csrc/csr_kernels.cpp: sketch_csr_contract_kernel, and sketch_csr_kernel + the contraction)
PER ELEMENT through fdx_prepare_csr_ex_dev, beyond one trip through their grid-stride loops: every column of H, XtX and YtY
against the float64 reference over the stored entries (tests/prepare_csr_ref.py), H prefilled with a sentinel at
ldh = n_rows + 5.  Every case first asserts what fdx_sketch_csr_path answers for it; tests/test_prepare_csr_host.py has already
checked, without a GPU, that each case reaches the branch it was written for.

The cases (prepare_csr_ref.CASES):
    instantiations    all eight (NB, TT) pairs of the fused kernel x {float32, float64} x {raw, log_cpm_sparse}, d no multiple of
                      256, K no multiple of 16, a row above NE x 64 stored entries followed by an empty row;
    boundaries        d = 4, 252, 260, 1020, 1024 at K = 8 and K = 1, 16, 17, 32, 33, 48, 49, 64 at d = 256 (fused); d = 1028,
                      d = 254, K = 33 at d = 512 and K = 65 (scatter kernel + contraction);
    fused trips       n = 1, 15, 16, 17, 4096, 4097 and 8192 + 16 + 5 (three trips of workgroup 0, a ragged last group of 5) at
                      d = 1024; in the three-trip case, under FDX_CSR_KEEP_CAP=64: in wave 0 a row above NE x 64, then an empty
                      row, then a row of 70; in wave 15 the reverse; a row overflowing the keep buffer in trip 2; a row with
                      nothing selected in the ragged group;
    scatter trips     n = 1, 3, 4, 5, 16384, 16385, 2 * 16384 + 7 at d = 6 with the same successions per wave;
    chunk seam        n = 2^18 + 6: the second chunk of queue_rows_to_h (row0, H + r0, row_sq + r0);
    row map           a permutation of all rows at a two-trip n, 700 of 1000 rows scrambled (the other rows hold 1e30), and the
                      identity map against the same reference as NULL - both paths;
    row forms         descending and shuffled columns, a selected gene stored 2x and 5x and an unselected one 3x (log mode: log1p
                      of each stored entry), stored zeros, a row of stored zeros only, counts of 63, 64, 70, 640 beside small
                      counts and non-integers, negative values in raw (every raw case has them), a NaN and an Inf entry - both
                      paths, both modes, both dtypes; the log cases once more under FDX_NO_LOG_TABLE=1;
    selection         selected columns 0, 31, 32, 63 and G_all - 1 with G_all = 1003; one selected gene; all selected with a NULL
                      gene_idx; 65535 selected genes of 65600 (fused, the highest rank is 65534) and 65536 (16-bit ranks cannot
                      hold them: the scatter kernel; before csr_contract_ok looked at the count this shape was refused);
    pearson weights   other weights on the signature side, raw.

The bound is test_gpu_prepare.py's, its spot-side data terms taken from the stored entries (prepare_csr_ref.py); nothing in it
is fitted to the device's output.  Largest observed err / (2^-53 * M) per family on an MI355X (recorded here, NOT used as a
limit), the range of the derived c, and the largest share of its own c that a case used:
    family                              H: observed   c               share  | YtY: observed   c                share
    fused, instantiations                  3.894      225 .. 2943     0.014  |    1.736        275 .. 2939      0.004
    fused, boundaries                      3.847      275 .. 2994     0.010  |    2.819        325 .. 2987      0.004
    fused, fused trips                     5.497      1035 .. 2909    0.004  |    9.046        1032 .. 10976    0.002
    fused, row map                         3.761      269 .. 797      0.012  |    2.821        402 .. 4422      0.004
    fused, row forms                       3.758      267 .. 696      0.009  |    2.780        303 .. 345       0.009
    fused, selection                       3.660      263 .. 66738    0.008  |    1.210        115 .. 343       0.006
    fused, pearson weights                 2.411      269 .. 272      0.009  |    1.886        395              0.005
    scatter, boundaries                    4.813      279 .. 3008     0.006  |    0.866        329 .. 3009      0.001
    scatter, scatter trips                 1.792      191 .. 2229     0.009  |    1.726        14 .. 34850      0.084
    scatter, chunk seam                    1.182      80              0.015  |    2.595        262171           0.000
    scatter, row map                       1.553      104 .. 637      0.012  |    1.834        154 .. 16452     0.006
    scatter, row forms                     1.902      85 .. 527       0.022  |    2.680        57 .. 95         0.044
    scatter, selection                     1.803      13 .. 66751     0.027  |    1.550        53 .. 189        0.029
    scatter, pearson weights               1.496      103 .. 109      0.014  |    0.000        149 .. 151       0.000
(the c of 66738 and 66751: the signature side's row sum has 65535 and 65536 addends in log mode.)  The file takes 2 s on that
machine (195 cases); the 2^18 + 6 case, the largest, 0.1 s.

What the cases found.  The 65535 and 65536 selected-gene cases failed when they were written, twice over: the fused launch
refused 65536 selected genes although the scatter kernel serves them (csr_contract_ok did not look at the count), and the
SIGNATURE side refused either shape, because a dense row of more genes than LDS holds had no sketch kernel
(sketch_rows_stream_kernel, csrc/sketch_kernels.cpp, now takes such rows).  No case found a wrong number in either CSR kernel.
"""
import ctypes
import time

import numpy as np
import pytest
from scipy import sparse

import prepare_csr_ref as cr
import test_gpu_prepare as tp

pytestmark = pytest.mark.gpu

_t0 = [None]


@pytest.fixture(scope="module", autouse=True)
def _report_the_largest_ratios():
    _t0[0] = time.time()
    yield
    print(f"\n[test_gpu_prepare_csr] {time.time() - _t0[0]:.1f} s; largest err / (eps * M) per family (derived c: min .. max; largest share):")
    for fam in sorted(tp._worst):
        if fam.startswith("CSR"):
            r, lo, hi, part = tp._worst[fam]
            print(f"[test_gpu_prepare_csr]   {fam:<44s} {r:10.3f}   c = {lo:g} .. {hi:g}   {part:.4f}")


def _ids(cases):
    return [c["id"] for c in cases]


def _matrix(b):
    n = len(b["indptr"]) - 1
    return sparse.csr_matrix((b["data"], b["indices"], b["indptr"]), shape=(n, b["G_all"]))


def _run(case, b, row_map="case", n_rows=None):
    """One launch of the case as built: the rows uploaded as stored (unsorted, repeated), the case's row map unless another is given"""
    if isinstance(row_map, str):
        row_map, n_rows = b["row_map"], b["n_rows"]
    return tp.run_csr(_matrix(b), b["gene_idx"], b["G"], b["X"], b["bucket"], b["wy"], b["wx"], case["d"], case["mode"], n_rows + 5,
                      ex=(row_map, n_rows), sort=False)


def _reference(case, b, rows="case"):
    rows = b["row_map"] if isinstance(rows, str) else rows
    return cr.triplet_reference(b["indptr"], b["indices"], b["data"], b["G_all"], b["gene_idx"], b["X"], b["bucket"], b["wy"], b["wx"],
                                case["d"], case["mode"], case["mode"], rows=rows)


def _family(case):
    return ("CSR scatter", "CSR fused")[case["path"]] + ", " + case["family"]


def _assert_path(case, b):
    path, dims = cr.csr_path(case["dtype"], case["G_all"], b["G"], case["d"], case["K"], case["mode"])
    assert path == case["path"], (case["id"], path, dims)
    if path == 1:
        assert (dims["NB"], dims["TT"]) == (case["NB"], case["TT"]), dims
    return dims


def _check(case, monkeypatch, extra_env=()):
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    b = cr.build_case(case)
    dims = _assert_path(case, b)
    ref = _reference(case, b)
    got = _run(case, b)
    tp.compare(got, ref, b["n_rows"], b["G"], case["d"], case["mode"], case["mode"], False, _family(case), case["bad_spots"])
    for name in extra_env:                            # the same launch under a switch, against the same reference
        monkeypatch.setenv(name, "1")
        again = _run(case, b)
        monkeypatch.delenv(name)
        tp.compare(again, ref, b["n_rows"], b["G"], case["d"], case["mode"], case["mode"], False, _family(case), case["bad_spots"])
    return b, ref, got, dims


@pytest.mark.parametrize("case", cr.cases_of("instantiations"), ids=_ids(cr.cases_of("instantiations")))
def test_every_fused_instantiation(case, monkeypatch):
    """(NB, TT) = blocks of 256 buckets x type tiles of 16: eight kernels per dtype and mode; d = 256 NB - 56 leaves the last
    block's upper lanes outside the sketch (the c0 < d guards), the long row continues past the registers, the empty row follows
    it in the next wave."""
    b, ref, got, dims = _check(case, monkeypatch)
    assert np.all(got["H"][:, 8] == 0.0)              # the empty row behind the long one


@pytest.mark.parametrize("case", cr.cases_of("boundaries"), ids=_ids(cr.cases_of("boundaries")))
def test_both_sides_of_what_the_fused_kernel_takes(case, monkeypatch):
    _check(case, monkeypatch)


@pytest.mark.parametrize("case", cr.cases_of("fused trips"), ids=_ids(cr.cases_of("fused trips")))
def test_trips_of_the_fused_kernel(case, monkeypatch):
    """A workgroup's second and third group: the row fetched in two parts around the contraction, the hand-over of the extents,
    the extents two groups ahead, the accumulator rows after they served as the reduction buffer."""
    b, ref, got, dims = _check(case, monkeypatch)
    if case["trips"] == 3:
        assert dims["cap"] == 64
        for p in (4096, 4096 + 15, 8192 + 16 + 1):    # the empty rows behind the long and the short one; the row with nothing selected
            assert np.all(got["H"][:, p] == 0.0), p


@pytest.mark.parametrize("case", cr.cases_of("scatter trips"), ids=_ids(cr.cases_of("scatter trips")))
def test_trips_of_the_scatter_kernel(case, monkeypatch):
    """A wave's second and third row: the extents fetched a trip ahead, the accumulators zeroed behind the previous row's reads."""
    b, ref, got, dims = _check(case, monkeypatch)
    if case["trips"] == 3:
        for p in (16384, 16384 + 5, 32767, 32768 + 6):
            assert np.all(got["H"][:, p] == 0.0), p


@pytest.mark.parametrize("case", cr.cases_of("chunk seam"), ids=_ids(cr.cases_of("chunk seam")))
def test_the_second_chunk_of_the_two_kernel_path(case, monkeypatch):
    b, ref, got, dims = _check(case, monkeypatch)
    seam = dims["chunk_rows"]
    assert b["n_rows"] == seam + 6
    assert np.abs(got["H"][:, seam - 3:seam + 6]).max() > 0.0     # (compared above like every column: the rows on both sides hold something)


@pytest.mark.parametrize("case", cr.cases_of("row map"), ids=_ids(cr.cases_of("row map")))
def test_a_row_map(case, monkeypatch):
    """Column p of H is row row_map[p]: the solver order of a fit (a permutation), the subset of a shard (rows that are not listed
    hold 1e30 and would blow the bound if read).  The identity map and NULL meet the same reference - not the same bits: the order
    of the LDS adds within a bucket is the hardware's."""
    b, ref, got, dims = _check(case, monkeypatch)
    if case["rowmap"] == "identity":
        plain = _run(case, b, row_map=None, n_rows=case["n"])
        tp.compare(plain, ref, case["n"], b["G"], case["d"], case["mode"], case["mode"], False, _family(case))
        lead = _run(case, b, row_map=None, n_rows=137)            # NULL with fewer rows than the matrix has: its leading rows
        tp.compare(lead, _reference(case, b, rows=np.arange(137)), 137, b["G"], case["d"], case["mode"], case["mode"], False, _family(case))
        old = tp.run_csr(_matrix(b), b["gene_idx"], b["G"], b["X"], b["bucket"], b["wy"], b["wx"], case["d"], case["mode"], case["n"] + 5)
        tp.compare(old, ref, case["n"], b["G"], case["d"], case["mode"], case["mode"], False, _family(case))   # the forwarder


@pytest.mark.parametrize("case", cr.cases_of("row forms"), ids=_ids(cr.cases_of("row forms")))
def test_row_forms(case, monkeypatch):
    """Rows scipy would not hand over: unsorted, repeated columns (the atomics; log mode: log1p of each stored entry), stored
    zeros, a library size of zero from stored zeros, table hits beside counts >= 64 and non-integers, non-finite entries that
    stay in their spots."""
    b, ref, got, dims = _check(case, monkeypatch, extra_env=("FDX_NO_LOG_TABLE",) if case["mode"] == cr.LOG else ())
    if case["form"] == "stored_zeros":
        assert np.all(got["H"][:, 11] == 0.0)
    if case["form"] == "nonfinite":
        assert not np.isfinite(got["YtY"]) and not np.isfinite(got["H"][:, list(case["bad_spots"])]).any()


@pytest.mark.parametrize("case", cr.cases_of("selection"), ids=_ids(cr.cases_of("selection")))
def test_selection_edges(case, monkeypatch):
    _check(case, monkeypatch)


@pytest.mark.parametrize("case", cr.cases_of("pearson weights"), ids=_ids(cr.cases_of("pearson weights")))
def test_pearson_style_weights(case, monkeypatch):
    _check(case, monkeypatch)


def test_every_case_is_run():
    used = {"instantiations", "boundaries", "fused trips", "scatter trips", "chunk seam", "row map", "row forms", "selection",
            "pearson weights"}
    assert {c["family"] for c in cr.CASES} == used


def test_refusals_of_the_row_map_entry_and_of_the_query():
    from flashdeconv_amd import _lib
    lib = _lib.load()
    case = next(c for c in cr.CASES if c["id"] == "map-identity-p1-float32-log_cpm_sparse")
    b = cr.build_case(case)
    n, d = case["n"], case["d"]

    def run(**kw):
        a = dict(row_map=None, n_rows=n, ldh=n + 5, mode=case["mode"])
        a.update(kw)
        return tp.run_csr(_matrix(b), b["gene_idx"], b["G"], b["X"], b["bucket"], b["wy"], b["wx"], d, a["mode"], a["ldh"],
                          ex=(a["row_map"], a["n_rows"]), sort=False)

    with pytest.raises(_lib.FdxError, match="bad number of rows"):
        run(n_rows=-1, ldh=n)
    with pytest.raises(_lib.FdxError, match="bad number of rows"):
        run(n_rows=n + 1, ldh=n + 6)                  # more rows than the matrix has, and no map
    with pytest.raises(_lib.FdxError, match="leading dimension too small"):
        run(n_rows=n, ldh=n - 1)
    with pytest.raises(_lib.FdxError, match="mode_y must be"):
        run(mode=_lib.PRE_LOG_CPM)
    with pytest.raises(_lib.FdxError, match="mode_y must be"):
        run(mode=7)
    z = np.zeros(1)
    zi = np.zeros(1, dtype=np.int32)
    assert lib.fdx_prepare_csr_ex_dev(None, None, 1, _lib.ptr_f64(z), 1, _lib.ptr_i32(zi), _lib.ptr_f64(z), _lib.ptr_f64(z), 4, 0, 0, None, 1,
                                      None, None, None, None, 0, None) != 0
    # the query
    path, dims = ctypes.c_int32(-1), np.zeros(8, dtype=np.int32)
    ok = (_lib.FDX_F32, 900, 500, 256, 8, _lib.PRE_RAW)
    assert lib.fdx_sketch_csr_path(*ok, ctypes.byref(path), _lib.ptr_i32(dims)) == 0 and path.value == 1
    assert lib.fdx_sketch_csr_path(*ok, None, _lib.ptr_i32(dims)) != 0
    assert lib.fdx_sketch_csr_path(*ok, ctypes.byref(path), None) != 0
    for bad in ((5, 900, 500, 256, 8, 0), (0, 0, 500, 256, 8, 0), (0, 900, 0, 256, 8, 0), (0, 900, 901, 256, 8, 0), (0, 900, 500, 0, 8, 0),
                (0, 900, 500, 256, 0, 0), (0, 900, 500, 256, 8, 1), (0, 900, 500, 256, 8, 7)):
        assert lib.fdx_sketch_csr_path(*bad, ctypes.byref(path), _lib.ptr_i32(dims)) != 0, bad
