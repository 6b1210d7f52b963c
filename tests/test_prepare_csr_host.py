"""The triplet reference of the CSR sketch -> H stage (tests/prepare_csr_ref.py) and the case table of
tests/test_gpu_prepare_csr.py, checked without a GPU.

What the GPU file relies on: on canonical matrices the reference over stored entries is test_gpu_prepare.reference on the
densified matrix and scipy's own evaluation of the original's rule (transform on `.data`, then csr @ Omega), both within the
float64 reference's own 4 units; with repeated columns in log mode it is NOT the densified evaluation (log1p of each stored
entry, not of their sum), by orders of magnitude above the bound - so the case can tell the two rules apart; the comparator of
the GPU tests fails, by at least 1e3 times the bound, on each fault a CSR kernel can plausibly have - an entry dropped, an entry
added to the neighbouring spot, a weight with the wrong sign, two columns of H swapped, a stale entry carried over from another
row; and every case of the table takes the branch it claims, by the answer of fdx_sketch_csr_path (the dispatch's own functions).
"""
import numpy as np
import pytest
from scipy import sparse

import prepare_csr_ref as cr
import test_gpu_prepare as tp

E64 = tp.E64


def _case(cid):
    return next(c for c in cr.CASES if c["id"] == cid)


def _ref(case, b, **over):
    a = dict(b, **over)
    return cr.triplet_reference(a["indptr"], a["indices"], a["data"], a["G_all"], a["gene_idx"], a["X"], a["bucket"], a["wy"], a["wx"],
                                case["d"], case["mode"], case["mode"], rows=a["row_map"])


def _dense_selected(b):
    n = len(b["indptr"]) - 1
    A = sparse.csr_matrix((b["data"].astype(np.float64), b["indices"], b["indptr"]), shape=(n, b["G_all"]))
    A.sum_duplicates()
    return A if b["gene_idx"] is None else A[:, b["gene_idx"]]


CANONICAL = ["inst-1x1-float64-raw", "inst-2x2-float32-log_cpm_sparse", "edge-d4-float32-log_cpm_sparse", "far-d254-K8-float64-raw",
             "sel-edges-p1-float32-log_cpm_sparse", "sel-all-p0-float64-raw", "form-stored_zeros-p1-float64-log_cpm_sparse",
             "form-mixed_counts-p0-float32-log_cpm_sparse", "pearson-p1-float64", "fused-n4097-float32-log_cpm_sparse"]


@pytest.mark.parametrize("cid", CANONICAL)
def test_on_canonical_rows_it_is_the_dense_reference_and_scipys_product(cid):
    case = _case(cid)
    b = cr.build_case(case)
    d, mode = case["d"], case["mode"]
    got = _ref(case, b)
    A = _dense_selected(b)
    want = tp.reference(A.toarray(), b["X"], b["bucket"], b["wy"], b["wx"], d, mode, mode)
    for key, mag in (("H", "M"), ("XtX", "Mxx")):
        assert np.all(np.abs(got[key] - want[key]) <= 4 * E64 * want[mag]), (cid, key)
    assert np.array_equal(got["M"] > 0, want["M"] > 0)
    assert abs(got["YtY"] - want["YtY"]) <= 4 * E64 * want["Myy"]
    assert got["occ_y"] <= want["occ"] and got["addends_y"] <= b["G"]       # canonical rows: the data terms never exceed the dense ones
    # the original's rule in scipy's own words: deconv.py:181-188 on .data, sketching.py:194-199 as a sparse product
    T = sparse.csr_matrix(A, dtype=np.float64, copy=True)
    T.sort_indices()
    if mode != cr.RAW:
        lib = np.asarray(A.sum(axis=1)).ravel()
        lib[lib == 0.0] = 1.0
        T.data = np.log1p(T.data / np.repeat(lib, np.diff(T.indptr)) * 1e4)
    Omega = sparse.csr_matrix((b["wy"], (np.arange(b["G"]), b["bucket"])), shape=(b["G"], d))
    Sy = np.asarray((T @ Omega).todense())
    Tx = tp.transform(b["X"], mode)
    H = tp.sketch(Tx, b["bucket"], b["wx"], d) @ Sy.T
    assert np.all(np.abs(got["H"] - H) <= 4 * E64 * want["M"]), cid


@pytest.mark.parametrize("dtype", [cr.F32, cr.F64])
@pytest.mark.parametrize("path", [0, 1])
def test_repeated_columns_in_log_mode_are_not_the_densified_matrix(path, dtype):
    case = _case(f"form-repeated-p{path}-{dtype}-{cr.LOG}")
    b = cr.build_case(case)
    got = _ref(case, b)
    want = tp.reference(_dense_selected(b).toarray(), b["X"], b["bucket"], b["wy"], b["wx"], case["d"], case["mode"], case["mode"])
    c_h = tp.bounds(got, case["n"], b["G"], case["d"], case["mode"], case["mode"], False)[0]
    excess = np.abs(got["H"] - want["H"]) / (c_h * E64 * np.where(got["M"] > 0, got["M"], 1.0))
    rows = np.flatnonzero((excess > 1.0).any(axis=0))
    print(f"repeated columns, path {path} {dtype}: densified rule off by {excess.max():.3g} bounds in spots {rows}")
    # spots 3 and 7 repeat a selected gene; spot 9 repeats an unselected one, which changes nothing under either rule
    assert set(rows) == {3, 7} and excess[:, [3, 7]].max(axis=0).min() >= 1e3
    # ... and in raw mode the two rules are one: the case then checks the atomics alone
    case = _case(f"form-repeated-p{path}-{dtype}-{cr.RAW}")
    b = cr.build_case(case)
    got = _ref(case, b)
    want = tp.reference(_dense_selected(b).toarray(), b["X"], b["bucket"], b["wy"], b["wx"], case["d"], cr.RAW, cr.RAW)
    assert np.all(np.abs(got["H"] - want["H"]) <= 4 * E64 * want["M"])
    assert got["occ_y"] >= 5


# ---------------------------------------------------------------------------------------------- planted faults
def _as_run(ref, n):
    H = np.full((ref["H"].shape[0], n + 5), tp.SENTINEL)
    H[:, :n] = ref["H"]
    return dict(H=H, XtX=ref["XtX"].copy(), XtX_host=ref["XtX"].copy(), YtY=ref["YtY"])


def _drop_entry(b, row):
    q = b["indptr"][row] + np.flatnonzero(cr.selection_map(b["G_all"], b["gene_idx"], b["G"])[b["indices"][b["indptr"][row]:b["indptr"][row + 1]]] >= 0)[0]
    ptr = b["indptr"].copy()
    ptr[row + 1:] -= 1
    return dict(indptr=ptr, indices=np.delete(b["indices"], q), data=np.delete(b["data"], q))


def _add_entry(b, row, col, val):
    q = b["indptr"][row + 1]
    ptr = b["indptr"].copy()
    ptr[row + 1:] += 1
    return dict(indptr=ptr, indices=np.insert(b["indices"], q, col), data=np.insert(b["data"], q, val))


def _first_selected(b, row):
    s = slice(b["indptr"][row], b["indptr"][row + 1])
    k = np.flatnonzero(cr.selection_map(b["G_all"], b["gene_idx"], b["G"])[b["indices"][s]] >= 0)[0]
    return int(b["indices"][s][k]), b["data"][s][k]


FAULTS = ("one dropped entry", "one entry added to the neighbouring spot", "one weight with the wrong sign", "two columns of H swapped",
          "one stale entry carried from another row")


@pytest.mark.parametrize("fault", FAULTS)
@pytest.mark.parametrize("cid", ["inst-1x1-float64-raw", "inst-1x2-float32-log_cpm_sparse", "far-d254-K8-float32-log_cpm_sparse"])
def test_the_comparator_fails_on_planted_faults(cid, fault):
    case = _case(cid)
    b = cr.build_case(case)
    n, d, mode = case["n"], case["d"], case["mode"]
    ref = _ref(case, b)
    tp.compare(_as_run(ref, n), ref, n, b["G"], d, mode, mode, False, "host")      # the comparator passes what is right
    row = 20 + int(np.flatnonzero(cr.row_lengths(b)[1][20:] >= 2)[0])       # a short row with selected entries
    if fault == "one dropped entry":
        bad = _ref(case, b, **_drop_entry(b, row))
    elif fault == "one entry added to the neighbouring spot":
        bad = _ref(case, b, **_add_entry(b, row + 1, *_first_selected(b, row)))
    elif fault == "one weight with the wrong sign":
        j = int(cr.selection_map(b["G_all"], b["gene_idx"], b["G"])[_first_selected(b, row)[0]])
        wy = b["wy"].copy()
        wy[j] = -wy[j]
        bad = _ref(case, b, wy=wy, wx=b["wx"])
    elif fault == "two columns of H swapped":
        bad = dict(ref, H=ref["H"].copy())
        bad["H"][:, [row, row + 1]] = ref["H"][:, [row + 1, row]]
    else:                                            # the long row's last register slot left in the next row's (an empty row's) place
        assert b["indptr"][8] - b["indptr"][7] == cr.LONG and b["indptr"][9] == b["indptr"][8]
        k = np.flatnonzero(cr.selection_map(b["G_all"], b["gene_idx"], b["G"])[b["indices"][b["indptr"][7]:b["indptr"][8]]] >= 0)[-1]
        col, val = b["indices"][b["indptr"][7] + k], b["data"][b["indptr"][7] + k]
        bad = _ref(case, b, **_add_entry(b, 8, col, val))
    c_h = tp.bounds(ref, n, b["G"], d, mode, mode, False)[0]
    M, err = ref["M"], np.abs(bad["H"] - ref["H"])
    with np.errstate(all="ignore"):               # (an empty row's magnitude sums are zero: any error there is beyond every bound)
        excess = float(np.where(err > 0, err / (c_h * E64 * M), 0.0).max())
    print(f"{cid}: {fault}: {excess:.3g} times the bound")
    assert excess >= 1e3
    with pytest.raises(AssertionError):
        tp.compare(_as_run(bad, n), ref, n, b["G"], d, mode, mode, False, "host")


# ---------------------------------------------------------------------------------------------- what the cases claim
def test_the_case_table_lists_what_the_kernels_can_get_wrong():
    cs = cr.CASES
    fused = [c for c in cs if c["path"] == 1]
    assert {(c["NB"], c["TT"]) for c in fused} == {(1, 1), (1, 2), (1, 3), (1, 4), (2, 1), (2, 2), (3, 1), (4, 1)}
    for pair in {(c["NB"], c["TT"]) for c in fused}:
        assert {(c["dtype"], c["mode"]) for c in fused if (c["NB"], c["TT"]) == pair and c["family"] == "instantiations"} == \
            {(t, m) for t in (cr.F32, cr.F64) for m in (cr.RAW, cr.LOG)}
    for path in (0, 1):
        assert {c["trips"] for c in cs if c["path"] == path and c["family"].endswith("trips")} == {1, 2, 3}
        assert {c["rowmap"] for c in cs if c["path"] == path} >= {"perm", "subset", "identity"}
    assert {c["n_sel"] for c in cs if c["path"] == 1} >= {65535} and {c["n_sel"] for c in cs if c["path"] == 0} >= {65536}
    assert any(c["chunks"] == 2 for c in cs)
    assert any(c["d"] % 256 for c in fused)


@pytest.mark.parametrize("case", cr.CASES, ids=[c["id"] for c in cr.CASES])
def test_every_gpu_case_takes_the_branch_it_claims(case, monkeypatch):
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    b = cr.build_case(case)
    n_rows = b["n_rows"]
    path, dims = cr.csr_path(case["dtype"], case["G_all"], b["G"], case["d"], case["K"], case["mode"])
    assert path == case["path"], (path, dims)
    assert dims["lds"] <= 160 * 1024, dims
    lens, sel_lens = cr.row_lengths(b)
    if b["row_map"] is not None:
        lens, sel_lens = lens[b["row_map"]], sel_lens[b["row_map"]]
    if path == 1:
        assert (dims["NB"], dims["TT"]) == (case["NB"], case["TT"]), dims
        assert dims["spots_per_trip"] == 4096 and -(-n_rows // dims["spots_per_trip"]) == case["trips"], dims
        assert (lens.max() > dims["NE"] * 64) == case["long"], (lens.max(), dims)
        if case["overflow"]:
            assert sel_lens.max() > dims["cap"]
            over = np.flatnonzero((sel_lens > dims["cap"]) & (lens <= dims["NE"] * 64))     # overflows from the registers alone
            assert len(over) and np.any((over // 4096) == 1), over
        assert 0 < dims["NE1"] < dims["NE"] and dims["cap"] >= 64 and dims["cap"] % 64 == 0
    else:
        launch = min(n_rows, dims["chunk_rows"])
        assert -(-launch // dims["rows_per_trip"]) == case["trips"], dims
        assert -(-n_rows // dims["chunk_rows"]) == case["chunks"], dims
        assert dims["rows_per_trip"] == dims["waves"] * 4096
    if case["place"] in ("fused_successions", "scatter_successions"):
        step = dims["spots_per_trip"] if path == 1 else dims["rows_per_trip"]
        a, z = (0, 15) if path == 1 else (0, 5)
        assert [int(lens[a + t * step]) for t in range(3)] == [cr.LONG, 0, 70]
        assert [int(lens[z + t * step]) for t in range(3)] == [70, 0, cr.LONG]
        ragged = n_rows - 1 if path == 0 else n_rows - 4
        assert lens[ragged] > 0 and sel_lens[ragged] == 0
    if case["place"] == "long_and_empty":
        assert lens[7] == cr.LONG and lens[8] == 0
    if case["place"] == "last_columns":
        col2j = cr.selection_map(b["G_all"], b["gene_idx"], b["G"])
        assert col2j[b["indices"]].max() == b["G"] - 1 == case["n_sel"] - 1
    if case["form"] in ("descending", "shuffled"):
        rows_sorted = [np.all(np.diff(b["indices"][b["indptr"][r]:b["indptr"][r + 1]]) > 0) for r in range(case["n"])]
        assert not all(rows_sorted)
    if case["sel"] == "edges":
        assert case["G_all"] % 32 != 0 and set([0, 31, 32, 63, case["G_all"] - 1]) <= set(b["gene_idx"])
    # every stored column is a column of the matrix: nothing a kernel indexes with is out of range
    assert b["indices"].min() >= 0 and b["indices"].max() < case["G_all"]
    assert b["row_map"] is None or (b["row_map"].min() >= 0 and b["row_map"].max() < case["n"])


def test_the_query_follows_the_keep_buffer_switch_and_the_selected_count(monkeypatch):
    path, dims = cr.csr_path(cr.F32, 2000, 1000, 1024, 8, cr.LOG)
    assert path == 1 and 64 < dims["cap"] < 1024, dims            # d = 1024: the natural buffer is small
    natural = dims["cap"]
    monkeypatch.setenv("FDX_CSR_KEEP_CAP", "64")
    assert cr.csr_path(cr.F32, 2000, 1000, 1024, 8, cr.LOG)[1]["cap"] == 64
    monkeypatch.setenv("FDX_CSR_KEEP_CAP", "100000")
    assert cr.csr_path(cr.F32, 2000, 1000, 1024, 8, cr.LOG)[1]["cap"] == natural
    monkeypatch.delenv("FDX_CSR_KEEP_CAP")
    assert cr.csr_path(cr.F64, 2000, 1000, 1024, 8, cr.LOG)[1]["cap"] < natural      # 8-byte values: fewer entries fit
    # ranks are 16-bit: one selected gene more than 65535 and the scatter kernel takes the matrix
    assert cr.csr_path(cr.F32, 70000, 65535, 64, 4, cr.RAW)[0] == 1
    assert cr.csr_path(cr.F32, 70000, 65536, 64, 4, cr.RAW)[0] == 0
    small = cr.csr_path(cr.F32, 900, 500, 256, 8, cr.LOG)[1]
    assert small["sel_in_lds"] == 1 and (small["NE"], small["NE1"]) == (24, 12)
    assert [cr.csr_path(cr.F64, 900, 500, 256, K, cr.LOG)[1][k] for K in (32, 33) for k in ("NE", "NE1")] == [16, 6, 16, 8]
