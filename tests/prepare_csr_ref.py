"""The sketch -> H stage of a CSR matrix evaluated on its STORED ENTRIES (indptr, indices, data) in float64 numpy, and the
case table of tests/test_gpu_prepare_csr.py as data.

The reference never densifies: a selection maps column -> gene j or none; the library size of a row is the sum of its selected
stored values (the sparse rule: 0 -> 1); the transform is applied to every stored entry (repeated columns: log1p of EACH stored
entry, as the original's `.data` rule does, not of their sum); np.add.at adds weight * value into S[row, bucket[j]], and the same
with absolute values into the magnitude matrix.  H, XtX, YtY and the magnitude sums M, Mxx, Myy are then formed exactly as
reference() of test_gpu_prepare.py forms them.  With a row map the reference is that of the listed rows in the listed order.

The bound is the one derived in test_gpu_prepare.py's docstring with its two spot-side data terms taken from the stored entries:
    occ_y       the most stored selected entries of ONE row that fall into one bucket (canonical rows: at most the bucket's
                occupancy; repeated columns raise it) - the addends of a bucket sum of that row;
    addends_y   the longest selected row (the addends of a library size), not G.
The signature side stays dense: bucket occupancy and G.

The cases (CASES) are data: what to build (build_case) and what each case CLAIMS about itself - the path and instantiation the
dispatch takes for it, that its longest row exceeds the register-resident part, that a row overflows the keep buffer, how many
trips a workgroup makes through the grid-stride loop.  tests/test_prepare_csr_host.py checks every claim against
fdx_sketch_csr_path without a device; the GPU file asserts the path again and compares every column of H.
"""
import numpy as np

from test_gpu_prepare import csr_sketch_path, sketch, transform

F32, F64 = "float32", "float64"
RAW, LOG = "raw", "log_cpm_sparse"


# ---------------------------------------------------------------------------------------------- the reference
def selection_map(G_all, gene_idx, G):
    col2j = np.full(G_all, -1, dtype=np.int64)
    col2j[np.arange(G) if gene_idx is None else np.asarray(gene_idx, dtype=np.int64)] = np.arange(G)
    return col2j


def listed_entries(indptr, rows):
    """(entry index, output position) of every stored entry of the listed rows, in the listed order"""
    indptr = np.asarray(indptr, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.int64)
    lens = indptr[rows + 1] - indptr[rows]
    pos = np.repeat(np.arange(len(rows)), lens)
    start = np.concatenate(([0], np.cumsum(lens)))[:-1]
    e = indptr[rows][pos] + (np.arange(int(lens.sum())) - start[pos])
    return e, pos


def sketch_entries(indptr, indices, data, G_all, gene_idx, bucket, w, d, mode, rows=None):
    """S, |S| magnitudes, occ_y and addends_y of the listed rows from the stored entries"""
    n = len(indptr) - 1
    rows = np.arange(n) if rows is None else np.asarray(rows)
    G = len(bucket)
    e, pos = listed_entries(indptr, rows)
    j = selection_map(G_all, gene_idx, G)[np.asarray(indices)[e]]
    sel = j >= 0
    e, pos, j = e[sel], pos[sel], j[sel]
    v = np.asarray(data)[e].astype(np.float64)
    with np.errstate(all="ignore"):
        if mode != RAW:
            lib = np.zeros(len(rows))
            np.add.at(lib, pos, v)
            lib = np.where(lib == 0.0, 1.0, lib)
            v = np.log1p(v / lib[pos] * 1e4)
        S, A = np.zeros((len(rows), d)), np.zeros((len(rows), d))
        b = np.asarray(bucket, dtype=np.int64)[j]
        np.add.at(S, (pos, b), v * w[j])
        np.add.at(A, (pos, b), np.abs(v) * np.abs(w[j]))
    occ_y = int(np.bincount(pos * d + b).max()) if len(pos) else 0
    addends_y = int(np.bincount(pos).max()) if len(pos) else 0
    return S, A, occ_y, addends_y


def triplet_reference(indptr, indices, data, G_all, gene_idx, X, bucket, wy, wx, d, mode_y, mode_x, rows=None):
    Sy, Ay, occ_y, addends_y = sketch_entries(indptr, indices, data, G_all, gene_idx, bucket, wy, d, mode_y, rows)
    Tx = transform(X, mode_x)
    Sx, Ax = sketch(Tx, bucket, wx, d), sketch(np.abs(Tx), bucket, np.abs(wx), d)
    occ = int(np.bincount(bucket, minlength=d).max())
    with np.errstate(all="ignore"):
        return dict(H=Sx @ Sy.T, M=Ax @ Ay.T, XtX=Sx @ Sx.T, Mxx=Ax @ Ax.T, YtY=float((Sy * Sy).sum()),
                    Myy=float((Ay * Ay).sum()), occ=occ, occ_y=occ_y, addends_y=addends_y)


# ---------------------------------------------------------------------------------------------- the path query
FUSED_DIMS = ("NB", "TT", "NE", "NE1", "cap", "sel_in_lds", "spots_per_trip", "lds")
SCATTER_DIMS = ("waves", "rows_per_trip", "chunk_rows", "lds")


def csr_path(dtype, G_all, n_sel, d, K, mode):
    """(path, dims by name) of fdx_sketch_csr_path: 0 = scatter kernel + contraction, 1 = fused; needs no device"""
    path, dims = csr_sketch_path(dtype, G_all, n_sel, d, K, mode)
    return path, dict(zip(FUSED_DIMS if path == 1 else SCATTER_DIMS, dims))


# ---------------------------------------------------------------------------------------------- matrices
def base_matrix(rs, n, G_all, max_len, mode, dtype):
    """Canonical short rows: 1..max_len distinct sorted columns each.  raw: signed reals; log: counts, every third row
    non-integers, a count of 70 now and then."""
    L = rs.randint(1, max_len + 1, size=n)
    C = rs.randint(0, G_all, size=(n, max_len))
    C[np.arange(max_len)[None, :] >= L[:, None]] = G_all
    C.sort(axis=1)
    ok = C < G_all
    ok[:, 1:] &= C[:, 1:] != C[:, :-1]
    lens = ok.sum(axis=1)
    indptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    indices = C[ok].astype(np.int32)
    row_of = np.repeat(np.arange(n), lens)
    if mode == RAW:
        data = rs.randn(len(indices)) * np.exp(rs.randn(len(indices)))
    else:
        data = 1.0 + rs.poisson(2.0, size=len(indices))
        data = np.where(row_of % 3 == 1, data * rs.uniform(0.3, 2.5, size=len(indices)), data)
        data[rs.rand(len(indices)) < 0.01] = 70.0
    return indptr, indices, data.astype(dtype)


def with_rows(indptr, indices, data, repl):
    """The matrix with the rows of `repl` {row: (columns, values)} replaced"""
    n, nnz = len(indptr) - 1, len(indices)
    lens = np.diff(indptr)
    for r, (c, v) in repl.items():
        assert 0 <= r < n and len(c) == len(v)
        lens[r] = len(c)
    ptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    idx, dat = np.empty(ptr[-1], dtype=np.int32), np.empty(ptr[-1], dtype=data.dtype)
    row_of = np.repeat(np.arange(n), np.diff(indptr))
    keep = np.ones(n, dtype=bool)
    keep[list(repl)] = False
    m = keep[row_of]
    dst = ptr[row_of[m]] + (np.arange(nnz)[m] - indptr[row_of[m]])
    idx[dst], dat[dst] = indices[m], data[m]
    for r, (c, v) in repl.items():
        idx[ptr[r]:ptr[r + 1]], dat[ptr[r]:ptr[r + 1]] = c, v
    return ptr, idx, dat


def row_of_length(rs, G_all, L, mode, dtype, cols=None):
    cols = np.sort(rs.choice(G_all, size=L, replace=False)) if cols is None else np.asarray(cols)
    vals = rs.randn(len(cols)) * 2.0 if mode == RAW else 1.0 + rs.poisson(3.0, size=len(cols))
    return cols.astype(np.int32), np.asarray(vals).astype(dtype)


LONG = 1700          # stored entries of a "long" row: above 24 x 64, the largest register-resident part
OVER = 400           # a row of which more than 64 entries are selected (half the columns are) and fewer than 1024 stored


def succession(rs, G_all, mode, dtype, gene_idx, spots, kinds):
    """{spot: row} for one wave's successive rows"""
    unsel = np.setdiff1d(np.arange(G_all), gene_idx)
    out = {}
    for p, kind in zip(spots, kinds):
        if kind == "long":
            out[p] = row_of_length(rs, G_all, LONG, mode, dtype)
        elif kind == "empty":
            out[p] = (np.zeros(0, np.int32), np.zeros(0, dtype))
        elif kind == "short":
            out[p] = row_of_length(rs, G_all, 70, mode, dtype)
        elif kind == "over":
            out[p] = row_of_length(rs, G_all, OVER, mode, dtype)
        elif kind == "unselected":
            out[p] = row_of_length(rs, G_all, 20, mode, dtype, cols=unsel[:: max(1, len(unsel) // 20)][:20])
        else:
            raise ValueError(kind)
    return out


# ---------------------------------------------------------------------------------------------- the case table
def _case(cid, family, n, G_all, n_sel, K, d, dtype, mode, path, **kw):
    c = dict(id=cid, family=family, n=n, G_all=G_all, n_sel=n_sel, K=K, d=d, dtype=dtype, mode=mode, path=path, max_len=12,
             place=None, form=None, rowmap=None, pearson=False, env={}, sel="random", long=False, overflow=False, trips=1,
             chunks=1, NB=None, TT=None, bad_spots=())
    c.update(kw)
    if path == 1:
        c["NB"], c["TT"] = (d + 255) // 256 if c["NB"] is None else c["NB"], (K + 15) // 16 if c["TT"] is None else c["TT"]
    return c


def _cases():
    out = []
    both = [(F32, RAW), (F32, LOG), (F64, RAW), (F64, LOG)]
    two = [(F32, LOG), (F64, RAW)]
    # every fused instantiation: d no multiple of 256, K no multiple of 16; one row above NE x 64 and one empty row
    for NB, TT in [(1, 1), (1, 2), (1, 3), (1, 4), (2, 1), (2, 2), (3, 1), (4, 1)]:
        for dtype, mode in both:
            out.append(_case(f"inst-{NB}x{TT}-{dtype}-{mode}", "instantiations", 50, 1800, 1000, 16 * TT - 3, 256 * NB - 56, dtype,
                             mode, 1, NB=NB, TT=TT, place="long_and_empty", long=True))
    # the boundaries of csr_contract_ok and their far sides
    for d in (4, 252, 260, 1020, 1024):
        for dtype, mode in two:
            out.append(_case(f"edge-d{d}-{dtype}-{mode}", "boundaries", 50, 1800, 1000, 8, d, dtype, mode, 1, place="long_and_empty",
                             long=True))
    for K in (1, 16, 17, 32, 33, 48, 49, 64):
        for dtype, mode in two:
            out.append(_case(f"edge-K{K}-{dtype}-{mode}", "boundaries", 50, 1800, 1000, K, 256, dtype, mode, 1, place="long_and_empty",
                             long=True))
    for d, K in ((1028, 8), (254, 8), (512, 33), (256, 65)):
        for dtype, mode in two:
            out.append(_case(f"far-d{d}-K{K}-{dtype}-{mode}", "boundaries", 50, 1800, 1000, K, d, dtype, mode, 0,
                             place="long_and_empty"))
    # trips of the fused kernel: 256 workgroups x 16 spots; d = 1024, where the keep buffer is smallest
    for n, trips in ((1, 1), (15, 1), (16, 1), (17, 1), (4096, 1), (4097, 2), (8192 + 16 + 5, 3)):
        for dtype, mode in ((F32, LOG), (F64, LOG), (F32, RAW)):
            three = trips == 3
            out.append(_case(f"fused-n{n}-{dtype}-{mode}", "fused trips", n, 2000, 1000, 8, 1024, dtype, mode, 1, trips=trips,
                             place="fused_successions" if three else None, long=three, overflow=three,
                             env={"FDX_CSR_KEEP_CAP": "64"} if three else {}))
    # trips of the scatter kernel: 4096 workgroups x 4 rows at d = 6
    for n, trips in ((1, 1), (3, 1), (4, 1), (5, 1), (16384, 1), (16385, 2), (2 * 16384 + 7, 3)):
        for dtype, mode in ((F32, LOG), (F64, LOG), (F32, RAW)):
            out.append(_case(f"scatter-n{n}-{dtype}-{mode}", "scatter trips", n, 2000, 1000, 8, 6, dtype, mode, 0, trips=trips,
                             place="scatter_successions" if trips == 3 else None))
    out.append(_case("chunk-seam", "chunk seam", 2 ** 18 + 6, 500, 300, 2, 6, F32, RAW, 0, max_len=5, trips=16, chunks=2))
    # the row map on both paths
    for path, d, n in ((1, 256, 4096 + 16 + 5), (0, 6, 16384 + 9)):
        for dtype, mode in two:
            out.append(_case(f"map-perm-p{path}-{dtype}-{mode}", "row map", n, 900, 500, 8, d, dtype, mode, path, rowmap="perm", trips=2))
            out.append(_case(f"map-subset-p{path}-{dtype}-{mode}", "row map", 1000, 900, 500, 8, d, dtype, mode, path, rowmap="subset"))
            out.append(_case(f"map-identity-p{path}-{dtype}-{mode}", "row map", 300, 900, 500, 8, d, dtype, mode, path, rowmap="identity"))
    # row forms
    for path, d in ((1, 256), (0, 6)):
        for dtype, mode in both:
            for form in ("descending", "shuffled", "repeated", "stored_zeros", "mixed_counts", "negative", "nonfinite"):
                if form == "negative" and mode != RAW:
                    continue
                out.append(_case(f"form-{form}-p{path}-{dtype}-{mode}", "row forms", 40, 700, 400, 8, d, dtype, mode, path, form=form,
                                 bad_spots=(4, 20) if form == "nonfinite" else ()))
    # selection edges
    for path, d in ((1, 256), (0, 6)):
        for dtype, mode in two:
            out.append(_case(f"sel-edges-p{path}-{dtype}-{mode}", "selection", 40, 1003, 300, 8, d, dtype, mode, path, sel="edges"))
            out.append(_case(f"sel-one-p{path}-{dtype}-{mode}", "selection", 40, 1003, 1, 8, d, dtype, mode, path, sel="one"))
            out.append(_case(f"sel-all-p{path}-{dtype}-{mode}", "selection", 40, 1003, None, 8, d, dtype, mode, path))
    for dtype, mode in two:
        out.append(_case(f"sel-65535-{dtype}-{mode}", "selection", 40, 65600, 65535, 4, 64, dtype, mode, 1, sel="most", place="last_columns"))
        out.append(_case(f"sel-65536-{dtype}-{mode}", "selection", 40, 65600, 65536, 4, 64, dtype, mode, 0, sel="most", place="last_columns"))
    # "pearson": raw, other weights on the signature side
    for path, d in ((1, 256), (0, 6)):
        for dtype in (F32, F64):
            out.append(_case(f"pearson-p{path}-{dtype}", "pearson weights", 130, 900, 500, 8, d, dtype, RAW, path, pearson=True))
    assert len({c["id"] for c in out}) == len(out)
    return out


CASES = _cases()


def cases_of(*families):
    return [c for c in CASES if c["family"] in families]


def case_seed(case):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(case["id"])) % (2 ** 31 - 1)


def build_case(case):
    """Everything a run of the case needs, as numpy arrays: the CSR triplet (not necessarily canonical), the selection, the
    signatures, Omega, the row map (None or int32) and the rows whose column of H is non-finite."""
    rs = np.random.RandomState(case_seed(case))
    n, G_all, K, d, mode = case["n"], case["G_all"], case["K"], case["d"], case["mode"]
    dtype = np.dtype(case["dtype"])
    # the selection
    if case["n_sel"] is None:
        gene_idx, G = None, G_all
    elif case["sel"] == "edges":
        must = np.array([0, 31, 32, 63, G_all - 1])
        rest = np.setdiff1d(np.arange(G_all), must)
        gene_idx = np.sort(np.concatenate((must, rs.choice(rest, size=case["n_sel"] - len(must), replace=False)))).astype(np.int32)
    elif case["sel"] == "one":
        gene_idx = np.array([37], dtype=np.int32)
    elif case["sel"] == "most":                      # all but a few columns spread over the matrix; the last column is selected
        drop = (np.arange(G_all - case["n_sel"]) * 1000 + 500)
        gene_idx = np.setdiff1d(np.arange(G_all), drop).astype(np.int32)
    else:
        gene_idx = np.sort(rs.choice(G_all, size=case["n_sel"], replace=False)).astype(np.int32)
    if gene_idx is not None:
        G = len(gene_idx)
        assert G == case["n_sel"]
    sel_cols = np.arange(G_all) if gene_idx is None else gene_idx
    indptr, indices, data = base_matrix(rs, n, G_all, case["max_len"], mode, dtype)
    repl = {}
    place = case["place"]
    if place == "long_and_empty":
        repl.update(succession(rs, G_all, mode, dtype, sel_cols, (7, 8), ("long", "empty")))
    elif place == "fused_successions":                # spot = 16 * group + wave; workgroup b takes groups b, b + 256, b + 512
        assert n == 8192 + 16 + 5
        repl.update(succession(rs, G_all, mode, dtype, sel_cols, (0, 4096, 8192), ("long", "empty", "short")))             # wave 0
        repl.update(succession(rs, G_all, mode, dtype, sel_cols, (15, 4096 + 15, 8192 + 15), ("short", "empty", "long")))  # wave 15
        repl.update(succession(rs, G_all, mode, dtype, sel_cols, (2 * 16 + 3, 4096 + 2 * 16 + 3), ("short", "over")))      # trip 2
        repl.update(succession(rs, G_all, mode, dtype, sel_cols, (8192 + 16 + 1,), ("unselected",)))                       # ragged group
    elif place == "scatter_successions":              # row p, p + 16384, p + 32768 are one wave's
        assert n == 2 * 16384 + 7
        repl.update(succession(rs, G_all, mode, dtype, sel_cols, (0, 16384, 32768), ("long", "empty", "short")))
        repl.update(succession(rs, G_all, mode, dtype, sel_cols, (5, 16384 + 5, 32768 + 5), ("short", "empty", "long")))
        repl.update(succession(rs, G_all, mode, dtype, sel_cols, (16383, 32767), ("long", "empty")))
        repl.update(succession(rs, G_all, mode, dtype, sel_cols, (32768 + 6,), ("unselected",)))
    elif place == "last_columns":                     # entries on the last selected columns: the highest ranks
        for r in range(0, n, 3):
            repl[r] = row_of_length(rs, G_all, 30, mode, dtype, cols=sel_cols[len(sel_cols) - 30 - r:len(sel_cols) - r])
        repl[1] = row_of_length(rs, G_all, 3, mode, dtype, cols=[sel_cols[0], sel_cols[-2], sel_cols[-1]])
    if case["sel"] == "edges":
        repl[2] = row_of_length(rs, G_all, 5, mode, dtype, cols=[0, 31, 32, 63, G_all - 1])
        repl[3] = row_of_length(rs, G_all, 6, mode, dtype, cols=[0, 1, 30, 33, 64, G_all - 1])
    if case["sel"] == "one":
        repl[2] = row_of_length(rs, G_all, 3, mode, dtype, cols=[36, 37, 38])
        repl[3] = row_of_length(rs, G_all, 1, mode, dtype, cols=[37])
        repl[5] = row_of_length(rs, G_all, 2, mode, dtype, cols=[5, 38])
    form = case["form"]
    sel_l = [int(c) for c in sel_cols]
    unsel = np.setdiff1d(np.arange(G_all), sel_cols)
    if form == "repeated":
        a, b, u = sel_l[10], sel_l[200], int(unsel[7])
        for r, extra in ((3, [a, a]), (7, [b] * 5), (9, [u] * 3 + [a])):
            c0, v0 = indices[indptr[r]:indptr[r + 1]], data[indptr[r]:indptr[r + 1]]
            c1, v1 = row_of_length(rs, G_all, len(extra), mode, dtype, cols=extra)
            repl[r] = (np.concatenate((c0[c0 != extra[0]], c1)), np.concatenate((v0[c0 != extra[0]], v1)))
    elif form == "stored_zeros":
        for r in (2, 5):
            c0, v0 = indices[indptr[r]:indptr[r + 1]], data[indptr[r]:indptr[r + 1]]
            extra = np.setdiff1d(np.array(sel_l[5:9] + [int(unsel[3])]), c0)
            repl[r] = (np.concatenate((c0, extra)).astype(np.int32), np.concatenate((v0, np.zeros(len(extra), dtype))))
        repl[11] = (np.array(sel_l[20:26], dtype=np.int32), np.zeros(6, dtype))       # library size 0 -> 1
    elif form == "mixed_counts":
        vals = np.array([1.0, 5.0, 63.0, 64.0, 70.0, 2.5, 0.25, 63.0, 17.0, 640.0])
        repl[6] = (np.array(sel_l[30:40], dtype=np.int32), vals.astype(dtype))
        repl[12] = (np.array(sel_l[30:34], dtype=np.int32), np.array([63.0, 1.0, 2.0, 3.0], dtype))
        repl[13] = (np.array(sel_l[30:34], dtype=np.int32), np.array([64.0, 1.0, 2.0, 3.0], dtype))
    elif form == "negative":
        for r in (2, 9):
            c0 = indices[indptr[r]:indptr[r + 1]]
            repl[r] = (c0, -(1.0 + np.arange(len(c0))).astype(dtype))
    elif form == "nonfinite":
        for r, bad in ((4, np.nan), (20, np.inf)):
            c0, v0 = indices[indptr[r]:indptr[r + 1]], data[indptr[r]:indptr[r + 1]]
            keep = c0 != sel_l[50]
            repl[r] = (np.concatenate((c0[keep], [sel_l[50]])).astype(np.int32), np.concatenate((v0[keep], np.array([bad], dtype))))
    # the row map
    row_map, n_rows = None, n
    if case["rowmap"] == "perm":
        row_map = rs.permutation(n).astype(np.int32)
    elif case["rowmap"] == "identity":
        row_map = np.arange(n, dtype=np.int32)
    elif case["rowmap"] == "subset":
        row_map = rs.permutation(n)[:700].astype(np.int32)
        n_rows = 700
        big = np.dtype(dtype).type(1e30)
        for r in np.setdiff1d(np.arange(n), row_map):          # rows nobody may read
            c0 = indices[indptr[r]:indptr[r + 1]]
            repl[int(r)] = (c0, np.full(len(c0), big, dtype))
    if repl:
        indptr, indices, data = with_rows(indptr, indices, data, repl)
    if form in ("descending", "shuffled"):
        for r in range(n):
            s = slice(indptr[r], indptr[r + 1])
            o = np.arange(indptr[r + 1] - indptr[r])[::-1] if form == "descending" else rs.permutation(indptr[r + 1] - indptr[r])
            indices[s], data[s] = indices[s][o], data[s][o]
    X = np.ascontiguousarray(np.exp(rs.randn(K, G) * 0.5))
    bucket = rs.randint(0, d, size=G).astype(np.int32)
    sign = rs.choice([-1.0, 1.0], size=G)
    wy = sign * rs.uniform(0.5, 2.0, size=G)
    wx = sign * rs.uniform(0.5, 2.0, size=G) if case["pearson"] else wy
    return dict(indptr=indptr, indices=indices, data=data, G_all=G_all, gene_idx=gene_idx, G=G, X=X, bucket=bucket, wy=wy, wx=wx,
                row_map=row_map, n_rows=n_rows)


def row_lengths(b):
    """(stored entries, selected stored entries) per row of a built case"""
    col2j = selection_map(b["G_all"], b["gene_idx"], b["G"])
    n = len(b["indptr"]) - 1
    row_of = np.repeat(np.arange(n), np.diff(b["indptr"]))
    return np.diff(b["indptr"]), np.bincount(row_of[col2j[b["indices"]] >= 0], minlength=n)
