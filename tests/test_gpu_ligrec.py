"""-m gpu tests of the ligand-receptor test between spot groups (csrc/label_gene_kernels.cpp: fdx_label_gene_sums_dev / _csr_dev;
utils.ligrec, FlashDeconv.get_ligand_receptor, tl.deconvolve(ligrec_pairs=...)).

Reference (tests/ligrec_ref.py): u^r = Y[l^r == c].sum(0) on float64 with l^r = labels[permutation_indices(seed, r, n)], the
statistic with the same three operations, the accumulation in permutation order.

Exact cases use integer-valued Y: every sum is an exact integer far below 2^53 in any order, so u, null, nnz and label_counts must
equal the reference bit for bit and count_ge / count_le exactly (real ties occur and are asserted to: both >= and <= are
exercised); sum_d is held within (R + 2) 2^-52 sum|d| of the reference and sumsq_d within the same bound on sum d^2 - the rounding
bound of an R-term sum with room for a contracted square.  Continuous cases (gamma float32 values, 70 % zeros) hold u^r within
n 2^-53 sum_{i in c}|y|, the bound of any summation order, and compare the counts wherever the reference's |T^r - T| exceeds the
band this implies for T (twice the bound over the smaller n_c); the cases inside the band are at most 0.1 % of a test's.

Geometry crossed: one launcher shape for every C (B = 16 permutations, tiles of 16 genes, segments of 2,048 spots; LDS above
64 KiB from C = 33); n in {1, 2, 63, 64, 65, 257, 1000} and n = 4,500 (three segments, the last ragged); S in {1, 15, 16, 17, 40};
R around the group of 16, a capped batch of 24, the full chain of 64 groups (63 at C = 64) and the chain behind it."""
import functools

import numpy as np
import pytest
from scipy import sparse

import ligrec_ref as ref

pytestmark = pytest.mark.gpu

C_LIST = (1, 2, 16, 17, 32, 33, 64)
KINDS = ("random", "minus", "missing", "one", "none")
N_LIST = (1, 2, 63, 64, 65, 257, 1000, 4500)
EPS52, EPS53 = 2.0 ** -52, 2.0 ** -53


def _labels(n, C, kind, seed=0):
    """The label kinds of tests/test_gpu_nhood.py."""
    rs = np.random.RandomState(1000 * C + seed)
    if kind == "random":
        lab = rs.randint(0, C, n)
    elif kind == "minus":                                  # about 10 % left out
        lab = rs.randint(0, C, n)
        lab[rs.rand(n) < 0.1] = -1
    elif kind == "missing":                                # label C // 2 never occurs (C = 1: nobody is labelled)
        lab = rs.randint(0, C, n)
        lab[lab == C // 2] = (C // 2 + 1) % C if C > 1 else -1
    elif kind == "one":                                    # every spot in the last label
        lab = np.full(n, C - 1)
    else:                                                  # every spot left out
        lab = np.full(n, -1)
    return lab.astype(np.int64)


def _pairs(G, S, P=0, seed=0):
    """Pairs over S distinct columns of [0, G), drawn in no order: ligand == receptor, every column named, a duplicate pair, and
    - up to P pairs - the first column in many pairs."""
    rs = np.random.RandomState(seed)
    pool = rs.permutation(G)[:S]
    rows = [[pool[0], pool[0]]] + [[pool[s], pool[(s + 1) % S]] for s in range(S)]
    rows.append(rows[1])
    while len(rows) < P:
        rows.append([pool[0], pool[rs.randint(S)]] if len(rows) % 2 else [pool[rs.randint(S)], pool[0]])
    return np.array(rows, dtype=np.int64)


def _int_Y(n, G, seed=0, dtype=np.float32):
    return np.random.RandomState(seed).poisson(0.7, (n, G)).astype(dtype)


def _gamma_Y(n, G, seed=0):
    rs = np.random.RandomState(seed)
    return (rs.gamma(2.0, 1.5, (n, G)) * (rs.rand(n, G) >= 0.7)).astype(np.float32)


def _sums(Y, labels, pairs, C, **kw):
    from flashdeconv_amd.utils.ligrec import label_gene_sums
    return label_gene_sums(Y, labels, pairs, n_labels=C, **kw)


@functools.lru_cache(maxsize=None)
def _exact_case(n, C, S, P, R, seed=3, kind="minus"):
    """One integer-valued problem and its reference, computed once and shared (read-only)."""
    G = max(S + 3, 24)
    Y = _int_Y(n, G, seed)
    labels = _labels(n, C, kind)
    pairs = _pairs(G, S, P, seed)
    genes = ref.gene_list(pairs)
    Yg = ref.dense64(Y)[:, genes]
    counts = ref.label_counts(labels, C)
    u = ref.group_sums(Yg, labels, C)
    null = ref.null_sums(Yg, labels, C, seed, 0, R)
    T = ref.statistic_fast(u, counts, pairs, genes)
    Tr = np.stack([ref.statistic_fast(v, counts, pairs, genes) for v in null]) if R else np.zeros((0,) + T.shape)
    out = dict(Y=Y, labels=labels, pairs=pairs, genes=genes, counts=counts, u=u, nnz=ref.group_nnz(Yg, labels, C), null=null, T=T, Tr=Tr,
               seed=seed, C=C)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _check_observed(got, c, tag=None):
    assert got["u"].dtype == np.float64 and got["nnz"].dtype == np.int64 and got["label_counts"].dtype == np.int64, tag
    assert np.array_equal(got["genes"], c["genes"]), tag
    assert got["u"].shape == c["u"].shape and got["u"].tobytes() == c["u"].tobytes(), tag
    assert np.array_equal(got["nnz"], c["nnz"]) and np.array_equal(got["label_counts"], c["counts"]), tag
    assert got["n"] == c["Y"].shape[0], tag


def _check_null(got, c, R, tag=None):
    """The null bit for bit, the counts exactly, the sums within the rounding bound of an R-term sum."""
    assert got["null"].dtype == np.float64 and got["null"].shape == c["null"][:R].shape, tag
    bad = [r for r in range(R) if got["null"][r].tobytes() != c["null"][r].tobytes()]
    assert not bad, (tag, bad)
    ge, le, sd, sq, sa = ref.accumulate(c["Tr"][:R], c["T"])
    assert got["count_ge"].dtype == np.int64 and np.array_equal(got["count_ge"], ge) and np.array_equal(got["count_le"], le), tag
    assert np.all(np.abs(got["sum_d"] - sd) <= (R + 2) * EPS52 * sa), tag
    assert np.all(np.abs(got["sumsq_d"] - sq) <= (R + 2) * EPS52 * sq), tag
    return ge, le


# ---------------------------------------------------------------- 1. observed sums, every n, C and label kind
@pytest.mark.parametrize("n", N_LIST)
def test_observed_sums(n):
    for C in C_LIST:
        for kind in KINDS:
            c = _exact_case(n, C, 17, 0, 0, kind=kind)
            got = _sums(c["Y"], c["labels"], c["pairs"], C)
            tag = (n, C, kind)
            _check_observed(got, c, tag)
            if kind == "none":
                assert not got["u"].any() and not got["nnz"].any() and not got["label_counts"].any(), tag
            if kind == "one":
                assert got["u"][C - 1].tobytes() == ref.dense64(c["Y"])[:, c["genes"]].sum(axis=0).tobytes(), tag
            assert got["n_permutations"] == 0 and got["batch"] == 0 and "null" not in got, tag
            P = c["pairs"].shape[0]
            for k in ("count_ge", "count_le", "sum_d", "sumsq_d"):
                assert got[k].shape == (P, C, C) and not got[k].any(), (tag, k)


@pytest.mark.parametrize("S", [1, 15, 16, 17, 40])
def test_gene_counts_around_the_tile(S):
    for n, C in ((257, 3), (4500, 33)):
        c = _exact_case(n, C, S, 0, 18)
        got = _sums(c["Y"], c["labels"], c["pairs"], C, seed=c["seed"], n_permutations=18, return_null=True)
        _check_observed(got, c, (S, n, C))
        _check_null(got, c, 18, (S, n, C))


# ---------------------------------------------------------------- 2. the null, exact
@pytest.mark.parametrize("n,C", [(1000, 5), (65, 2)])
def test_null_exact_with_ties(n, C):
    """Two shapes with 8 genes, 24 pairs and 64 permutations in which exact ties between T^r and T occur, so >= and <= both count."""
    R = 64
    c = _exact_case(n, C, 8, 24, R)
    assert c["pairs"].shape == (24, 2) and c["genes"].shape == (8,)
    ties = int((c["Tr"] == c["T"]).sum())
    assert ties > 0 and ties < c["Tr"].size // 10, ties
    results = []
    for max_batch in (0, 1, 5, 24):
        got = _sums(c["Y"], c["labels"], c["pairs"], C, seed=c["seed"], n_permutations=R, max_batch=max_batch, return_null=True)
        assert got["batch"] == (R if max_batch == 0 else max_batch), (max_batch, got["batch"])
        _check_observed(got, c, max_batch)
        ge, le = _check_null(got, c, R, max_batch)
        assert int((ge + le).sum()) == c["Tr"].size + ties                 # a tie is counted on both sides
        results.append(got)
    for k in ("u", "null", "count_ge", "count_le", "sum_d", "sumsq_d"):      # max_batch moves no bit, the sums' included
        assert all(r[k].tobytes() == results[0][k].tobytes() for r in results), k
    # the edges of a group of 16 permutations and of a capped batch of 24
    for R2, max_batch in [(r, 0) for r in (1, 15, 16, 17, 31, 32, 33)] + [(23, 24), (24, 24), (25, 24)]:
        got = _sums(c["Y"], c["labels"], c["pairs"], C, seed=c["seed"], n_permutations=R2, max_batch=max_batch, return_null=True)
        assert got["batch"] == min(R2, max_batch or R2)
        _check_null(got, c, R2, (R2, max_batch))
    # a range split into two calls: the null bit for bit, the counts add exactly
    a = _sums(c["Y"], c["labels"], c["pairs"], C, seed=c["seed"], first_perm=0, n_permutations=27, return_null=True)
    b = _sums(c["Y"], c["labels"], c["pairs"], C, seed=c["seed"], first_perm=27, n_permutations=R - 27, return_null=True)
    one = results[0]
    assert np.concatenate([a["null"], b["null"]]).tobytes() == one["null"].tobytes()
    for k in ("count_ge", "count_le"):
        assert np.array_equal(a[k] + b[k], one[k]), k
    other = _sums(c["Y"], c["labels"], c["pairs"], C, seed=c["seed"] + 1, n_permutations=R, return_null=True)
    assert other["null"].tobytes() != one["null"].tobytes() and other["u"].tobytes() == one["u"].tobytes()


@pytest.mark.parametrize("C", C_LIST)
def test_null_exact_every_label_count(C):
    """Every C of the list (LDS from 2 KiB to 128 KiB) with several segments and a ragged last one, every label kind at n = 257."""
    R = 19
    c = _exact_case(4500, C, 17, 0, R)
    got = _sums(c["Y"], c["labels"], c["pairs"], C, seed=c["seed"], n_permutations=R, return_null=True)
    _check_observed(got, c, C)
    _check_null(got, c, R, C)
    for kind in KINDS:
        k = _exact_case(257, C, 5, 0, R, kind=kind)
        got = _sums(k["Y"], k["labels"], k["pairs"], C, seed=k["seed"], n_permutations=R, return_null=True)
        _check_observed(got, k, (C, kind))
        _check_null(got, k, R, (C, kind))
        empty = k["counts"] < 1
        for key in ("count_ge", "count_le", "sum_d", "sumsq_d"):            # an empty group: nothing counted, nothing added
            assert not got[key][:, empty, :].any() and not got[key][:, :, empty].any(), (C, kind, key)


@pytest.mark.parametrize("C", [5, 64])
def test_full_batch_and_the_chain_behind_it(C):
    """All groups of a launch chain (64 of 16 permutations; 63 at C = 64, where the fold's planes bound them) and a second chain."""
    full = 16 * min(64, 65535 // (16 * C))
    c = _exact_case(257, C, 3, 0, full + 1)
    for R in (full - 1, full, full + 1):
        got = _sums(c["Y"], c["labels"], c["pairs"], C, seed=c["seed"], n_permutations=R, return_null=True)
        assert got["batch"] == min(R, full)
        _check_null(got, c, R, (C, R))


# ---------------------------------------------------------------- 3. continuous values
@pytest.mark.parametrize("n,C,seed", [(1000, 5, 21), (257, 3, 22)])
def test_continuous_values_within_the_bound_of_any_order(n, C, seed):
    R, G = 64, 24
    Y = _gamma_Y(n, G, seed)
    assert 0.68 < (Y == 0).mean() < 0.72
    labels = _labels(n, C, "minus", seed)
    pairs = _pairs(G, 8, 24, seed)
    genes = ref.gene_list(pairs)
    Yg = ref.dense64(Y)[:, genes]
    counts = ref.label_counts(labels, C)
    from flashdeconv_amd.utils.spatial_stats import permutation_indices
    got = _sums(Y, labels, pairs, C, seed=seed, n_permutations=R, return_null=True)
    u = ref.group_sums(Yg, labels, C)
    bound_u = n * EPS53 * ref.abs_sums(Yg, labels, C)
    assert np.all(np.abs(got["u"] - u) <= bound_u)
    assert np.array_equal(got["nnz"], ref.group_nnz(Yg, labels, C)) and np.array_equal(got["label_counts"], counts)
    null = ref.null_sums(Yg, labels, C, seed, 0, R)
    slot = np.searchsorted(genes, pairs)
    T = ref.statistic_fast(u, counts, pairs, genes)
    small = np.minimum(counts[:, None], counts[None, :]).astype(np.float64)[None]         # the smaller n_c of (a, b)
    sure_ge, sure_le, inside = np.zeros(T.shape, dtype=np.int64), np.zeros(T.shape, dtype=np.int64), np.zeros(T.shape, dtype=np.int64)
    for r in range(R):
        bound_r = n * EPS53 * ref.abs_sums(Yg, labels[permutation_indices(seed, r, n)], C)
        assert np.all(np.abs(got["null"][r] - null[r]) <= bound_r), r
        b = np.maximum(bound_u, bound_r)                                                  # of either sum a case compares
        band = 2.0 * np.maximum(b[:, slot[:, 0]].T[:, :, None], b[:, slot[:, 1]].T[:, None, :]) / small
        Tr = ref.statistic_fast(null[r], counts, pairs, genes)
        out = np.abs(Tr - T) > band
        sure_ge += out & (Tr > T)
        sure_le += out & (Tr < T)
        inside += ~out
    total = R * T.size
    assert int(inside.sum()) <= total // 1000, (int(inside.sum()), total)                  # the cap: 0.1 % of the cases
    assert np.all(got["count_ge"] >= sure_ge) and np.all(got["count_ge"] <= sure_ge + inside)
    assert np.all(got["count_le"] >= sure_le) and np.all(got["count_le"] <= sure_le + inside)
    assert int(inside.sum()) == 0                                                          # these seeds leave no case out


def test_negative_values_and_signed_zeros():
    """Only exact zeros are skipped: negative values are added, -0.0 is a zero (not counted in nnz, changes no sum)."""
    n, C = 300, 4
    rs = np.random.RandomState(8)
    Y = rs.randint(-3, 4, (n, 20)).astype(np.float32)
    Y[rs.rand(n, 20) < 0.2] = -0.0
    labels = _labels(n, C, "minus")
    pairs = _pairs(20, 6, 0, 1)
    genes = ref.gene_list(pairs)
    Yg = ref.dense64(Y)[:, genes]
    got = _sums(Y, labels, pairs, C, seed=4, n_permutations=9, return_null=True)
    assert np.array_equal(got["u"], ref.group_sums(Yg, labels, C)) and (got["u"] < 0).any()
    assert np.array_equal(got["nnz"], ref.group_nnz(Yg, labels, C))
    assert np.array_equal(got["null"], ref.null_sums(Yg, labels, C, 4, 0, 9))


# ---------------------------------------------------------------- 4. invariance, bit for bit
def test_invariance():
    n, C, R, G = 1000, 6, 40, 64
    Y = _gamma_Y(n, G, 5)
    labels = _labels(n, C, "minus")
    pairs = _pairs(G, 40, 0, 2)
    kw = dict(seed=9, n_permutations=R, return_null=True)
    base = _sums(Y, labels, pairs, C, **kw)
    keys = ("u", "nnz", "label_counts", "null", "count_ge", "count_le", "sum_d", "sumsq_d")

    def same(other, what, which=keys):
        for k in which:
            assert other[k].tobytes() == base[k].tobytes(), (what, k)

    same(_sums(Y, labels, pairs, C, **kw), "two calls")
    for max_batch in (1, 7):
        same(_sums(Y, labels, pairs, C, max_batch=max_batch, **kw), f"max_batch {max_batch}")
    # a forced small stripe of the gather: one tile of 16 float32 genes at a time, three stripes
    same(_sums(Y, labels, pairs, C, max_gather_bytes=n * 16 * 4, **kw), "stripes")
    same(_sums(Y, labels, pairs, C, max_gather_bytes=1, max_batch=3, **kw), "stripes and batches")
    # CSR against the dense matrix of the same values
    same(_sums(sparse.csr_matrix(Y), labels, pairs, C, **kw), "csr")
    same(_sums(sparse.csr_matrix(Y), labels, pairs, C, max_gather_bytes=1, **kw), "csr stripes")
    # a range of permutations split into two calls
    a = _sums(Y, labels, pairs, C, seed=9, first_perm=0, n_permutations=13, return_null=True)
    b = _sums(Y, labels, pairs, C, seed=9, first_perm=13, n_permutations=R - 13, return_null=True)
    assert np.concatenate([a["null"], b["null"]]).tobytes() == base["null"].tobytes()
    assert np.array_equal(a["count_ge"] + b["count_ge"], base["count_ge"]) and np.array_equal(a["count_le"] + b["count_le"], base["count_le"])
    # the same pairs in another order and with further pairs (and genes) added: a gene's sums do not change
    rs = np.random.RandomState(3)
    more = np.concatenate([pairs[rs.permutation(len(pairs))], rs.randint(0, G, (15, 2))])
    other = _sums(Y, labels, more, C, **kw)
    assert other["genes"].shape[0] > base["genes"].shape[0]
    at = np.searchsorted(other["genes"], base["genes"])
    assert other["u"][:, at].tobytes() == base["u"].tobytes() and np.array_equal(other["nnz"][:, at], base["nnz"])
    assert np.ascontiguousarray(other["null"][:, :, at]).tobytes() == base["null"].tobytes()
    # and a pair's statistics do not depend on the other pairs
    first = {tuple(p): i for i, p in reversed(list(enumerate(more.tolist())))}
    rows = [first[tuple(p)] for p in pairs.tolist()]
    for k in ("count_ge", "count_le", "sum_d", "sumsq_d"):
        assert np.ascontiguousarray(other[k][rows]).tobytes() == base[k].tobytes(), k


# ---------------------------------------------------------------- 5. inputs
def test_inputs_give_the_same_result():
    import torch
    n, C, G, R = 300, 5, 30, 21
    Y32 = _int_Y(n, G, 6)
    labels = _labels(n, C, "minus")
    pairs = _pairs(G, 17, 0, 4)
    kw = dict(seed=2, n_permutations=R, return_null=True)
    base = _sums(Y32, labels, pairs, C, **kw)
    genes = ref.gene_list(pairs)
    Yg = ref.dense64(Y32)[:, genes]
    assert base["u"].tobytes() == ref.group_sums(Yg, labels, C).tobytes()
    assert base["null"].tobytes() == ref.null_sums(Yg, labels, C, 2, 0, R).tobytes() and isinstance(base["null"], np.ndarray)
    keys = ("u", "nnz", "label_counts", "count_ge", "count_le", "sum_d", "sumsq_d")

    def same(other, what):
        null = other["null"].cpu().numpy() if torch.is_tensor(other["null"]) else other["null"]
        assert null.tobytes() == base["null"].tobytes(), what
        for k in keys:
            assert other[k].tobytes() == base[k].tobytes(), (what, k)

    # dense float32 and float64 with a row stride above G, host and CUDA
    wide32, wide64 = np.zeros((n, G + 7), dtype=np.float32), np.zeros((n, G + 5), dtype=np.float64)
    wide32[:, :G], wide64[:, :G] = Y32, Y32
    wide32[:, G:], wide64[:, G:] = 99.0, 77.0
    same(_sums(wide32[:, :G], labels, pairs, C, **kw), "host float32 view")
    same(_sums(wide64[:, :G], labels, pairs, C, **kw), "host float64 view")
    for wide in (wide32, wide64):
        t = torch.as_tensor(wide, device="cuda:0")[:, :G]
        assert t.stride(0) > G
        got = _sums(t, labels, pairs, C, **kw)
        assert torch.is_tensor(got["null"]) and got["null"].is_cuda and got["null"].dtype == torch.float64
        same(got, f"cuda {wide.dtype}")
    same(_sums(torch.as_tensor(Y32.astype(np.int32), device="cuda:0"), labels, pairs, C, **kw), "cuda int32 counts")
    # scipy CSR with unsorted columns and stored zeros
    csr = sparse.csr_matrix(Y32)
    rs = np.random.RandomState(0)
    indptr, cols, vals = [0], [], []
    for i in range(n):
        row = np.flatnonzero(Y32[i])
        extra = np.setdiff1d(np.arange(G), row)[:2]                        # two stored zeros a row
        idx = np.concatenate([row, extra])[rs.permutation(len(row) + len(extra))]
        cols.append(idx)
        vals.append(Y32[i, idx])
        indptr.append(indptr[-1] + len(idx))
    messy = sparse.csr_matrix((np.concatenate(vals), np.concatenate(cols), np.array(indptr)), shape=(n, G))
    assert not messy.has_sorted_indices and messy.nnz == csr.nnz + 2 * n
    same(_sums(messy, labels, pairs, C, **kw), "scipy csr, unsorted, stored zeros")
    same(_sums(csr.astype(np.float64), labels, pairs, C, **kw), "scipy csr float64")
    tcsr = torch.sparse_csr_tensor(torch.as_tensor(csr.indptr.astype(np.int64)), torch.as_tensor(csr.indices.astype(np.int64)),
                                   torch.as_tensor(csr.data), size=(n, G)).to("cuda:0")
    got = _sums(tcsr, labels, pairs, C, **kw)
    assert torch.is_tensor(got["null"]) and got["null"].is_cuda
    same(got, "cuda csr")
    # CUDA labels of every integer dtype; the number of labels inferred on the device
    for dtype in (torch.int8, torch.int16, torch.int32, torch.int64):
        got = _sums(Y32, torch.as_tensor(labels, device="cuda:0").to(dtype), pairs, C, **kw)
        assert torch.is_tensor(got["null"]) and got["null"].is_cuda
        same(got, dtype)
    pos = np.where(labels < 0, 0, labels)
    a = _sums(Y32, pos, pairs, C, **kw)
    b = _sums(Y32, torch.as_tensor(pos, device="cuda:0").to(torch.uint8), pairs, None, **kw)
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k
    # the range of device labels is checked on the device and reported, not faulted on
    for bad in (C, -2, 1 << 40):
        lab = torch.as_tensor(labels, device="cuda:0").clone()
        lab[17] = bad
        with pytest.raises(ValueError, match=r"labels must lie in \[-1, 5\)"):
            _sums(Y32, lab, pairs, C)
    with pytest.raises(TypeError, match="labels must be integers"):
        _sums(Y32, torch.zeros(n, device="cuda:0"), pairs, C)


# ---------------------------------------------------------------- 6. the public surface
def _expected(Y, labels, pairs, C, seed, R, sums, threshold=0.01):
    """``host_statistics`` of the reference's sums and counts; sum_d / sumsq_d (held to their rounding bound first) are the device's."""
    genes = ref.gene_list(pairs)
    Yg = ref.dense64(Y)[:, genes]
    counts = ref.label_counts(labels, C)
    u, nnz = ref.group_sums(Yg, labels, C), ref.group_nnz(Yg, labels, C)
    T = ref.statistic_fast(u, counts, pairs, genes)
    Tr = [ref.statistic_fast(v, counts, pairs, genes) for v in ref.null_sums(Yg, labels, C, seed, 0, R)]
    ge, le, sd, sq, sa = ref.accumulate(Tr, T)
    if R:
        assert np.all(np.abs(sums["sum_d"] - sd) <= (R + 2) * EPS52 * sa) and np.all(np.abs(sums["sumsq_d"] - sq) <= (R + 2) * EPS52 * sq)
        sd, sq = sums["sum_d"], sums["sumsq_d"]
    return ref.host_statistics(pairs, genes, u, nnz, counts, ge, le, sd, sq, R, threshold)


def _same_statistics(got, want, tag):
    for k, v in want.items():
        if k == "n_permutations":
            assert got[k] == v, tag
        else:
            np.testing.assert_array_equal(got[k], v, err_msg=f"{tag} {k}")


def test_ligand_receptor_test():
    from flashdeconv_amd.utils.ligrec import ligand_receptor_test
    n, C, G, R = 400, 4, 40, 33
    Y = _int_Y(n, G, 12)
    Y[:, 5] = 0.0                                                          # a gene nobody expresses: its pairs are not tested
    Y[:, 6] *= (np.arange(n) % 50 == 0)                                    # and one under the 1 % threshold in most groups
    labels = _labels(n, C, "minus")
    pairs = np.concatenate([_pairs(G, 9, 14, 5), [[5, 1], [2, 5], [6, 6]]])
    sums = _sums(Y, labels, pairs, C, seed=7, n_permutations=R)
    for threshold in (0.01, 0.3):
        got = ligand_receptor_test(Y, labels, pairs, n_labels=C, n_permutations=R, random_state=7, threshold=threshold, n_top=5,
                                   return_null=True)
        want = _expected(Y, labels, pairs, C, 7, R, sums, threshold)
        assert set(got) == set(want) | {"pairs", "genes", "label_counts", "n", "null", "top"}
        _same_statistics(got, want, threshold)
        assert np.array_equal(got["top"], got["order"][:5]) and np.array_equal(got["pairs"], pairs) and got["n"] == n
        assert got["null"].shape == (R, C, len(got["genes"]))
        assert np.isnan(got["p_greater"][-3]).all() and not got["expressed"][-3].any() and not np.isnan(got["means"][-3]).any()
        assert got["expressed"].any()
    none = ligand_receptor_test(Y, labels, pairs, n_labels=C, n_permutations=0)
    assert "p_greater" not in none and "null" not in none
    _same_statistics(none, _expected(Y, labels, pairs, C, 0, 0, None), "R = 0")


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def test_model_method():
    import datagen
    from flashdeconv_amd import FlashDeconv
    from flashdeconv_amd.utils.neighborhoods import neighborhood_enrichment
    from flashdeconv_amd.utils.spatial_stats import _permutation_seed
    Y, X, coords, _ = datagen.count_like(300, 300, 4, 0.1, seed=9)
    R = 19
    explicit = np.random.RandomState(4).randint(-1, 3, 300)
    pairs = _pairs(300, 7, 10, 6)
    for output in ("numpy", "torch"):
        m = FlashDeconv(sketch_dim=64, max_iter=20).fit(Y, X, coords, output=output)
        seed = _permutation_seed(m.random_state)
        dominant = _host(m.get_dominant_cell_type())
        niches = _host(m.get_spatial_niches(3)["labels"])
        for kw, labels, C, sd in (({}, dominant, 4, seed), ({"n_niches": 3}, niches, 3, seed),
                                  ({"labels": explicit, "n_labels": 3, "random_state": 12}, explicit, 3, 12)):
            got = m.get_ligand_receptor(Y, pairs, n_permutations=R, **kw)
            sums = _sums(Y, labels, pairs, C, seed=sd, n_permutations=R)
            want = _expected(Y, labels, pairs, C, sd, R, sums)
            assert set(got) == set(want) | {"pairs", "genes", "label_counts", "n"}, (output, kw)
            _same_statistics(got, want, f"{output} {kw}")
            # the neighbourhood enrichment on the same model and labels: what the entry called directly returns
            ne = m.get_neighborhood_enrichment(n_permutations=R, **kw)
            direct = neighborhood_enrichment(labels, m, n_labels=C, n_permutations=R, random_state=sd)
            assert set(ne) == set(direct)
            for k, v in direct.items():
                np.testing.assert_array_equal(ne[k], v, err_msg=f"{output} {kw} {k}")
        with pytest.raises(ValueError, match="at most one of labels and n_niches"):
            m.get_ligand_receptor(Y, pairs, labels=explicit, n_niches=3)
        with pytest.raises(ValueError, match="labels must have the 300 spots"):
            m.get_ligand_receptor(Y, pairs, labels=explicit[:10])
        with pytest.raises(ValueError, match="spots of the fit"):
            m.get_ligand_receptor(Y[:50], pairs)
        with pytest.raises(ValueError, match="outside"):
            m.get_ligand_receptor(Y, [[0, 300]], n_niches=3)
        with pytest.raises(TypeError, match="unexpected keyword"):
            m.get_ligand_receptor(Y, pairs, nonsense=1)
        assert "p_greater" not in m.get_ligand_receptor(Y, pairs, n_permutations=0)


def test_deconvolve_writes_the_ligrec_tables_on_request():
    import datagen
    import flashdeconv_amd as fd
    from flashdeconv_amd.io import prepare_data
    case = datagen.anndata_case()
    kw = dict(cell_type_key="celltype", sketch_dim=64, k_neighbors=4, n_hvg=300, n_markers_per_type=20)
    st, rf = datagen.anndata_objects(case)
    Y, X, coords, names, genes = prepare_data(st, rf, cell_type_key="celltype")
    named = [(str(genes[3]), str(genes[10])), (str(genes[10]), str(genes[10])), (str(genes[40]), str(genes[3]))]
    idx = np.array([[3, 10], [10, 10], [40, 3]])
    assert fd.tl.deconvolve(st, rf, n_niches=3, ligrec_pairs=named, ligrec_permutations=50, **kw) is None
    res = st.uns["flashdeconv_ligrec"]
    assert set(res) == {"means", "pvalues", "qvalues"} and st.uns["flashdeconv_params"]["ligrec"] == 50
    m = fd.FlashDeconv(sketch_dim=64, k_neighbors=4, n_hvg=300, n_markers_per_type=20).fit(Y, X, coords)
    labels = np.asarray(st.obs["flashdeconv_niche"]).astype(np.int64)
    want = m.get_ligand_receptor(Y, idx, labels=labels, n_labels=3, n_permutations=50, random_state=0)
    sums = _sums(Y, labels, idx, 3, seed=0, n_permutations=50)
    _same_statistics(want, _expected(Y, labels, idx, 3, 0, 50, sums), "niches")
    for key, src in (("means", "means"), ("pvalues", "p_greater"), ("qvalues", "q_value")):
        assert list(res[key].index) == [f"{a}_{b}" for a, b in named] and res[key].index.name == "ligand_receptor", key
        assert list(res[key].columns.names) == ["source", "target"], key
        assert list(res[key].columns) == [(a, b) for a in range(3) for b in range(3)], key
        np.testing.assert_array_equal(res[key].values, want[src].reshape(3, 9), err_msg=key)
    # without niches: the dominant cell types, by name
    st2, rf2 = datagen.anndata_objects(case)
    fd.tl.deconvolve(st2, rf2, ligrec_pairs=named, ligrec_permutations=20, **kw)
    res2 = st2.uns["flashdeconv_ligrec"]
    types = [str(t) for t in names]
    dom = m.get_ligand_receptor(Y, idx, n_permutations=20, random_state=0)
    assert st2.uns["flashdeconv_params"]["ligrec"] == 20 and "flashdeconv_niche" not in st2.obs
    for key, src in (("means", "means"), ("pvalues", "p_greater"), ("qvalues", "q_value")):
        assert list(res2[key].columns) == [(a, b) for a in types for b in types], key
        np.testing.assert_array_equal(res2[key].values, dom[src].reshape(3, len(types) ** 2), err_msg=key)
