"""-m gpu tests of the marker-gene sums (csrc/gene_group_kernels.cpp: fdx_gene_group_sums_dev / _csr_dev; utils.group_genes;
FlashDeconv.get_niche_genes; tl.deconvolve(niche_genes=True)).

Reference: tests/group_genes_ref.py (``scipy.stats.rankdata`` per column over the used rows).  In every test ``R2``, ``nnz``, ``T``,
``n_rows`` and ``n_used`` must EQUAL the reference as integers, and ``u`` / ``q`` must equal ``weighted_gene_sums(Y, ones, groups)``
bit for bit.  The statistics are held to the host bound of tests/test_group_genes_host.py."""
import functools

import numpy as np
import pytest

import datagen
import group_genes_ref as gr

pytestmark = pytest.mark.gpu


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _check(Yc, Yref, groups, C, what, **kw):
    """One call on the container Yc against the reference on the dense float64 Yref and against the weighted gene sums."""
    from flashdeconv_amd.utils.expression import weighted_gene_sums
    from flashdeconv_amd.utils.group_genes import gene_group_sums
    got = gene_group_sums(Yc, groups, n_groups=C, **kw)
    want = gr.sums(Yref, groups, C)
    for key in ("R2", "nnz", "T", "n_rows"):
        assert got[key].dtype == np.int64 and got[key].shape == want[key].shape, (what, key)
        assert np.array_equal(got[key], want[key]), (what, key, np.argwhere(got[key] != want[key])[:4].tolist())
    assert got["n_used"] == want["n_used"], what
    ws = weighted_gene_sums(Yc, np.ones((Yref.shape[0], 1)), groups=groups, n_groups=C)
    for key in ("u", "q"):
        assert _same_bits(got[key], np.asarray(ws[key]).reshape(got[key].shape)), (what, key)
    return got


@functools.lru_cache(maxsize=None)
def _dense_case(n, G):
    """Mostly-zero counts with ties, a few negatives, labels in [-1, 3)."""
    rs = np.random.RandomState(1000 * G + n)
    Y = gr.expression_like(n, G, n + G, density=0.3, dtype=np.float64)
    Y -= 2.0 * (rs.random_sample(Y.shape) < 0.03)
    g = rs.randint(-1, 3, size=n)
    for a in (Y, g):
        a.setflags(write=False)
    return Y, g


def _dense_container(Y, storage):
    import torch
    if storage == "f32":
        return Y.astype(np.float32)
    if storage == "f64":
        return Y.astype(np.float64)
    if storage == "int32":
        return Y.astype(np.int32)
    wide = torch.full((Y.shape[0], Y.shape[1] + 7), 99.0, dtype=torch.float32, device="cuda")     # row stride G + 7
    wide[:, 3:3 + Y.shape[1]] = torch.as_tensor(Y.astype(np.float32)).cuda()
    return wide[:, 3:3 + Y.shape[1]]


@pytest.mark.parametrize("storage", ["f32", "f64", "int32", "cuda_strided"])
@pytest.mark.parametrize("G", [1, 65])
@pytest.mark.parametrize("n", [1, 2, 257, 2049])
def test_dense_routes(n, G, storage):
    Y, g = _dense_case(n, G)
    _check(_dense_container(Y, storage), Y, g, 3, (n, G, storage))


@functools.lru_cache(maxsize=None)
def _csr_case():
    rs = np.random.RandomState(5)
    Y = gr.expression_like(300, 70, 8, density=0.2, dtype=np.float64)
    Y -= 3.0 * (rs.random_sample(Y.shape) < 0.02)
    Y[:, 33] = 0.0                                             # a gene with no stored entry
    Y[::7] = 0.0                                               # empty rows
    g = rs.randint(-1, 4, size=300)
    for a in (Y, g):
        a.setflags(write=False)
    return Y, g


def _csr_container(Y, form):
    import torch
    from scipy import sparse
    dtype = np.float64 if form in ("f64", "cuda") else np.float32
    m = sparse.csr_matrix(Y.astype(dtype))
    if form == "unsorted":                                     # every row's columns reversed
        idx, dat = m.indices.copy(), m.data.copy()
        for i in range(m.shape[0]):
            a, b = m.indptr[i], m.indptr[i + 1]
            idx[a:b], dat[a:b] = idx[a:b][::-1], dat[a:b][::-1]
        m = sparse.csr_matrix((dat, idx, m.indptr), shape=m.shape)
        assert not m.has_sorted_indices
    if form == "stored_zeros":                                 # every third stored value becomes a stored 0, some of them -0.0
        m.data[::3] = 0.0
        m.data[::9] = -0.0
        assert m.nnz == m.data.size and np.count_nonzero(m.data) < m.nnz
    if form == "cuda":
        return m, torch.sparse_csr_tensor(torch.as_tensor(m.indptr.astype(np.int64)), torch.as_tensor(m.indices.astype(np.int32)),
                                          torch.as_tensor(m.data), size=m.shape).cuda()
    return m, m


@pytest.mark.parametrize("form", ["f32", "f64", "unsorted", "stored_zeros", "cuda"])
def test_csr_routes(form):
    Y, g = _csr_case()
    m, container = _csr_container(Y, form)
    _check(container, gr.dense64(m), g, 4, form)


@pytest.mark.parametrize("labels", ["some_left_out", "all_left_out", "empty_group", "one_group", "C256", "none", "cuda"])
@pytest.mark.parametrize("route", ["dense", "csr"])
def test_labels(labels, route):
    import torch
    from scipy import sparse
    Y, _ = _csr_case()
    n = Y.shape[0]
    rs = np.random.RandomState(3)
    g, C = {"some_left_out": (np.where(rs.random_sample(n) < 0.4, -1, rs.randint(0, 3, size=n)), 3),
            "all_left_out": (np.full(n, -1), 2),
            "empty_group": (rs.randint(0, 2, size=n) * 2, 4),          # groups 1 and 3 are empty
            "one_group": (np.zeros(n, dtype=np.int64), 1),
            "C256": (rs.randint(-1, 256, size=n), 256),
            "none": (None, 1),
            "cuda": (rs.randint(-1, 5, size=n), 5)}[labels]
    Yc = Y.astype(np.float32) if route == "dense" else sparse.csr_matrix(Y.astype(np.float32))
    if labels == "cuda":
        from flashdeconv_amd.utils.group_genes import gene_group_sums
        got = gene_group_sums(Yc, torch.as_tensor(g).cuda(), n_groups=None)
        want = gr.sums(Y, g, 5)
        for key in ("R2", "nnz", "T", "n_rows"):
            assert np.array_equal(got[key], want[key]), key
        with pytest.raises(ValueError, match=r"groups must lie in \[-1, 3\)"):
            gene_group_sums(Yc, torch.as_tensor(g).cuda(), n_groups=3)
        return
    got = _check(Yc, Y, g, C, (labels, route))
    if labels == "all_left_out":
        assert got["n_used"] == 0 and not got["R2"].any() and not got["T"].any() and not got["u"].any()


def _values_case():
    """One column per special value pattern, float64; labels in [-1, 3)."""
    rs = np.random.RandomState(11)
    n = 400
    g = rs.randint(-1, 3, size=n)
    Y = np.zeros((n, 8))
    Y[:, 0] = rs.randint(0, 3, size=n) * (rs.random_sample(n) < 0.5)          # ties among the nonzeros, across the groups
    Y[:, 1] = rs.randint(-2, 3, size=n)                                        # negatives: ranked before the zero run
    Y[:, 2] = np.where(rs.random_sample(n) < 0.5, -0.0, rs.randint(0, 2, size=n))      # -0.0 is a zero
    Y[:, 3] = 0.0                                                              # an all-zero gene
    Y[:, 4] = 2.5                                                              # a constant nonzero gene
    a = 1.0 + 2.0 ** -30                                                       # equal to 1.0 as float32, distinct as float64
    assert np.float32(a) == np.float32(1.0) and a != 1.0
    Y[:, 5] = np.where(rs.random_sample(n) < 0.5, a, 1.0) * (rs.random_sample(n) < 0.7)
    Y[:, 6] = -np.abs(rs.randn(n))                                             # all negative, all distinct
    Y[:, 7] = rs.randn(n) * (rs.random_sample(n) < 0.2)
    return Y, g


@pytest.mark.parametrize("route", ["dense_f64", "csr_f64", "dense_f32", "csr_f32"])
def test_values(route):
    from scipy import sparse
    Y, g = _values_case()
    dtype = np.float64 if route.endswith("f64") else np.float32
    Ys = Y.astype(dtype)                                        # float32: the two values of gene 5 become one - the reference too
    Yc = Ys if route.startswith("dense") else sparse.csr_matrix(Ys)
    got = _check(Yc, gr.dense64(Ys), g, 3, route)
    N = got["n_used"]
    assert got["T"][3] == N ** 3 - N and got["T"][4] == N ** 3 - N and got["T"][6] == 0
    assert np.array_equal(got["R2"][:, 3], got["n_rows"] * (N + 1)) and np.array_equal(got["R2"][:, 4], got["n_rows"] * (N + 1))
    assert np.array_equal(got["nnz"][:, 2], [np.count_nonzero(Y[g == c, 2]) for c in range(3)])
    if dtype == np.float64:                                     # the 64-bit keys keep the two values apart
        assert got["T"][5] != gr.sums(Y.astype(np.float32), g, 3)["T"][5]


def test_stripes_change_nothing():
    from flashdeconv_amd.utils.group_genes import gene_group_sums
    from scipy import sparse
    Y, g = _csr_case()
    for Yc in (Y.astype(np.float32), Y.astype(np.float64), sparse.csr_matrix(Y.astype(np.float64))):
        whole = _check(Yc, Y, g, 4, "default budget")
        assert whole["stripes"] == 1 and whole["stripe_entries"] == int(whole["nnz"].sum())
        for budget in (1, 16_000):                              # a gene a stripe; a few genes a stripe
            cut = gene_group_sums(Yc, g, n_groups=4, max_sort_bytes=budget)
            assert cut["stripes"] >= 3 and cut["stripe_entries"] < whole["stripe_entries"]
            for key in ("R2", "nnz", "T", "n_rows"):
                assert np.array_equal(cut[key], whole[key]), (budget, key)
            assert _same_bits(cut["u"], whole["u"]) and _same_bits(cut["q"], whole["q"])
        assert gene_group_sums(Yc, g, n_groups=4, max_sort_bytes=1)["stripes"] == Y.shape[1]


def test_width_sums_beyond_32_bits():
    n = 70_000
    rs = np.random.RandomState(2)
    Y = np.empty((n, 2), dtype=np.float32)
    Y[:, 0] = 3.0                                              # all ties
    Y[:, 1] = rs.permutation(n) + 1.0                          # all distinct (exact in float32)
    g = (rs.random_sample(n) < 0.06).astype(np.int64)          # group 0 holds about 94 % of the spots
    got = _check(Y, Y, g, 2, "width")
    assert got["T"][0] == n ** 3 - n and got["T"][0] > 2 ** 32 and got["T"][1] == 0
    assert got["R2"][0, 0] > 2 ** 32 and got["R2"][0, 1] > 2 ** 32
    assert got["R2"][:, 1].sum() == n * (n + 1)


def test_two_calls_give_the_same_bits():
    from flashdeconv_amd.utils.group_genes import gene_group_sums
    from scipy import sparse
    Y, g = _dense_case(2049, 65)
    for Yc in (Y.astype(np.float32), sparse.csr_matrix(Y)):
        first, again = gene_group_sums(Yc, g, n_groups=3), gene_group_sums(Yc, g, n_groups=3)
        for key in ("R2", "nnz", "T", "n_rows"):
            assert np.array_equal(first[key], again[key]), key
        assert _same_bits(first["u"], again["u"]) and _same_bits(first["q"], again["q"])


def test_c_entry_refuses_what_it_must():
    import ctypes
    import torch
    from flashdeconv_amd import _lib
    lib = _lib.load()
    Y = torch.ones((4, 3), dtype=torch.float32, device="cuda")
    lab = torch.tensor([0, 1, 5, -1], dtype=torch.int32, device="cuda")
    f = [torch.empty((2, 3), dtype=torch.float64, device="cuda") for _ in range(2)]
    i = [torch.empty((2, 3), dtype=torch.int64, device="cuda") for _ in range(3)]
    n_c, N = np.zeros(2, dtype=np.int64), np.zeros(1, dtype=np.int64)

    def call(n=4, C=2, budget=0, labels=lab):
        return lib.fdx_gene_group_sums_dev(ctypes.c_void_p(Y.data_ptr()), _lib.FDX_F32, n, 3, 3, ctypes.c_void_p(labels.data_ptr()), C,
                                           budget, *(ctypes.c_void_p(t.data_ptr()) for t in f + i), _lib.ptr_i64(n_c), _lib.ptr_i64(N),
                                           None, None)
    for kw, message in ((dict(C=0), "C must be 1 .. 256"), (dict(C=257), "C must be 1 .. 256"), (dict(n=2_000_001), "at most 2000000 rows"),
                        (dict(budget=-1), "max_sort_bytes < 0"), (dict(), "a label lies outside [-1, C)")):
        assert call(**kw) != 0 and message in lib.fdx_last_error().decode(), message
    torch.cuda.synchronize()


def test_rank_genes_groups_matches_scipy():
    import torch
    from test_group_genes_host import HOST_BOUND, assert_matches_scipy, host_cases
    from flashdeconv_amd.utils.group_genes import rank_genes_groups
    Y, g, C = host_cases()[0]                                  # 300 x 40, 4 groups, float32 counts: u and q are exact
    got = rank_genes_groups(Y, g, n_groups=C, n_top=5)
    assert_matches_scipy(got, gr.scipy_tests(Y, g, C), HOST_BOUND, "300 x 40 x 4")
    want = gr.sums(Y, g, C)
    for key in ("R2", "nnz", "T", "n_rows"):
        assert np.array_equal(got[key], want[key]), key
    assert got["top"].shape == (C, 5) and np.array_equal(got["top"], got["order"][:, :5]) and got["n_used"] == want["n_used"]
    on_device = rank_genes_groups(torch.as_tensor(Y).cuda(), g, n_groups=C, output="torch")
    for key in ("z_score", "q_value", "order", "R2"):
        assert on_device[key].is_cuda and np.array_equal(on_device[key].cpu().numpy(), got[key], equal_nan=True), key


KEYS = {"z_score", "auc", "p_value", "q_value", "t", "t_dof", "t_p_value", "t_q_value", "log2_fold_change", "mean", "mean_rest", "var",
        "var_rest", "pct", "pct_rest", "order", "u", "q", "nnz", "R2", "T", "n_rows", "n_used"}


def test_get_niche_genes_on_a_fitted_model():
    from flashdeconv_amd import FlashDeconv
    from flashdeconv_amd.utils.group_genes import rank_genes_groups
    Y, X, coords, _ = datagen.count_like(800, 300, 6, 0.1, 3)
    model = FlashDeconv(sketch_dim=64, max_iter=25).fit(Y, X, coords)
    out = model.get_niche_genes(Y, n_niches=3, n_top=10)
    assert set(out) == KEYS | {"top"}
    for key in KEYS - {"T", "n_rows", "n_used"}:
        assert out[key].shape == (3, 300), key
    assert out["T"].shape == (300,) and out["n_rows"].shape == (3,) and out["n_rows"].sum() == out["n_used"] == 800
    assert out["top"].shape == (3, 10) and out["order"].dtype == np.int64
    labels = model.get_spatial_niches(3)["labels"]
    assert np.array_equal(out["n_rows"], np.bincount(labels, minlength=3))
    mine = model.get_niche_genes(Y, groups=labels, n_groups=3)
    for key in KEYS - {"n_used"}:
        assert np.array_equal(mine[key], out[key], equal_nan=True), key
    direct = rank_genes_groups(Y, labels, n_groups=3)
    assert np.array_equal(direct["z_score"], out["z_score"], equal_nan=True)
    with pytest.raises(ValueError, match="spots of the fit as rows"):
        model.get_niche_genes(Y[:-1], n_niches=3)


def test_deconvolve_writes_the_niche_genes_on_request_only():
    import flashdeconv_amd as fd
    from flashdeconv_amd.io import prepare_data
    case = datagen.anndata_case()
    kw = dict(cell_type_key="celltype", sketch_dim=64, k_neighbors=4, n_hvg=300, n_markers_per_type=20, n_niches=3)
    st0, ref0 = datagen.anndata_objects(case)
    assert fd.tl.deconvolve(st0, ref0, **kw) is None
    st, ref = datagen.anndata_objects(case)
    Y, _, _, _, genes = prepare_data(st, ref, cell_type_key="celltype")
    assert fd.tl.deconvolve(st, ref, niche_genes=True, **kw) is None
    assert set(st.uns) == set(st0.uns) | {"flashdeconv_niche_genes"} and set(st.obsm) == set(st0.obsm)
    assert set(st.uns["flashdeconv_params"]) == set(st0.uns["flashdeconv_params"]) | {"niche_genes"}
    assert st.uns["flashdeconv_params"]["niche_genes"] is True
    assert np.array_equal(np.asarray(st.obs["flashdeconv_niche"]), np.asarray(st0.obs["flashdeconv_niche"]))
    table = st.uns["flashdeconv_niche_genes"]
    assert list(table.columns) == ["niche", "gene", "z_score", "auc", "log2_fold_change", "pct", "pct_rest", "q_value"]
    assert len(table) == 3 * 50 and list(table["niche"]) == [c for c in range(3) for _ in range(50)]
    want = fd.utils.rank_genes_groups(Y, np.asarray(st.obs["flashdeconv_niche"]).astype(np.int64), n_groups=3)
    names = [str(x) for x in genes]
    for c in range(3):
        rows = table[table["niche"] == c]
        assert list(rows["gene"]) == [names[j] for j in want["order"][c, :50]]
        assert np.array_equal(rows["z_score"].to_numpy(), want["z_score"][c, want["order"][c, :50]], equal_nan=True)
        assert np.array_equal(rows["q_value"].to_numpy(), want["q_value"][c, want["order"][c, :50]], equal_nan=True)
