"""-m gpu tests of the neighbourhood enrichment (csrc/label_pair_kernels.cpp: fdx_label_pair_counts_dev; utils.neighborhoods,
FlashDeconv.get_neighborhood_enrichment, tl.deconvolve(nhood_enrichment=True)).

Reference (tests/nhood_ref.py), in NumPy int64: N = O' A O with O the one-hot of the labels >= 0 and A the graph's truth (the
oracle's adjacency, never the device graph's own export), the null by labels[permutation_indices(seed, r, n)], the accumulation in
permutation order.  Every comparison of counts is exact integer equality; sum_d and sumsq_d are compared bit for bit (all terms
are integers far below 2^53 at these sizes, so the float64 sums are exact in any order and equal in permutation order).

Paths of the launcher crossed: B = 16 with 256 threads (C <= 16), B = 16 with 1024 threads (17 <= C <= 32), B = 8 with 1024
threads (33 <= C <= 64, LDS above 64 KiB from C = 46) - C in {1, 2, 16, 17, 32, 33, 64}; one slice and several, a ragged last
slice (n = 1, 2, 64, 65, 257, 1000); a launch chain of one group, of several, of all 64 with a second chain behind it, ragged
groups (R around 8, 16, a capped batch of 24 and the full batch); more slices than the grid has waves (n = 20,000 with 64 groups:
every wave walks several slices)."""
import functools

import numpy as np
import pytest
from scipy import sparse

import gpu_graphs as gg
import nhood_ref as ref

pytestmark = pytest.mark.gpu

C_LIST = (1, 2, 16, 17, 32, 33, 64)
KINDS = ("random", "minus", "missing", "one", "none")

GRAPHS = {
    "knn1": lambda: gg._knn(1), "knn2": lambda: gg._knn(2), "knn64": lambda: gg._knn(64), "knn65": lambda: gg._knn(65),
    "knn257": lambda: gg._knn(257), "knn1000": lambda: gg._knn(1000), "untiled300": lambda: gg._knn_untiled(300),
    "hub300": lambda: gg._hub(300), "radius": gg._radius_isolated, "grid": gg._grid,
}


def _labels(n, C, kind, seed=0):
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


def _counts(G, labels, C, **kw):
    from flashdeconv_amd.utils.neighborhoods import label_pair_counts
    return label_pair_counts(labels, G.g, n_labels=C, **kw)


@functools.lru_cache(maxsize=None)
def _null_ref(name, C, kind, seed, first, R):
    G = GRAPHS[name]()
    labels = _labels(G.n, C, kind)
    null = ref.null_counts(G.A, labels, C, seed, first, R)
    null.setflags(write=False)
    return null


def _check_sums(got, obs, null):
    ge, le, sd, sq = ref.accumulate(null, obs)
    assert np.array_equal(got["count_ge"], ge) and np.array_equal(got["count_le"], le)
    assert got["sum_d"].dtype == np.float64 and got["sumsq_d"].dtype == np.float64
    assert got["sum_d"].tobytes() == sd.tobytes() and got["sumsq_d"].tobytes() == sq.tobytes()


# ---------------------------------------------------------------- 1. observed counts
@pytest.mark.parametrize("name", list(GRAPHS))
def test_observed_counts(name):
    G = GRAPHS[name]()
    if name in ("knn257", "knn1000"):
        gg._assert_tiled(G)                                # the tiled, Morton-ordered graph: the order is not the identity
    n, W, sdeg2 = ref.graph_counts(G.A)
    assert n == G.n
    for C in C_LIST:
        for kind in KINDS:
            labels = _labels(n, C, kind)
            got = _counts(G, labels, C)
            want = ref.pair_counts(G.A, labels, C)
            tag = (name, C, kind)
            assert got["count"].dtype == np.int64 and got["count"].shape == (C, C), tag
            assert np.array_equal(got["count"], want), tag
            assert np.array_equal(got["count"], got["count"].T), tag
            assert np.array_equal(got["label_counts"], ref.label_counts(labels, C)), tag
            assert (got["n"], got["W"], got["sum_deg_sq"]) == (n, W, sdeg2), tag
            if kind in ("random", "missing", "one") and (labels >= 0).all():
                assert int(got["count"].sum()) == W, tag
            if kind == "one":
                assert got["count"][C - 1, C - 1] == W, tag
            if kind == "none":
                assert not got["count"].any() and not got["label_counts"].any(), tag
            # no permutations: the permutation outputs stay zero
            assert got["n_permutations"] == 0 and got["batch"] == 0, tag
            for k in ("count_ge", "count_le", "sum_d", "sumsq_d"):
                assert got[k].shape == (C, C) and not got[k].any(), (tag, k)


# ---------------------------------------------------------------- 2. the null
@pytest.mark.parametrize("name", ["knn257", "hub300"])
@pytest.mark.parametrize("C", [5, 64])
def test_null_against_the_reference(name, C):
    G = GRAPHS[name]()
    labels = _labels(G.n, C, "minus")
    obs = ref.pair_counts(G.A, labels, C)
    seed, R = 7, 37
    null = _null_ref(name, C, "minus", seed, 0, R)
    width = 16 if C <= 32 else 8
    results = []
    for max_batch in (0, 1, 5, 24):
        got = _counts(G, labels, C, seed=seed, n_permutations=R, max_batch=max_batch, return_null=True)
        assert got["batch"] == (R if max_batch == 0 else max_batch), (max_batch, got["batch"])
        assert got["null"].dtype == np.int64 and got["null"].shape == (R, C, C)
        assert np.array_equal(got["count"], obs)
        bad = [r for r in range(R) if not np.array_equal(got["null"][r], null[r])]
        assert not bad, (max_batch, bad)
        _check_sums(got, obs, null)
        results.append(got)
    # the edges of a group's width (8 or 16 permutations a position) and of a capped batch of 24
    for R2, max_batch in [(r, 0) for r in (1, width - 1, width, width + 1, 2 * width - 1, 2 * width, 2 * width + 1)] + \
                         [(23, 24), (24, 24), (25, 24)]:
        got = _counts(G, labels, C, seed=seed, n_permutations=R2, max_batch=max_batch, return_null=True)
        assert got["batch"] == min(R2, max_batch or R2)
        assert np.array_equal(got["null"], null[:R2]), (R2, max_batch)
        _check_sums(got, obs, null[:R2])
    # split calls add up exactly
    a = _counts(G, labels, C, seed=seed, first_perm=0, n_permutations=20, return_null=True)
    b = _counts(G, labels, C, seed=seed, first_perm=20, n_permutations=17, return_null=True)
    one = results[0]
    assert np.array_equal(np.concatenate([a["null"], b["null"]]), one["null"])
    for k in ("count_ge", "count_le"):
        assert np.array_equal(a[k] + b[k], one[k])
    for k in ("sum_d", "sumsq_d"):
        assert (a[k] + b[k]).tobytes() == one[k].tobytes()
    # another seed gives another null
    other = _counts(G, labels, C, seed=seed + 1, n_permutations=R, return_null=True)
    assert not np.array_equal(other["null"], one["null"])


@pytest.mark.parametrize("C", [5, 64])
def test_full_batch_and_the_chain_behind_it(C):
    """All 64 groups of a launch chain (1024 permutations at C = 5, 512 at C = 64) and a second chain."""
    G = GRAPHS["knn257"]()
    labels = _labels(G.n, C, "minus")
    full = 64 * (16 if C <= 32 else 8)
    for R in (full - 1, full, full + 1):
        got = _counts(G, labels, C, seed=3, n_permutations=R, return_null=True)
        assert got["batch"] == min(R, full)
        null = _null_ref("knn257", C, "minus", 3, 0, full + 1)[:R]
        assert np.array_equal(got["null"], null), R
        _check_sums(got, ref.pair_counts(G.A, labels, C), null)


@pytest.mark.parametrize("C", [10, 40])
def test_more_slices_than_waves(C):
    """n = 20,000 with 64 groups in flight: the grid has fewer waves than the graph has slices, so every wave walks several."""
    G = gg._knn(20000)
    n = G.n
    labels = _labels(n, C, "minus")
    obs = ref.pair_counts(G.A, labels, C)
    width = 16 if C <= 32 else 8
    R = 64 * width
    got = _counts(G, labels, C, seed=11, n_permutations=R, return_null=True)
    assert got["batch"] == R and np.array_equal(got["count"], obs)
    from flashdeconv_amd.utils.spatial_stats import permutation_indices
    for r in (0, 1, width - 1, width, R // 2, R - width, R - 1):
        want = ref.pair_counts(G.A, labels[permutation_indices(11, r, n)], C)
        assert np.array_equal(got["null"][r], want), r
    # every N^r keeps the marginals a permutation cannot change: symmetric, and the counted edges of all pairs together
    assert np.array_equal(got["null"], np.transpose(got["null"], (0, 2, 1)))
    ge, le, sd, sq = ref.accumulate(got["null"], obs)
    assert np.array_equal(got["count_ge"], ge) and np.array_equal(got["count_le"], le)
    assert got["sum_d"].tobytes() == sd.tobytes() and got["sumsq_d"].tobytes() == sq.tobytes()


# ---------------------------------------------------------------- 3. determinism and inputs
def test_two_calls_return_the_same_arrays():
    G = GRAPHS["knn1000"]()
    labels = _labels(G.n, 17, "minus")
    a = _counts(G, labels, 17, seed=5, n_permutations=40, return_null=True)
    b = _counts(G, labels, 17, seed=5, n_permutations=40, return_null=True)
    for k in ("count", "label_counts", "count_ge", "count_le", "sum_d", "sumsq_d", "null"):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_inputs_give_the_same_result():
    import torch
    from flashdeconv_amd.utils.neighborhoods import label_pair_counts, neighborhood_enrichment
    G = GRAPHS["untiled300"]()
    C = 6
    labels = _labels(G.n, C, "minus")
    base = label_pair_counts(labels.astype(np.int32), G.g, n_labels=C, seed=2, n_permutations=21, return_null=True)
    cuda = label_pair_counts(torch.as_tensor(labels, device="cuda:0"), G.g, n_labels=C, seed=2, n_permutations=21, return_null=True)
    adj = label_pair_counts(labels.astype(np.int8), G.A, n_labels=C, seed=2, n_permutations=21, return_null=True)
    inferred = label_pair_counts(torch.as_tensor(labels, device="cuda:0", dtype=torch.int16), G.g, seed=2, n_permutations=21)
    assert torch.is_tensor(cuda["null"]) and cuda["null"].is_cuda and cuda["null"].dtype == torch.int64
    assert isinstance(base["null"], np.ndarray)
    assert np.array_equal(cuda["null"].cpu().numpy(), base["null"]) and np.array_equal(adj["null"], base["null"])
    for k in ("count", "label_counts", "count_ge", "count_le", "sum_d", "sumsq_d"):
        assert np.array_equal(cuda[k], base[k]) and np.array_equal(adj[k], base[k]) and np.array_equal(inferred[k], base[k]), k
    assert np.array_equal(base["count"], ref.pair_counts(G.A, labels, C))
    # the range of device labels is checked on the device and reported, not faulted on
    for bad in (C, -2, 1 << 40):
        lab = torch.as_tensor(labels, device="cuda:0").clone()
        lab[17] = bad
        with pytest.raises(ValueError, match=r"labels must lie in \[-1, 6\)"):
            label_pair_counts(lab, G.g, n_labels=C)
    with pytest.raises(TypeError, match="labels must be integers"):
        label_pair_counts(torch.zeros(G.n, device="cuda:0"), G.g)
    # the assembled entry on the same sums
    out = neighborhood_enrichment(labels, G.g, n_labels=C, n_permutations=21, random_state=2, return_null=True)
    from flashdeconv_amd.utils.neighborhoods import assemble_enrichment
    n, W, sdeg2 = ref.graph_counts(G.A)
    obs = ref.pair_counts(G.A, labels, C)
    null = ref.null_counts(G.A, labels, C, 2, 0, 21)
    want = assemble_enrichment(obs, ref.label_counts(labels, C), n, W, sdeg2, *ref.accumulate(null, obs), 21)
    assert set(out) == set(want) | {"n", "n_edges", "null"} and out["n"] == n and out["n_edges"] == W // 2
    assert np.array_equal(out["null"], null)
    for k, v in want.items():
        np.testing.assert_array_equal(out[k], v, err_msg=k)


# ---------------------------------------------------------------- 4. model and AnnData surface
def _model_adjacency(m):
    indptr, indices = m._graph.to_csr_arrays()
    n = indptr.shape[0] - 1
    return sparse.csr_matrix((np.ones(indices.shape[0], dtype=np.int8), indices, indptr), shape=(n, n))


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def test_model_method():
    import datagen
    from flashdeconv_amd import FlashDeconv
    from flashdeconv_amd.utils.neighborhoods import assemble_enrichment
    from flashdeconv_amd.utils.spatial_stats import _permutation_seed
    Y, X, coords, _ = datagen.count_like(300, 300, 4, 0.1, seed=9)
    R = 19
    rs = np.random.RandomState(4)
    explicit = rs.randint(-1, 3, 300)
    for output in ("numpy", "torch"):
        m = FlashDeconv(sketch_dim=64, max_iter=20).fit(Y, X, coords, output=output)
        A = _model_adjacency(m)
        n, W, sdeg2 = ref.graph_counts(A)
        seed = _permutation_seed(m.random_state)
        dominant = _host(m.get_dominant_cell_type())
        niches = _host(m.get_spatial_niches(3)["labels"])
        for kw, labels, C, sd in (({}, dominant, 4, seed), ({"n_niches": 3}, niches, 3, seed),
                                  ({"labels": explicit, "n_labels": 3, "random_state": 12}, explicit, 3, 12)):
            got = m.get_neighborhood_enrichment(n_permutations=R, **kw)
            obs = ref.pair_counts(A, labels, C)
            null = ref.null_counts(A, labels, C, sd, 0, R)
            want = assemble_enrichment(obs, ref.label_counts(labels, C), n, W, sdeg2, *ref.accumulate(null, obs), R)
            assert set(got) == set(want) | {"n", "n_edges"}, (output, kw)
            for k, v in want.items():
                np.testing.assert_array_equal(got[k], v, err_msg=f"{output} {kw} {k}")
        with pytest.raises(ValueError, match="at most one of labels and n_niches"):
            m.get_neighborhood_enrichment(labels=explicit, n_niches=3)
        with pytest.raises(ValueError, match="labels must have the 300 spots"):
            m.get_neighborhood_enrichment(labels=explicit[:10])
        with pytest.raises(ValueError, match="n_permutations must be an int >= 0"):
            m.get_neighborhood_enrichment(n_permutations=-1)
        assert "p_value" not in m.get_neighborhood_enrichment(n_permutations=0)


def test_deconvolve_writes_the_enrichment_on_request():
    import datagen
    import flashdeconv_amd as fd
    from flashdeconv_amd.io import prepare_data
    case = datagen.anndata_case()
    kw = dict(cell_type_key="celltype", sketch_dim=64, k_neighbors=4, n_hvg=300, n_markers_per_type=20)
    st, rf = datagen.anndata_objects(case)
    assert fd.tl.deconvolve(st, rf, n_niches=3, nhood_enrichment=True, **kw) is None
    res = st.uns["flashdeconv_nhood_enrichment"]
    assert set(res) == {"count", "zscore", "pvalue"} and st.uns["flashdeconv_params"]["nhood_enrichment"] == 999
    Y, X, coords, names, _ = prepare_data(st, rf, cell_type_key="celltype")
    m = fd.FlashDeconv(sketch_dim=64, k_neighbors=4, n_hvg=300, n_markers_per_type=20).fit(Y, X, coords)
    labels = np.asarray(st.obs["flashdeconv_niche"]).astype(np.int64)
    want = m.get_neighborhood_enrichment(labels=labels, n_labels=3, n_permutations=999, random_state=0)
    for key, src in (("count", "count"), ("zscore", "z_sim"), ("pvalue", "p_value")):
        assert list(res[key].index) == [0, 1, 2] and list(res[key].columns) == [0, 1, 2], key
        np.testing.assert_array_equal(res[key].values, want[src], err_msg=key)
    assert np.array_equal(res["count"].values, ref.pair_counts(_model_adjacency(m), labels, 3))
    # without niches: the dominant cell types, indexed by name; the number of permutations follows spatial_permutations
    st2, rf2 = datagen.anndata_objects(case)
    fd.tl.deconvolve(st2, rf2, nhood_enrichment=True, spatial_permutations=50, **kw)
    res2 = st2.uns["flashdeconv_nhood_enrichment"]
    types = [str(t) for t in names]
    assert st2.uns["flashdeconv_params"]["nhood_enrichment"] == 50 and "flashdeconv_niche" not in st2.obs
    dom = m.get_neighborhood_enrichment(n_permutations=50, random_state=0)
    for key, src in (("count", "count"), ("zscore", "z_sim"), ("pvalue", "p_value")):
        assert list(res2[key].index) == types and list(res2[key].columns) == types, key
        np.testing.assert_array_equal(res2[key].values, dom[src], err_msg=key)
