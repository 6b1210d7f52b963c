"""CPU tests of the ligand-receptor test between spot groups (utils.ligrec): every refusal of ``check_request`` with its exception
type, and ``assemble_ligrec`` against the independent spelling of tests/ligrec_ref.py - the NaN rules (an empty group, a pair that
is not expressed, R = 0, a null that does not vary), Benjamini-Hochberg and the order with ties.  No GPU."""
import numpy as np
import pytest

import ligrec_ref as ref


def _case(seed=0, n=120, G=9, C=4, R=23, empty=None, integer=True):
    rs = np.random.RandomState(seed)
    Y = rs.poisson(0.6, (n, G)).astype(np.float64) if integer else rs.gamma(2.0, 1.0, (n, G)) * (rs.rand(n, G) < 0.3)
    labels = rs.randint(-1, C, n)
    if empty is not None:
        labels[labels == empty] = -1
    pairs = np.array([[0, 1], [1, 0], [2, 2], [0, 1], [3, 8], [8, 2], [0, 5]])
    genes = ref.gene_list(pairs)
    Yg = Y[:, genes]
    counts = ref.label_counts(labels, C)
    u, nnz = ref.group_sums(Yg, labels, C), ref.group_nnz(Yg, labels, C)
    T = ref.statistic(u, counts, pairs, genes)
    null = ref.null_sums(Yg, labels, C, 5, 0, R)
    ge, le, sd, sq, _ = ref.accumulate([ref.statistic(v, counts, pairs, genes) for v in null], T)
    return dict(pairs=pairs, genes=genes, u=u, nnz=nnz, counts=counts, ge=ge, le=le, sd=sd, sq=sq, R=R, T=T)


def _assemble(c, **kw):
    from flashdeconv_amd.utils.ligrec import assemble_ligrec
    R = kw.pop("R", c["R"])
    return assemble_ligrec(c["pairs"], c["genes"], c["u"], c["nnz"], c["counts"], c["ge"], c["le"], c["sd"], c["sq"], R, **kw)


def _same(got, want):
    assert set(got) == set(want), set(got) ^ set(want)
    for k, v in want.items():
        if k == "n_permutations":
            assert got[k] == v
        else:
            assert np.asarray(got[k]).shape == np.asarray(v).shape, k
            np.testing.assert_array_equal(got[k], v, err_msg=k)


@pytest.mark.parametrize("threshold", [0.0, 0.01, 0.35, 1.0])
def test_assemble_matches_the_reference(threshold):
    c = _case()
    got = _assemble(c, threshold=threshold)
    want = ref.host_statistics(c["pairs"], c["genes"], c["u"], c["nnz"], c["counts"], c["ge"], c["le"], c["sd"], c["sq"], c["R"], threshold)
    _same(got, want)
    assert got["means"].dtype == np.float64 and got["expressed"].dtype == bool and got["order"].dtype == np.int64
    assert got["means"].tobytes() == c["T"].tobytes()                      # the three operations, bit for bit
    if threshold == 0.35:
        assert got["expressed"].any() and not got["expressed"].all()       # the threshold cuts through this case
    if threshold == 0.0:
        assert got["expressed"].all() and not np.isnan(got["p_greater"]).any()


def test_an_empty_group_is_nan_everywhere():
    c = _case(seed=1, empty=2)
    assert c["counts"][2] == 0
    got = _assemble(c)
    _same(got, ref.host_statistics(c["pairs"], c["genes"], c["u"], c["nnz"], c["counts"], c["ge"], c["le"], c["sd"], c["sq"], c["R"]))
    for k in ("means", "p_greater", "p_less", "p_value", "z_sim", "null_mean", "null_std", "q_value"):
        assert np.isnan(got[k][:, 2, :]).all() and np.isnan(got[k][:, :, 2]).all(), k
        assert not np.isnan(got[k][:, 0, 1]).all(), k
    assert np.isnan(got["pct"][2]).all() and not got["expressed"][:, 2, :].any() and not got["expressed"][:, :, 2].any()
    # NaN goes last in the order
    tail = got["order"][-int(np.isnan(got["means"]).sum()):]
    assert all(a == 2 or b == 2 for _, a, b in tail.tolist())


def test_without_permutations_only_the_observed_part():
    c = _case(seed=2)
    got = _assemble(c, R=0)
    assert set(got) == {"means", "pct", "expressed", "order"}
    _same(got, ref.host_statistics(c["pairs"], c["genes"], c["u"], c["nnz"], c["counts"], None, None, None, None, 0))
    from flashdeconv_amd.utils.ligrec import assemble_ligrec
    same = assemble_ligrec(c["pairs"], c["genes"], c["u"], c["nnz"], c["counts"])
    np.testing.assert_array_equal(same["order"], got["order"])
    # by descending means, ties (the duplicate pair 0 and 3) by ascending flat index
    m = got["means"][tuple(got["order"].T)]
    assert np.all(np.diff(m) <= 0)
    flat = np.ravel_multi_index(tuple(got["order"].T), got["means"].shape)
    assert all(flat[i] < flat[i + 1] for i in range(len(m) - 1) if m[i] == m[i + 1])
    assert any(m[i] == m[i + 1] for i in range(len(m) - 1))


def test_a_null_that_does_not_vary_has_no_z():
    c = _case(seed=3)
    c["sd"][...] = 0.0
    c["sq"][...] = 0.0
    c["ge"][...] = c["R"]
    c["le"][...] = c["R"]
    got = _assemble(c, threshold=0.0)
    assert np.isnan(got["z_sim"]).all() and (got["null_std"] == 0).all()
    assert (got["p_greater"] == 1.0).all() and (got["p_value"] == 1.0).all() and (got["q_value"] == 1.0).all()
    np.testing.assert_array_equal(got["null_mean"], got["means"])
    _same(got, ref.host_statistics(c["pairs"], c["genes"], c["u"], c["nnz"], c["counts"], c["ge"], c["le"], c["sd"], c["sq"], c["R"], 0.0))


def test_benjamini_hochberg_and_the_order_with_ties():
    c = _case(seed=4, R=7)                                                 # few permutations: many tied p values
    got = _assemble(c, threshold=0.0)
    p = got["p_greater"]
    assert np.unique(p).size < p.size // 4
    np.testing.assert_array_equal(got["q_value"], ref.bh(p))
    assert np.all(got["q_value"] >= p) and np.all(got["q_value"] <= 1.0)
    flat = np.ravel_multi_index(tuple(got["order"].T), p.shape)
    assert sorted(flat.tolist()) == list(range(p.size))
    keys = [(p.ravel()[i], -got["means"].ravel()[i], i) for i in flat]
    assert keys == sorted(keys)
    # p = (1 + count) / (R + 1): never 0, unlike count / R
    assert p.min() >= 1.0 / 8.0
    np.testing.assert_array_equal(p, (1.0 + c["ge"]) / 8.0)
    # means is not zeroed where one of the two means is 0
    c["u"][0, :] = 0.0
    got0 = _assemble(c, threshold=0.0)
    assert (got0["means"][0, 0, 1] == 0.5 * (c["u"][1, 1] / c["counts"][1])) and got0["means"][0, 0, 1] > 0


def test_assemble_refuses_bad_shapes():
    from flashdeconv_amd.utils.ligrec import assemble_ligrec
    c = _case(seed=5)
    args = [c["pairs"], c["genes"], c["u"], c["nnz"], c["counts"], c["ge"], c["le"], c["sd"], c["sq"], c["R"]]
    for i, bad in ((0, c["pairs"][:, :1]), (2, c["u"][:, :-1]), (3, c["nnz"][:-1]), (4, c["counts"][:-1]), (5, c["ge"][:-1]),
                   (8, c["sq"][..., :-1]), (9, -1), (9, 1.5)):
        a = list(args)
        a[i] = bad
        with pytest.raises(ValueError):
            assemble_ligrec(*a)
    with pytest.raises(ValueError, match="are needed"):
        assemble_ligrec(*args[:5], n_permutations=3)
    with pytest.raises(ValueError, match="does not list"):
        assemble_ligrec(np.array([[0, 7]]), c["genes"], c["u"], c["nnz"], c["counts"])
    for bad in (-0.1, 1.1, "a", None, True, float("nan")):
        with pytest.raises(ValueError, match="threshold"):
            assemble_ligrec(*args, threshold=bad)


def test_check_request_refusals():
    from flashdeconv_amd.utils import ligrec
    n, G = 50, 12
    labels = np.arange(n) % 3
    pairs = np.array([[0, 1], [5, 5], [0, 1]])
    out = ligrec.check_request((n, G), pairs, labels, None, 9, 2, 4, 0.5)
    assert out[0].dtype == np.int32 and out[0].shape == (3, 2) and out[1].tolist() == [0, 1, 5] and out[1].dtype == np.int32
    assert out[2].dtype == np.int32 and out[3:] == (3, 9, 2, 4, 0.5)
    assert ligrec.check_request((n, G), pairs.tolist(), labels.astype(np.int8), 64)[3] == 64

    def refused(exc, match, Y_shape=(n, G), pairs=pairs, labels=labels, n_labels=None, **kw):
        with pytest.raises(exc, match=match):
            ligrec.check_request(Y_shape, pairs, labels, n_labels, **kw)

    refused(ValueError, "2-D", Y_shape=(n,))
    refused(ValueError, "at least one gene", Y_shape=(n, 0))
    refused(ValueError, "spots", Y_shape=(0, G), labels=labels[:0])
    refused(ValueError, "spots", Y_shape=(ligrec.MAX_SPOTS + 1, G))
    refused(ValueError, r"\(P, 2\)", pairs=np.zeros((3, 3), dtype=np.int64))
    refused(ValueError, r"\(P, 2\)", pairs=np.zeros(4, dtype=np.int64))
    refused(ValueError, "at least one pair", pairs=np.zeros((0, 2), dtype=np.int64))
    refused(ValueError, "integer dtype", pairs=np.zeros((2, 2)))
    refused(ValueError, r"outside \[0, 12\)", pairs=np.array([[0, 12]]))
    refused(ValueError, r"outside \[0, 12\)", pairs=np.array([[-1, 3]]))
    refused(TypeError, "labels must be integers", labels=labels.astype(np.float64))
    refused(ValueError, "1-D", labels=labels.reshape(5, 10))
    refused(ValueError, "one entry per spot", labels=labels[:-1])
    refused(ValueError, r"labels must lie in \[-1, 3\)", labels=labels - 2, n_labels=3)
    refused(ValueError, r"labels must lie in \[-1, 2\)", n_labels=2)
    refused(ValueError, "at most 64 labels", labels=np.arange(n) + 20)
    for bad in (0, 65, 2.0, True):
        refused(ValueError, "n_labels must be an int from 1 to 64", n_labels=bad)
    for name in ("n_permutations", "first_perm", "max_batch"):
        for bad in (-1, 1.0, True, None):
            refused(ValueError, f"{name} must be an int >= 0", **{name: bad})
    for bad in (-0.01, 1.01, "x", None, False):
        refused(ValueError, "threshold must be a number in", threshold=bad)
    # the caps: distinct genes and P * C^2
    big = np.stack([np.arange(ligrec.MAX_GENES + 1), np.arange(ligrec.MAX_GENES + 1)], axis=1)
    refused(ValueError, "at most 4096 distinct genes", Y_shape=(n, 5000), pairs=big)
    ligrec.check_request((n, 5000), big[:-1], labels)                      # 4096 genes, 4096 * 9 triples: accepted
    many = np.zeros((ligrec.MAX_STATISTICS // (64 * 64) + 1, 2), dtype=np.int64)
    refused(ValueError, r"P \* C\^2 must be at most 4194304", pairs=many, n_labels=64)
    ligrec.check_request((n, G), many[:-1], labels, 64)
    assert ligrec.MAX_STATISTICS == 1 << 22 and ligrec.MAX_GENES == 4096


def test_the_entries_refuse_before_the_gpu():
    """Bad arguments raise from the public entries without a device (none is needed to reach the checks)."""
    from flashdeconv_amd import utils
    from flashdeconv_amd.utils import ligrec
    Y = np.zeros((20, 4), dtype=np.float32)
    labels = np.zeros(20, dtype=np.int64)
    pairs = [[0, 1]]
    for fn in (ligrec.label_gene_sums, ligrec.ligand_receptor_test):
        with pytest.raises(ValueError, match="outside"):
            fn(Y, labels, [[0, 4]])
        with pytest.raises(ValueError, match="one entry per spot"):
            fn(Y, labels[:5], pairs)
        with pytest.raises(ValueError, match="n_permutations"):
            fn(Y, labels, pairs, n_permutations=-3)
        with pytest.raises(ValueError, match="return_null"):
            fn(Y, labels, pairs, return_null=1)
        with pytest.raises(ValueError, match="2-D"):
            fn(Y[0], labels, pairs)
    with pytest.raises(ValueError, match="threshold"):
        ligrec.ligand_receptor_test(Y, labels, pairs, threshold=2)
    with pytest.raises(ValueError, match="n_top"):
        ligrec.ligand_receptor_test(Y, labels, pairs, n_top=-1)
    with pytest.raises(ValueError, match="max_gather_bytes"):
        ligrec.label_gene_sums(Y, labels, pairs, max_gather_bytes=0)
    with pytest.raises(ValueError, match="random_state"):
        ligrec.ligand_receptor_test(Y, labels, pairs, random_state=-1)
    assert set(ligrec.__all__) >= {"ligand_receptor_test", "label_gene_sums", "assemble_ligrec", "check_request", "MAX_STATISTICS"}
    for name in ("ligand_receptor_test", "label_gene_sums", "assemble_ligrec"):
        assert name in utils.__all__ and callable(getattr(utils, name))


def test_the_library_exports_the_entries():
    from flashdeconv_amd import _lib
    lib = _lib.load()
    assert lib.fdx_version() >= 211
    assert hasattr(lib, "fdx_label_gene_sums_dev") and hasattr(lib, "fdx_label_gene_sums_csr_dev")


def test_deconvolve_refuses_bad_ligrec_arguments_before_the_fit(monkeypatch):
    import datagen
    import flashdeconv_amd as fd
    from flashdeconv_amd.core import deconv
    monkeypatch.setattr(deconv.FlashDeconv, "fit_transform", lambda *a, **k: pytest.fail("the fit was reached"))
    case = datagen.anndata_case()
    st, rf = datagen.anndata_objects(case)
    from flashdeconv_amd.io import prepare_data
    genes = prepare_data(st, rf, cell_type_key="celltype")[4]
    good = (str(genes[0]), str(genes[1]))
    for bad, match in (([], "non-empty sequence"), ([("a",)], "non-empty sequence"), ([(good[0], "no such gene")], "names the gene")):
        with pytest.raises(ValueError, match=match):
            fd.tl.deconvolve(st, rf, cell_type_key="celltype", ligrec_pairs=bad)
    for bad in (-1, 2.5, True):
        with pytest.raises(ValueError, match="ligrec_permutations"):
            fd.tl.deconvolve(st, rf, cell_type_key="celltype", ligrec_pairs=[good], ligrec_permutations=bad)
