"""Host tests of the marker-gene statistics (flashdeconv_amd/utils/group_genes.py): ``assemble_group_tests`` on the reference's sums
against scipy's tests, every NaN rule, and every argument check ahead of the GPU.  No GPU is needed.

Reference: tests/group_genes_ref.py (``scipy.stats.rankdata``, ``mannwhitneyu(method="asymptotic", use_continuity=False)``,
``ttest_ind(equal_var=False)``)."""
import inspect

import numpy as np
import pytest

import group_genes_ref as gr

# The largest relative deviation of p_value, auc, t, t_dof and t_p_value from scipy over host_cases(), measured on the CPU:
#   p_value 3.0e-15    auc 0    t 1.1e-15    t_dof 1.1e-15    t_p_value 5.1e-15
# The bound is 16 times the largest (and would be capped at 1e-9).
HOST_MEASURED = 5.2e-15
HOST_BOUND = min(16 * HOST_MEASURED, 1e-9)
STATISTICS = ("p_value", "auc", "t", "t_dof", "t_p_value")


def host_cases():
    """(Y, groups, C): mostly-zero counts in float32, half-dense float64 with negatives, continuous values, a small dense case."""
    cases = []
    for seed, (n, G, C, density, dtype) in enumerate([(300, 40, 4, 0.1, np.float32), (500, 30, 3, 0.5, np.float64),
                                                      (200, 25, 5, 1.0, np.float32), (64, 20, 2, 0.3, np.float64)]):
        Y = gr.expression_like(n, G, seed, density, dtype)
        if seed == 1:
            Y = Y - 1.0 * (np.random.RandomState(9).random_sample(Y.shape) < 0.05)
        if seed == 2:
            Y = Y + np.random.RandomState(3).random_sample(Y.shape).astype(dtype)
        cases.append((Y, np.random.RandomState(seed + 10).randint(-1, C, size=n), C))
    return cases


def assert_matches_scipy(got, want, bound, what):
    for key in STATISTICS:
        a, b = np.asarray(got[key]), want[key]
        assert np.array_equal(np.isnan(a), np.isnan(b)), (what, key)
        ok = ~np.isnan(b)
        dev = float((np.abs(a[ok] - b[ok]) / np.maximum(np.abs(b[ok]), 1e-300)).max()) if ok.any() else 0.0
        print(f"{what} {key}: largest relative deviation {dev:.3e} (bound {bound:.3e})")
        assert dev <= bound, (what, key, dev)
    ok = ~np.isnan(want["z_sign"])
    z = np.asarray(got["z_score"])
    assert np.array_equal(np.isnan(z), ~ok) and np.array_equal(np.sign(z[ok]), want["z_sign"][ok]), what


@pytest.mark.parametrize("case", range(4))
def test_assembly_matches_scipy(case):
    from scipy.special import erfc
    from flashdeconv_amd.utils.group_genes import assemble_group_tests
    Y, g, C = host_cases()[case]
    s = gr.sums(Y, g, C)
    u, q = gr.float_sums(Y, g, C)
    got = assemble_group_tests(s["n_rows"], u, q, s["nnz"], s["R2"], s["T"])
    assert_matches_scipy(got, gr.scipy_tests(Y, g, C), HOST_BOUND, f"case {case}")
    assert np.array_equal(got["p_value"], erfc(np.abs(got["z_score"]) / np.sqrt(2.0)), equal_nan=True)
    # the descriptives against their definitions on the rows themselves
    Y64 = gr.dense64(Y)
    for c in range(C):
        mine, rest = Y64[g == c], Y64[(g >= 0) & (g != c)]
        np.testing.assert_allclose(got["mean"][c], mine.mean(axis=0), rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(got["mean_rest"][c], rest.mean(axis=0), rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(got["var"][c], mine.var(axis=0, ddof=1), rtol=1e-10, atol=1e-14)
        np.testing.assert_allclose(got["var_rest"][c], rest.var(axis=0, ddof=1), rtol=1e-10, atol=1e-14)
        assert np.array_equal(got["pct"][c], (mine != 0).sum(axis=0) / mine.shape[0])
        assert np.array_equal(got["pct_rest"][c], (rest != 0).sum(axis=0) / rest.shape[0])
        want_lfc = np.log2((got["mean"][c] + 1e-9) / (got["mean_rest"][c] + 1e-9))
        assert np.array_equal(got["log2_fold_change"][c], want_lfc)


def test_order_q_values_and_pseudocount():
    from flashdeconv_amd.utils.group_genes import assemble_group_tests
    from flashdeconv_amd.utils.spatial_genes import _benjamini_hochberg
    Y, g, C = host_cases()[0]
    Y = Y.copy()
    Y[:, 7] = 2.0                                              # a constant gene: NaN, last in every order
    Y[:, 11] = Y[:, 12]                                        # two genes with the same z: the lower index first
    s = gr.sums(Y, g, C)
    u, q = gr.float_sums(Y, g, C)
    got = assemble_group_tests(s["n_rows"], u, q, s["nnz"], s["R2"], s["T"], pseudocount=1.0)
    G = Y.shape[1]
    assert got["order"].dtype == np.int64 and got["order"].shape == (C, G)
    for c in range(C):
        order, z = got["order"][c], got["z_score"][c]
        assert sorted(order.tolist()) == list(range(G)) and order[-1] == 7 and np.isnan(z[7])
        assert list(order).index(11) + 1 == list(order).index(12)
        alive = z[order[:-1]]
        assert np.all(alive[:-1] >= alive[1:])
        assert np.array_equal(got["q_value"][c], _benjamini_hochberg(got["p_value"][c]), equal_nan=True)
        assert np.array_equal(got["t_q_value"][c], _benjamini_hochberg(got["t_p_value"][c]), equal_nan=True)
        assert np.isnan(got["q_value"][c, 7])
    assert np.array_equal(got["log2_fold_change"], np.log2((got["mean"] + 1.0) / (got["mean_rest"] + 1.0)))


ALL_FLOAT = ("mean", "mean_rest", "var", "var_rest", "pct", "pct_rest", "log2_fold_change", "t", "t_dof", "t_p_value", "t_q_value",
             "auc", "z_score", "p_value", "q_value")
TESTS = ("log2_fold_change", "t", "t_dof", "t_p_value", "t_q_value", "auc", "z_score", "p_value", "q_value")


def _assemble(Y, g, C):
    from flashdeconv_amd.utils.group_genes import assemble_group_tests
    s = gr.sums(Y, g, C)
    u, q = gr.float_sums(Y, g, C)
    with np.errstate(all="raise"):                             # "nothing raises", and nothing warns either
        return assemble_group_tests(s["n_rows"], u, q, s["nnz"], s["R2"], s["T"])


def test_nan_rules_one_group_of_everything():
    Y = gr.expression_like(30, 5, 1, 0.5)
    got = _assemble(Y, np.zeros(30, dtype=np.int64), 1)        # C = 1: the rest is empty
    for key in TESTS + ("mean_rest", "var_rest", "pct_rest"):
        assert np.all(np.isnan(got[key])), key
    np.testing.assert_allclose(got["mean"][0], gr.dense64(Y).mean(axis=0), rtol=1e-13)
    assert not np.any(np.isnan(got["var"])) and not np.any(np.isnan(got["pct"]))
    assert np.array_equal(got["order"][0], np.arange(5))


def test_nan_rules_empty_group_and_single_spot_group():
    Y = gr.expression_like(40, 6, 2, 0.6)
    g = np.random.RandomState(0).randint(0, 2, size=40) * 2    # labels 0 and 2; group 1 is empty; group 3 holds one spot
    g[5] = 3
    got = _assemble(Y, g, 4)
    for key in TESTS + ("mean", "var", "pct"):
        assert np.all(np.isnan(got[key][1])), key
    assert not np.any(np.isnan(got["mean_rest"][1]))           # the rest of an empty group is everything
    assert np.all(np.isnan(got["var"][3])) and np.all(np.isnan(got["t"][3])) and not np.any(np.isnan(got["mean"][3]))
    varying = np.ptp(gr.dense64(Y)[g >= 0], axis=0) > 0
    assert not np.any(np.isnan(got["z_score"][3][varying]))    # one spot against the rest is a rank-sum test still
    assert not np.any(np.isnan(got["z_score"][0][varying])) and not np.any(np.isnan(got["t"][0][varying]))


def test_nan_rules_no_used_spot():
    Y = gr.expression_like(10, 4, 3, 0.5)
    got = _assemble(Y, np.full(10, -1), 3)
    for key in ALL_FLOAT:
        assert got[key].shape == (3, 4) and np.all(np.isnan(got[key])), key
    assert np.array_equal(got["order"], np.tile(np.arange(4), (3, 1)))


def test_nan_rules_constant_and_all_zero_genes():
    Y = gr.expression_like(50, 6, 4, 0.5).astype(np.float64)
    Y[:, 1] = 0.0                                              # an all-zero gene
    Y[:, 3] = 2.5                                              # a constant nonzero gene
    Y[:, 4] = -0.0
    g = np.random.RandomState(1).randint(-1, 3, size=50)
    s = gr.sums(Y, g, 3)
    N = s["n_used"]
    assert s["T"][1] == s["T"][3] == s["T"][4] == N ** 3 - N
    got = _assemble(Y, g, 3)
    for j in (1, 3, 4):
        for key in ("z_score", "p_value", "q_value", "t", "t_dof", "t_p_value", "t_q_value"):
            assert np.all(np.isnan(got[key][:, j])), (j, key)
        assert np.all(got["auc"][:, j] == 0.5)                 # all tied: every rank is the mean rank
        assert np.all(got["var"][:, j] == 0.0) and np.all(got["var_rest"][:, j] == 0.0)
    assert np.all(got["pct"][:, 1] == 0.0) and np.all(got["pct"][:, 3] == 1.0) and np.all(got["pct"][:, 4] == 0.0)
    assert np.all(got["log2_fold_change"][:, 1] == 0.0)
    for j in (0, 2, 5):
        assert not np.any(np.isnan(got["z_score"][:, j]))


def test_sigma_is_decided_on_the_exact_integer():
    """N = 2 000 000 all tied: N^3 - N is not a float64, T / (N (N - 1)) in floating point would not give N + 1."""
    from flashdeconv_amd.utils.group_genes import assemble_group_tests
    N = 2_000_000
    n_rows = np.array([N // 4, N - N // 4])
    R2 = (n_rows * (N + 1))[:, None]
    got = assemble_group_tests(n_rows, np.zeros((2, 1)), np.zeros((2, 1)), np.zeros((2, 1), dtype=np.int64), R2,
                               np.array([N ** 3 - N], dtype=np.int64))
    assert np.all(np.isnan(got["z_score"])) and np.all(got["auc"] == 0.5)
    one_pair = assemble_group_tests(n_rows, np.zeros((2, 1)), np.zeros((2, 1)), np.zeros((2, 1), dtype=np.int64), R2,
                                    np.array([N ** 3 - N - 6], dtype=np.int64))     # a run one shorter: sigma > 0, z = 0
    assert np.all(one_pair["z_score"] == 0.0) and np.all(one_pair["p_value"] == 1.0)


# ---------------------------------------------------------------- argument checks
def _bad_calls():
    Y = np.ones((6, 4), dtype=np.float32)
    g = np.array([0, 1, 0, 1, -1, 1])
    return [
        ("Y must be a 2-D", dict(Y=np.ones(6), groups=g)),
        ("at least one gene", dict(Y=np.ones((6, 0)), groups=g)),
        ("at least one spot", dict(Y=np.ones((0, 4)), groups=g[:0])),
        ("groups must be a 1-D array of 6 labels", dict(Y=Y, groups=g[:5])),
        ("groups must be a 1-D array of 6 labels", dict(Y=Y, groups=g[:, None])),
        ("groups must be integers", dict(Y=Y, groups=g.astype(np.float64))),
        (r"groups must lie in \[-1, 2\)", dict(Y=Y, groups=np.array([0, 1, 0, 1, -2, 1]))),
        (r"groups must lie in \[-1, 2\)", dict(Y=Y, groups=np.array([0, 1, 0, 2, -1, 1]), n_groups=2)),
        ("at most 256 groups", dict(Y=Y, groups=np.array([0, 1, 0, 256, -1, 1]))),
        ("n_groups must be an int from 1 to 256", dict(Y=Y, groups=g, n_groups=257)),
        ("n_groups must be an int from 1", dict(Y=Y, groups=g, n_groups=0)),
        ("n_groups must be an int from 1", dict(Y=Y, groups=g, n_groups=2.0)),
        ("n_groups = 3 without groups", dict(Y=Y, groups=None, n_groups=3)),
        ("pseudocount must be a finite number >= 0", dict(Y=Y, groups=g, pseudocount=-1.0)),
        ("pseudocount must be a finite number >= 0", dict(Y=Y, groups=g, pseudocount=float("nan"))),
        ("pseudocount must be a finite number >= 0", dict(Y=Y, groups=g, pseudocount="1")),
        ("n_top must be an int >= 0 or None", dict(Y=Y, groups=g, n_top=-1)),
        ("n_top must be an int >= 0 or None", dict(Y=Y, groups=g, n_top=2.5)),
        ("Unknown output", dict(Y=Y, groups=g, output="cupy")),
    ]


@pytest.mark.parametrize("match,kw", _bad_calls(), ids=[f"{i}" for i in range(len(_bad_calls()))])
def test_the_entries_check_their_arguments_before_the_gpu(match, kw, monkeypatch):
    from flashdeconv_amd import _lib
    from flashdeconv_amd.utils import group_genes

    def no_gpu():
        raise AssertionError("the GPU was asked for before the arguments were checked")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    with pytest.raises(ValueError, match=match):
        group_genes.rank_genes_groups(**kw)
    if set(kw) <= {"Y", "groups", "n_groups"}:
        with pytest.raises(ValueError, match=match):
            group_genes.gene_group_sums(**kw)


def test_too_many_spots_and_max_sort_bytes_are_refused_before_the_gpu(monkeypatch):
    from flashdeconv_amd import _lib
    from flashdeconv_amd.utils import group_genes

    def no_gpu():
        raise AssertionError("the GPU was asked for before the arguments were checked")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)

    class Tall:                                                # a shape is all the check may look at
        shape = (2_000_001, 3)
    with pytest.raises(ValueError, match="at most 2000000 spots"):
        group_genes.check_request(Tall.shape, None)
    for bad in (0, -5, 1.5, True):
        with pytest.raises(ValueError, match="max_sort_bytes must be an int >= 1 or None"):
            group_genes.gene_group_sums(np.ones((4, 2)), np.zeros(4, dtype=np.int64), max_sort_bytes=bad)
    with pytest.raises(AssertionError, match="the GPU was asked for"):      # a good call gets as far as the device
        group_genes.gene_group_sums(np.ones((4, 2)), np.zeros(4, dtype=np.int64), max_sort_bytes=64)


def test_assemble_checks_its_shapes():
    from flashdeconv_amd.utils.group_genes import assemble_group_tests
    z = np.zeros((2, 3))
    zi = np.zeros((2, 3), dtype=np.int64)
    with pytest.raises(ValueError, match="are required"):
        assemble_group_tests(np.zeros(3, dtype=np.int64), z, z, zi, zi, np.zeros(3, dtype=np.int64))
    with pytest.raises(ValueError, match="are required"):
        assemble_group_tests(np.zeros(2, dtype=np.int64), z, z, zi, zi, np.zeros(2, dtype=np.int64))
    with pytest.raises(ValueError, match="pseudocount"):
        assemble_group_tests(np.zeros(2, dtype=np.int64), z, z, zi, zi, np.zeros(3, dtype=np.int64), pseudocount=-1)


def test_model_method_and_deconvolve_fail_early():
    import flashdeconv_amd as fd
    with pytest.raises(ValueError, match="exactly one of groups and n_niches"):
        fd.FlashDeconv().get_niche_genes(np.ones((3, 2)))
    with pytest.raises(ValueError, match="exactly one of groups and n_niches"):
        fd.FlashDeconv().get_niche_genes(np.ones((3, 2)), groups=np.zeros(3, dtype=int), n_niches=2)
    with pytest.raises(RuntimeError, match="has not been fitted"):
        fd.FlashDeconv().get_niche_genes(np.ones((3, 2)), n_niches=2)
    for bad in ("yes", 1, None):
        with pytest.raises(ValueError, match="niche_genes must be True or False"):
            fd.tl.deconvolve(None, None, niche_genes=bad)          # before the data is looked at, let alone fitted
    with pytest.raises(ValueError, match="niche_genes=True needs n_niches"):
        fd.tl.deconvolve(None, None, niche_genes=True)
    assert inspect.signature(fd.tl.deconvolve).parameters["niche_genes"].default is False
    assert list(inspect.signature(fd.FlashDeconv.get_niche_genes).parameters) == ["self", "Y", "groups", "n_niches", "kw"]
    params = inspect.signature(fd.utils.rank_genes_groups).parameters
    assert list(params) == ["Y", "groups", "n_groups", "pseudocount", "n_top", "output"]
    assert [params[k].default for k in list(params)[2:]] == [None, 1e-9, None, "numpy"]


# ---------------------------------------------------------------- C ABI and exports
def test_symbols_version_and_exports():
    from flashdeconv_amd import _lib, utils
    from flashdeconv_amd.utils import group_genes
    lib = _lib.load()
    assert lib.fdx_version() >= 208
    header = open(_lib.LIB_PATH.replace("flashdeconv_amd/libfdx.so", "include/fdx.h")).read()
    for name, n_args in (("fdx_gene_group_sums_dev", 17), ("fdx_gene_group_sums_csr_dev", 13)):
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == n_args and name in header
    assert set(group_genes.__all__) == {"rank_genes_groups", "gene_group_sums", "assemble_group_tests", "check_request", "MAX_GROUPS",
                                        "MAX_SPOTS"}
    assert group_genes.MAX_GROUPS == 256 and group_genes.MAX_SPOTS == 2_000_000
    for name in ("rank_genes_groups", "gene_group_sums", "assemble_group_tests"):
        assert name in utils.__all__ and callable(getattr(utils, name))
    for text in ("**Inputs.**", "**Sums**", "**Statistics**", "**NaN rules.**", "**Out of scope.**", "eps * mean^2 / var",
                 "by subtraction", "use_continuity=False", "order[c]"):
        assert text in group_genes.__doc__, text
    for text in ("FDX_GENE_GROUP_MAX_ROWS 2000000", "max_sort_bytes", "no floating-point atomic", "C must be 1 .. 256"):
        assert text in header, text
