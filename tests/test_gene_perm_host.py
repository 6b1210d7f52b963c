"""CPU tests of the permutation test per gene (flashdeconv_amd/utils/gene_permutations.py): the package's host arithmetic against
the NumPy definition in tests/gene_perm_ref.py, the NaN rules, the argument checks, the C ABI, and the conditions on the reference
that the GPU tests (tests/test_gpu_gene_perm.py) rest on.  No GPU."""
import numpy as np
import pytest
from scipy import sparse

import fdx_oracle as orc
import fit_tail_ref
import gene_perm_ref as gr
import spatial_genes_ref as sr

_REF = {}


def _rook_grid(rows=25, cols=24):
    """The rook adjacency of a rows x cols lattice, spot i at x = i % cols, y = i // cols (the order of planted_case)."""
    path = lambda k: sparse.diags([np.ones(k - 1), np.ones(k - 1)], [-1, 1])      # noqa: E731
    return sparse.csr_matrix(sparse.kron(sparse.identity(rows), path(cols)) + sparse.kron(path(rows), sparse.identity(cols)))


def _knn_adjacency(n, seed=11):
    return orc.knn_graph_kdtree(fit_tail_ref.tie_free_coords(n, 2, seed), 6)


def _case(key, make_Y, A, seed, R):
    """(Y, observed, null) of a case, computed once and shared read-only."""
    if key not in _REF:
        Y = make_Y()
        o, null = gr.observed(Y, A), gr.null_sums(Y, A, seed, 0, R)
        for a in [Y, null] + [v for v in o.values() if isinstance(v, np.ndarray)]:
            a.setflags(write=False)
        _REF[key] = (Y, o, null)
    return _REF[key]


def _assemble(fn, o, **kw):
    return fn(o["n"], o["W"], *(o[name] for name in gr.OBS_PLANES), **kw)


def _assert_same(got, want):
    assert set(got) == set(want)
    for key in want:
        a, b = np.asarray(got[key]), np.asarray(want[key])
        assert a.shape == b.shape and a.dtype == b.dtype, (key, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(a, b, equal_nan=True), key


# ---------------------------------------------------------------- the package's host arithmetic
@pytest.mark.parametrize("n,S,seed,constant,R", [(300, 7, 0, (), 19), (600, 12, 1, (2, 5), 7), (65, 5, 2, (0,), 33), (4, 3, 3, (), 5),
                                                  (3, 3, 4, (), 5), (300, 4, 5, (), 0)])
def test_assemble_gene_permutation_equals_the_reference(n, S, seed, constant, R):
    from flashdeconv_amd.utils.gene_permutations import assemble_gene_permutation, merge_null_counts
    A = _knn_adjacency(n) if n > 4 else sparse.csr_matrix(np.ones((n, n)) - np.eye(n))
    for Y in (gr.generic_case(n, S, seed, constant), gr.exact_case(n, S, seed)):
        o, null = gr.observed(Y, A), gr.null_sums(Y, A, 9, 2, R)
        want = _assemble(gr.assemble, o, null=null)
        _assert_same(_assemble(assemble_gene_permutation, o, null=null), want)
        assert set(want) == ({"morans_i", "gearys_c", "n_permutations"} if R == 0 else
                             {"morans_i", "gearys_c", "n_permutations", "p_sim", "p_sim_less", "gearys_p_sim", "z_sim", "null_mean",
                              "null_std", "q_sim"})
        if R:
            # merged chunk by chunk: the same bits, the null never kept whole
            counts = None
            for lo in range(0, R, 3):
                counts = merge_null_counts(counts, o["n"], o["W"], *(o[name] for name in gr.OBS_PLANES), null[lo:lo + 3])
            _assert_same(_assemble(assemble_gene_permutation, o, counts=counts), want)
            live = ~np.isnan(want["morans_i"])
            assert np.all((want["p_sim"][live] >= 1 / (R + 1)) & (want["p_sim"][live] <= 1)) and np.all(want["q_sim"][live] >= want["p_sim"][live])
            assert np.all(want["p_sim"][live] + want["p_sim_less"][live] >= 1)       # every permutation is counted on a side
        # the observed part is the per-gene module's
        s = sr.planes(Y, A)
        full = sr.assemble(s["n"], s["W"], s["sum_deg_sq"], *(s[name] for name in sr.PLANES))
        assert np.array_equal(want["morans_i"], full["morans_i"], equal_nan=True)
        assert np.array_equal(want["gearys_c"], full["gearys_c"], equal_nan=True)


def test_nan_rules():
    from flashdeconv_amd.utils.gene_permutations import assemble_gene_permutation
    keys = ("morans_i", "gearys_c", "p_sim", "p_sim_less", "gearys_p_sim", "z_sim", "null_mean", "null_std", "q_sim")
    A = _knn_adjacency(100)
    Y = gr.generic_case(100, 3, 5)
    Y[:, 1] = np.float64(np.float32(0.1))                   # constant: decided by ymin == ymax, whatever m2 rounds to
    o, null = gr.observed(Y, A), gr.null_sums(Y, A, 0, 0, 9)
    assert o["q"][1] - o["u"][1] ** 2 / 100 != 0.0
    for fn in (gr.assemble, assemble_gene_permutation):
        out = _assemble(fn, o, null=null)
        for key in keys:
            assert np.isnan(out[key][1]) and not np.isnan(out[key][[0, 2]]).any(), key
    A0 = sparse.csr_matrix((100, 100))                      # W = 0: nothing has a statistic
    o0, null0 = gr.observed(Y, A0), gr.null_sums(Y, A0, 0, 0, 4)
    for fn in (gr.assemble, assemble_gene_permutation):
        out = _assemble(fn, o0, null=null0)
        assert all(np.isnan(out[key]).all() for key in keys)
    Y1, A1 = gr.generic_case(1, 2, 6), sparse.csr_matrix((1, 1))                   # n = 1
    for fn in (gr.assemble, assemble_gene_permutation):
        out = _assemble(fn, gr.observed(Y1, A1), null=gr.null_sums(Y1, A1, 0, 0, 3))
        assert all(np.isnan(out[key]).all() for key in keys)
    # a null that does not vary: z_sim is NaN, the p values are 1
    flat = np.broadcast_to(np.stack([o["P"], o["D"], o["H"]])[None], (5, 3, 3)).copy()
    for fn in (gr.assemble, assemble_gene_permutation):
        out = _assemble(fn, o, null=flat)
        assert np.isnan(out["z_sim"]).all() and np.array_equal(out["null_std"][[0, 2]], [0.0, 0.0])
        assert np.array_equal(out["p_sim"][[0, 2]], [1.0, 1.0]) and np.array_equal(out["gearys_p_sim"][[0, 2]], [1.0, 1.0])
    with pytest.raises(ValueError, match="seven sums"):
        assemble_gene_permutation(3, 2, *[np.ones(2)] * 6, np.ones(3))
    with pytest.raises(ValueError, match=r"\(R, 3, S\)"):
        _assemble(assemble_gene_permutation, o, null=np.zeros((4, 2, 3)))
    with pytest.raises(ValueError, match="not both"):
        _assemble(assemble_gene_permutation, o, null=null, counts={})


# ---------------------------------------------------------------- conditions on the reference alone
def test_exact_case_null_is_exact_in_any_order():
    """exact_case(600, 64, 3) on the 25 x 24 rook grid: every term of P_r, D_r, H_r is an integer far below 2^53, so any
    summation order is exact and the device must return the reference's numbers."""
    A = _rook_grid()
    Y, o, null = _case("exact", lambda: gr.exact_case(600, 64, 3), A, 0, 999)
    assert np.array_equal(np.rint(Y), Y) and Y.min() >= 0 and Y.max() <= 7 and int(sr.degrees(A).max()) == 4
    assert np.array_equal(np.rint(null), null)
    print(f"largest null sum {null.max():.0f}")
    assert null.max() < 2 ** 20 and 7 ** 2 * 600 * (1 + 4) < 2 ** 53
    # integer arithmetic agrees
    from flashdeconv_amd.utils.spatial_stats import permutation_indices
    Yi, Ai, deg = Y.astype(np.int64), A.astype(np.int64), sr.degrees(A)
    for r in (0, 998):
        V = Yi[permutation_indices(0, r, 600)]
        assert np.array_equal(null[r], np.stack([(V * (Ai @ V)).sum(0), deg @ V, deg @ V ** 2]))
    # a permutation moves values, it makes none: the invariants of the definition
    assert np.array_equal(np.sort(Yi[permutation_indices(0, 5, 600)], axis=0), np.sort(Yi, axis=0))


def test_planted_case_separates_in_the_reference():
    """25 x 24 rook grid, seed 0, R = 199: the gradient's I is never reached by a permutation, the shuffled gene's often."""
    A = _rook_grid()
    Y, o, null = _case("planted", gr.planted_case, A, 0, 199)
    out = _assemble(gr.assemble, o, null=null)
    print("planted p_sim", out["p_sim"], "z_sim", out["z_sim"])
    assert out["p_sim"][0] == 1 / 200 and out["p_sim"][1] > 0.2 and np.isnan(out["p_sim"][2])
    assert out["gearys_p_sim"][0] == 1 / 200 and out["z_sim"][0] > 10 and out["q_sim"][0] == 1 / 100
    # the queen grid of the GPU tests (tests/gpu_graphs._grid) separates likewise
    yy, xx = np.mgrid[0:25, 0:24]
    Aq = orc.grid_graph(np.stack([xx.ravel(), yy.ravel()], 1).astype(np.float64))
    outq = _assemble(gr.assemble, gr.observed(Y, Aq), null=gr.null_sums(Y, Aq, 0, 0, 199))
    print("planted (8 neighbours) p_sim", outq["p_sim"])
    assert outq["p_sim"][0] == 1 / 200 and outq["p_sim"][1] > 0.2 and np.isnan(outq["p_sim"][2])


def test_null_moments_match_the_randomisation_moments():
    """exact_case(600, 64, 3), seed 0, R = 999: the null's standard deviation against Cliff and Ord's exact variance, its mean
    against E = -1 / (n - 1).  A non-uniform permutation would miss both."""
    A = _rook_grid()
    Y, o, null = _case("exact", lambda: gr.exact_case(600, 64, 3), A, 0, 999)
    out = _assemble(gr.assemble, o, null=null)
    s = sr.planes(Y, A)
    full = sr.assemble(s["n"], s["W"], s["sum_deg_sq"], *(s[name] for name in sr.PLANES))
    ratio = out["null_std"] / np.sqrt(full["variance_i_rand"])
    dev = np.abs(out["null_mean"] - full["expected_i"]) / (out["null_std"] / np.sqrt(999.0))
    print(f"null_std / sqrt(variance_i_rand) in [{ratio.min():.3f}, {ratio.max():.3f}]; worst mean deviation {dev.max():.2f} standard errors")
    assert np.all((ratio >= 0.9) & (ratio <= 1.1))
    assert np.all(dev <= 4.0)


# ---------------------------------------------------------------- argument checks (nothing touches a GPU)
def _bad_calls():
    Y = np.ones((6, 4), dtype=np.float32)
    A = sparse.csr_matrix(np.roll(np.eye(6), 1, axis=1) + np.roll(np.eye(6), -1, axis=1))
    return [
        (ValueError, "Y must be a 2-D", dict(Y=np.ones(6), graph=A)),
        (ValueError, "at least one gene", dict(Y=np.ones((6, 0)), graph=A)),
        (ValueError, "at least one spot", dict(Y=np.ones((0, 4)), graph=sparse.csr_matrix((0, 0)))),
        (ValueError, "values has 6 rows but the graph has 5 spots", dict(Y=Y, graph=A[:5, :5])),
        (ValueError, "must be symmetric", dict(Y=Y, graph=sparse.csr_matrix(np.roll(np.eye(6), 1, axis=1)))),
        (TypeError, "graph must be a fitted FlashDeconv", dict(Y=Y, graph=np.eye(6))),
        (ValueError, "genes must be a 1-D", dict(Y=Y, graph=A, genes=np.zeros((2, 2), dtype=np.int64))),
        (ValueError, "integer dtype", dict(Y=Y, graph=A, genes=np.array([0.0, 1.0]))),
        (ValueError, "at least one gene index", dict(Y=Y, graph=A, genes=np.zeros(0, dtype=np.int64))),
        (ValueError, r"gene index 4 outside \[0, 4\)", dict(Y=Y, graph=A, genes=[0, 4])),
        (ValueError, r"gene index -1 outside \[0, 4\)", dict(Y=Y, graph=A, genes=[-1, 2])),
        (ValueError, "gene index 2 twice", dict(Y=Y, graph=A, genes=[2, 1, 2])),
        (ValueError, "n_permutations must be an int >= 0", dict(Y=Y, graph=A, n_permutations=-1)),
        (ValueError, "n_permutations must be an int >= 0", dict(Y=Y, graph=A, n_permutations=9.0)),
        (ValueError, "n_permutations must be an int >= 0", dict(Y=Y, graph=A, n_permutations=True)),
    ]


@pytest.mark.parametrize("error,match,kw", _bad_calls(), ids=[f"{i}" for i in range(len(_bad_calls()))])
def test_the_entries_check_their_arguments_before_the_gpu(error, match, kw, monkeypatch):
    from flashdeconv_amd import _lib
    from flashdeconv_amd.utils import gene_permutations

    def no_gpu():
        raise AssertionError("the GPU was asked for before the arguments were checked")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    with pytest.raises(error, match=match):
        gene_permutations.spatial_gene_permutation_test(**kw)
    with pytest.raises(error, match=match):
        gene_permutations.gene_permutation_sums(**kw)


def test_further_checks_and_the_model_and_deconvolve_fail_early(monkeypatch):
    import flashdeconv_amd as fd
    from flashdeconv_amd import _lib
    from flashdeconv_amd.utils import gene_permutations as gp
    monkeypatch.setattr(_lib, "require_gpu", lambda: (_ for _ in ()).throw(AssertionError("the GPU was asked for")))
    Y = np.ones((6, 4), dtype=np.float32)
    A = sparse.csr_matrix(np.roll(np.eye(6), 1, axis=1) + np.roll(np.eye(6), -1, axis=1))
    for match, kw in (("first_perm must be an int >= 0", dict(first_perm=-1)), ("max_batch must be an int >= 0", dict(max_batch=-2)),
                      ("max_lds_bytes must be an int >= 1", dict(max_lds_bytes=0)),
                      ("max_gather_bytes must be an int >= 1", dict(max_gather_bytes=0)), ("random_state must be in", dict(seed=-1))):
        with pytest.raises(ValueError, match=match):
            gp.gene_permutation_sums(Y, A, **kw)
    with pytest.raises(ValueError, match="n_top must be an int >= 0 or None"):
        gp.spatial_gene_permutation_test(Y, A, n_top=-1)
    genes, R, first, batch, lds, gather = gp.check_request((6, 4), [3, 1], 5, 2, 1, None, 4096)
    assert genes.dtype == np.int32 and list(genes) == [3, 1] and (R, first, batch, lds, gather) == (5, 2, 1, 0, 4096)
    assert list(gp.check_request((6, 4))[0]) == [0, 1, 2, 3]
    with pytest.raises(ValueError, match="n_permutations must be an int >= 0"):
        fd.FlashDeconv().get_spatially_variable_genes(np.ones((3, 2)), n_permutations=-1)      # before "has not been fitted"
    with pytest.raises(ValueError, match="gene index 2 outside"):
        fd.FlashDeconv().get_spatially_variable_genes(np.ones((3, 2)), n_permutations=5, permutation_genes=[2])
    with pytest.raises(RuntimeError, match="has not been fitted"):
        fd.FlashDeconv().get_spatially_variable_genes(np.ones((3, 2)), n_permutations=5)
    # without permutations the call is today's: a gene list that is never used is not looked at, today's errors come first
    for kw in (dict(permutation_genes=[2]), dict(permutation_genes="no list")):
        with pytest.raises(RuntimeError, match="has not been fitted"):
            fd.FlashDeconv().get_spatially_variable_genes(np.ones((3, 2)), n_permutations=0, **kw)
    with pytest.raises(RuntimeError, match="has not been fitted"):
        fd.FlashDeconv().get_spatially_variable_genes(np.ones(3))
    for bad in (-1, 2.0, True, "9"):
        with pytest.raises(ValueError, match="gene_permutations must be an int >= 0"):
            fd.tl.deconvolve(None, None, spatial_genes=True, gene_permutations=bad)        # before the data is looked at
    with pytest.raises(ValueError, match="needs spatial_genes=True"):
        fd.tl.deconvolve(None, None, gene_permutations=9)


def test_order_by_p_then_z():
    from flashdeconv_amd.utils.gene_permutations import _order
    p = np.array([0.2, np.nan, 0.05, 0.2, 0.05, 0.2])
    z = np.array([1.0, np.nan, 2.0, 3.0, np.nan, 1.0])
    got = _order(p, z)
    assert got.dtype == np.int64 and list(got) == [2, 4, 3, 0, 5, 1]


# ---------------------------------------------------------------- C ABI and exports
def test_symbols_version_and_exports():
    import inspect
    import flashdeconv_amd as fd
    from flashdeconv_amd import _lib, utils
    from flashdeconv_amd.utils import gene_modules, gene_pairs, gene_permutations, spatial_genes
    lib = _lib.load()
    assert lib.fdx_version() >= 209
    for name, n_args in (("fdx_gene_spatial_perm_dev", 19), ("fdx_gene_spatial_perm_csr_dev", 15)):
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == n_args
    root = _lib.LIB_PATH.replace("flashdeconv_amd/libfdx.so", "")
    header = open(root + "include/fdx.h").read()
    for name in ("fdx_gene_spatial_perm_dev", "fdx_gene_spatial_perm_csr_dev", "null_dev (n_perm, 3, S)", "obs_dev (7, S)"):
        assert name in header
    assert "gene_perm_kernels.cpp" in open(root + "flashdeconv_amd/csrc/Makefile").read()
    assert "fdx_gene_spatial_perm_dev" in open(root + "INTEGRATION.md").read()
    assert gene_permutations.OBS_PLANES == gr.OBS_PLANES and gene_permutations.NULL_PLANES == gr.NULL_PLANES
    for name in ("spatial_gene_permutation_test", "gene_permutation_sums", "assemble_gene_permutation"):
        assert name in utils.__all__ and name in gene_permutations.__all__ and callable(getattr(utils, name))
    assert "check_request" in gene_permutations.__all__
    # the module and the reference state the same definition, word for word
    start, end = "**Definition.**", "allowed and returns the observed part only."
    block = gr.__doc__[gr.__doc__.index(start):gr.__doc__.index(end) + len(end)]
    assert len(block) > 1500 and block in gene_permutations.__doc__
    for text in ("I(P, D) = (n / W) (P - 2 m D + m^2 W) / m2", "C(P, H) = ((n - 1) / (2 W)) (2 H - 2 P) / m2",
                 "p_sim        = (1 + #{r : I_r >= I_obs}) / (R + 1)", "gearys_p_sim = (1 + #{r : C_r <= C_obs}) / (R + 1)"):
        assert text in block
    # the per-gene module is as it was, and points here; the pair modules keep their sentence
    assert set(spatial_genes.__all__) == {"spatially_variable_genes", "gene_spatial_sums", "assemble_genes", "check_request", "PLANES"}
    assert "permutation p values per gene" in spatial_genes.__doc__ and "utils.gene_permutations" in spatial_genes.__doc__
    assert "Permutation p values per pair" in gene_pairs.__doc__ and "permutation p values per pair" in gene_modules.__doc__
    params = list(inspect.signature(fd.FlashDeconv.get_spatially_variable_genes).parameters)
    assert params[-4:] == ["n_permutations", "random_state", "permutation_genes", "kw"]
    sig = inspect.signature(fd.tl.deconvolve).parameters
    assert sig["gene_permutations"].default == 0 and sig["gene_permutations"].kind is inspect.Parameter.KEYWORD_ONLY
