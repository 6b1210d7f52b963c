"""CPU tests of the cell-type expression statistics (flashdeconv_amd/utils/expression.py): the NumPy definition in
tests/expression_ref.py against scipy, the conditions the GPU tests (tests/test_gpu_expression.py) rest on, the argument checks and
the C ABI.  No GPU."""
import numpy as np
import pytest

import expression_ref as er


# ---------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("n,G,K,seed", [(300, 12, 10, 11), (1000, 12, 20, 12), (2000, 10, 30, 13), (5000, 8, 30, 14)])
def test_reference_agrees_with_scipy_nnls(n, G, K, seed):
    """Dirichlet weights, Poisson counts, tol 1e-10, cond(A) <= 100 asserted.  Bound: at the stop every coordinate moved by at most
    tol max(s) in the last sweep, so the gradient on the support is at most ||A||_inf tol max(s) (the KKT bound below) and the
    distance to the minimiser at most ||A_PP^-1||_2 times its 2-norm: sqrt(K) ||A||_inf / lambda_min <= K cond(A) - so
    max |s - s*| <= K cond(A) tol max(s)."""
    from scipy.optimize import nnls
    Y, W = er.generic_case(n, G, K, seed)
    A, B, _, _, _ = er.sums(Y, W)
    cond = np.linalg.cond(A[0])
    assert cond <= 100, cond
    S, n_iter, conv = er.coordinate_descent(A[0], B[0], 0.0, 10000, 1e-10)
    assert conv.all() and n_iter.max() < 10000
    for g in range(G):
        want = nnls(W, Y[:, g], maxiter=10 * K)[0]
        assert np.abs(S[:, g] - want).max() <= K * cond * 1e-10 * want.max(), (g, np.abs(S[:, g] - want).max() / want.max())


def _generic_inputs():
    for (n, G, K, seed) in er.GENERIC_CASES:
        Y, W = er.generic_case(n, G, K, seed)
        yield (n, G, K, seed), Y, W, None, None, 0.0
    n, G, K, seed = er.GENERIC_GROUPS_CASE
    Y, W = er.generic_case(n, G, K, seed)
    g, C = er.group_labels(n, "three", seed)
    yield er.GENERIC_GROUPS_CASE, Y, W, g, C, 0.0
    n, G, K, seed, ridge = er.RIDGE_CASE
    Y, W = er.generic_case(n, G, K, seed)
    yield er.RIDGE_CASE, Y, W, None, None, ridge


def test_every_gpu_solve_input_converges_in_the_reference_and_meets_the_kkt_bound():
    """A condition on the inputs of tests/test_gpu_expression.py: every (group, gene) of every generic case converges within
    max_iter at both tolerances - no GPU test leaves a gene out - and the reference's own KKT residual stays below the bound
    (measured: at most 0.26 of it)."""
    worst = 0.0
    for label, Y, W, g, C, ridge in _generic_inputs():
        A, B, _, _, _ = er.sums(Y, W, g, C)
        for tol in er.GENERIC_TOLS:
            for c in range(A.shape[0]):
                S, n_iter, conv = er.coordinate_descent(A[c], B[c], ridge, er.GENERIC_MAX_ITER, tol)
                assert conv.all(), (label, tol, c, int((~conv).sum()))
                if ridge == 0.0:
                    worst = max(worst, er.kkt_worst(A[c], B[c], S, tol))
    assert worst <= 1.0, worst


def test_exact_cases_are_exact_in_any_order():
    """Weights in sixteenths and counts 0 .. 7: 256 A, 16 B, q and u are integers far below 2^53, so every partial sum of every
    order is exactly representable and the device must return the reference's numbers, not close ones."""
    for n, G, K in ((1000, 300, 130), (4097, 65, 33), (2049, 257, 65)):
        W, Y = er.dyadic_weights(n, K, 3), er.integer_counts(n, G, 3)
        Wi, Yi = np.rint(W * 16).astype(np.int64), Y.astype(np.int64)
        assert np.array_equal(Wi / 16.0, W) and np.array_equal(Yi, Y)
        A, B, q, u, n_rows = er.sums(Y, W)
        assert np.array_equal(A[0] * 256, Wi.T @ Wi) and np.array_equal(B[0] * 16, Wi.T @ Yi)
        assert np.array_equal(q[0], (Yi * Yi).sum(0)) and np.array_equal(u[0], Yi.sum(0)) and n_rows[0] == n
        assert max((Wi * Wi).sum(), (Wi.sum(0) * 7 * n).max(), 49 * n) < 2 ** 40


def test_reference_outputs_follow_the_definition():
    Y, W = er.generic_case(200, 9, 4, 21)
    Y[:, 3] = 0.0                                    # an all-zero gene: tss 0, r2 NaN, s = 0 after one sweep
    g, C = er.group_labels(200, "empty", 21)
    W[g == 1, 2] = 0.0                               # type 2 absent from group 1
    out = er.celltype_expression(Y, W, g, C)
    assert out["expression"].shape == (4, 4, 9) and out["n_iter"].dtype == np.int32 and out["converged"].dtype == bool
    assert out["n_rows"][2] == 0 and not out["estimable"][2].any() and np.all(out["expression"][2] == 0)
    assert np.all(out["tss"][2] == 0) and np.all(np.isnan(out["r2"][2]))
    assert not out["estimable"][1, 2] and np.all(out["expression"][1, 2] == 0) and out["estimable"][1, [0, 1, 3]].all()
    assert np.all(np.isnan(out["r2"][:, 3])) and np.all(out["n_iter"][:, 3] == 1) and out["converged"].all()
    flat = er.celltype_expression(Y, W)
    assert flat["expression"].shape == (4, 9) and flat["gram"].shape == (4, 4) and flat["n_rows"] == 200
    # one sweep: only the all-zero gene has converged
    one = er.celltype_expression(Y, W, max_iter=1)
    assert one["converged"].tolist() == [False, False, False, True, False, False, False, False, False]


# ---------------------------------------------------------------- argument checks (nothing touches a GPU)
def _bad_calls():
    Y, W = np.ones((6, 4), dtype=np.float32), np.full((6, 3), 0.25)
    g = np.array([0, 1, -1, 0, 1, 1])
    return [
        ("Y must be a 2-D", dict(Y=np.ones(6), weights=W)),
        ("at least one gene", dict(Y=np.ones((6, 0)), weights=W)),
        ("weights must be a 2-D", dict(Y=Y, weights=np.ones(6))),
        ("Y has 6 rows but weights has 5", dict(Y=Y, weights=W[:5])),
        ("1 to 272 columns", dict(Y=Y, weights=np.ones((6, 273)))),
        ("1 to 272 columns", dict(Y=Y, weights=np.ones((6, 0)))),
        ("weights must be numeric", dict(Y=Y, weights=np.full((6, 3), "a"))),
        ("weights must be finite", dict(Y=Y, weights=np.where(np.eye(6, 3) > 0, np.nan, W))),
        ("weights must be finite", dict(Y=Y, weights=np.where(np.eye(6, 3) > 0, np.inf, W))),
        ("weights must be non-negative", dict(Y=Y, weights=W - np.eye(6, 3))),
        ("groups must be a 1-D array of 6 labels", dict(Y=Y, weights=W, groups=g[:5])),
        ("groups must be a 1-D array of 6 labels", dict(Y=Y, weights=W, groups=g[:, None])),
        ("groups must be integers", dict(Y=Y, weights=W, groups=g.astype(np.float64))),
        (r"groups must lie in \[-1, 1\), got labels from -2 to 0", dict(Y=Y, weights=W, groups=g - 1)),
        (r"groups must lie in \[-1, 1\)", dict(Y=Y, weights=W, groups=g, n_groups=1)),
        ("n_groups must be an int from 1 to 65535", dict(Y=Y, weights=W, groups=g, n_groups=0)),
        ("n_groups must be an int from 1 to 65535", dict(Y=Y, weights=W, groups=g, n_groups=2.0)),
        ("n_groups = 3 without groups", dict(Y=Y, weights=W, n_groups=3)),
        ("ridge must be a finite number >= 0", dict(Y=Y, weights=W, ridge=-1e-3)),
        ("ridge must be a finite number >= 0", dict(Y=Y, weights=W, ridge=np.nan)),
        ("max_iter must be an int >= 1", dict(Y=Y, weights=W, max_iter=0)),
        ("max_iter must be an int >= 1", dict(Y=Y, weights=W, max_iter=10.0)),
        ("tol must be a finite number > 0", dict(Y=Y, weights=W, tol=0.0)),
        ("tol must be a finite number > 0", dict(Y=Y, weights=W, tol=np.inf)),
        ("Unknown output", dict(Y=Y, weights=W, output="cupy")),
    ]


@pytest.mark.parametrize("match,kw", _bad_calls(), ids=[f"{i}" for i in range(len(_bad_calls()))])
def test_celltype_expression_checks_its_arguments_before_the_gpu(match, kw, monkeypatch):
    from flashdeconv_amd import _lib
    from flashdeconv_amd.utils import expression

    def no_gpu():
        raise AssertionError("the GPU was asked for before the arguments were checked")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    with pytest.raises(ValueError, match=match):
        expression.celltype_expression(**kw)
    sums_kw = {k: v for k, v in kw.items() if k in ("Y", "weights", "groups", "n_groups")}
    if len(sums_kw) == len(kw):
        with pytest.raises(ValueError, match=match):
            expression.weighted_gene_sums(**sums_kw)


def test_nnls_gram_checks_its_arguments_before_the_gpu(monkeypatch):
    from flashdeconv_amd import _lib
    from flashdeconv_amd.utils.expression import nnls_gram

    def no_gpu():
        raise AssertionError("the GPU was asked for before the arguments were checked")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    A, B = np.eye(3), np.ones((3, 5))
    for match, args, kw in [
        ("A must be", (np.eye(4), B), {}), ("A must be", (np.ones((2, 3, 3)), B), {}), ("A must be", (A, np.ones(3)), {}),
        ("A must be", (np.ones((2, 3, 3)), np.ones((3, 3, 5))), {}), ("A must be symmetric", (A + np.eye(3, k=1), B), {}),
        ("A must be finite", (A * np.nan, B), {}), ("B must be finite", (A, B * np.inf), {}),
        ("q must have shape", (A, B), dict(q=np.ones(4))), ("q must be finite", (A, B), dict(q=np.full(5, np.nan))),
        ("1 to 272 types", (np.eye(273), np.ones((273, 2))), {}),
        ("ridge must be", (A, B), dict(ridge=-1.0)), ("max_iter must be", (A, B), dict(max_iter=0)), ("tol must be", (A, B), dict(tol=-1.0)),
    ]:
        with pytest.raises(ValueError, match=match):
            nnls_gram(*args, **kw)


def test_model_method_and_deconvolve_fail_early():
    import flashdeconv_amd as fd
    with pytest.raises(RuntimeError, match="has not been fitted"):
        fd.FlashDeconv().get_celltype_expression(np.ones((3, 2)))
    with pytest.raises(ValueError, match="celltype_expression must be True or False"):
        fd.tl.deconvolve(None, None, celltype_expression="yes")          # before the data is looked at, let alone fitted


# ---------------------------------------------------------------- C ABI and exports
def test_symbols_version_and_exports():
    from flashdeconv_amd import _lib, utils
    from flashdeconv_amd.utils import expression
    lib = _lib.load()
    assert lib.fdx_version() >= 204
    for name, n_args in (("fdx_weighted_gene_sums_dev", 16), ("fdx_weighted_gene_sums_csr_dev", 12), ("fdx_nnls_gram_dev", 14)):
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == n_args
    header = open(_lib.LIB_PATH.replace("flashdeconv_amd/libfdx.so", "include/fdx.h")).read()
    for name in ("fdx_weighted_gene_sums_dev", "fdx_weighted_gene_sums_csr_dev", "fdx_nnls_gram_dev", "FDX_EXPRESSION_SEGMENT_ROWS 2048"):
        assert name in header
    assert "FDX_EXPR_STRIPE_SEGMENTS" in dict(_lib.runtime_switches())
    assert set(expression.__all__) == {"celltype_expression", "weighted_gene_sums", "nnls_gram", "check_request", "MAX_TYPES"}
    for name in ("celltype_expression", "weighted_gene_sums", "nnls_gram"):
        assert name in utils.__all__ and callable(getattr(utils, name))
    # the module and the reference state the same definition
    for text in ("A_c    = sum_i w_i w_i'", "new  = max(0, (b_k - sum_{j != k} A_c[k,j] s_j) / D_k)   if D_k > 0 else 0",
                 "if dmax <= tol * max_k s_k: converged, stop"):
        assert text in expression.__doc__ and text in er.__doc__
