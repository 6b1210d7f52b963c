"""CPU tests of the local spatial statistics (flashdeconv_amd/utils/local_stats.py): the conditional draw against its restatement in
plain Python integers (tests/local_stats_ref.py), its uniformity, the host assembly against the definitions written out element
by element, the NumPy null against sampling-without-replacement theory, the argument checks and the declarations."""
import os
import re

import numpy as np
import pytest
from scipy import sparse

import local_stats_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- 1. the draw
@pytest.mark.parametrize("n", [2, 3, 5, 64, 65, 257, 4097])
def test_conditional_indices_equal_the_restatement(n):
    from flashdeconv_amd.utils.local_stats import conditional_indices
    for count in (0, 1, n - 1):
        for seed, r, spot in ((0, 0, 0), (12345, 7, n - 1), (2 ** 64 - 1, 998, n // 2)):
            got = conditional_indices(seed, r, spot, n, count)
            assert got.dtype == np.int64 and got.shape == (count,)
            assert list(got) == list(ref.conditional_indices(seed, r, spot, n, count)), (seed, r, spot, count)
            assert len(set(got.tolist())) == count and np.all((got >= 0) & (got < n)) and spot not in got
            assert np.array_equal(got, conditional_indices(seed, r, spot, n, count))          # deterministic
    full = conditional_indices(5, 2, 1, n, n - 1)
    assert sorted(full.tolist()) == [i for i in range(n) if i != 1]                          # count = n - 1 draws everybody else
    if n >= 64:
        base = conditional_indices(5, 2, 1, n, 6)
        for other in ((5, 3, 1), (5, 2, 2), (6, 2, 1)):
            assert not np.array_equal(base, conditional_indices(*other, n, 6)), other
        assert np.array_equal(base, full[:6])                                                # a shorter draw is a prefix


def test_batched_restatement_equals_the_loop():
    from flashdeconv_amd.utils.local_stats import conditional_indices
    for n, count, spot in ((5, 4, 2), (64, 6, 0), (257, 256, 256), (500, 6, 17)):
        b = ref.conditional_indices_batch(9, 3, 5, spot, n, count)
        for j in range(5):
            assert tuple(b[j]) == ref.conditional_indices(9, 3 + j, spot, n, count)
            assert np.array_equal(b[j], conditional_indices(9, 3 + j, spot, n, count))


def test_conditional_indices_argument_checks():
    from flashdeconv_amd.utils.local_stats import conditional_indices
    for args in ((0, 0, 0, 5, 5), (0, 0, 0, 5, -1), (0, -1, 0, 5, 2), (-1, 0, 0, 5, 2), (0, 0, -1, 5, 2), (0, 0, 5, 5, 2),
                 (0, 0, 0, 0, 0), (0, 0, 0, -3, 0), (0, 0, 0, 1, 1), (0, 0, 0, 2 ** 31, 2)):
        with pytest.raises(ValueError):
            conditional_indices(*args)
    assert conditional_indices(0, 0, 0, 1, 0).shape == (0,)


@pytest.mark.parametrize("n,R,chi_recorded", [(50, 2000, 2190.4), (37, 2000, 1144.4), (130, 1000, 16116.0)])
def test_draws_are_uniform_over_the_other_spots(n, R, chi_recorded):
    """Inclusion counts of every ordered pair (spot, other) over R draws of d = 6 with seed 3: chi^2 against R d / (n - 1) has
    n (n - 2) degrees of freedom (n - 2 per spot: the counts of a spot sum to R d) and, the d draws of one permutation being
    without replacement, the expectation dof (1 - d / (n - 1)).  Held to 5 sqrt(2 dof); the figures recorded in DESIGN.md
    (2190.4 / 1144.4 / 16116.0, 1.2 - 1.4 sqrt(2 dof) away) are reproduced."""
    from flashdeconv_amd.utils.local_stats import conditional_indices
    d, seed = 6, 3
    counts = np.zeros((n, n))
    for i in range(n):
        draws = ref.conditional_indices_batch(seed, 0, R, i, n, d)                           # the R keys at once: seconds, not a minute
        for r in (0, (7 * i + 1) % R, R - 1):
            assert np.array_equal(draws[r], conditional_indices(seed, r, i, n, d)), (i, r)
        np.add.at(counts[i], draws.ravel(), 1)
    assert not counts.diagonal().any() and np.all(counts.sum(1) == R * d)
    e = R * d / (n - 1.0)
    chi = float((((counts - e) ** 2) / e)[~np.eye(n, dtype=bool)].sum())
    dof = n * (n - 2)
    want = dof * (1.0 - d / (n - 1.0))
    print(f"n = {n}: chi^2 {chi:.1f}, expected {want:.1f}, off by {abs(chi - want) / np.sqrt(2 * dof):.2f} sqrt(2 dof)")
    assert abs(chi - want) <= 5 * np.sqrt(2 * dof)
    assert abs(chi - chi_recorded) < 0.06


# ---------------------------------------------------------------- 2. the assembly
def _seven():
    """7 spots: a path 0-1-2-3, spot 4 on 1 and 2, spot 5 hanging on 3, spot 6 isolated; column 3 is constant."""
    edges = [(0, 1), (1, 2), (2, 3), (4, 1), (4, 2), (3, 5)]
    A = np.zeros((7, 7))
    for i, j in edges:
        A[i, j] = A[j, i] = 1
    rs = np.random.RandomState(4)
    V = rs.dirichlet(np.full(3, 0.5), 7)
    V = np.concatenate([V, np.full((7, 1), 0.25)], 1)          # column 3 is dead (constant)
    return A, V


def test_assemble_local_follows_the_definitions_element_by_element():
    from flashdeconv_amd.utils.local_stats import assemble_local
    from flashdeconv_amd.utils.spatial_stats import assemble
    A, V = _seven()
    n, K = V.shape
    deg = A.sum(1).astype(np.int64)
    W = int(deg.sum())
    mean = V.sum(0) / n
    mean[3] = 0.25
    Z = V - mean
    m2 = (Z * Z).sum(0)
    assert m2[3] == 0.0
    S = A @ V
    out = assemble_local(V, S, deg, mean, m2, n, W)
    assert set(out) == {"local_i", "gi_star", "quadrant"} and out["quadrant"].dtype == np.int8
    for i in range(n):
        for a in range(K):
            z, lag = V[i, a] - mean[a], S[i, a] - deg[i] * mean[a]
            li = (n * n / W) * z * lag / m2[a] if m2[a] > 0 else np.nan
            np.testing.assert_allclose(out["local_i"][i, a], li, rtol=1e-14, equal_nan=True)
            q = 1 if (z > 0 and lag > 0) else 2 if (z < 0 and lag > 0) else 3 if (z < 0 and lag < 0) else 4 if (z > 0 and lag < 0) else 0
            assert out["quadrant"][i, a] == q, (i, a)
            w = deg[i] + 1.0
            den = np.sqrt(m2[a] / n) * np.sqrt((n * w - w * w) / (n - 1.0))
            gi = (S[i, a] + V[i, a] - w * mean[a]) / den if den > 0 else np.nan
            np.testing.assert_allclose(out["gi_star"][i, a], gi, rtol=1e-14, equal_nan=True)
    assert np.isnan(out["local_i"][:, 3]).all() and np.isnan(out["gi_star"][:, 3]).all()       # the dead column
    assert np.all(out["quadrant"][:, 3] == 0)                                                  # Z == 0 and lag == 0 exactly
    assert np.all(out["quadrant"][6] == 0) and np.all(out["local_i"][6, :3] == 0)              # deg = 0: lag = 0
    assert set(np.unique(out["quadrant"][:6, :3])) <= {1, 2, 3, 4} and len(np.unique(out["quadrant"][:6, :3])) >= 2
    # the mean of the local statistic is the global one
    C = Z.T @ (A @ Z)
    np.testing.assert_allclose(out["local_i"][:, :3].mean(0), assemble(n, W, int((deg * deg).sum()), m2, C)["morans_i"][:3],
                               rtol=1e-12)


def test_assemble_local_permutation_keys_and_nan_rules():
    from flashdeconv_amd.utils.local_stats import assemble_local
    A, V = _seven()
    n, K = V.shape
    deg = A.sum(1).astype(np.int64)
    W = int(deg.sum())
    mean = V.sum(0) / n
    mean[3] = 0.25
    m2 = ((V - mean) ** 2).sum(0)
    S = A @ V
    R = 9
    rs = np.random.RandomState(1)
    ge = rs.randint(0, R + 1, (n, K))
    le = R - ge + rs.randint(0, 2, (n, K)) * (ge > 0)
    d = rs.randn(R, n, K)
    d[:, 4, 1] = 0.125                                        # a null without spread at (4, 1)
    sd, sq = d.sum(0), (d * d).sum(0)
    out = assemble_local(V, S, deg, mean, m2, n, W, ge, le, sd, sq, n_permutations=R)
    assert set(out) == {"local_i", "gi_star", "quadrant", "n_permutations", "p_greater", "p_less", "p_value", "z_sim",
                        "local_i_p_greater"} and out["n_permutations"] == R
    Z = V - mean
    for i in range(n):
        for a in range(K):
            got = {k: out[k][i, a] for k in ("p_greater", "p_less", "p_value", "z_sim", "local_i_p_greater")}
            if deg[i] == 0:
                assert all(np.isnan(v) for v in got.values()), (i, a)
                continue
            pg, pl = (1 + ge[i, a]) / (R + 1), (1 + le[i, a]) / (R + 1)
            assert got["p_greater"] == pg and got["p_less"] == pl and got["p_value"] == min(1.0, 2 * min(pg, pl))
            assert got["local_i_p_greater"] == (pg if Z[i, a] > 0 else pl if Z[i, a] < 0 else 1.0)
            m = d[:, i, a].mean()
            v = max((d[:, i, a] ** 2).mean() - m * m, 0.0)
            if (i, a) == (4, 1):
                assert np.isnan(got["z_sim"])
            else:
                np.testing.assert_allclose(got["z_sim"], -m / np.sqrt(v), rtol=1e-9)
    assert np.all(out["local_i_p_greater"][:6, 3] == 1.0)                                      # Z == 0: 1
    # W = 0: no local_i, Gi* stays defined (it does not divide by W); every permutation key is NaN (every deg is 0)
    empty = assemble_local(V, np.zeros_like(V), np.zeros(n, dtype=np.int32), mean, m2, n, 0, ge * 0 + R, le * 0 + R, sd * 0,
                           sq * 0, n_permutations=R)
    assert np.isnan(empty["local_i"]).all() and np.isfinite(empty["gi_star"][:, :3]).all() and np.all(empty["quadrant"] == 0)
    for k in ("p_greater", "p_less", "p_value", "z_sim", "local_i_p_greater"):
        assert np.isnan(empty[k]).all(), k
    # n = 1: everything NaN, nothing raises
    one = assemble_local(V[:1], np.zeros((1, K)), np.zeros(1, dtype=np.int32), V[0], np.zeros(K), 1, 0)
    assert np.isnan(one["local_i"]).all() and np.isnan(one["gi_star"]).all() and np.all(one["quadrant"] == 0)
    # a spot adjacent to every other spot: w = n, the Gi* denominator is 0
    star = assemble_local(V, S, np.full(n, n - 1), mean, m2, n, n * (n - 1))
    assert np.isnan(star["gi_star"]).all()
    with pytest.raises(ValueError, match="must be"):
        assemble_local(V, S[:, :2], deg, mean, m2, n, W)
    with pytest.raises(ValueError, match="counts and sums must be"):
        assemble_local(V, S, deg, mean, m2, n, W, ge, le, sd, None, n_permutations=R)
    with pytest.raises(ValueError, match="rows"):
        assemble_local(V, S, deg, mean, m2, n + 1, W)


# ---------------------------------------------------------------- 3. the null distribution
def test_null_mean_and_variance_match_sampling_without_replacement():
    """n = 500, 6-NN (symmetrised: degrees 6 .. 11), Dirichlet(0.3) with K = 4, seed 3, R = 2000.  The sum of d draws without
    replacement from the N = n - 1 other rows has mean d mu and variance d sigma^2 (N - d) / (N - 1) (mu, sigma^2 the others'
    mean and ddof-0 variance).  The null mean is held to 5 standard errors (measured: 3.89 at the worst of the 2000 (spot, column)
    pairs).  The null variance over theory: measured max |ratio - 1| = 0.1183; the same statistic with the draws made by
    RandomState(1).choice(n - 1, d, replace=False) on the same data is 0.1035, and the margin is that plus half as much again,
    0.1553."""
    import fdx_oracle as orc
    from flashdeconv_amd.utils.local_stats import conditional_indices
    n, K, R, seed = 500, 4, 2000, 3
    rs = np.random.RandomState(0)
    coords = rs.rand(n, 2)
    V = rs.dirichlet(np.full(K, 0.3), n)
    A = sparse.csr_matrix(orc.knn_graph_kdtree(coords, 6))
    deg = np.diff(A.indptr)
    N = n - 1
    zmax = rmax = 0.0
    for i in range(n):
        d = int(deg[i])
        draws = ref.conditional_indices_batch(seed, 0, R, i, n, d)                      # (R, d)
        for r in (0, (11 * i + 3) % R, R - 1):                                          # ... which are the package's draws
            assert np.array_equal(draws[r], conditional_indices(seed, r, i, n, d)), (i, r)
        Sr = V[draws].sum(1)                                                            # (R, K)
        others = np.delete(V, i, 0)
        mu, var = d * others.mean(0), d * others.var(0) * (N - d) / (N - 1.0)
        zmax = max(zmax, float((np.abs(Sr.mean(0) - mu) / np.sqrt(var / R)).max()))
        rmax = max(rmax, float(np.abs(Sr.var(0) / var - 1.0).max()))
    print(f"null mean: worst {zmax:.2f} standard errors; null variance / theory: worst |ratio - 1| {rmax:.4f}")
    assert zmax <= 5.0
    assert rmax <= 1.5 * 0.1035


# ---------------------------------------------------------------- 4. checks and declarations
def test_argument_checks_come_before_the_gpu(monkeypatch):
    from flashdeconv_amd import _lib
    from flashdeconv_amd.utils import local_stats as ls

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_gpu)
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    n = 6
    i = np.arange(n)
    ring = sparse.csr_matrix((np.ones(2 * n), (np.r_[i, i], np.r_[(i + 1) % n, (i - 1) % n])), shape=(n, n))
    V = np.random.RandomState(0).rand(n, 3)
    for fn in (ls.local_spatial_statistics, ls.local_sums):
        for bad in (-1, 2.5, "10", None, True, 10.0):
            with pytest.raises(ValueError, match="n_permutations must be an int >= 0"):
                fn(V, ring, n_permutations=bad)
        with pytest.raises(ValueError, match="below 2\\^31"):
            fn(V, ring, n_permutations=2 ** 31)
        with pytest.raises(ValueError, match="must be a 2-D"):
            fn(V[:, 0], ring)
        with pytest.raises(ValueError, match="must not be empty"):
            fn(V[:, :0], ring)
        with pytest.raises(ValueError, match="5 rows but the graph has 6 spots"):
            fn(V[:5], ring)
        asym = ring.tolil()
        asym[0, 3] = 1.0
        with pytest.raises(ValueError, match="must be symmetric"):
            fn(V, asym.tocsr())
        with pytest.raises(TypeError, match="graph must be"):
            fn(V, np.eye(n))
    with pytest.raises(ValueError, match="random_state"):
        ls.local_spatial_statistics(V, ring, n_permutations=3, random_state=-1)
    with pytest.raises(ValueError):
        ls.local_spatial_statistics(V, ring, n_permutations=3, random_state="seed")
    with pytest.raises(ValueError, match="first_perm must be an int >= 0"):
        ls.local_sums(V, ring, first_perm=-1)


def test_model_method_checks_come_before_the_fit_state_is_used():
    from flashdeconv_amd import FlashDeconv
    with pytest.raises(RuntimeError, match=r"Model has not been fitted\. Call fit\(\) first\."):
        FlashDeconv().get_local_spatial_statistics(n_permutations=9)


def test_entries_are_declared_exported_and_bound():
    import ctypes
    import inspect
    from flashdeconv_amd import FlashDeconv, _lib, tl, utils
    from flashdeconv_amd.utils import local_stats
    text = open(os.path.join(ROOT, "include", "fdx.h")).read()
    for name, n_want in (("fdx_local_stats_dev", 17), ("fdx_conditional_indices_dev", 7)):
        decl = re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert decl is not None, name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(decl.group(1).split(",")) == n_want
        assert callable(getattr(_lib.load(), name))
    args = _lib.SIGNATURES["fdx_local_stats_dev"][1]
    assert args[4] is ctypes.c_uint64 and args[5] is ctypes.c_int64 and args[6] is ctypes.c_int64 and args[15] is _lib.p_i64
    assert _lib.SIGNATURES["fdx_conditional_indices_dev"][1][0] is ctypes.c_uint64
    assert _lib.load().fdx_version() >= 202
    assert set(local_stats.__all__) == {"local_spatial_statistics", "local_sums", "assemble_local", "conditional_indices"}
    for name in ("local_spatial_statistics", "conditional_indices"):
        assert name in utils.__all__ and callable(getattr(utils, name))
    assert inspect.signature(tl.deconvolve).parameters["local_stats"].default is False
    params = inspect.signature(FlashDeconv.get_local_spatial_statistics).parameters
    assert params["what"].default == "proportions" and params["n_permutations"].default == 0
    assert params["random_state"].default is None
    assert "local_stats_kernels.cpp" in open(os.path.join(ROOT, "flashdeconv_amd", "csrc", "Makefile")).read()
