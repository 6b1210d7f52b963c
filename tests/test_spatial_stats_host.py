"""CPU-only tests of the spatial-statistics surface: the host assembly of Moran's I / the bivariate Moran matrix / the z scores from
the device's sums, the shape checks that come before anything touches the GPU, and the C entry's declaration, export and binding."""
import os
import re

import numpy as np
import pytest
from scipy import sparse

from conftest import ROOT


def _formulas(n, W, sdeg2, m2, C):
    """The definitions, written out entry by entry."""
    K = len(m2)
    cross = np.full((K, K), np.nan)
    for a in range(K):
        for b in range(K):
            if W > 0 and n >= 2 and m2[a] > 0 and m2[b] > 0:
                cross[a, b] = (n / W) * C[a, b] / np.sqrt(m2[a] * m2[b])
    E = -1.0 / (n - 1) if n >= 2 else np.nan
    var = np.nan
    if n >= 2 and W > 0:
        var = (n ** 2 * 2 * W - n * 4 * sdeg2 + 3 * W ** 2) / ((n ** 2 - 1) * W ** 2) - E ** 2
    z = np.array([(cross[a, a] - E) / np.sqrt(var) if var > 0 else np.nan for a in range(K)])
    return cross, E, var, z


def test_assembly_against_the_formulas():
    from flashdeconv_amd.utils.spatial_stats import assemble
    rs = np.random.RandomState(0)
    n, K = 50, 4
    deg = rs.randint(1, 7, n)
    W, sdeg2 = int(deg.sum()), int((deg * deg).sum())
    m2 = rs.rand(K) + 0.5
    C = rs.randn(K, K)
    out = assemble(n, W, sdeg2, m2, C)
    cross, E, var, z = _formulas(n, W, sdeg2, m2, C)
    assert set(out) == {"cross", "morans_i", "expected_i", "variance_i", "z_score"}
    np.testing.assert_allclose(out["cross"], cross, rtol=1e-14)
    np.testing.assert_array_equal(out["morans_i"], np.diagonal(out["cross"]))
    assert out["expected_i"] == E
    np.testing.assert_allclose(out["variance_i"], var, rtol=1e-13)
    np.testing.assert_allclose(out["z_score"], z, rtol=1e-12)
    assert out["cross"].shape == (K, K) and out["morans_i"].shape == (K,) and out["z_score"].shape == (K,)


def test_assembly_of_a_ring_by_hand():
    """+1 / -1 alternating on a ring of 8: C = -2 n, m2 = n, W = 2 n, deg = 2: I = -1; Var = (64 * 32 - 8 * 128 + 3 * 256) /
    (63 * 256) - 1 / 49."""
    from flashdeconv_amd.utils.spatial_stats import assemble
    out = assemble(8, 16, 32, [8.0], [[-16.0]])
    assert out["morans_i"][0] == -1.0 and out["expected_i"] == -1.0 / 7.0
    var = 1792.0 / 16128.0 - 1.0 / 49.0
    np.testing.assert_allclose(out["variance_i"], var, rtol=1e-14)
    np.testing.assert_allclose(out["z_score"][0], (-1.0 + 1.0 / 7.0) / np.sqrt(var), rtol=1e-14)


def test_assembly_nan_cases():
    from flashdeconv_amd.utils.spatial_stats import assemble
    C = np.array([[1.0, 0.5, 0.2], [0.5, 2.0, 0.1], [0.2, 0.1, 0.0]])
    # a column without variance: its row and column of cross, its I and its z score; the others stand
    out = assemble(10, 20, 44, [1.0, 2.0, 0.0], C)
    assert np.isnan(out["cross"][2, :]).all() and np.isnan(out["cross"][:, 2]).all()
    assert np.isfinite(out["cross"][:2, :2]).all() and np.isnan(out["morans_i"][2]) and np.isnan(out["z_score"][2])
    assert np.isfinite(out["z_score"][:2]).all() and np.isfinite(out["variance_i"])
    # no edges: everything that divides by W
    out = assemble(10, 0, 0, [1.0, 2.0, 3.0], C)
    assert np.isnan(out["cross"]).all() and np.isnan(out["morans_i"]).all() and np.isnan(out["z_score"]).all()
    assert np.isnan(out["variance_i"]) and out["expected_i"] == -1.0 / 9.0
    # one spot
    out = assemble(1, 0, 0, [0.0], [[0.0]])
    assert np.isnan(out["cross"]).all() and np.isnan(out["z_score"]).all() and np.isnan(out["expected_i"]) and np.isnan(out["variance_i"])
    # two spots joined by an edge: the normal variance is exactly 0, so there is no z score - I itself stands
    out = assemble(2, 2, 2, [2.0], [[-2.0]])
    assert out["morans_i"][0] == -1.0 and out["variance_i"] == 0.0 and np.isnan(out["z_score"]).all()
    # nothing raises on NaN sums either
    out = assemble(10, 20, 44, [np.nan, 1.0], [[1.0, 1.0], [1.0, 1.0]])
    assert np.isnan(out["cross"][0, :]).all() and np.isfinite(out["cross"][1, 1])
    with pytest.raises(ValueError, match="m2 must be"):
        assemble(10, 20, 44, [1.0, 2.0], np.zeros((3, 3)))


def test_shape_checks_come_before_the_gpu(monkeypatch):
    """Every ValueError below is raised from shapes and host-side structure alone: the library is never loaded."""
    from flashdeconv_amd import _lib
    from flashdeconv_amd.utils import spatial_stats as ss

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_gpu)
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    n = 6
    i = np.arange(n)
    ring = sparse.csr_matrix((np.ones(2 * n), (np.r_[i, i], np.r_[(i + 1) % n, (i - 1) % n])), shape=(n, n))
    V = np.random.RandomState(0).rand(n, 3)
    for fn in (ss.spatial_autocorrelation, ss.spatial_sums):
        with pytest.raises(ValueError, match="must be a 2-D"):
            fn(V[:, 0], ring)
        with pytest.raises(ValueError, match="must be a 2-D"):
            fn(V[None], ring)
        with pytest.raises(ValueError, match="must not be empty"):
            fn(V[:, :0], ring)
        with pytest.raises(ValueError, match="5 rows but the graph has 6 spots"):
            fn(V[:5], ring)
        asym = ring.tolil()
        asym[0, 3] = 1.0
        with pytest.raises(ValueError, match="must be symmetric"):
            fn(V, asym.tocsr())
        loop = ring.tolil()
        loop[2, 2] = 1.0
        with pytest.raises(ValueError, match="no self loops"):
            fn(V, loop.tocsr())
        with pytest.raises(ValueError, match="square"):
            fn(V, sparse.csr_matrix((n, n + 1)))
        with pytest.raises(TypeError, match="graph must be"):
            fn(V, np.eye(n))


def test_model_method_needs_a_fit():
    from flashdeconv_amd import FlashDeconv
    from flashdeconv_amd.utils.spatial_stats import spatial_autocorrelation
    m = FlashDeconv()
    for kw in ({}, {"what": "abundances"}, {"neighbor_mean": True}):
        with pytest.raises(RuntimeError, match=r"Model has not been fitted\. Call fit\(\) first\."):
            m.get_spatial_autocorrelation(**kw)
    with pytest.raises(RuntimeError, match=r"Model has not been fitted\. Call fit\(\) first\."):
        spatial_autocorrelation(np.zeros((4, 2)), m)


def test_entry_is_declared_exported_and_bound():
    import ctypes
    import inspect
    from flashdeconv_amd import _lib, tl, utils
    text = open(os.path.join(ROOT, "include", "fdx.h")).read()
    decl = re.search(r"int\s+fdx_spatial_autocorr_dev\s*\(([^;]*)\)\s*;", text)
    assert decl is not None
    n_args = len(decl.group(1).split(","))
    res, args = _lib.SIGNATURES["fdx_spatial_autocorr_dev"]
    assert res is ctypes.c_int and len(args) == n_args == 10
    assert args[2] is ctypes.c_int64 and args[3] is ctypes.c_int32 and args[7] is _lib.p_i64
    assert callable(_lib.load().fdx_spatial_autocorr_dev)
    assert "spatial_autocorrelation" in utils.__all__ and callable(utils.spatial_autocorrelation)
    assert inspect.signature(tl.deconvolve).parameters["spatial_stats"].default is False
