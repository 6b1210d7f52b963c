"""CPU tests of the spatial correlogram: the NumPy reference of tests/correlogram_ref.py against scipy, the host assembly
(utils.correlogram.assemble_correlogram) against the formulas written out, the argument checks, and the precondition that makes
the GPU tests' exact comparisons exact.  Nothing here touches a GPU."""
import numpy as np
import pytest
from scipy import sparse
from scipy.spatial import cKDTree

import correlogram_ref as cr
from flashdeconv_amd.utils.correlogram import assemble_correlogram, correlogram_sums, spatial_correlogram


@pytest.fixture(scope="module")
def sets():
    return cr.coord_sets()


# ---------------------------------------------------------------- 1. the reference against scipy
@pytest.mark.parametrize("name", sorted(cr.coord_sets()))
def test_reference_bands_are_scipy_radius_graphs(sets, name):
    coords, radii = sets[name]
    n = coords.shape[0]
    K = 3
    V = cr.dirichlet_values(n, K, 7)
    ref = cr.band_reference(V, coords, radii)
    tree = cKDTree(coords)
    cum = sparse.csr_matrix((n, n))
    for b, r in enumerate(radii):
        cum = cum + ref["A"][b]
        pairs = tree.query_pairs(r, output_type="ndarray")
        i, j = pairs[:, 0], pairs[:, 1]
        want = sparse.csr_matrix((np.ones(2 * len(i)), (np.concatenate([i, j]), np.concatenate([j, i]))), shape=(n, n))
        assert (cum != want).nnz == 0, (name, b)
        assert cum.nnz == 0 or cum.data.max() == 1.0                      # the bands are disjoint
        np.testing.assert_array_equal(ref["C"][b], ref["Z"].T @ (ref["A"][b] @ ref["Z"]))
        assert ref["W"][b] == ref["A"][b].nnz and ref["sum_deg_sq"][b] == int((ref["deg"][:, b] ** 2).sum())
        assert (ref["A"][b] != ref["A"][b].T).nnz == 0 and not ref["A"][b].diagonal().any()


# ---------------------------------------------------------------- 2. interior degrees
def test_interior_degrees_of_the_unit_lattice():
    coords = cr.square_lattice(12)
    ref = cr.band_reference(np.ones((144, 1)), coords, [1.0, 1.5, 2.0, 5.0])
    interior = np.all((coords >= 5) & (coords <= 6), axis=1)
    assert interior.sum() == 4
    # <= at d = 2 (band 3 holds the four (2, 0) pairs) and at d = 5 (band 4 holds (5, 0) and the 3-4-5 pairs)
    assert np.array_equal(ref["deg"][interior], np.tile([4, 4, 4, 68], (4, 1)))


# ---------------------------------------------------------------- 3. assembly
def test_assemble_correlogram_is_the_written_formulas():
    rs = np.random.RandomState(0)
    n, K, B = 50, 3, 4
    W = np.array([120, 200, 0, 340])
    sds = np.array([400, 900, 0, 2600])
    Z = rs.randn(n, K)
    Z -= Z.mean(0)
    m2, m4 = (Z ** 2).sum(0), (Z ** 4).sum(0)
    C = rs.randn(B, K, K)
    got = assemble_correlogram(n, W, sds, m2, m4, C)
    assert set(got) == {"cross", "morans_i", "z_score", "expected_i", "variance_i", "variance_i_rand", "z_score_rand"}
    assert got["cross"].shape == (B, K, K) and got["morans_i"].shape == (B, K) and got["variance_i"].shape == (B,)
    E = -1.0 / (n - 1)
    for b in (0, 1, 3):
        cross = (n / W[b]) * C[b] / np.sqrt(np.outer(m2, m2))
        np.testing.assert_allclose(got["cross"][b], cross, rtol=1e-14)
        np.testing.assert_allclose(got["morans_i"][b], np.diagonal(cross), rtol=1e-14)
        S1, S2 = 2.0 * W[b], 4.0 * sds[b]
        var = (n * n * S1 - n * S2 + 3.0 * W[b] ** 2) / ((n * n - 1.0) * W[b] ** 2) - E * E
        np.testing.assert_allclose(got["variance_i"][b], var, rtol=1e-12)
        np.testing.assert_allclose(got["z_score"][b], (np.diagonal(cross) - E) / np.sqrt(var), rtol=1e-12)
        b2 = n * m4 / m2 ** 2
        e2 = (n * ((n * n - 3 * n + 3) * S1 - n * S2 + 3.0 * W[b] ** 2)
              - b2 * ((n * n - n) * S1 - 2 * n * S2 + 6.0 * W[b] ** 2)) / ((n - 1.0) * (n - 2.0) * (n - 3.0) * W[b] ** 2)
        np.testing.assert_allclose(got["variance_i_rand"][b], e2 - E * E, rtol=1e-10)
        np.testing.assert_allclose(got["z_score_rand"][b], (np.diagonal(cross) - E) / np.sqrt(e2 - E * E), rtol=1e-10)
        assert got["expected_i"][b] == E
    # an empty band: every statistic NaN, nothing raises
    for key in ("cross", "morans_i", "z_score", "variance_i", "variance_i_rand", "z_score_rand"):
        assert np.all(np.isnan(got[key][2])), key


def test_assemble_correlogram_nan_rules():
    # a constant column: NaN in its row and column of cross and in its Moran's I, the others are untouched
    m2, m4 = np.array([2.0, 0.0]), np.array([1.5, 0.0])
    got = assemble_correlogram(10, [20], [60], m2, m4, np.ones((1, 2, 2)))
    assert np.isfinite(got["cross"][0, 0, 0]) and np.isfinite(got["z_score"][0, 0]) and np.isfinite(got["z_score_rand"][0, 0])
    assert np.isnan(got["cross"][0, 1]).all() and np.isnan(got["cross"][0, :, 1]).all()
    assert np.isnan(got["morans_i"][0, 1]) and np.isnan(got["z_score"][0, 1]) and np.isnan(got["z_score_rand"][0, 1])
    # n = 1: nothing is defined
    one = assemble_correlogram(1, [0, 0], [0, 0], np.zeros(2), np.zeros(2), np.zeros((2, 2, 2)))
    for key, val in one.items():
        assert np.all(np.isnan(val)), key
    with pytest.raises(ValueError, match="C \\(B, K, K\\)"):
        assemble_correlogram(10, [20], [60], m2, m4, np.ones((2, 2, 2)))


# ---------------------------------------------------------------- 4. validation: before anything touches the GPU
@pytest.mark.parametrize("fn", [spatial_correlogram, correlogram_sums])
def test_argument_checks_raise_value_error(fn, monkeypatch):
    from flashdeconv_amd import _lib

    def no_gpu(*a, **k):
        raise AssertionError("an argument check let the call through to the GPU")

    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    monkeypatch.setattr(_lib, "load", no_gpu)
    V, xy, r = np.ones((6, 2)), np.zeros((6, 2)), [1.0, 2.0]
    bad = [((np.ones(6), xy, r), "2-D"), ((np.ones((0, 2)), np.zeros((0, 2)), r), "must not be empty"),
           ((V, np.zeros(6), r), "coords must be 2D"), ((V, np.zeros((6, 0)), r), "coords must be 2D"),
           ((V, np.zeros((6, 4)), r), "1 to 3 coordinate dimensions"), ((V, np.zeros((5, 2)), r), "6 rows but coords has 5"),
           ((V, xy, []), "non-empty"), ((V, xy, [[1.0, 2.0]]), "1-D"), ((V, xy, [1.0, 1.0]), "strictly ascending"),
           ((V, xy, [2.0, 1.0]), "strictly ascending"), ((V, xy, [0.0, 1.0]), "positive"), ((V, xy, [-1.0]), "positive"),
           ((V, xy, [1.0, np.inf]), "finite"), ((V, xy, [np.nan]), "finite"),
           ((V, xy, np.arange(1, 34, dtype=float)), "at most 32")]
    for args, match in bad:
        with pytest.raises(ValueError, match=match):
            fn(*args)
    with pytest.raises(ValueError, match="max_candidates must be an int >= 1"):
        fn(V, xy, r, max_candidates=0)
    if fn is correlogram_sums:
        with pytest.raises(ValueError, match="max_bands_per_pass must be an int >= 0"):
            fn(V, xy, r, max_bands_per_pass=-1)
    else:
        for nb, match in ((0, "n_bands must be an int >= 1"), (33, "at most 32 bands"), (2.5, "n_bands must be an int")):
            with pytest.raises(ValueError, match=match):
                fn(V, xy, None, n_bands=nb)


# ---------------------------------------------------------------- 5. the exactness precondition of the GPU tests
@pytest.mark.parametrize("name,K,seed", cr.exact_cases())
def test_exact_cases_are_exact_in_any_order(sets, name, K, seed):
    coords, radii = sets[name]
    n = coords.shape[0]
    V = cr.exact_values(n, K, seed)
    assert V.shape == (n, K)
    assert np.all(V.sum(0) == 0.0) and np.all(V[::-1].sum(0) == 0.0)          # the mean is exactly 0, so Z = V
    assert np.all(V * 16 == np.round(V * 16)) and np.abs(V).max() <= 0.5
    ref = cr.band_reference(V, coords, radii)
    # every product is a multiple of 1 / 256 below 1 / 4: a sum of W_b of them is an integer below 2^53 over 256 - exact in any
    # order, with a wide margin (Z^4 terms likewise: multiples of 2^-16 below 2^-4, n of them)
    assert ref["W"].max() < 2 ** 24 and n < 2 ** 24
    assert np.all(ref["mean"] == 0.0) and np.array_equal(ref["Z"], V)
    assert np.all(ref["C"] * 256 == np.round(ref["C"] * 256))


def test_size_edge_case_has_coincident_pairs(sets):
    coords, _ = sets["cloud257"]
    assert len(np.unique(coords, axis=0)) < len(coords)


def test_library_has_the_entry():
    from flashdeconv_amd import _lib
    lib = _lib.load()
    assert lib.fdx_version() >= 203 and hasattr(lib, "fdx_spatial_correlogram_dev")
    from flashdeconv_amd import utils
    assert utils.spatial_correlogram is spatial_correlogram


# ---------------------------------------------------------------- 6. the request of tl.deconvolve
def test_correlogram_request():
    from flashdeconv_amd.utils.correlogram import correlogram_request
    for off in (False, None, np.False_):
        assert correlogram_request(off) is None
    assert correlogram_request(True) == {} and correlogram_request(np.True_) == {}
    assert correlogram_request(3) == {"n_bands": 3} and correlogram_request(np.int64(32)) == {"n_bands": 32}
    assert correlogram_request([1, 2.5]) == {"radii": [1.0, 2.5]} and correlogram_request(np.array([0.5])) == {"radii": [0.5]}
    for bad, match in ((0, "n_bands must be an int >= 1"), (-2, "n_bands"), (33, "at most 32 bands"), ([2.0, 1.0], "ascending"),
                       ([], "non-empty"), ([0.0, 1.0], "positive"), ([1.0, np.inf], "finite"), (2.5, "correlogram must be"),
                       ("abc", "correlogram must be"), (list(range(1, 34)), "at most 32 radii")):
        with pytest.raises(ValueError, match=match):
            correlogram_request(bad)


def test_deconvolve_refuses_a_bad_request_before_the_fit():
    import flashdeconv_amd as fd
    for bad in (0, 33, [2.0, 1.0], "abc"):
        with pytest.raises(ValueError):
            fd.tl.deconvolve(None, None, correlogram=bad)      # nothing of the data is touched: there is none


def test_candidate_count_restatement():
    # 2 x 2 cells of edge just above 1 holding 1, 2, 3, 4 points: every cell sees all ten
    pts = np.array([[0.0, 0.0]] + [[1.5, 0.2]] * 2 + [[0.3, 1.6]] * 3 + [[2.0, 2.0]] * 4)
    got, cells = cr.candidate_count(pts, 1.0)
    assert cells == (2, 2, 1) and got == 100
    # a chain of 6 cells of 1 point: 2 + 3 * 4 + 2
    got, cells = cr.candidate_count(np.arange(6.0)[:, None] * 1.01, 1.0)
    assert cells == (6, 1, 1) and got == 16
