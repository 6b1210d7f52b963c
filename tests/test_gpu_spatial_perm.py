"""-m gpu tests of the permutation test of the spatial statistics (fdx_spatial_perm_dev, fdx_permutation_indices_dev,
utils.spatial_stats.spatial_permutation_test / spatial_permutation_sums, FlashDeconv.get_spatial_autocorrelation(n_permutations=),
tl.deconvolve(spatial_permutations=)).

Reference, in NumPy float64: pi_r = permutation_indices(seed, r, n) (the definition the device must match bit for bit),
    mean = V.sum(0) / n,  Zr = V[pi_r] - mean,  C_r = Zr.T @ (A @ Zr)
on the graph's own exported adjacency A (symmetric, binary, no diagonal, caller's spot order).

Tolerances (u = 2^-53).  Every C_r is held to the order-independent bound of tests/test_gpu_spatial_stats.py, restated here: with
aZ = |Zr|, AaZ = A @ aZ, s = AaZ.sum(0), vmax = |V|.max(0), W = nnz(A),
    |C_r - ref| <= 4 (W + n) u (aZ' AaZ + outer(vmax, s) + outer(s, vmax))
(W products summed in any order on both sides - the factor 4 - and the two outer terms carry the summation error of the means into
Z).  count_ge / count_le must lie between the reference counts taken where the reference difference C_r - C_obs clears, or stays
within, the sum of the two bounds (that of C_r and that of C_obs: "C_obs +- 2 tol").  m4 = sum Z^4: 4 n u sum Z^4 for the sum in
any order on both sides, plus the mean's own bound 4 n u vmax carried through d(z^4) = 4 |z|^3 dz.
p values are ratios of integers and compared exactly; z_sim, assembled from the device's own null in NumPy, is compared with the
one the sums give at the rounding of sums of R terms, carried to first order (see _z_sim_tol).
"""
import ctypes

import numpy as np
import pytest
from scipy import sparse

import datagen

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
N_LIST = [1, 2, 3, 5, 64, 65, 257, 1000, 4097, 65537]
PERM_KEYS = {"n_permutations", "cross_p_greater", "cross_p_less", "cross_p_value", "cross_null_mean", "cross_null_std",
             "cross_z_sim", "p_value", "p_greater", "p_less", "z_sim"}
BASE_KEYS = {"morans_i", "z_score", "mean", "m2", "m4", "cross", "expected_i", "variance_i", "n", "n_edges", "variance_i_rand",
             "z_score_rand"}


# ---------------------------------------------------------------- helpers
def _device_graph(coords, method, k=6, radius=0.0):
    import torch
    from flashdeconv_amd import _lib
    coords = np.ascontiguousarray(coords, dtype=np.float64)
    cd = torch.as_tensor(coords, device="cuda:0")
    h = ctypes.c_void_p()
    _lib.check(_lib.load().fdx_graph_build_dev(ctypes.c_void_p(cd.data_ptr()), coords.shape[0], coords.shape[1], method, int(k),
                                               float(radius), None, ctypes.byref(h)))
    g = _lib.Graph(h.value)
    g.info()
    torch.cuda.synchronize()
    return g


def _adjacency(g):
    indptr, indices = g.to_csr_arrays()
    n = len(indptr) - 1
    A = sparse.csr_matrix((np.ones(len(indices)), indices.astype(np.int64), indptr), shape=(n, n))
    assert (A != A.T).nnz == 0 and not A.diagonal().any()
    return A


def _graph_perm(g, n):
    import torch
    from flashdeconv_amd import _lib
    perm_d = torch.empty(n, dtype=torch.int32, device="cuda:0")
    _lib.check(_lib.load().fdx_graph_perm_dev(g.handle, ctypes.c_void_p(perm_d.data_ptr()), None))
    torch.cuda.synchronize()
    return perm_d.cpu().numpy().astype(np.int64)


def _values(n, K, seed):
    rs = np.random.RandomState(seed)
    return rs.dirichlet(np.full(K, 0.3), n) if K > 1 else rs.rand(n, 1)


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def _c_and_tol(Z, A, vmax, W):
    """C = Z' A Z and the order-independent bound of the module docstring."""
    n = Z.shape[0]
    aZ = np.abs(Z)
    AaZ = A @ aZ
    s = AaZ.sum(0)
    return Z.T @ (A @ Z), 4 * (W + n) * U * (aZ.T @ AaZ + np.outer(vmax, s) + np.outer(s, vmax))


def _reference(V, A, seed, first, R):
    from flashdeconv_amd.utils.spatial_stats import permutation_indices
    V = np.asarray(V, dtype=np.float64)
    n, K = V.shape
    mean = V.sum(0) / n
    vmax = np.abs(V).max(0)
    deg = np.asarray(A.sum(1)).ravel().astype(np.int64)
    W = int(deg.sum())
    Z = V - mean
    C, tolC = _c_and_tol(Z, A, vmax, W)
    null, tol = np.empty((R, K, K)), np.empty((R, K, K))
    for r in range(R):
        pi = permutation_indices(seed, first + r, n)
        null[r], tol[r] = _c_and_tol(V[pi] - mean, A, vmax, W)
    z4 = (Z ** 4).sum(0)
    tol_m4 = 4 * n * U * z4 + 4 * (np.abs(Z) ** 3).sum(0) * (4 * n * U * vmax)
    return {"mean": mean, "C": C, "tol_C": tolC, "null": null, "tol": tol, "m4": z4, "tol_m4": tol_m4, "n": n, "W": W,
            "sum_deg_sq": int((deg * deg).sum()), "m2": (Z * Z).sum(0)}


def _z_sim_tol(d):
    """First-order bound of the difference between z = -m / sqrt(v), m = mean(d), v = mean(d^2) - m^2, from sums of the R values
    of d taken in two different orders (4 R u sum |terms| between two sums), plus a few roundings of the final arithmetic."""
    R = d.shape[0]
    m, ad, q = d.mean(0), np.abs(d).mean(0), (d * d).mean(0)
    v = np.maximum(q - m * m, 0.0)
    dm = 4 * R * U * ad
    dv = 4 * R * U * q + 2 * np.abs(m) * dm + 4 * U * (q + m * m)
    with np.errstate(divide="ignore", invalid="ignore"):
        return dm / np.sqrt(v) + np.abs(m) * dv / (2 * v ** 1.5) + 16 * U * np.abs(m) / np.sqrt(v)


def _check_null(V, graph, A, R, seed=11, label="", max_batch=0):
    """Device sums with the null on (V, graph) against the reference on A: every C_r, the counts, m4, and the unpermuted sums bit
    for bit against spatial_sums."""
    from flashdeconv_amd.utils.spatial_stats import assemble_permutation, spatial_permutation_sums, spatial_sums
    got = spatial_permutation_sums(V, graph, seed=seed, n_permutations=R, max_batch=max_batch, return_null=True)
    ref = _reference(_host(V), A, seed, 0, R)
    K = ref["mean"].shape[0]
    null = _host(got["null"])
    assert null.shape == (R, K, K) and null.dtype == np.float64 and got["n_permutations"] == R
    err = np.abs(null - ref["null"])
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = float(np.nanmax(np.where(ref["tol"] > 0, err / ref["tol"], np.where(err > 0, np.inf, 0.0)))) if err.size else 0.0
    print(f"{label} null: max |err| {float(err.max()) if err.size else 0.0:.3e}, worst err / bound {worst:.3e}, B = {got['batch']}")
    assert np.all(err <= ref["tol"]), (label, worst)
    # the unpermuted sums: what spatial_sums returns, bit for bit
    base = spatial_sums(V, graph)
    for key in ("mean", "m2", "C"):
        assert np.array_equal(got[key], base[key]), (label, key)
    assert (got["n"], got["W"], got["sum_deg_sq"]) == (base["n"], base["W"], base["sum_deg_sq"]) == (ref["n"], ref["W"], ref["sum_deg_sq"])
    assert np.all(np.abs(got["m4"] - ref["m4"]) <= ref["tol_m4"]), (label, "m4")
    # counts: between the reference counts where the difference clears the two bounds and where it stays within them
    dref = ref["null"] - ref["C"]
    t2 = ref["tol"] + ref["tol_C"]
    assert np.all((dref >= t2).sum(0) <= got["count_ge"]) and np.all(got["count_ge"] <= (dref >= -t2).sum(0)), label
    assert np.all((dref <= -t2).sum(0) <= got["count_le"]) and np.all(got["count_le"] <= (dref <= t2).sum(0)), label
    assert got["count_ge"].dtype == np.int64 and np.all(got["count_ge"] + got["count_le"] >= R)
    # ... and exactly those of the device's own null; the sums at the rounding of R terms
    d = null - got["C"]
    assert np.array_equal(got["count_ge"], (null >= got["C"]).sum(0)) and np.array_equal(got["count_le"], (null <= got["C"]).sum(0))
    assert np.all(np.abs(got["sum_d"] - d.sum(0)) <= 4 * R * U * np.abs(d).sum(0))
    assert np.all(np.abs(got["sumsq_d"] - (d * d).sum(0)) <= 4 * R * U * (d * d).sum(0))
    if R >= 1:
        out = assemble_permutation(got["n"], got["W"], got["m2"], got["C"], got["count_ge"], got["count_le"], got["sum_d"],
                                   got["sumsq_d"], R)
        own = assemble_permutation(got["n"], got["W"], got["m2"], got["C"], (null >= got["C"]).sum(0), (null <= got["C"]).sum(0),
                                   d.sum(0), (d * d).sum(0), R)
        for key in ("cross_p_greater", "cross_p_less", "cross_p_value"):
            assert np.array_equal(out[key], own[key], equal_nan=True), (label, key)
        ztol = _z_sim_tol(d)
        both = np.isfinite(out["cross_z_sim"]) & np.isfinite(own["cross_z_sim"]) & np.isfinite(ztol)
        assert np.all(np.abs(out["cross_z_sim"] - own["cross_z_sim"])[both] <= ztol[both]), label
    return got, ref


@pytest.fixture(scope="module")
def knn130():
    from flashdeconv_amd import _lib
    rs = np.random.RandomState(130)
    g = _device_graph(rs.rand(130, 2) * np.sqrt(130.0), _lib.GRAPH_KNN, 6)
    yield g, _adjacency(g)
    g.close()


# ---------------------------------------------------------------- 1. the bijection on the device
@pytest.mark.parametrize("n", N_LIST)
def test_device_indices_equal_the_definition(n):
    import torch
    from flashdeconv_amd import _lib
    from flashdeconv_amd.utils.spatial_stats import permutation_indices
    lib = _lib.load()
    for seed, r in ((0, 0), (12345, 7), (2 ** 64 - 1, 998)):
        out = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda:0")
        _lib.check(lib.fdx_permutation_indices_dev(ctypes.c_uint64(seed), r, n, ctypes.c_void_p(out.data_ptr()), None))
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert got[n] == -7                                                 # nothing past n
        assert np.array_equal(got[:n].astype(np.int64), permutation_indices(seed, r, n)), (seed, r)


def test_device_indices_argument_checks():
    from flashdeconv_amd import _lib
    lib = _lib.load()
    for args, msg in (((0, 0, 5, None), "null argument"), ((0, -1, 5, None), "r must not be negative"), ((0, 0, -1, None), "n must be")):
        with pytest.raises(_lib.FdxError, match=msg):
            _lib.check(lib.fdx_permutation_indices_dev(ctypes.c_uint64(args[0]), args[1], args[2], args[3], None))
    _lib.check(lib.fdx_permutation_indices_dev(ctypes.c_uint64(0), 0, 0, None, None))


# ---------------------------------------------------------------- 2. the null against NumPy
@pytest.mark.parametrize("n", [1, 2, 37, 64, 65, 257])
def test_null_slice_tails(n):
    from flashdeconv_amd import _lib
    V = _values(n, 5, n)
    if n <= 2:
        A = sparse.csr_matrix(np.ones((n, n)) - np.eye(n))
        _check_null(V, A, A, 7, label=f"n={n}")
    else:
        rs = np.random.RandomState(n)
        g = _device_graph(rs.rand(n, 2) * np.sqrt(float(n)), _lib.GRAPH_KNN, 6)
        try:
            _check_null(V, g, _adjacency(g), 7, label=f"n={n}")
        finally:
            g.close()


@pytest.mark.parametrize("K", [1, 8, 9, 17, 33, 65])
def test_null_k_coverage(knn130, K):
    g, A = knn130
    _check_null(_values(130, K, 2000 + K), g, A, 5, label=f"K={K}")


def test_null_on_a_graph_with_a_non_identity_permutation():
    from flashdeconv_amd import _lib
    n = 300
    rs = np.random.RandomState(3)
    g = _device_graph(rs.rand(n, 2) * np.sqrt(float(n)), _lib.GRAPH_KNN, 6)
    try:
        assert not np.array_equal(_graph_perm(g, n), np.arange(n))
        _check_null(_values(n, 7, 3), g, _adjacency(g), 5, label="knn300")
    finally:
        g.close()


def test_null_on_a_radius_graph_with_isolated_spots():
    from flashdeconv_amd import _lib
    coords = datagen.gaussian_raw(300, 4, 2, seed=0)[2]
    g = _device_graph(coords, _lib.GRAPH_RADIUS, radius=0.6)
    try:
        A = _adjacency(g)
        deg = np.diff(A.indptr)
        assert (deg == 0).any() and (deg > 0).any()
        _check_null(_values(300, 4, 4), g, A, 5, label="radius")
    finally:
        g.close()


def test_null_on_a_from_csr_identity_order_graph():
    from scipy.spatial import cKDTree
    n, k = 80, 70
    rs = np.random.RandomState(80)
    coords = rs.rand(n, 2)
    idx = cKDTree(coords).query(coords, k=k + 1)[1][:, 1:]
    A = sparse.csr_matrix((np.ones(n * k), (np.repeat(np.arange(n), k), idx.ravel())), shape=(n, n))
    A = ((A + A.T) > 0).astype(np.float64).tocsr()
    _check_null(_values(n, 6, 80), A, A, 5, label="from_csr")


# ---------------------------------------------------------------- 3. batching and splitting
def test_batches_and_split_calls_return_the_same_bits(knn130):
    from flashdeconv_amd.utils.spatial_stats import spatial_permutation_sums
    g, A = knn130
    V, R, seed = _values(130, 9, 77), 7, 5
    runs = {mb: spatial_permutation_sums(V, g, seed=seed, n_permutations=R, max_batch=mb, return_null=True) for mb in (1, 3, 7, 0)}
    assert [runs[mb]["batch"] for mb in (1, 3, 7, 0)] == [1, 3, 7, 7]
    a = spatial_permutation_sums(V, g, seed=seed, first_perm=0, n_permutations=4, return_null=True)
    b = spatial_permutation_sums(V, g, seed=seed, first_perm=4, n_permutations=3, return_null=True)
    base = runs[0]
    assert not np.array_equal(base["null"][0], base["null"][1])
    split = {"null": np.concatenate([a["null"], b["null"]]), "count_ge": a["count_ge"] + b["count_ge"],
             "count_le": a["count_le"] + b["count_le"], "sum_d": a["sum_d"] + b["sum_d"], "sumsq_d": a["sumsq_d"] + b["sumsq_d"]}
    d = base["null"] - base["C"]
    for other in [runs[1], runs[3], runs[7], split]:
        for key in ("null", "count_ge", "count_le"):
            assert np.array_equal(other[key], base[key]), key
        assert np.all(np.abs(other["sum_d"] - base["sum_d"]) <= 4 * R * U * np.abs(d).sum(0))
        assert np.all(np.abs(other["sumsq_d"] - base["sumsq_d"]) <= 4 * R * U * (d * d).sum(0))
    for other in (runs[1], runs[3], runs[7], a, b):
        for key in ("mean", "m2", "m4", "C"):
            assert np.array_equal(other[key], base[key]), key
    # without a null buffer of the caller's the device keeps its own: the same counts and sums
    quiet = spatial_permutation_sums(V, g, seed=seed, n_permutations=R, max_batch=3)
    assert "null" not in quiet
    for key in ("count_ge", "count_le", "sum_d", "sumsq_d"):
        assert np.array_equal(quiet[key], runs[3][key]), key


# ---------------------------------------------------------------- 4. a decisive case
def test_gradient_and_noise_on_a_lattice():
    """16 x 16 lattice (4 neighbours), R = 199, seed 0: a gradient column is more autocorrelated than every permutation of itself
    (p_greater = 1 / 200); an i.i.d. column and the pair are not significant.  The NumPy restatement decides the same."""
    from flashdeconv_amd import _lib
    from flashdeconv_amd.utils.spatial_stats import spatial_permutation_test
    m, R, seed = 16, 199, 0
    xx, yy = np.meshgrid(np.arange(float(m)), np.arange(float(m)), indexing="ij")
    coords = np.stack([xx.ravel(), yy.ravel()], axis=1)
    V = np.stack([xx.ravel() + 0.5 * yy.ravel(), np.random.RandomState(16).rand(m * m)], axis=1)
    g = _device_graph(coords, _lib.GRAPH_RADIUS, radius=1.1)
    try:
        A = _adjacency(g)
        assert A.nnz == 2 * 2 * m * (m - 1)
        out = spatial_permutation_test(V, g, n_permutations=R, random_state=seed)
    finally:
        g.close()
    ref = _reference(V, A, seed, 0, R)
    ge, le = (ref["null"] >= ref["C"]).sum(0), (ref["null"] <= ref["C"]).sum(0)
    greater, less = (1.0 + ge) / (R + 1.0), (1.0 + le) / (R + 1.0)
    p = np.minimum(1.0, 2.0 * np.minimum(greater, less))
    assert greater[0, 0] == 1.0 / 200 and p[1, 1] > 0.05 and p[0, 1] > 0.05                 # the CPU restatement
    assert set(out) == BASE_KEYS | PERM_KEYS and out["n_permutations"] == R
    assert out["p_greater"][0] == 1.0 / 200 and out["p_value"][0] == 0.01 and out["morans_i"][0] > 0.9
    assert out["p_value"][1] > 0.05 and out["cross_p_value"][0, 1] > 0.05 and out["cross_p_value"][1, 0] > 0.05
    np.testing.assert_array_equal(out["cross_p_greater"], greater)
    np.testing.assert_array_equal(out["cross_p_value"], p)
    assert out["z_sim"][0] > 10 and abs(out["z_sim"][1]) < 3 and out["z_score_rand"][0] > 10
    np.testing.assert_allclose(out["z_sim"][0], out["z_score_rand"][0], rtol=0.25)         # two estimates of one null's spread
    se = np.diagonal(out["cross_null_std"]) / np.sqrt(R)
    assert np.all(np.abs(np.diagonal(out["cross_null_mean"]) + 1.0 / (m * m - 1)) <= 4 * se)       # E[I] = -1 / (n - 1)


# ---------------------------------------------------------------- 5. edges and regressions
def test_constant_column_gives_nan_rows_and_columns(knn130):
    from flashdeconv_amd.utils.spatial_stats import spatial_permutation_test
    g, A = knn130
    V = _values(130, 4, 44)
    V[:, 2] = 0.25
    out = spatial_permutation_test(V, g, n_permutations=9, random_state=1, return_null=True)
    assert set(out) == BASE_KEYS | PERM_KEYS | {"cross_null"}
    keep = [0, 1, 3]
    for key in PERM_KEYS - {"n_permutations"}:
        a = out[key]
        if a.ndim == 2:
            assert np.isnan(a[2, :]).all() and np.isnan(a[:, 2]).all() and np.isfinite(a[np.ix_(keep, keep)]).all(), key
        else:
            assert np.isnan(a[2]) and np.isfinite(a[keep]).all(), key
    assert np.isnan(out["variance_i_rand"][2]) and np.isnan(out["z_score_rand"][2]) and np.isfinite(out["z_score_rand"][keep]).all()
    null = out["cross_null"]
    assert isinstance(null, np.ndarray) and null.shape == (9, 4, 4)
    assert np.isnan(null[:, 2, :]).all() and np.isnan(null[:, :, 2]).all() and np.isfinite(null[:, keep][:, :, keep]).all()
    np.testing.assert_allclose(null.mean(0)[np.ix_(keep, keep)], out["cross_null_mean"][np.ix_(keep, keep)], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(null.std(0)[np.ix_(keep, keep)], out["cross_null_std"][np.ix_(keep, keep)], rtol=1e-9)


def test_graph_without_edges_gives_nan():
    from flashdeconv_amd.utils.spatial_stats import spatial_permutation_test
    n = 37
    A = sparse.csr_matrix((n, n))
    out = spatial_permutation_test(_values(n, 3, 5), A, n_permutations=5)
    for key in (PERM_KEYS - {"n_permutations"}) | {"morans_i", "cross", "variance_i_rand", "z_score_rand"}:
        assert np.isnan(out[key]).all(), key
    assert out["n_edges"] == 0 and out["n_permutations"] == 5


def test_no_permutations_leaves_the_permutation_keys_out(knn130):
    from flashdeconv_amd.utils.spatial_stats import randomization_variance, spatial_autocorrelation, spatial_permutation_test
    g, A = knn130
    V = _values(130, 5, 8)
    out, base = spatial_permutation_test(V, g, n_permutations=0, return_null=True), spatial_autocorrelation(V, g)
    assert set(out) == BASE_KEYS
    for key in base:
        assert np.array_equal(np.asarray(out[key]), np.asarray(base[key]), equal_nan=True), key
    Z = V - V.mean(0)
    deg = np.diff(A.indptr)
    want = randomization_variance(130, int(deg.sum()), int((deg * deg).sum()), (Z * Z).sum(0), (Z ** 4).sum(0))
    np.testing.assert_allclose(out["variance_i_rand"], want, rtol=1e-10)
    np.testing.assert_allclose(out["z_score_rand"], (out["morans_i"] - out["expected_i"]) / np.sqrt(want), rtol=1e-10)


@pytest.mark.parametrize("K", [5, 33])
def test_two_calls_return_the_same_bits(knn130, K):
    from flashdeconv_amd.utils.spatial_stats import spatial_permutation_test
    g, _ = knn130
    V = _values(130, K, 7)
    a, b = (spatial_permutation_test(V, g, n_permutations=11, random_state=3, return_null=True) for _ in range(2))
    assert set(a) == set(b) == BASE_KEYS | PERM_KEYS | {"cross_null"}
    for key in a:
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key]), equal_nan=True), key
    c = spatial_permutation_test(V, g, n_permutations=11, random_state=4, return_null=True)
    assert not np.array_equal(a["cross_null"], c["cross_null"]) and np.array_equal(a["cross"], c["cross"])
    rs_a, rs_b = np.random.RandomState(5), np.random.RandomState(5)
    d, e = (spatial_permutation_test(V, g, n_permutations=11, random_state=rs) for rs in (rs_a, rs_b))
    assert np.array_equal(d["cross_z_sim"], e["cross_z_sim"], equal_nan=True)


def test_input_kinds(knn130):
    import torch
    from flashdeconv_amd.utils.spatial_stats import spatial_permutation_test
    g, A = knn130
    V = _values(130, 5, 8)
    V32 = V.astype(np.float32)
    kw = dict(n_permutations=6, random_state=2, return_null=True)
    want, want32 = spatial_permutation_test(V, g, **kw), spatial_permutation_test(V32.astype(np.float64), g, **kw)
    assert isinstance(want["cross_null"], np.ndarray) and "cross_null" not in spatial_permutation_test(V, g, n_permutations=6)

    def same(out, ref, cuda):
        assert set(out) == set(ref)
        for key in ref:
            v = out[key]
            if key == "cross_null":
                assert (isinstance(v, torch.Tensor) and v.is_cuda and v.shape == (6, 5, 5)) if cuda else isinstance(v, np.ndarray)
                v = _host(v)
            assert np.array_equal(np.asarray(v), np.asarray(ref[key]), equal_nan=True), key

    same(spatial_permutation_test(V32, g, **kw), want32, False)
    same(spatial_permutation_test(torch.as_tensor(V, device="cuda:0"), g, **kw), want, True)
    same(spatial_permutation_test(torch.as_tensor(V32, device="cuda:0"), g, **kw), want32, True)
    wide = torch.full((130, 11), float("nan"), dtype=torch.float64, device="cuda:0")
    wide[:, :5] = torch.as_tensor(V, device="cuda:0")
    same(spatial_permutation_test(wide[:, :5], g, **kw), want, True)                   # row stride 11, read in place
    # the same graph uploaded for the call keeps the caller's order: other summation orders, the same integers
    up = spatial_permutation_test(V, A, **kw)
    for key in ("cross_p_greater", "cross_p_less", "cross_p_value", "n", "n_edges"):
        assert np.array_equal(up[key], want[key]), key
    np.testing.assert_allclose(up["cross_null"], want["cross_null"], rtol=1e-9, atol=1e-12)


def test_host_null_is_fetched_in_pieces(knn130, monkeypatch):
    """return_null on a NumPy input with a device budget of two permutations per call: the same null, counts and sums."""
    from flashdeconv_amd.utils import spatial_stats as ss
    g, _ = knn130
    V = _values(130, 5, 8)
    want = ss.spatial_permutation_sums(V, g, seed=9, n_permutations=7, return_null=True)
    monkeypatch.setattr(ss, "_NULL_CALL_BYTES", 2 * 8 * 25)
    got = ss.spatial_permutation_sums(V, g, seed=9, n_permutations=7, return_null=True)
    for key in ("null", "count_ge", "count_le", "C", "m4"):
        assert np.array_equal(got[key], want[key]), key
    assert got["batch"] == 2 and want["batch"] == 7
    np.testing.assert_allclose(got["sum_d"], want["sum_d"], rtol=1e-12, atol=1e-15)


def test_stage_level_entry_refusals():
    import torch
    from flashdeconv_amd import _lib
    lib = _lib.load()
    n, K = 600, 4
    rs = np.random.RandomState(10)
    g = _device_graph(rs.rand(n, 2) * np.sqrt(float(n)), _lib.GRAPH_KNN, 6)
    try:
        Vd = torch.as_tensor(_values(n, K, 10), device="cuda:0")
        f, i = (lambda *s: np.zeros(s)), (lambda *s: np.zeros(s, dtype=np.int64))
        bufs = [f(K), f(K), f(K, K), i(3), f(K), i(K, K), i(K, K), f(K, K), f(K, K)]

        def call(gh=g.handle, vp=Vd.data_ptr(), ld=K, k=K, first=0, cnt=2, mb=0, drop=None):
            ptrs = [(_lib.ptr_i64(b) if b.dtype == np.int64 else _lib.ptr_f64(b)) for b in bufs]
            if drop is not None:
                ptrs[drop] = None
            return lib.fdx_spatial_perm_dev(gh, ctypes.c_void_p(vp), ld, k, ctypes.c_uint64(1), first, cnt, mb, None, *ptrs, None, None)

        _lib.check(call())
        assert bufs[3][0] == n and np.all(bufs[5] + bufs[6] >= 2)
        for bad, msg in ((dict(drop=0), "null argument"), (dict(drop=4), "null argument"), (dict(drop=8), "null argument"),
                         (dict(vp=None), "null argument"), (dict(gh=None), "null argument"), (dict(ld=K - 1), "ldv at least K"),
                         (dict(k=0), "K must be positive"), (dict(first=-1), "must not be negative"),
                         (dict(cnt=-1), "must not be negative"), (dict(mb=-1), "must not be negative")):
            with pytest.raises(_lib.FdxError, match=msg):
                _lib.check(call(**bad))
        local = ctypes.c_void_p()
        bounds = np.array([0, 256, n], dtype=np.int64)
        _lib.check(lib.fdx_graph_localize(g.handle, 2, _lib.ptr_i64(bounds), 0, None, ctypes.byref(local)))
        shard = _lib.Graph(local.value)
        try:
            with pytest.raises(_lib.FdxError, match="shard"):
                _lib.check(call(gh=shard.handle))
        finally:
            shard.close()
    finally:
        g.close()


# ---------------------------------------------------------------- 6. model and AnnData surface
@pytest.mark.parametrize("output", ["numpy", "torch"])
def test_model_method(output):
    from flashdeconv_amd import FlashDeconv
    from flashdeconv_amd.utils.spatial_stats import spatial_permutation_test
    Y, X, coords, _ = datagen.count_like(200, 300, 5, 0.1, seed=9)
    m = FlashDeconv(sketch_dim=64, max_iter=20, random_state=3).fit(Y, X, coords, output=output)
    with pytest.raises(ValueError, match="n_permutations must be an int >= 0"):
        m.get_spatial_autocorrelation(n_permutations=-1)
    got = m.get_spatial_autocorrelation(n_permutations=19)
    want = spatial_permutation_test(m.proportions_, m, n_permutations=19, random_state=3)
    assert set(got) == set(want) == BASE_KEYS | PERM_KEYS and got["n_permutations"] == 19
    for key in want:
        assert np.array_equal(np.asarray(got[key]), np.asarray(want[key]), equal_nan=True), key
    other = m.get_spatial_autocorrelation(n_permutations=19, random_state=4)
    assert not np.array_equal(other["cross_z_sim"], got["cross_z_sim"]) and np.array_equal(other["cross"], got["cross"])
    plain = m.get_spatial_autocorrelation()
    assert set(plain) == {"morans_i", "z_score", "mean", "m2", "cross", "expected_i", "variance_i", "n", "n_edges"}
    for key in plain:
        assert np.array_equal(np.asarray(plain[key]), np.asarray(got[key]), equal_nan=True), key
    with_nm = m.get_spatial_autocorrelation(what="abundances", neighbor_mean=True, n_permutations=3)
    assert set(with_nm) == BASE_KEYS | PERM_KEYS | {"neighbor_mean"}
    assert isinstance(with_nm["neighbor_mean"], np.ndarray) == (output == "numpy")
    assert np.all((got["p_value"] > 0) & (got["p_value"] <= 1)) and np.isfinite(got["z_sim"]).all()


def test_deconvolve_writes_the_p_values_on_request_only():
    import flashdeconv_amd as fd
    from flashdeconv_amd.io import prepare_data
    case = datagen.anndata_case()
    kw = dict(cell_type_key="celltype", sketch_dim=64, k_neighbors=4, n_hvg=300, n_markers_per_type=20)
    st, ref = datagen.anndata_objects(case)
    assert fd.tl.deconvolve(st, ref, spatial_stats=True, **kw) is None
    assert set(st.uns) == {"flashdeconv_params", "flashdeconv_moran", "flashdeconv_colocalization"}
    assert list(st.uns["flashdeconv_moran"].columns) == ["I", "z_score"]
    assert "spatial_permutations" not in st.uns["flashdeconv_params"]

    st2, ref2 = datagen.anndata_objects(case)
    assert fd.tl.deconvolve(st2, ref2, spatial_stats=True, spatial_permutations=29, **kw) is None
    assert set(st2.uns) == {"flashdeconv_params", "flashdeconv_moran", "flashdeconv_colocalization",
                            "flashdeconv_colocalization_pvalue"}
    assert set(st2.uns["flashdeconv_params"]) == set(st.uns["flashdeconv_params"]) | {"spatial_permutations"}
    assert st2.uns["flashdeconv_params"]["spatial_permutations"] == 29
    Y, X, coords, names, _ = prepare_data(st2, ref2, cell_type_key="celltype")
    m = fd.FlashDeconv(sketch_dim=64, k_neighbors=4, n_hvg=300, n_markers_per_type=20).fit(Y, X, coords)
    want = m.get_spatial_autocorrelation(n_permutations=29)
    moran, pv = st2.uns["flashdeconv_moran"], st2.uns["flashdeconv_colocalization_pvalue"]
    types = [str(t) for t in names]
    assert list(moran.index) == types and list(moran.columns) == ["I", "z_score", "p_value", "z_sim"]
    assert list(pv.index) == types and list(pv.columns) == types
    for col, key in (("I", "morans_i"), ("z_score", "z_score"), ("p_value", "p_value"), ("z_sim", "z_sim")):
        np.testing.assert_array_equal(moran[col].values, want[key])
    np.testing.assert_array_equal(pv.values, want["cross_p_value"])
    np.testing.assert_array_equal(st2.uns["flashdeconv_colocalization"].values, st.uns["flashdeconv_colocalization"].values)
    assert np.all((pv.values >= 2.0 / 30) & (pv.values <= 1.0))

    # spatial_permutations without spatial_stats writes nothing
    st3, ref3 = datagen.anndata_objects(case)
    assert fd.tl.deconvolve(st3, ref3, spatial_permutations=29, **kw) is None
    assert set(st3.uns) == {"flashdeconv_params"}
