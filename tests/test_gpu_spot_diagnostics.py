"""-m gpu tests of the per-spot fit diagnostics (spot_diagnostics_kernel in csrc/finish_kernels.cpp, fdx_spot_diagnostics_dev,
fdx_fit_params.spot_diag_out_dev, FlashDeconv.fit(spot_diagnostics=True), tl.deconvolve(spot_diagnostics=True)).

The reference values are formed in NumPy from the oracle's sketches and the MODEL'S OWN abundances, so the kernel is checked
apart from solver differences (bounded elsewhere):
    direct = ||s_i - beta_i Xs||^2,   y2 = ||s_i||^2,   nb_i = 0.5 * sum_{j in N(i)} ||beta_i - beta_j||^2.

Tolerances.  In float64 the expanded form the kernel evaluates differs from `direct` by at most 1.5e-15 * y2 per spot
(measured with the oracle on the count_like and gaussian_raw families); the device accumulates H and row_sq in another order, and
the per-element sketch -> H checks assert 1e-13.  Hence, for float64 inputs,
    sketch_sq    rtol 1e-12,
    residual_sq  |residual_sq - direct| <= 1e-11 * y2   (with direct / y2 > 1e-3 asserted: below 1e-8 of the residual itself),
    neighbor_sq  rtol 1e-12 (a plain sum of squares of differences, no cancellation).
float32 inputs run the float32 tile / CSR sketch: their bound is 10 x the error measured on the MI355X against the oracle fed the
same values in float64 (F32_MEASURED below), the factor covering run-to-run differences in accumulation order.
"""
import ctypes

import numpy as np
import pytest
from scipy import sparse

import datagen
import fdx_oracle as orc

pytestmark = pytest.mark.gpu

NAMES = ("residual_sq", "sketch_sq", "neighbor_sq")
RES_TOL, SKETCH_RTOL, NB_RTOL = 1e-11, 1e-12, 1e-12
# max |residual_sq - direct| / y2 and max |sketch_sq / y2 - 1| measured on the MI355X for the two float32 cases of
# test_float32_inputs (dense 100 x 500 x 5 d=64 log_cpm, CSR 300 x 900 x 5 d=64 log_cpm with gene selection)
# dense: the float32 tile sketch; csr: counts are exact in float32 and the CSR kernels compute in float64 - the figures are those of
# the float64 path, bit for bit, in three runs each
F32_MEASURED = {"dense": (2.341533e-09, 1.220010e-07), "csr": (5.652155e-16, 4.440892e-16)}


def _sketches(Y, X, d, pre, **kw):
    """Y_sketch (n, d), X_sketch (K, d) of the pinned oracle for these inputs (its solve is skipped: max_iter=0)."""
    want = orc.fit(Y, X, np.zeros((Y.shape[0], 2)), sketch_dim=d, preprocess_method=pre, max_iter=0, k_neighbors=1,
                   lambda_spatial=0.0, **kw)
    return want["Y_sketch"], want["X_sketch"]


def _host(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def _reference(model, Ys, Xs):
    beta = _host(model.beta_)
    direct = ((Ys - beta @ Xs) ** 2).sum(1)
    y2 = (Ys ** 2).sum(1)
    A = model.adjacency_
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    nb = 0.5 * np.bincount(rows, weights=((beta[rows] - beta[A.indices]) ** 2).sum(1), minlength=A.shape[0])
    return direct, y2, nb


def _errors(model, Ys, Xs):
    """(max |residual_sq - direct| / y2, max |sketch_sq / y2 - 1|, min direct / y2): printed by every check, asserted by it."""
    direct, y2, _ = _reference(model, Ys, Xs)
    dg = {k: _host(v) for k, v in model.spot_diagnostics_.items()}
    return (float(np.max(np.abs(dg["residual_sq"] - direct) / y2)), float(np.max(np.abs(dg["sketch_sq"] / y2 - 1.0))),
            float(np.min(direct / y2)))


def _check(model, Ys, Xs, res_tol=RES_TOL, sketch_rtol=SKETCH_RTOL):
    n = Ys.shape[0]
    dg = model.spot_diagnostics_
    assert set(dg) == set(NAMES)
    for k in NAMES:
        assert tuple(dg[k].shape) == (n,) and str(dg[k].dtype).endswith("float64")
    dg = {k: _host(v) for k, v in dg.items()}
    direct, y2, nb = _reference(model, Ys, Xs)
    res_err, sk_err, floor = _errors(model, Ys, Xs)
    print(f"residual err / y2 {res_err:.3e}  sketch_sq rel err {sk_err:.3e}  min direct / y2 {floor:.3e}")
    assert floor > 1e-3                                   # the bound on the residual below keeps its meaning
    np.testing.assert_allclose(dg["sketch_sq"], y2, rtol=sketch_rtol)
    assert np.all(np.abs(dg["residual_sq"] - direct) <= res_tol * y2)
    np.testing.assert_allclose(dg["neighbor_sq"], nb, rtol=NB_RTOL, atol=1e-300)
    assert np.all(dg["residual_sq"] >= 0) and np.all(dg["neighbor_sq"] >= 0)
    deg = np.diff(model.adjacency_.indptr)
    assert np.all(dg["neighbor_sq"][deg == 0] == 0.0)
    assert model.timings_["diagnostics_ms"] >= 0.0
    return dg


def _objective_identity(model, dg, Xs):
    rho_eff = model.rho_sparsity * np.mean(np.diag(Xs @ Xs.T))
    total = 0.5 * dg["residual_sq"].sum() + 0.5 * model.lambda_used_ * dg["neighbor_sq"].sum() + rho_eff * _host(model.beta_).sum()
    np.testing.assert_allclose(total, model.info_["final_objective"], rtol=1e-10)


# ---------------------------------------------------------------- 1. slice tails and tiny problems
@pytest.mark.parametrize("pre", ["log_cpm", "raw"])
@pytest.mark.parametrize("n,G,K,d", [(37, 90, 3, 16), (64, 40, 4, 33), (257, 700, 6, 100), (1, 30, 2, 8)])
def test_slice_tails_and_tiny_problems(n, G, K, d, pre):
    """Counts with half of the entries dropped: at these few genes the plain count_like family is fitted to below the 1e-3 floor
    that _check asserts on its inputs (measured with the oracle: 2e-4 under "raw", 9e-4 at 40 genes under "log_cpm")."""
    from flashdeconv_amd import FlashDeconv
    Y, X, coords, _ = datagen.count_like(n, G, K, 0.1, seed=n + G)
    Y = (Y * (np.random.RandomState(n).rand(n, G) < 0.5)).astype(np.float64)
    m = FlashDeconv(sketch_dim=d, preprocess=pre, max_iter=20).fit(Y, X, coords, spot_diagnostics=True)
    dg = _check(m, *_sketches(Y, X, d, pre))
    if n == 1:
        assert dg["neighbor_sq"][0] == 0.0


# ---------------------------------------------------------------- 2. every sweep family
@pytest.mark.parametrize("K", [1, 5, 63, 64, 70, 96, 100])
def test_every_sweep_family(K):
    """1-64 register-resident sweeps (63 / 64 straddle the LDS tile of the diagnostics kernel), 70 / 96 the padded planes with the
    bordered XtX (row stride 72 / 96), 100 the sweep above 96."""
    from flashdeconv_amd import FlashDeconv
    Y, X, coords, _ = datagen.gaussian_raw(130, 300, K, seed=K, noise=0.1)
    m = FlashDeconv(sketch_dim=64, preprocess="raw", max_iter=5).fit(Y, X, coords, spot_diagnostics=True)
    _check(m, *_sketches(Y, X, 64, "raw"))


# ---------------------------------------------------------------- 3. graph kinds
def _graph_case(n, seed=3):
    Y, X, coords, _ = datagen.gaussian_raw(n, 400, 5, seed=seed)
    return Y, X, coords, _sketches(Y, X, 64, "raw")


def test_radius_graph_with_isolated_spots():
    from flashdeconv_amd import FlashDeconv
    Y, X, coords, sk = _graph_case(300)
    m = FlashDeconv(sketch_dim=64, preprocess="raw", spatial_method="radius", radius=0.6, max_iter=20).fit(
        Y, X, coords, spot_diagnostics=True)
    dg = _check(m, *sk)
    deg = np.diff(m.adjacency_.indptr)
    assert (deg == 0).sum() >= 1 and (deg > 0).sum() >= 1
    assert np.all(dg["neighbor_sq"][deg == 0] == 0.0) and np.any(dg["neighbor_sq"][deg > 0] > 0)


def test_grid_graph():
    from flashdeconv_amd import FlashDeconv
    Y, X, coords, sk = _graph_case(300)
    m = FlashDeconv(sketch_dim=64, preprocess="raw", spatial_method="grid", max_iter=20).fit(Y, X, coords, spot_diagnostics=True)
    _check(m, *sk)


def test_host_adjacency_route_above_63_neighbours():
    """k = 70 at 80 spots: the lists come from the host, the graph is uploaded in the caller's order (no permutation)."""
    from flashdeconv_amd import FlashDeconv
    Y, X, coords, sk = _graph_case(80)
    m = FlashDeconv(sketch_dim=64, preprocess="raw", k_neighbors=70, max_iter=20).fit(Y, X, coords, spot_diagnostics=True)
    assert np.diff(m.adjacency_.indptr).min() >= 70           # (symmetrised: 70 to 79 neighbours of 79 possible)
    _check(m, *sk)


@pytest.mark.parametrize("ties", ["auto", "index"])
def test_lattice(ties):
    """12 x 12 integer lattice: under "auto" the first call stops on ties (it writes nothing) and the diagnostics come from the
    second call, which takes the first one's sketch -> H stage and row norms over as a carry."""
    import warnings
    from flashdeconv_amd import FlashDeconv
    Y, X, _, _ = datagen.gaussian_raw(144, 400, 5, seed=4)
    gx, gy = np.meshgrid(np.arange(12.0), np.arange(12.0))
    coords = np.stack([gx.ravel(), gy.ravel()], 1)
    m = FlashDeconv(sketch_dim=64, preprocess="raw", max_iter=20, knn_ties=ties)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)      # "index": the tie warning
        m.fit(Y, X, coords, spot_diagnostics=True)
    assert m.info_["knn_ties"] > 0
    _check(m, *_sketches(Y, X, 64, "raw"))


# ---------------------------------------------------------------- 4. inputs and outputs
def test_csr_float64_with_gene_selection():
    from flashdeconv_amd import FlashDeconv
    Y, X, coords, _ = datagen.count_like(300, 900, 5, 0.1, seed=7)
    Ys = sparse.csr_matrix(Y.astype(np.float64))
    kw = dict(n_hvg=250, n_markers_per_type=10)
    m = FlashDeconv(sketch_dim=64, max_iter=20, **kw).fit(Ys, X, coords, spot_diagnostics=True)
    assert len(m.gene_idx_) < 900
    _check(m, *_sketches(Ys, X, 64, "log_cpm", **kw))


def _f32_case(kind):
    if kind == "dense":
        Y, X, coords, _ = datagen.count_like(100, 500, 5, 0.1, seed=42)
        Y32, kw = Y.astype(np.float32), {}
        Y64 = Y32.astype(np.float64)
    else:
        Y, X, coords, _ = datagen.count_like(300, 900, 5, 0.1, seed=7)
        Y32, kw = sparse.csr_matrix(Y.astype(np.float32)), dict(n_hvg=250, n_markers_per_type=10)
        Y64 = sparse.csr_matrix(Y.astype(np.float32).astype(np.float64))
    return Y32, Y64, X, coords, kw


@pytest.mark.parametrize("kind", ["dense", "csr"])
def test_float32_inputs(kind):
    """The float32 sketch paths against the oracle fed the same values in float64.  Measured on the MI355X (three fits each, the
    same figures every time): dense max |residual_sq - direct| / y2 = 2.34e-9, max |sketch_sq / y2 - 1| = 1.22e-7; csr 5.65e-16 and
    4.44e-16.  Asserted at 10 x the measured value."""
    from flashdeconv_amd import FlashDeconv
    Y32, Y64, X, coords, kw = _f32_case(kind)
    m = FlashDeconv(sketch_dim=64, max_iter=20, **kw).fit(Y32, X, coords, spot_diagnostics=True)
    res_meas, sk_meas = F32_MEASURED[kind]
    _check(m, *_sketches(Y64, X, 64, "log_cpm", **kw), res_tol=10 * res_meas, sketch_rtol=10 * sk_meas)


def test_int64_counts():
    from flashdeconv_amd import FlashDeconv
    Y, X, coords, _ = datagen.count_like(100, 500, 5, 0.1, seed=42)
    Y = Y.astype(np.int64)
    m = FlashDeconv(sketch_dim=64, max_iter=20).fit(Y, X, coords, spot_diagnostics=True)
    _check(m, *_sketches(Y, X, 64, "log_cpm"))


def test_cuda_tensors_in_and_out():
    import torch
    from flashdeconv_amd import FlashDeconv
    Y, X, coords, _ = datagen.count_like(100, 500, 5, 0.1, seed=42)
    Y = Y.astype(np.float64)
    Yd, cd = torch.from_numpy(Y).cuda(), torch.from_numpy(coords).cuda()
    m = FlashDeconv(sketch_dim=64, max_iter=20).fit(Yd, X, cd, output="torch", spot_diagnostics=True)
    for k in NAMES:
        v = m.spot_diagnostics_[k]
        assert isinstance(v, torch.Tensor) and v.is_cuda and v.device == Yd.device and v.dtype == torch.float64
    base = m.spot_diagnostics_["residual_sq"].untyped_storage().data_ptr()
    assert all(m.spot_diagnostics_[k].untyped_storage().data_ptr() == base for k in NAMES)      # views of one 3n block
    dg = _check(m, *_sketches(Y, X, 64, "log_cpm"))
    r = m.get_spot_residuals()
    assert isinstance(r, torch.Tensor) and r.is_cuda and tuple(r.shape) == (100,)
    np.testing.assert_allclose(r.cpu().numpy(), np.sqrt(dg["residual_sq"] / dg["sketch_sq"]), rtol=1e-14)
    np.testing.assert_allclose(m.get_spot_residuals(relative=False).cpu().numpy(), np.sqrt(dg["residual_sq"]), rtol=1e-14)


# ---------------------------------------------------------------- 5. no sweep at all
def test_max_iter_zero_reports_the_uniform_start():
    from flashdeconv_amd import FlashDeconv
    Y, X, coords, _ = datagen.count_like(100, 500, 5, 0.1, seed=42)
    Y = Y.astype(np.float64)
    m = FlashDeconv(sketch_dim=64, max_iter=0).fit(Y, X, coords, spot_diagnostics=True)
    assert np.array_equal(m.beta_, np.full((100, 5), 1.0 / 5))
    dg = _check(m, *_sketches(Y, X, 64, "log_cpm"))
    assert np.all(dg["neighbor_sq"] == 0.0)


# ---------------------------------------------------------------- 6. the caller's order, whatever the solver's
def test_rows_follow_the_callers_spot_order():
    from flashdeconv_amd import FlashDeconv
    Y, X, coords, _ = datagen.gaussian_raw(257, 300, 6, seed=6)
    kw = dict(sketch_dim=64, preprocess="raw", max_iter=20, tol=1e-12, random_state=0)
    a = FlashDeconv(**kw).fit(Y, X, coords, spot_diagnostics=True)
    sh = np.random.RandomState(1).permutation(257)
    b = FlashDeconv(**kw).fit(Y[sh], X, coords[sh], spot_diagnostics=True)
    assert a.info_["knn_ties"] == 0 and a.info_["n_iterations"] == b.info_["n_iterations"]
    inv = np.argsort(sh)
    for k in NAMES:
        assert not np.allclose(b.spot_diagnostics_[k], a.spot_diagnostics_[k], rtol=1e-9)       # the shuffle moved the rows ...
        np.testing.assert_allclose(b.spot_diagnostics_[k][inv], a.spot_diagnostics_[k], rtol=1e-9)   # ... and only moved them


# ---------------------------------------------------------------- 7. off means off
def test_off_means_off():
    from flashdeconv_amd import FlashDeconv
    Y, X, coords, _ = datagen.count_like(100, 500, 5, 0.1, seed=42)
    Y = Y.astype(np.float64)
    m = FlashDeconv(sketch_dim=64)
    m.fit(Y, X, coords)
    assert m.spot_diagnostics_ is None and "diagnostics_ms" not in m.timings_
    keys_off = set(m.timings_)
    with pytest.raises(RuntimeError, match="spot_diagnostics=True"):
        m.get_spot_residuals()
    beta_off = m.beta_.copy()
    m.fit(Y, X, coords, spot_diagnostics=True)
    assert set(m.spot_diagnostics_) == set(NAMES) and set(m.timings_) == keys_off | {"diagnostics_ms"}
    assert np.array_equal(m.beta_, beta_off)
    r = m.get_spot_residuals()
    assert isinstance(r, np.ndarray) and r.shape == (100,) and np.all(r > 0) and np.all(r < 1)
    np.testing.assert_array_equal(m.get_spot_residuals(relative=False), np.sqrt(m.spot_diagnostics_["residual_sq"]))
    m.fit(Y, X, coords)
    assert m.spot_diagnostics_ is None and set(m.timings_) == keys_off
    with pytest.raises(RuntimeError, match="spot_diagnostics=True"):
        m.get_spot_residuals()


# ---------------------------------------------------------------- the three planes decompose the objective
@pytest.mark.parametrize("rho", [0.0, 0.01])
def test_the_planes_sum_to_the_objective(rho):
    """0.5 sum residual_sq + 0.5 lambda sum neighbor_sq + rho_eff sum beta = final_objective: holds only when the difference form is
    summed over a symmetric graph and every spot is written exactly once.  With rho = 0 nothing of the oracle enters."""
    from flashdeconv_amd import FlashDeconv
    Y, X, coords, _ = datagen.count_like(300, 900, 7, 0.1, seed=9)
    Y = Y.astype(np.float64)
    m = FlashDeconv(sketch_dim=128, rho_sparsity=rho).fit(Y, X, coords, spot_diagnostics=True)
    dg = m.spot_diagnostics_
    Xs = np.zeros((7, 128)) if rho == 0.0 else _sketches(Y, X, 128, "log_cpm")[1]
    _objective_identity(m, dg, Xs)


# ---------------------------------------------------------------- 8. the stage-level entry
def test_stage_level_entry():
    """fdx_spot_diagnostics_dev on a device-built graph: random positive beta and H, a random SPD XtX taken from inside a wider matrix
    (row stride ldg > K), row_sq small on a few spots so that the clamp fires.  residual_sq against the same expansion in NumPy."""
    import torch
    from flashdeconv_amd import _lib
    lib = _lib.load()
    n, K, ldg = 200, 4, 7
    rs = np.random.RandomState(8)
    coords = rs.rand(n, 2) * np.sqrt(n)
    cd = torch.as_tensor(coords, device="cuda:0")
    h = ctypes.c_void_p()
    _lib.check(lib.fdx_graph_build_dev(ctypes.c_void_p(cd.data_ptr()), n, 2, _lib.GRAPH_KNN, 6, 0.0, None, ctypes.byref(h)))
    g = _lib.Graph(h.value)
    try:
        perm_d = torch.empty(n, dtype=torch.int32, device="cuda:0")
        _lib.check(lib.fdx_graph_perm_dev(g.handle, ctypes.c_void_p(perm_d.data_ptr()), None))
        torch.cuda.synchronize()
        perm = perm_d.cpu().numpy().astype(np.int64)
        assert not np.array_equal(perm, np.arange(n))
        indptr, indices = g.to_csr_arrays()
        beta = rs.rand(n, K) + 0.1
        M = rs.randn(K, K + 3)
        G = M @ M.T + np.eye(K)
        # h_i = XtX beta_i (1 + noise): cross ~ quad, so the expansion is ~ row_sq - quad
        Hm = (beta @ G) * (1.0 + 0.01 * rs.randn(n, K))
        quad = np.einsum("ik,kl,il->i", beta, G, beta)
        row_sq = quad * (3.0 + rs.rand(n))
        small = rs.choice(n, 9, replace=False)
        row_sq[small] = quad[small] * 1e-3
        ld = (n + 1 + 63) // 64 * 64
        ldh = ld + 64
        bt, Ht = np.zeros((K, ld)), np.full((K, ldh), np.nan)
        bt[:, :n], Ht[:, :n] = beta[perm].T, Hm[perm].T
        Gw = np.full((K, ldg), np.nan)
        Gw[:, :K] = G
        dev = [torch.as_tensor(a, device="cuda:0") for a in (bt, Ht, Gw, row_sq[perm])]
        out = torch.full((3 * n,), np.nan, dtype=torch.float64, device="cuda:0")
        _lib.check(lib.fdx_spot_diagnostics_dev(g.handle, ctypes.c_void_p(dev[0].data_ptr()), ld, ctypes.c_void_p(dev[1].data_ptr()), ldh,
                                                ctypes.c_void_p(dev[2].data_ptr()), ldg, K, ctypes.c_void_p(dev[3].data_ptr()),
                                                ctypes.c_void_p(out.data_ptr()), None))
        torch.cuda.synchronize()
        got = out.cpu().numpy().reshape(3, n)
        want_res = np.maximum(row_sq - 2.0 * (beta * Hm).sum(1) + quad, 0.0)
        assert (want_res[small] == 0.0).all() and (want_res > 0).sum() == n - len(small)
        rows = np.repeat(np.arange(n), np.diff(indptr))
        want_nb = 0.5 * np.bincount(rows, weights=((beta[rows] - beta[indices]) ** 2).sum(1), minlength=n)
        np.testing.assert_allclose(got[0], want_res, rtol=1e-12)
        np.testing.assert_array_equal(got[1], row_sq)
        np.testing.assert_allclose(got[2], want_nb, rtol=1e-12)
        with pytest.raises(_lib.FdxError, match="ld must cover"):
            _lib.check(lib.fdx_spot_diagnostics_dev(g.handle, ctypes.c_void_p(dev[0].data_ptr()), n, ctypes.c_void_p(dev[1].data_ptr()), ldh,
                                                    ctypes.c_void_p(dev[2].data_ptr()), ldg, K, ctypes.c_void_p(dev[3].data_ptr()),
                                                    ctypes.c_void_p(out.data_ptr()), None))
        with pytest.raises(_lib.FdxError, match="null argument"):
            _lib.check(lib.fdx_spot_diagnostics_dev(g.handle, ctypes.c_void_p(dev[0].data_ptr()), ld, ctypes.c_void_p(dev[1].data_ptr()), ldh,
                                                    ctypes.c_void_p(dev[2].data_ptr()), ldg, K, None, ctypes.c_void_p(out.data_ptr()), None))
    finally:
        g.close()


# ---------------------------------------------------------------- 9. tl.deconvolve
def test_deconvolve_writes_the_two_columns_on_request_only():
    import flashdeconv_amd as fd
    from flashdeconv_amd.io import prepare_data
    case = datagen.anndata_case()
    kw = dict(cell_type_key="celltype", sketch_dim=64, k_neighbors=4, n_hvg=300, n_markers_per_type=20)
    st, ref = datagen.anndata_objects(case)
    assert fd.tl.deconvolve(st, ref, **kw) is None
    params_today = {"sketch_dim", "lambda_spatial", "rho_sparsity", "n_hvg", "n_markers_per_type", "spatial_method", "k_neighbors",
                    "radius", "preprocess", "n_genes_used", "n_cell_types", "cell_type_names", "random_state", "converged",
                    "n_iterations"}
    assert set(st.obs.columns) == {"flashdeconv_dominant"} and set(st.obsm) == {"spatial", "flashdeconv"}
    assert set(st.uns) == {"flashdeconv_params"} and set(st.uns["flashdeconv_params"]) == params_today

    st2, ref2 = datagen.anndata_objects(case)
    assert fd.tl.deconvolve(st2, ref2, spot_diagnostics=True, **kw) is None
    assert set(st2.obs.columns) == {"flashdeconv_dominant", "flashdeconv_residual", "flashdeconv_roughness"}
    assert set(st2.obsm) == {"spatial", "flashdeconv"}
    assert set(st2.uns["flashdeconv_params"]) == params_today | {"spot_diagnostics"}
    assert st2.uns["flashdeconv_params"]["spot_diagnostics"] is True
    res, rough = st2.obs["flashdeconv_residual"].values, st2.obs["flashdeconv_roughness"].values
    assert len(res) == 120 and len(rough) == 120
    assert np.all(np.isfinite(res)) and np.all(np.isfinite(rough)) and np.all(res >= 0) and np.all(rough >= 0)
    assert np.array_equal(st2.obsm["flashdeconv"].values, st.obsm["flashdeconv"].values)
    Y, X, coords, names, _ = prepare_data(st2, ref2, cell_type_key="celltype")
    m = fd.FlashDeconv(sketch_dim=64, k_neighbors=4, n_hvg=300, n_markers_per_type=20).fit(Y, X, coords, spot_diagnostics=True)
    np.testing.assert_array_equal(res, m.get_spot_residuals())
    np.testing.assert_array_equal(rough, m.spot_diagnostics_["neighbor_sq"])
