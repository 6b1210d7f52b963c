"""-m gpu tests of the spatial correlogram (csrc/correlogram_kernels.cpp, fdx_spatial_correlogram_dev, utils.correlogram,
FlashDeconv.get_spatial_correlogram, tl.deconvolve(correlogram=)).

Reference: tests/correlogram_ref.py (brute force over all pairs in NumPy; checked against scipy in tests/test_correlogram_host.py).

Exact values (correlogram_ref.exact_values: sixteenths up to 1 / 2 in magnitude whose columns sum to exactly zero) make every sum
the device forms exact in any order - the precondition is asserted in tests/test_correlogram_host.py - so C, m2, m4, W, sum_deg_sq
and degree must EQUAL the reference: no tolerance.  Generic values (Dirichlet) are held to the per-band bounds of
correlogram_ref's docstring; the counts stay exact.
"""
import numpy as np
import pytest

import correlogram_ref as cr
import datagen

pytestmark = pytest.mark.gpu

_SETS = cr.coord_sets()
_REF = {}


def _case(name, K, seed):
    """(V, coords, radii, reference) of an exact case, computed once."""
    key = (name, K, seed)
    if key not in _REF:
        coords, radii = _SETS[name]
        V = cr.exact_values(coords.shape[0], K, seed)
        ref = cr.band_reference(V, coords, radii)
        for a in [V, coords, radii] + [ref[k] for k in ("deg", "W", "sum_deg_sq", "C", "mean", "m2", "m4")]:
            a.setflags(write=False)
        _REF[key] = (V, coords, radii, ref)
    return _REF[key]


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def _assert_exact(got, ref, label):
    assert got["n"] == ref["n"]
    for key, want in (("W", ref["W"]), ("sum_deg_sq", ref["sum_deg_sq"]), ("mean", ref["mean"]), ("m2", ref["m2"]), ("m4", ref["m4"]),
                      ("C", ref["C"])):
        assert got[key].shape == want.shape, (label, key)
        assert np.array_equal(got[key], want), (label, key, np.abs(got[key] - want).max())
    deg = _host(got["degree"])
    assert deg.dtype == np.int32 and deg.shape == ref["deg"].shape and np.array_equal(deg, ref["deg"]), (label, "degree")


def _sums(V, coords, radii, **kw):
    from flashdeconv_amd.utils.correlogram import correlogram_sums
    return correlogram_sums(V, coords, radii, degree=True, **kw)


_LATTICE = [c for c in cr.exact_cases() if c[0] in ("square32", "cube8", "chain257")]
_B_EDGE = [c for c in cr.exact_cases() if c[0].startswith("square32_B")]
_SIZE = [c for c in cr.exact_cases() if c[0].startswith("cloud")]
_RAGGED = [c for c in cr.exact_cases() if c[0].startswith("ragged")]
_THIN = [c for c in cr.exact_cases() if c[0] in ("strip0", "strip_thin", "slab")]


# ---------------------------------------------------------------- 1. lattices, K and B edges, chunking
@pytest.mark.parametrize("name,K,seed", _LATTICE + _B_EDGE)
def test_lattices_exact(name, K, seed):
    V, coords, radii, ref = _case(name, K, seed)
    _assert_exact(_sums(V, coords, radii), ref, (name, K))


@pytest.mark.parametrize("name,K,seed", [("square32", 30, 130), ("square32_B10", 5, 610), ("cube8", 9, 209)])
def test_bands_per_pass_changes_no_bit(name, K, seed):
    V, coords, radii, ref = _case(name, K, seed)
    B = len(radii)
    base = _sums(V, coords, radii)
    assert base["bands_per_pass"] == B                       # these fit the scratch budget whole
    _assert_exact(base, ref, name)
    for cap in (1, 3):
        got = _sums(V, coords, radii, max_bands_per_pass=cap)
        assert got["bands_per_pass"] == min(cap, B)
        _assert_exact(got, ref, (name, cap))
    # generic values: the bits, not only the exact sums, are the same whatever the chunk
    Vg = cr.dirichlet_values(coords.shape[0], K, 5)
    g0 = _sums(Vg, coords, radii)
    for cap in (1, 3):
        g = _sums(Vg, coords, radii, max_bands_per_pass=cap)
        for key in ("C", "mean", "m2", "m4", "W", "sum_deg_sq"):
            assert np.array_equal(g[key], g0[key]), (name, cap, key)


# ---------------------------------------------------------------- 2. size edges and coincident spots
@pytest.mark.parametrize("name,K,seed", _SIZE)
def test_size_edges_exact(name, K, seed):
    from flashdeconv_amd.utils.correlogram import spatial_correlogram
    V, coords, radii, ref = _case(name, K, seed)
    n = coords.shape[0]
    if n == 257:
        assert len(np.unique(coords, axis=0)) < n            # coincident spots: d = 0 lands in band 1
        i, j = ref["A"][0].nonzero()
        assert np.any(np.all(coords[i] == coords[j], axis=1))
    got = _sums(V, coords, radii)
    _assert_exact(got, ref, name)
    assert int(got["W"].sum()) == n * (n - 1)                # radius 100 holds every pair
    if n == 1:
        out = spatial_correlogram(V, coords, radii)
        assert np.all(out["n_pairs"] == 0) and out["n"] == 1
        for key in ("cross", "morans_i", "z_score", "expected_i", "variance_i", "variance_i_rand", "z_score_rand"):
            assert np.all(np.isnan(out[key])), key


# ---------------------------------------------------------------- 3. ragged cells
@pytest.mark.parametrize("name,K,seed", _RAGGED)
def test_ragged_cells_exact(name, K, seed):
    V, coords, radii, ref = _case(name, K, seed)
    got = _sums(V, coords, radii)
    _assert_exact(got, ref, name)
    assert np.all(_host(got["degree"])[-1] == 0)             # the spot at (10, 10) has no neighbour in any band
    assert ref["deg"].sum(1).max() > 64                      # the cluster: more than a wave of neighbours, cells above 64 points


@pytest.mark.parametrize("name,K,seed", _THIN)
def test_thin_axes_exact(name, K, seed):
    """An axis of one cell in front of an axis of many (a strip along y, a slab thin in x): the cell ids' strides tie."""
    V, coords, radii, ref = _case(name, K, seed)
    _assert_exact(_sums(V, coords, radii), ref, name)


# ---------------------------------------------------------------- 4. generic values
def test_generic_values_within_bounds():
    from flashdeconv_amd.utils.correlogram import assemble_correlogram
    coords, radii = _SETS["uniform3000"]
    V = cr.dirichlet_values(3000, 30, 21)
    ref = cr.band_reference(V, coords, radii)
    got = _sums(V, coords, radii)
    assert np.array_equal(got["W"], ref["W"]) and np.array_equal(got["sum_deg_sq"], ref["sum_deg_sq"])
    assert np.array_equal(_host(got["degree"]), ref["deg"])
    for key in ("mean", "m2", "m4", "C"):
        err, tol = np.abs(got[key] - ref[key]), ref["tol"][key]
        worst = float(np.max(np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))))
        print(f"uniform3000 {key}: max |err| {float(err.max()):.3e}, worst err / bound {worst:.3e}")
        assert np.all(err <= tol), (key, worst)
    sg = assemble_correlogram(got["n"], got["W"], got["sum_deg_sq"], got["m2"], got["m4"], got["C"])
    sr = assemble_correlogram(ref["n"], ref["W"], ref["sum_deg_sq"], ref["m2"], ref["m4"], ref["C"])
    for b in range(len(radii)):
        ctol = cr.cross_tol(ref, b, sr["cross"][b])
        err = np.abs(sg["cross"][b] - sr["cross"][b])
        worst = float(np.max(err / ctol))
        print(f"uniform3000 band {b} cross: max |err| {float(err.max()):.3e}, worst err / bound {worst:.3e}")
        assert np.all(np.isfinite(sr["cross"][b])) and np.all(err <= ctol), (b, worst)
        assert np.all(np.abs(sg["morans_i"][b] - sr["morans_i"][b]) <= np.diagonal(ctol))


# ---------------------------------------------------------------- 5. identity with the existing routes
@pytest.mark.parametrize("name,K,seed", [("square32", 9, 109), ("ragged2", 9, 501)])
def test_cumulative_bands_are_the_radius_graphs(name, K, seed):
    from flashdeconv_amd import _lib
    from flashdeconv_amd.utils.spatial_stats import spatial_sums
    V, coords, radii, ref = _case(name, K, seed)
    got = _sums(V, coords, radii)
    for b, r in enumerate(radii):
        g = _lib.Graph.from_coords_radius(coords, float(r))
        try:
            s = spatial_sums(V, g)
            assert int(got["W"][:b + 1].sum()) == g.info()[1] == s["W"], (name, b)
            assert np.array_equal(got["C"][:b + 1].sum(0), s["C"]), (name, b)
            assert np.array_equal(got["mean"], s["mean"]) and np.array_equal(got["m2"], s["m2"]), (name, b)
        finally:
            g.close()


def test_default_radii_band_one_is_the_grid_graph():
    from flashdeconv_amd.utils.correlogram import spatial_correlogram
    from flashdeconv_amd.utils.graph import build_grid_graph, grid_radius
    coords, radii = _SETS["square23"]
    V = cr.exact_values(coords.shape[0], 4, 77)
    out = spatial_correlogram(V, coords, n_bands=3, degree=True)
    assert np.array_equal(out["radii"], grid_radius(coords) * np.arange(1, 4)) and np.array_equal(out["radii"], radii)
    A = build_grid_graph(coords)
    assert np.array_equal(out["degree"][:, 0], np.asarray(A.sum(1)).ravel().astype(np.int32))
    assert out["n_pairs"][0] * 2 == A.nnz


# ---------------------------------------------------------------- 6. analytic
def test_checkerboard():
    from flashdeconv_amd.utils.correlogram import spatial_correlogram
    coords, radii = _SETS["checker32"]
    V = ((-1.0) ** (coords[:, 0] + coords[:, 1]))[:, None]
    out = spatial_correlogram(V, coords, radii)
    # band 1: the four opposite-colour neighbours; band 2: the diagonals; band 3: the (2, 0) pairs - both the same colour
    np.testing.assert_allclose(out["morans_i"][:, 0], [-1.0, 1.0, 1.0], rtol=0, atol=1e-14)


# ---------------------------------------------------------------- 7. determinism and order
def test_two_calls_same_bits_and_row_order():
    coords, radii = _SETS["uniform3000"]
    V = cr.dirichlet_values(3000, 30, 21)
    a, b = _sums(V, coords, radii), _sums(V, coords, radii)
    for key in ("C", "mean", "m2", "m4", "W", "sum_deg_sq", "degree"):
        assert np.array_equal(a[key], b[key]), key
    Ve, ce, re_, ref = _case("ragged2", 9, 501)
    p = np.random.RandomState(1).permutation(ce.shape[0])
    s = _sums(Ve[p], ce[p], re_)
    base = _sums(Ve, ce, re_)
    for key in ("C", "m2", "m4", "W", "sum_deg_sq"):
        assert np.array_equal(s[key], base[key]), key
    assert np.array_equal(s["degree"], base["degree"][p])


# ---------------------------------------------------------------- 8. input forms
def test_input_forms_give_the_same_bits():
    import torch
    V, coords, radii, ref = _case("square32", 9, 109)
    base = _sums(V, coords, radii)
    assert isinstance(base["degree"], np.ndarray)
    f32 = _sums(V.astype(np.float32), coords, radii)               # sixteenths: float32 holds them
    wide = torch.zeros((V.shape[0], 14), dtype=torch.float64, device="cuda:0")
    wide[:, 3:12] = torch.as_tensor(V.copy(), device="cuda:0")
    sl = _sums(wide[:, 3:12], coords, radii)                        # ldv = 14 > K = 9
    cd = _sums(V, torch.as_tensor(coords.copy(), device="cuda:0"), radii)
    both = _sums(wide[:, 3:12], torch.as_tensor(coords.copy(), device="cuda:0"), radii)
    assert getattr(sl["degree"], "is_cuda", False) and getattr(both["degree"], "is_cuda", False) and sl["degree"].dtype == torch.int32
    assert isinstance(cd["degree"], np.ndarray)
    for other in (f32, sl, cd, both):
        for key in ("C", "mean", "m2", "m4", "W", "sum_deg_sq"):
            assert np.array_equal(other[key], base[key]), key
        assert np.array_equal(_host(other["degree"]), base["degree"])
    _assert_exact(base, ref, "square32")


# ---------------------------------------------------------------- 9. guard
@pytest.mark.parametrize("name", cr.CANDIDATE_SETS)
def test_candidate_count_is_the_host_sum(name):
    """The guard's number, exactly: sum over cells of count(cell) x count(3^dim block), on lattices in 1-3 dimensions, one cell
    in all, and grids whose leading axis has a single cell (strips, a slab)."""
    coords, radii = _SETS[name]
    want, cells = cr.candidate_count(coords, radii[-1])
    if name in ("strip0", "strip_thin", "slab"):
        assert cells[0] == 1 and max(cells[1:]) > 3
    got = _sums(np.ones((coords.shape[0], 1)), coords, radii)
    assert got["candidates"] == want, (name, cells)


def test_candidate_guard_refuses_then_the_next_call_works():
    from flashdeconv_amd import _lib
    V, coords, radii, ref = _case("square32", 9, 109)
    ok = _sums(V, coords, radii)
    assert ok["candidates"] >= int(ref["W"].sum()) + coords.shape[0]       # every member pair and every self pair is a candidate
    with pytest.raises(_lib.FdxError, match="candidate pairs, more than max_candidates = 1000"):
        _sums(V, coords, radii, max_candidates=1000)
    _assert_exact(_sums(V, coords, radii, max_candidates=ok["candidates"]), ref, "at the limit")
    _assert_exact(_sums(V, coords, radii), ref, "after the refusal")


# ---------------------------------------------------------------- 10. surface
@pytest.mark.parametrize("output", ["numpy", "torch"])
def test_model_method(output):
    from flashdeconv_amd import FlashDeconv
    from flashdeconv_amd.utils.correlogram import spatial_correlogram
    Y, X, coords, _ = datagen.count_like(200, 300, 5, 0.1, seed=9)
    m = FlashDeconv(sketch_dim=64, max_iter=20, random_state=3).fit(Y, X, coords, output=output)
    with pytest.raises(ValueError, match="Unknown what"):
        m.get_spatial_correlogram(coords, what="counts")
    from flashdeconv_amd.utils.graph import grid_radius
    assert np.array_equal(coords, _SETS["fit200"][0])
    radii = _SETS["fit200"][1]
    np.testing.assert_allclose(radii[0], grid_radius(coords), rtol=1e-14)
    for what, values in (("proportions", m.proportions_), ("abundances", m.beta_)):
        got = m.get_spatial_correlogram(coords, radii, what=what)
        want = spatial_correlogram(values, coords, radii)
        assert set(got) == set(want) >= {"radii", "n_pairs", "n", "mean", "m2", "cross", "morans_i", "z_score", "expected_i",
                                         "variance_i", "variance_i_rand", "z_score_rand"}
        for key in want:
            assert np.array_equal(np.asarray(got[key]), np.asarray(want[key]), equal_nan=True), (what, key)
        assert got["cross"].shape == (3, 5, 5) and got["n_pairs"].dtype == np.int64
    dflt = m.get_spatial_correlogram(coords, n_bands=4)
    assert dflt["radii"].shape == (4,) and np.array_equal(dflt["radii"], grid_radius(coords) * np.arange(1, 5))


def test_deconvolve_writes_the_correlogram_on_request_only():
    import flashdeconv_amd as fd
    from flashdeconv_amd.io import prepare_data
    case = datagen.anndata_case()
    kw = dict(cell_type_key="celltype", sketch_dim=64, k_neighbors=4, n_hvg=300, n_markers_per_type=20)
    st0, ref0 = datagen.anndata_objects(case)
    assert fd.tl.deconvolve(st0, ref0, **kw) is None
    st, ref1 = datagen.anndata_objects(case)
    assert fd.tl.deconvolve(st, ref1, correlogram=3, **kw) is None
    assert set(st.uns) == set(st0.uns) | {"flashdeconv_correlogram"}
    assert set(st.obsm) == set(st0.obsm) and set(st.obs.columns) == set(st0.obs.columns)
    assert set(st.uns["flashdeconv_params"]) == set(st0.uns["flashdeconv_params"]) | {"correlogram"}
    assert st.uns["flashdeconv_params"]["correlogram"] == 3
    Y, X, coords, names, _ = prepare_data(st, ref1, cell_type_key="celltype")
    assert np.array_equal(coords, _SETS["anndata120"][0])
    m = fd.FlashDeconv(sketch_dim=64, k_neighbors=4, n_hvg=300, n_markers_per_type=20).fit(Y, X, coords)
    want = m.get_spatial_correlogram(coords, n_bands=3)
    np.testing.assert_allclose(want["radii"], _SETS["anndata120"][1], rtol=1e-14)
    cg = st.uns["flashdeconv_correlogram"]
    assert set(cg) == {"radii", "n_pairs", "morans_i", "z_score", "cross"}
    types = [str(t) for t in names]
    for key in ("morans_i", "z_score"):
        assert list(cg[key].columns) == types and list(cg[key].index) == [0, 1, 2]
        np.testing.assert_array_equal(cg[key].values, want[key])
    np.testing.assert_array_equal(cg["cross"], want["cross"])
    np.testing.assert_array_equal(cg["radii"], want["radii"])
    np.testing.assert_array_equal(cg["n_pairs"], want["n_pairs"])
    assert cg["cross"].shape == (3, len(types), len(types))
    st2, ref2 = datagen.anndata_objects(case)
    assert fd.tl.deconvolve(st2, ref2, correlogram=[float(r) for r in want["radii"][:2]], **kw) is None
    # (other radii, another grid of cells: the same numbers to rounding; the same radii, the same bits)
    want2 = m.get_spatial_correlogram(coords, want["radii"][:2])
    np.testing.assert_array_equal(st2.uns["flashdeconv_correlogram"]["morans_i"].values, want2["morans_i"])
    np.testing.assert_allclose(want2["morans_i"], want["morans_i"][:2], rtol=0, atol=1e-12)
    assert st2.uns["flashdeconv_params"]["correlogram"] == [float(r) for r in want["radii"][:2]]
    st3, ref3 = datagen.anndata_objects(case)
    assert fd.tl.deconvolve(st3, ref3, correlogram=True, **kw) is None
    assert len(st3.uns["flashdeconv_correlogram"]["radii"]) == 10 and st3.uns["flashdeconv_params"]["correlogram"] is True
