"""-m gpu tests of the spatially-variable-gene statistics (csrc/gene_spatial_kernels.cpp: fdx_gene_spatial_sums_dev / _csr_dev;
utils.spatial_genes; FlashDeconv.get_spatially_variable_genes; tl.deconvolve(spatial_genes=True)).

Reference: tests/spatial_genes_ref.py (the NumPy definition; checked against the centred textbook definitions in
tests/test_spatial_genes_host.py, which also asserts the conditions used here: the exact cases are exactly representable in any
order, and the planted case separates in the reference).

Exact cases (integers in [0, 7]) must EQUAL the reference in all nine planes on every route and graph: no tolerance.  Generic cases
(non-negative lognormal values rounded to float32) are held, in planes 0-6, to ``rtol = 2 (nnz(A) + n) EPS`` - the worst-case bound
of ANY order of summing that many non-negative terms, each term carrying at most three roundings of its own; a CPU simulation with
reversed and permuted orders on the n = 600 case stayed 1000 x below it, so it excludes wrong terms and admits any correct order -
and planes 7, 8 (min, max) must be EQUAL.
"""
import ctypes

import numpy as np
import pytest
from scipy import sparse

import datagen
import gpu_graphs as gg
import spatial_genes_ref as sr
from conftest import load_golden
from test_gpu_expression import _route_Y

pytestmark = pytest.mark.gpu

ROUTES = ["host_f32", "host_f64", "host_int", "dev_f32", "dev_f64", "dev_strided", "csr_scipy", "csr_cuda", "csr_unsorted"]
GRAPHS = {"knn600": lambda: gg._knn(600), "untiled600": lambda: gg._knn_untiled(600), "hub300": lambda: gg._hub(300),
          "radius": gg._radius_isolated, "grid": gg._grid, "knn1": lambda: gg._knn(1), "knn2": lambda: gg._knn(2),
          "knn63": lambda: gg._knn(63), "knn64": lambda: gg._knn(64), "knn65": lambda: gg._knn(65), "knn257": lambda: gg._knn(257)}
_REF = {}


def _graph(name):
    G = GRAPHS[name]()
    if name == "knn600":
        assert G.perm is not None and not np.array_equal(G.perm, np.arange(G.n)), "the device-built graph kept the caller's order"
    if name == "untiled600":
        assert G.perm is None
    if name == "hub300":
        assert G.max_deg == G.n - 1
    if name == "radius":
        assert (sr.degrees(G.A) == 0).sum() >= 64
    return G


def _reference(key, make_Y, A):
    """(Y, planes) of a case, computed once and shared read-only."""
    if key not in _REF:
        Y = make_Y()
        s = sr.planes(Y, A)
        for a in [Y] + [v for v in s.values() if isinstance(v, np.ndarray)]:
            a.setflags(write=False)
        _REF[key] = (Y, s)
    return _REF[key]


def _assert_planes_equal(got, want, label):
    for name in sr.PLANES:
        assert got[name].shape == want[name].shape and got[name].dtype == np.float64, (label, name)
        assert np.array_equal(got[name], want[name]), (label, name, float(np.abs(got[name] - want[name]).max()))
    for name in ("n", "W", "sum_deg_sq"):
        assert got[name] == want[name] and isinstance(got[name], int), (label, name, got[name], want[name])


def _assert_planes_close(got, want, A, label):
    rtol = 2 * (sparse.csr_matrix(A).nnz + A.shape[0]) * sr.EPS
    for name in sr.PLANES[:7]:
        err = np.abs(got[name] - want[name])
        print(f"{label} {name}: worst relative difference {float((err / np.maximum(np.abs(want[name]), 1e-300)).max()):.3e} (bound {rtol:.3e})")
        assert np.all(err <= rtol * np.abs(want[name])), (label, name)
    for name in ("ymin", "ymax"):
        assert np.array_equal(got[name], want[name]), (label, name)
    for name in ("n", "W", "sum_deg_sq"):
        assert got[name] == want[name], (label, name)


def _exact_cases():
    cases = []
    for gi, graph in enumerate(GRAPHS):
        for ri, route in enumerate(ROUTES):
            cases.append((graph, route, sr.GENE_COUNTS[(gi + ri) % len(sr.GENE_COUNTS)]))
    for G in sr.GENE_COUNTS:                          # every gene count on a dense and on a sparse route, more than one segment
        cases += [("knn600", "dev_f32", G), ("knn257", "host_f64", G), ("knn600", "csr_scipy", G)]
    return sorted(set(cases))


@pytest.mark.parametrize("graph,route,G", _exact_cases())
def test_planes_equal_the_reference_exactly(graph, route, G):
    from flashdeconv_amd.utils.spatial_genes import gene_spatial_sums
    g = _graph(graph)
    density = 0.3 if route.startswith("csr") else 1.0
    Y, want = _reference(("exact", graph, G, density), lambda: sr.exact_case(g.n, G, len(graph) + G, density), g.A)
    got = gene_spatial_sums(_route_Y(Y, route), g.g)
    _assert_planes_equal(got, want, (graph, route, G))


@pytest.mark.parametrize("variant", ["holes", "full"])
@pytest.mark.parametrize("form", ["sorted", "shuffled", "cuda"])
@pytest.mark.parametrize("graph", ["knn600", "hub300", "knn65"])
def test_csr_contents_equal_the_reference_exactly(graph, form, variant):
    """Empty rows, an empty column, stored zeros, a column with negative values beside implicit zeros (its maximum is the implicit
    0); columns stored in every row - one of them negative throughout: no implicit zero - and a row storing all G columns."""
    import torch
    from flashdeconv_amd.utils.spatial_genes import gene_spatial_sums
    g = _graph(graph)
    m, Y = sr.csr_contents_case(g.n, 9, 2, variant)
    want = sr.planes(Y, g.A)
    assert want["ymax"][4] == 0 > want["ymin"][4] and want["ymin"][1] == want["ymax"][1] == 0
    if variant == "full":
        assert want["ymax"][5] < 0
    if form == "shuffled":                            # every row's columns in a random order
        rs = np.random.RandomState(0)
        idx, dat = m.indices.copy(), m.data.copy()
        for i in range(m.shape[0]):
            a, b = m.indptr[i], m.indptr[i + 1]
            p = rs.permutation(b - a)
            idx[a:b], dat[a:b] = idx[a:b][p], dat[a:b][p]
        m = sparse.csr_matrix((dat, idx, m.indptr), shape=m.shape)
        assert not m.has_sorted_indices and (m.data == 0).any()
    elif form == "cuda":
        m = torch.sparse_csr_tensor(torch.as_tensor(m.indptr.astype(np.int64)), torch.as_tensor(m.indices.astype(np.int32)),
                                    torch.as_tensor(m.data.astype(np.float64)), size=m.shape).cuda()
    _assert_planes_equal(gene_spatial_sums(m, g.g), want, (graph, form, variant))


def _generic_Y(g, G, seed, route):
    """A generic case with two planted constant columns; the CSR routes store about 40 % of the other columns."""
    def make():
        Y = sr.generic_case(g.n, G, seed, constant=(1, G - 1) if G > 2 else ())
        if route.startswith("csr"):
            keep = np.random.RandomState(seed).rand(g.n, G) < 0.4
            keep[:, [1, G - 1]] = True
            Y = Y * keep
        return Y
    return make


@pytest.mark.parametrize("graph,route,G", [
    ("knn600", "host_f32", 513), ("knn600", "dev_f64", 40), ("knn600", "csr_scipy", 40), ("knn600", "csr_unsorted", 1025),
    ("untiled600", "dev_strided", 40), ("hub300", "dev_f32", 511), ("hub300", "csr_cuda", 40), ("radius", "host_f64", 40),
    ("radius", "csr_scipy", 40), ("grid", "dev_f32", 1024), ("knn257", "csr_scipy", 40), ("knn257", "dev_strided", 512)])
def test_generic_planes_meet_the_summation_bound(graph, route, G):
    from flashdeconv_amd.utils.spatial_genes import gene_spatial_sums, spatially_variable_genes
    g = _graph(graph)
    Y, want = _reference(("generic", graph, G, route.startswith("csr")), _generic_Y(g, G, 3, route), g.A)
    Yc = _route_Y(Y, route)
    _assert_planes_close(gene_spatial_sums(Yc, g.g), want, g.A, (graph, route, G))
    out = spatially_variable_genes(Yc, g.g)
    assert int(np.isnan(out["morans_i"]).sum()) == 2 and np.isnan(out["morans_i"][[1, G - 1]]).all()
    ref = sr.assemble(want["n"], want["W"], want["sum_deg_sq"], *(want[name] for name in sr.PLANES))
    live = ~np.isnan(ref["morans_i"])
    np.testing.assert_allclose(out["morans_i"][live], ref["morans_i"][live], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(out["gearys_c"][live], ref["gearys_c"][live], rtol=1e-9, atol=1e-12)


def test_permuted_and_caller_order_graphs_give_the_same_planes():
    from flashdeconv_amd.utils.spatial_genes import gene_spatial_sums
    a, b = _graph("knn600"), _graph("untiled600")
    assert (a.A != b.A).nnz == 0
    Y = sr.generic_case(600, 70, 9)
    for route in ("dev_f32", "csr_scipy"):
        Yc = _route_Y(Y * (np.random.RandomState(1).rand(600, 70) < 0.5) if route == "csr_scipy" else Y, route)
        _assert_planes_close(gene_spatial_sums(Yc, a.g), gene_spatial_sums(Yc, b.g), a.A, ("perm", route))


@pytest.mark.parametrize("graph", ["knn600", "untiled600", "radius", "hub300", "knn1"])
@pytest.mark.parametrize("route", ["dev_f32", "csr_scipy"])
def test_degree_equals_the_adjacency_row_counts(graph, route):
    import torch
    from flashdeconv_amd.utils.spatial_genes import gene_spatial_sums
    g = _graph(graph)
    Y = sr.exact_case(g.n, 5, 1, 0.5)
    out = gene_spatial_sums(_route_Y(Y, route), g.g, return_degree=True)
    assert out["degree"].is_cuda and out["degree"].dtype == torch.int32 and out["degree"].shape == (g.n,)
    assert np.array_equal(out["degree"].cpu().numpy(), sr.degrees(g.A))
    assert "degree" not in gene_spatial_sums(_route_Y(Y, route), g.g)
    # a scipy adjacency is uploaded for the call: the same planes as the device-built graph's within the order bound (exact here)
    _assert_planes_equal(gene_spatial_sums(_route_Y(Y, route), g.A), {k: v for k, v in out.items() if k != "degree"}, (graph, route))


@pytest.mark.parametrize("route", ["dev_f32", "host_f64", "csr_scipy", "csr_unsorted"])
def test_two_calls_and_another_stripe_count_return_the_same_bits(route, monkeypatch):
    """Generic (inexact) data over three segments: a second call, and calls whose workgroups take 2 or 5 segments each
    (FDX_EXPR_STRIPE_SEGMENTS, the knob of every segment-wise gene pass), return the bits of the first."""
    from flashdeconv_amd.utils.spatial_genes import gene_spatial_sums
    g = _graph("knn600")
    assert g.n > 2 * 256                                    # FDX_GENE_SPATIAL_SEGMENT_POSITIONS: three segments
    Y = sr.generic_case(600, 530, 4) * (np.random.RandomState(2).rand(600, 530) < 0.4)
    Yc = _route_Y(Y, route)
    first = gene_spatial_sums(Yc, g.g)
    again = gene_spatial_sums(Yc, g.g)
    for name in sr.PLANES:
        assert np.array_equal(first[name], again[name]), name
    for stripe in ("2", "5"):
        monkeypatch.setenv("FDX_EXPR_STRIPE_SEGMENTS", stripe)
        other = gene_spatial_sums(Yc, g.g)
        for name in sr.PLANES:
            assert np.array_equal(first[name], other[name]), (stripe, name)


@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("route", ["host_f64", "dev_f32", "csr_scipy"])
def test_residual_sums_match_the_dense_residual(K, route):
    """Residual mode against R = Y - weights E formed densely, E taken from the device's own output (the solver's rounding does not
    enter).  atol_g = 4 T EPS S_g with T = nnz(A) + n (K + 1) and S_g the sum of the magnitudes of the terms of the array's expansion
    (tests/spatial_genes_ref.py:residual_sums)."""
    from flashdeconv_amd.utils.expression import celltype_expression
    from flashdeconv_amd.utils.spatial_genes import spatially_variable_genes
    g = _graph("knn600")
    rs = np.random.RandomState(10 + K)
    n, G = g.n, 48
    W = rs.dirichlet(np.full(K, 0.5), size=n) * rs.gamma(4.0, 0.25, size=(n, 1))
    Y = sr.generic_case(n, G, 5, constant=(7,))
    if route == "csr_scipy":
        Y = Y * (rs.rand(n, G) < 0.4)
        Y[:, 7] = 1.1
        Y = Y.astype(np.float32).astype(np.float64)
    Yc = _route_Y(Y, route)
    out = spatially_variable_genes(Yc, g.g, weights=W, n_top=5)
    E = out["expression"]
    assert E.shape == (K, G) and np.all(E >= 0) and set(out["residual_sums"]) == {"u", "q", "D", "P"}
    want, mags = sr.residual_sums(Y, g.A, W, E)
    T = sparse.csr_matrix(g.A).nnz + n * (K + 1)
    for name in ("u", "q", "D", "P"):
        err = np.abs(out["residual_sums"][name] - want[name])
        atol = 4 * T * sr.EPS * mags[name]
        ratio = err / np.where(atol > 0, atol, 1.0)                # (an all-zero gene: every term and the error are 0)
        print(f"residual K={K} {route} {name}: worst error / bound {float(ratio.max()):.3e}")
        assert np.all(err <= atol), (name, float(ratio.max()))
    # the statistics of the residual are those of its sums, NaN where the gene itself has none
    from flashdeconv_amd.utils.spatial_genes import _morans
    r = out["residual_sums"]
    _, _, morans_r = _morans(out["n"], 2 * out["n_edges"], r["u"], r["q"], r["D"], r["P"], np.isnan(out["morans_i"]))
    assert np.array_equal(out["residual_morans_i"], morans_r, equal_nan=True)
    assert np.isnan(out["morans_i"][7]) and np.isnan(out["residual_morans_i"][7]) and np.isnan(out["residual_z_score"][7])
    assert int(np.isnan(out["morans_i"]).sum()) == 1
    ref_r = sr.morans_from_sums(n, 2 * out["n_edges"], want["u"], want["q"], want["D"], want["P"], np.isnan(out["morans_i"]))[2]
    live = ~np.isnan(ref_r)
    np.testing.assert_allclose(out["residual_morans_i"][live], ref_r[live], rtol=1e-8, atol=1e-10)
    assert list(out["residual_order"][:3]) == list(sr.decreasing_order(out["residual_morans_i"])[:3])
    assert np.array_equal(out["top"], out["order"][:5])
    assert np.array_equal(out["r2"], celltype_expression(Yc, W)["r2"], equal_nan=True)


def test_statistics_equal_assemble_genes_of_the_sums():
    from flashdeconv_amd.utils.spatial_genes import assemble_genes, gene_spatial_sums, spatially_variable_genes
    g = _graph("radius")
    Y = sr.generic_case(g.n, 33, 6, constant=(4,))
    out = spatially_variable_genes(Y, g.g)
    s = gene_spatial_sums(Y, g.g)
    want = assemble_genes(s["n"], s["W"], s["sum_deg_sq"], *(s[name] for name in sr.PLANES))
    assert set(out) == set(want) | {"n", "n_edges"} and out["n"] == g.n and out["n_edges"] == g.nnz // 2
    for key, val in want.items():
        assert np.array_equal(np.asarray(out[key]), np.asarray(val), equal_nan=True), key
        assert isinstance(out[key], (np.ndarray, np.floating)), key
    ref = sr.assemble(s["n"], s["W"], s["sum_deg_sq"], *(s[name] for name in sr.PLANES))
    for key, val in ref.items():
        assert np.array_equal(np.asarray(out[key]), np.asarray(val), equal_nan=True), key


def test_planted_gradient_leads_and_the_constant_gene_is_nan():
    from flashdeconv_amd.utils.spatial_genes import spatially_variable_genes
    g = _graph("grid")
    for route in ("host_f64", "csr_scipy"):
        out = spatially_variable_genes(_route_Y(sr.planted_case(), route), g.g, n_top=1)
        assert out["order"][0] == 0 and list(out["top"]) == [0]
        assert out["morans_i"][0] > 0.8 > abs(out["morans_i"][1])
        assert np.isnan(out["morans_i"][2]) and np.isnan(out["gearys_c"][2]) and np.isnan(out["q_value"][2]) and out["order"][2] == 2
        assert out["q_value"][0] < 1e-6 and out["q_value"][1] > 0.05 and out["gearys_c"][0] < 0.2


def test_the_c_entries_refuse_bad_arguments():
    import torch
    from flashdeconv_amd import _lib
    lib = _lib.load()
    g = _graph("knn65")
    Y = torch.zeros((65, 4), dtype=torch.float32, device="cuda")
    sums = torch.zeros((9, 4), dtype=torch.float64, device="cuda")
    counts = np.zeros(3, dtype=np.int64)
    yp, sp = ctypes.c_void_p(Y.data_ptr()), ctypes.c_void_p(sums.data_ptr())
    for match, args in (("null argument", (None, yp, _lib.FDX_F32, 65, 4, 4, sp, None, _lib.ptr_i64(counts), None)),
                        ("null argument", (g.g.handle, None, _lib.FDX_F32, 65, 4, 4, sp, None, _lib.ptr_i64(counts), None)),
                        ("null argument", (g.g.handle, yp, _lib.FDX_F32, 65, 4, 4, None, None, _lib.ptr_i64(counts), None)),
                        ("null argument", (g.g.handle, yp, _lib.FDX_F32, 65, 4, 4, sp, None, None, None)),
                        ("G must be at least 1", (g.g.handle, yp, _lib.FDX_F32, 65, 0, 4, sp, None, _lib.ptr_i64(counts), None)),
                        ("ldy < G", (g.g.handle, yp, _lib.FDX_F32, 65, 4, 3, sp, None, _lib.ptr_i64(counts), None)),
                        ("64 rows but the graph has 65", (g.g.handle, yp, _lib.FDX_F32, 64, 4, 4, sp, None, _lib.ptr_i64(counts), None)),
                        ("n must be between", (g.g.handle, yp, _lib.FDX_F32, 2 ** 31 - 128, 4, 4, sp, None, _lib.ptr_i64(counts), None)),
                        ("dtype must be", (g.g.handle, yp, 7, 65, 4, 4, sp, None, _lib.ptr_i64(counts), None))):
        with pytest.raises(_lib.FdxError, match=match):
            _lib.check(lib.fdx_gene_spatial_sums_dev(*args))
    with pytest.raises(_lib.FdxError, match="null argument"):
        _lib.check(lib.fdx_gene_spatial_sums_csr_dev(g.g.handle, None, sp, None, _lib.ptr_i64(counts), None))


# ---------------------------------------------------------------- surface
@pytest.mark.parametrize("output", ["numpy", "torch"])
def test_model_method_equals_the_direct_call(output):
    from flashdeconv_amd import FlashDeconv
    from flashdeconv_amd.utils.spatial_genes import spatially_variable_genes
    gold = load_golden("fit_counts_100x500x5_d64.npz")
    Y, X, coords = gold["Y"], gold["X"], gold["coords"]
    m = FlashDeconv(sketch_dim=64, max_iter=30, random_state=0).fit(Y, X, coords, output=output)
    with pytest.raises(ValueError, match="Unknown what"):
        m.get_spatially_variable_genes(Y, what="counts")
    with pytest.raises(ValueError, match="spots of the fit as rows"):
        m.get_spatially_variable_genes(Y[:50])
    with pytest.raises(ValueError, match="spot_scale must be"):
        m.get_spatially_variable_genes(Y, residual=True, spot_scale=np.ones(7))
    host = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)     # noqa: E731

    def same(got, want):
        assert set(got) == set(want)
        for key in want:
            if key == "residual_sums":
                same(got[key], want[key])
            else:
                assert np.array_equal(host(got[key]), host(want[key]), equal_nan=True), key
    plain_keys = {"morans_i", "gearys_c", "z_score", "variance_i_rand", "z_score_rand", "p_value", "q_value", "mean", "m2", "m4",
                  "order", "expected_i", "variance_i", "n", "n_edges"}
    for Yc in (Y, sparse.csr_matrix(Y), Y[:, :123]):
        got = m.get_spatially_variable_genes(Yc)
        assert set(got) == plain_keys and got["morans_i"].shape == (Yc.shape[1],) and got["n"] == 100
        same(got, spatially_variable_genes(Yc, m))
    scale = Y.sum(axis=1) / Y.sum(axis=1).mean()
    for what, values in (("proportions", m.proportions_), ("abundances", m.beta_)):
        got = m.get_spatially_variable_genes(Y, residual=True, what=what, n_top=10)
        assert set(got) == plain_keys | {"residual_morans_i", "residual_z_score", "residual_order", "r2", "expression", "residual_sums",
                                         "top"}
        assert all(isinstance(v, (np.ndarray, np.floating, int, dict)) for v in got.values()) and got["expression"].shape == (5, 500)
        same(got, spatially_variable_genes(Y, m, weights=values, n_top=10))
        scaled = m.get_spatially_variable_genes(Y, residual=True, what=what, spot_scale=scale)
        want = spatially_variable_genes(Y, m, weights=host(values) * scale[:, None])
        np.testing.assert_allclose(scaled["expression"], want["expression"], rtol=1e-9, atol=1e-12)
        assert np.array_equal(scaled["morans_i"], got["morans_i"], equal_nan=True)


def test_deconvolve_writes_the_spatial_genes_on_request_only():
    import flashdeconv_amd as fd
    from flashdeconv_amd.io import prepare_data
    case = datagen.anndata_case()
    kw = dict(cell_type_key="celltype", sketch_dim=64, k_neighbors=4, n_hvg=300, n_markers_per_type=20)
    st0, ref0 = datagen.anndata_objects(case)
    assert fd.tl.deconvolve(st0, ref0, spatial_genes=False, **kw) is None
    st, ref1 = datagen.anndata_objects(case)
    assert fd.tl.deconvolve(st, ref1, spatial_genes=True, **kw) is None
    assert set(st.uns) == set(st0.uns) | {"flashdeconv_spatial_genes"}
    assert set(st.obsm) == set(st0.obsm) and set(st.obs.columns) == set(st0.obs.columns)
    assert set(st.uns["flashdeconv_params"]) == set(st0.uns["flashdeconv_params"]) | {"spatial_genes"}
    assert st.uns["flashdeconv_params"]["spatial_genes"] is True
    Y, X, coords, names, genes = prepare_data(st, ref1, cell_type_key="celltype")
    m = fd.FlashDeconv(sketch_dim=64, k_neighbors=4, n_hvg=300, n_markers_per_type=20).fit(Y, X, coords)
    want = m.get_spatially_variable_genes(Y, residual=True, spot_scale=Y.sum(axis=1) / Y.sum(axis=1).mean())
    frame = st.uns["flashdeconv_spatial_genes"]
    assert list(frame.index) == [str(x) for x in genes] and frame.shape == (470, 8)
    assert list(frame.columns) == ["I", "C", "z_score", "p_value", "q_value", "residual_I", "residual_z_score", "r2"]
    for column, key in (("I", "morans_i"), ("C", "gearys_c"), ("z_score", "z_score"), ("p_value", "p_value"), ("q_value", "q_value"),
                        ("residual_I", "residual_morans_i"), ("residual_z_score", "residual_z_score"), ("r2", "r2")):
        np.testing.assert_array_equal(frame[column].values, want[key])
    assert np.nanmax(frame["r2"].values) <= 1.0 and np.all((frame["q_value"].values >= frame["p_value"].values) | frame["p_value"].isna())
