"""-m gpu tests of the permutation test per gene (csrc/gene_perm_kernels.cpp: fdx_gene_spatial_perm_dev / _csr_dev;
utils.gene_permutations; FlashDeconv.get_spatially_variable_genes(n_permutations=...); tl.deconvolve(gene_permutations=...)).

Reference: tests/gene_perm_ref.py (the NumPy definition over ``permutation_indices``); tests/test_gene_perm_host.py asserts the
conditions used here on the CPU: the exact cases are exactly representable in any order, the planted case separates, and the null
of the reference has the randomisation moments.

Exact cases (integers in [0, 7]) must EQUAL the reference in ``obs`` and in the whole ``null`` on every route and graph: no
tolerance.  The order tests ask for equal BITS between calls that differ in what must not matter.  Generic cases (non-negative
lognormal values rounded to float32) are held to ``rtol = 2 (nnz(A) + n) EPS``, the project's worst-case bound of any order of
summing that many non-negative terms (tests/test_gpu_spatial_genes.py).
"""
import ctypes

import numpy as np
import pytest
from scipy import sparse

import datagen
import gene_perm_ref as gr
from conftest import load_golden
from test_gpu_expression import _route_Y
from test_gpu_spatial_genes import GRAPHS, ROUTES, _graph

pytestmark = pytest.mark.gpu

TILE = 4                                            # float32 genes of a tile (asserted against the module's export below); float64: 2
SIZES = (TILE - 1, TILE, TILE + 1, 1, 2)            # tile - 1, tile, tile + 1 of both tiles, and 1
F64_ROUTES = ("host_f64", "dev_f64", "csr_cuda")    # the routes that hand the device float64 values
R_EXACT = 7
RED_BYTES = 4 * (4 * 3 * TILE * 8)                  # LDS of the wave sums beside the tile: four ways (csrc/gene_perm_kernels.cpp)
_REF = {}


def _genes(G, S, seed):
    """S distinct columns of G in no particular order."""
    return np.random.RandomState(seed).permutation(G)[:S].astype(np.int64)


def _reference(key, make_Y, A, genes, seed, first, R):
    """(Y, observed planes, null) of a case, computed once and shared read-only."""
    if key not in _REF:
        Y = make_Y()
        o, null = gr.observed(Y, A, genes), gr.null_sums(Y, A, seed, first, R, genes)
        for a in [Y, null] + [v for v in o.values() if isinstance(v, np.ndarray)]:
            a.setflags(write=False)
        _REF[key] = (Y, o, null)
    return _REF[key]


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _assert_equal(got, o, null, label):
    for name in gr.OBS_PLANES:
        assert got[name].shape == o[name].shape and got[name].dtype == np.float64, (label, name)
        assert np.array_equal(got[name], o[name]), (label, name, float(np.abs(got[name] - o[name]).max()))
    for name in ("n", "W", "sum_deg_sq"):
        assert got[name] == o[name] and isinstance(got[name], int), (label, name, got[name], o[name])
    have = _host(got["null"])
    assert have.shape == null.shape and have.dtype == np.float64, (label, have.shape, null.shape)
    assert np.array_equal(have, null), (label, "null", float(np.abs(have - null).max()))


def _tile(route):
    return TILE // 2 if route in F64_ROUTES else TILE


def _lds_need(n, elem, tile, table=True):
    return RED_BYTES + n * (tile * elem + (4 if table else 0))


def _exact_cases():
    cases = []
    for gi, graph in enumerate(GRAPHS):
        for ri, route in enumerate(ROUTES):
            cases.append((graph, route, SIZES[(gi + ri) % len(SIZES)], 5 * ((gi + ri // 2) % 2)))
    for S in SIZES + (2 * TILE + 1,):                 # every size on a dense and on a sparse route with both offsets, three rows a thread
        cases += [("knn600", "dev_f32", S, 0), ("knn600", "dev_f32", S, 5), ("knn600", "csr_scipy", S, 0), ("knn257", "host_f64", S, 5)]
    return sorted(set(cases))


def test_the_cases_cover_what_they_claim():
    from flashdeconv_amd.utils import gene_permutations as gp
    assert gp.GENE_TILE == TILE
    cases = _exact_cases()
    assert {c[0] for c in cases} == set(GRAPHS) == {"knn1", "knn2", "knn63", "knn64", "knn65", "knn257", "knn600", "untiled600", "hub300",
                                                    "radius", "grid"}
    assert {c[1] for c in cases} == set(ROUTES) and {c[2] for c in cases} >= set(SIZES) and {c[3] for c in cases} == {0, 5}
    for graph in GRAPHS:
        assert len({c[1] for c in cases if c[0] == graph}) == len(ROUTES)


@pytest.mark.parametrize("graph,route,S,first", _exact_cases())
def test_obs_and_null_equal_the_reference_exactly(graph, route, S, first):
    from flashdeconv_amd.utils.gene_permutations import gene_permutation_sums
    from flashdeconv_amd.utils.spatial_genes import gene_spatial_sums
    g = _graph(graph)
    G = S + 3
    genes = _genes(G, S, S + len(graph))
    density = 0.3 if route.startswith("csr") else 1.0
    Y, o, null = _reference(("exact", graph, S, density, first), lambda: gr.exact_case(g.n, G, len(graph) + S, density), g.A, genes, 3,
                            first, R_EXACT)
    Yc = _route_Y(Y, route)
    got = gene_permutation_sums(Yc, g.g, genes=genes, seed=3, first_perm=first, n_permutations=R_EXACT)
    _assert_equal(got, o, null, (graph, route, S, first))
    assert got["n_permutations"] == R_EXACT and np.array_equal(got["genes"], genes) and got["genes"].dtype == np.int64
    assert got["tile"] == _tile(route) and got["route"] == "lds_table" and got["stripes"] == 1 and got["batch"] == R_EXACT
    # the observed planes are those of the per-gene pass on the same inputs
    planes = gene_spatial_sums(Yc, g.g)
    for name in gr.OBS_PLANES:
        assert np.array_equal(got[name], planes[name][genes]), (graph, route, name)
    assert (got["n"], got["W"], got["sum_deg_sq"]) == (planes["n"], planes["W"], planes["sum_deg_sq"])


@pytest.mark.parametrize("variant", ["holes", "full"])
@pytest.mark.parametrize("form", ["sorted", "cuda"])
@pytest.mark.parametrize("graph", ["knn600", "hub300", "knn65"])
def test_csr_contents_equal_the_reference_exactly(graph, form, variant):
    """Empty rows, an empty column, stored zeros, a negative column beside implicit zeros, columns stored in every row."""
    import torch
    from flashdeconv_amd.utils.gene_permutations import gene_permutation_sums
    g = _graph(graph)
    m, Y = gr.csr_contents_case(g.n, 9, 2, variant)
    genes = np.array([4, 1, 8, 2, 5, 0, 3], dtype=np.int64)
    o, null = gr.observed(Y, g.A, genes), gr.null_sums(Y, g.A, 11, 5, R_EXACT, genes)
    assert o["ymax"][0] == 0 > o["ymin"][0] and o["ymin"][1] == o["ymax"][1] == 0
    if form == "cuda":
        m = torch.sparse_csr_tensor(torch.as_tensor(m.indptr.astype(np.int64)), torch.as_tensor(m.indices.astype(np.int32)),
                                    torch.as_tensor(m.data.astype(np.float64)), size=m.shape).cuda()
    got = gene_permutation_sums(m, g.g, genes=genes, seed=11, first_perm=5, n_permutations=R_EXACT)
    _assert_equal(got, o, null, (graph, form, variant))
    assert got["null"].is_cuda if form == "cuda" else isinstance(got["null"], np.ndarray)


def _generic_Y(n, G, seed, route):
    Y = gr.generic_case(n, G, seed, constant=(1, G - 1))
    if route.startswith("csr"):
        keep = np.random.RandomState(seed).rand(n, G) < 0.4
        keep[:, [1, G - 1]] = True
        Y = Y * keep
    return Y


# ---------------------------------------------------------------- order: equal bits
@pytest.mark.parametrize("route", ["dev_f32", "host_f64", "csr_scipy", "dev_strided"])
def test_what_must_not_matter_moves_no_bit(route):
    """Generic (inexact) data, three positions a thread: a second call, a range of permutations split into two calls, the number of
    permutations in flight, every route of the null kernel (forced through max_lds_bytes) and every gene tile, the order of the gene
    list and a subset of it - bit for bit the numbers of the first call."""
    from flashdeconv_amd.utils.gene_permutations import gene_permutation_sums
    g = _graph("knn600")
    n, G, R = g.n, 14, 9
    assert n > 2 * 256
    Y = _generic_Y(n, G, 4, route)
    Yc = _route_Y(Y, route)
    genes = _genes(G, 11, 1)
    kw = dict(genes=genes, seed=77, first_perm=2, n_permutations=R)
    first = gene_permutation_sums(Yc, g.g, **kw)
    base = _host(first["null"])
    tile_max = _tile(route)
    assert first["route"] == "lds_table" and first["tile"] == tile_max and first["batch"] == R
    assert (first["ways"], first["chunk"]) == (3, 3)               # few tiles: workgroups of 3 permutations each, a way a permutation

    def same(other, label, rows=slice(None), cols=slice(None)):
        for name in gr.OBS_PLANES:
            assert np.array_equal(first[name][cols], other[name]), (label, name)
        assert np.array_equal(base[rows][:, :, cols], _host(other["null"])), (label, "null")

    same(gene_permutation_sums(Yc, g.g, **kw), "again")
    same(gene_permutation_sums(Yc, g.g, **dict(kw, n_permutations=4)), "head", rows=slice(0, 4))
    same(gene_permutation_sums(Yc, g.g, **dict(kw, first_perm=6, n_permutations=5)), "tail", rows=slice(4, 9))
    for max_batch, want in ((1, 1), (2, 2), (0, R)):
        other = gene_permutation_sums(Yc, g.g, max_batch=max_batch, **kw)
        assert other["batch"] == want
        same(other, ("max_batch", max_batch))
    elem = 8 if route == "host_f64" else 4
    seen = set()
    for tile, table in ((2, True), (1, True), (1, False), (0, False)):
        # just enough LDS for this tile (and table), too little for the next larger one; tile 0: nothing fits
        cap = _lds_need(n, elem, tile, table) if tile else 1
        other = gene_permutation_sums(Yc, g.g, max_lds_bytes=cap, **kw)
        want = ("lds_table" if table else "lds") if tile else "global"
        assert (other["tile"], other["route"]) == (min(tile, tile_max) if tile else tile_max, want), (cap, other["tile"], other["route"])
        same(other, ("max_lds_bytes", cap))
        seen.add(other["route"])
        if tile:                                                    # one byte less: the next smaller plan
            less = gene_permutation_sums(Yc, g.g, max_lds_bytes=cap - 1, **dict(kw, n_permutations=0))
            assert (less["tile"], less["route"]) != (other["tile"], other["route"]), cap
    assert seen == {"lds_table", "lds", "global"}
    tiles = -(-11 // tile_max)                                     # the gathered copy in stripes of two tiles and of one
    for cap, stripes in ((2 * n * tile_max * elem, -(-tiles // 2)), (1, tiles)):
        other = gene_permutation_sums(Yc, g.g, max_gather_bytes=cap, **kw)
        assert other["stripes"] == stripes > 1 and first["stripes"] == 1
        same(other, ("max_gather_bytes", cap))
    back = np.argsort(genes)                                       # another order: column for column the same bits
    other = gene_permutation_sums(Yc, g.g, **dict(kw, genes=genes[back]))
    same(other, "sorted", cols=back)
    same(gene_permutation_sums(Yc, g.g, **dict(kw, genes=genes[[7, 2]])), "subset", cols=[7, 2])
    same(gene_permutation_sums(Yc, g.g, max_lds_bytes=1, **dict(kw, genes=genes[[5]])), "one gene, global", cols=[5])
    # without the null: the counts are those of the null
    lean = gene_permutation_sums(Yc, g.g, return_null=False, **kw)
    assert "null" not in lean
    for key, val in first["counts"].items():
        assert np.array_equal(lean["counts"][key], val, equal_nan=True), key


MANY_S, MANY_R = 256, 300


@pytest.mark.parametrize("route", ["dev_f32", "csr_scipy"])
def test_workgroups_of_four_ways_and_several_rounds_equal_the_reference_exactly(route):
    """The shape every large call runs in: 64 tiles and 300 permutations, so a workgroup takes 10 permutations and walks them four
    at a time in three rounds (4, 4 and 2 ways at work: tables reloaded, the wave sums' scratch reused, idle ways at the
    barriers).  Exact data: EQUAL to the reference, and so is a call of one way and one round."""
    from flashdeconv_amd.utils.gene_permutations import gene_permutation_sums
    g = _graph("knn600")
    G = MANY_S + 4
    genes = _genes(G, MANY_S, 5)
    density = 0.3 if route.startswith("csr") else 1.0
    Y, o, null = _reference(("many", density), lambda: gr.exact_case(g.n, G, 17, density), g.A, genes, 8, 1, MANY_R)
    Yc = _route_Y(Y, route)
    kw = dict(genes=genes, seed=8, first_perm=1, n_permutations=MANY_R)
    got = gene_permutation_sums(Yc, g.g, **kw)
    assert (got["tile"], got["route"], got["ways"], got["chunk"], got["batch"]) == (TILE, "lds_table", 4, 10, MANY_R)
    assert got["chunk"] > 2 * got["ways"] and got["chunk"] % got["ways"] != 0
    _assert_equal(got, o, null, (route, "four ways"))
    one = gene_permutation_sums(Yc, g.g, max_batch=1, **kw)
    assert (one["ways"], one["chunk"], one["batch"]) == (1, 1, 1)
    _assert_equal(one, o, null, (route, "one way"))


@pytest.mark.parametrize("route", ["dev_f32", "host_f64", "csr_scipy"])
def test_ways_rounds_and_chunks_move_no_bit(route):
    """Generic (inexact) data in the same shape: four ways in three rounds against one way and one round (max_batch = 1), against
    batches of 7 (four ways, one round, then a batch of 6), against the one-table LDS plan and against the global route (one way,
    one permutation a workgroup) - the same bits."""
    from flashdeconv_amd.utils.gene_permutations import gene_permutation_sums
    g = _graph("knn600")
    n, G = g.n, MANY_S + 4
    genes = _genes(G, MANY_S, 6)
    Yc = _route_Y(_generic_Y(n, G, 12, route), route)
    kw = dict(genes=genes, seed=31, n_permutations=MANY_R, return_null=True)
    first = gene_permutation_sums(Yc, g.g, **kw)
    tile_max, elem = _tile(route), 8 if route == "host_f64" else 4
    chunk = -(-MANY_R // min(-(-MANY_R // 4), -(-2048 // (MANY_S // tile_max))))     # 10 with 64 tiles, 19 with 128
    assert (first["tile"], first["route"], first["ways"], first["chunk"]) == (tile_max, "lds_table", 4, chunk) and chunk > 8
    base = _host(first["null"])
    for label, extra, want in (("one way", dict(max_batch=1), (1, 1)), ("batches of 7", dict(max_batch=7), (4, 4)),
                               ("one table", dict(max_lds_bytes=_lds_need(n, elem, tile_max)), (1, chunk)),
                               ("global", dict(max_lds_bytes=1), (1, 1))):
        other = gene_permutation_sums(Yc, g.g, **dict(kw, **extra))
        assert (other["ways"], other["chunk"]) == want, (label, other["ways"], other["chunk"])
        for name in gr.OBS_PLANES:
            assert np.array_equal(first[name], other[name], equal_nan=True), (label, name)
        assert np.array_equal(base, _host(other["null"])), label


def test_permuted_and_caller_order_graphs_agree_exactly_on_exact_data():
    """The device-built graph (its own spot order) and the same adjacency in the caller's order: the permutation acts on the
    CALLER's spots, so the null is the same - exactly, on an exact case."""
    from flashdeconv_amd.utils.gene_permutations import gene_permutation_sums
    a, b = _graph("knn600"), _graph("untiled600")
    assert (a.A != b.A).nnz == 0
    Y = _route_Y(gr.exact_case(600, 6, 8), "dev_f32")
    x = gene_permutation_sums(Y, a.g, seed=5, n_permutations=5)
    y = gene_permutation_sums(Y, b.g, seed=5, n_permutations=5)
    assert np.array_equal(_host(x["null"]), _host(y["null"])) and np.array_equal(x["P"], y["P"])
    z = gene_permutation_sums(Y, a.A, seed=5, n_permutations=5)              # a scipy adjacency, uploaded for the call
    assert np.array_equal(_host(x["null"]), _host(z["null"]))
    assert not np.array_equal(_host(x["null"]), _host(gene_permutation_sums(Y, a.g, seed=6, n_permutations=5)["null"]))


# ---------------------------------------------------------------- generic cases
@pytest.mark.parametrize("graph,route,S", [("knn600", "host_f32", 9), ("knn600", "csr_scipy", 6), ("hub300", "dev_f64", 5),
                                           ("hub300", "csr_cuda", 4), ("radius", "csr_unsorted", 7), ("radius", "host_f64", 3),
                                           ("untiled600", "dev_strided", 8), ("grid", "dev_f32", 13), ("knn257", "host_int", 5)])
@pytest.mark.parametrize("max_lds_bytes", [None, 1])
def test_generic_sums_meet_the_summation_bound(graph, route, S, max_lds_bytes):
    from flashdeconv_amd.utils.gene_permutations import (OBS_PLANES, assemble_gene_permutation, gene_permutation_sums,
                                                         spatial_gene_permutation_test)
    g = _graph(graph)
    G, R = S + 2, 11
    genes = _genes(G, S, 2)
    if route == "host_int":
        make = lambda: np.floor(gr.generic_case(g.n, G, 3, constant=(1, G - 1)))   # noqa: E731
    else:
        make = lambda: _generic_Y(g.n, G, 3, route)                                 # noqa: E731
    Y, o, null = _reference(("generic", graph, S, route.startswith("csr"), route == "host_int"), make, g.A, genes, 21, 0, R)
    Yc = _route_Y(Y, route)
    got = gene_permutation_sums(Yc, g.g, genes=genes, seed=21, n_permutations=R, max_lds_bytes=max_lds_bytes)
    assert got["route"] == ("global" if max_lds_bytes else "lds_table")
    rtol = 2 * (sparse.csr_matrix(g.A).nnz + g.n) * gr.EPS
    have = _host(got["null"])
    err = np.abs(have - null)
    print(f"{graph} {route} null: worst relative difference {float((err / np.maximum(np.abs(null), 1e-300)).max()):.3e} (bound {rtol:.3e})")
    assert np.all(err <= rtol * np.abs(null))
    for name in ("D", "H", "P", "u", "q"):
        assert np.all(np.abs(got[name] - o[name]) <= rtol * np.abs(o[name])), name
    for name in ("ymin", "ymax"):
        assert np.array_equal(got[name], o[name]), name
    # the statistics are assemble_gene_permutation of the device's own sums, exactly
    out = spatial_gene_permutation_test(Yc, g.g, genes=genes, n_permutations=R, random_state=21, n_top=2)
    want = assemble_gene_permutation(got["n"], got["W"], *(got[name] for name in OBS_PLANES), null=have)
    assert set(out) == set(want) | {"genes", "n", "n_edges", "order", "top"}
    for key, val in want.items():
        assert np.array_equal(np.asarray(out[key]), np.asarray(val), equal_nan=True), key
    assert out["n"] == g.n and out["n_edges"] == g.nnz // 2 and np.array_equal(out["genes"], genes)
    dead = np.isin(genes, [1, G - 1])
    assert np.array_equal(np.isnan(out["p_sim"]), dead) and np.array_equal(np.isnan(out["morans_i"]), dead)
    assert np.array_equal(out["top"], out["order"][:2]) and sorted(out["order"]) == list(range(S))
    live = out["order"][:int((~dead).sum())]
    assert not np.isnan(out["p_sim"][live]).any() and np.all(np.diff(out["p_sim"][live]) >= 0)
    # and close to the reference's statistics
    ref = gr.assemble(o["n"], o["W"], *(o[name] for name in gr.OBS_PLANES), null)
    np.testing.assert_allclose(out["morans_i"][~dead], ref["morans_i"][~dead], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(out["null_mean"][~dead], ref["null_mean"][~dead], rtol=1e-8, atol=1e-11)


# ---------------------------------------------------------------- end to end
def test_planted_gradient_is_significant_and_the_constant_gene_is_nan():
    from flashdeconv_amd.utils.gene_permutations import spatial_gene_permutation_test
    g = _graph("grid")
    R = 199
    for route in ("host_f64", "csr_scipy"):
        out = spatial_gene_permutation_test(_route_Y(gr.planted_case(), route), g.g, n_permutations=R, random_state=0, return_null=True)
        assert out["p_sim"][0] == 1 / (R + 1) and out["p_sim"][1] > 0.2 and np.isnan(out["p_sim"][2])
        assert out["gearys_p_sim"][0] == 1 / (R + 1) and out["z_sim"][0] > 10 and np.isnan(out["z_sim"][2]) and np.isnan(out["q_sim"][2])
        assert list(out["order"]) == [0, 1, 2] and out["n_permutations"] == R and out["null_i"].shape == (R, 3)
        assert out["morans_i"][0] > out["null_i"][:, 0].max() and np.isnan(out["null_i"][:, 2]).all()
    zero = spatial_gene_permutation_test(gr.planted_case(), g.g, n_permutations=0)
    assert np.array_equal(zero["morans_i"], out["morans_i"], equal_nan=True) and np.isnan(zero["p_sim"]).all() and zero["n_permutations"] == 0


def test_the_c_entries_refuse_bad_arguments_and_skip_the_kernels_without_work():
    import torch
    from flashdeconv_amd import _lib
    lib = _lib.load()
    g = _graph("knn65")
    Y = torch.ones((65, 4), dtype=torch.float32, device="cuda")
    obs = torch.full((7, 2), 9.0, dtype=torch.float64, device="cuda")
    null = torch.full((3, 3, 2), 9.0, dtype=torch.float64, device="cuda")
    counts, info = np.zeros(3, dtype=np.int64), np.zeros(6, dtype=np.int64)
    genes = np.array([2, 0], dtype=np.int32)
    h, yp, op, np_, cp, fp = g.g.handle, ctypes.c_void_p(Y.data_ptr()), ctypes.c_void_p(obs.data_ptr()), ctypes.c_void_p(null.data_ptr()), \
        _lib.ptr_i64(counts), _lib.ptr_i64(info)
    ip = _lib.ptr_i32(genes)
    ints = lambda *v: _lib.ptr_i32(np.array(v, dtype=np.int32))                      # noqa: E731
    F = _lib.FDX_F32
    for match, args in (("null argument", (None, yp, F, 65, 4, 4, ip, 2, 0, 0, 3, 0, 0, 0, op, np_, cp, fp, None)),
                        ("null argument", (h, None, F, 65, 4, 4, ip, 2, 0, 0, 3, 0, 0, 0, op, np_, cp, fp, None)),
                        ("null argument", (h, yp, F, 65, 4, 4, None, 2, 0, 0, 3, 0, 0, 0, op, np_, cp, fp, None)),
                        ("null argument", (h, yp, F, 65, 4, 4, ip, 2, 0, 0, 3, 0, 0, 0, None, np_, cp, fp, None)),
                        ("null argument", (h, yp, F, 65, 4, 4, ip, 2, 0, 0, 3, 0, 0, 0, op, None, cp, fp, None)),
                        ("null argument", (h, yp, F, 65, 4, 4, ip, 2, 0, 0, 3, 0, 0, 0, op, np_, None, fp, None)),
                        ("dtype must be", (h, yp, 7, 65, 4, 4, ip, 2, 0, 0, 3, 0, 0, 0, op, np_, cp, fp, None)),
                        ("ldy < G", (h, yp, F, 65, 4, 3, ip, 2, 0, 0, 3, 0, 0, 0, op, np_, cp, fp, None)),
                        ("gene index out of range", (h, yp, F, 65, 4, 4, ints(0, 4), 2, 0, 0, 3, 0, 0, 0, op, np_, cp, fp, None)),
                        ("gene index out of range", (h, yp, F, 65, 4, 4, ints(-1, 2), 2, 0, 0, 3, 0, 0, 0, op, np_, cp, fp, None)),
                        ("gene listed twice", (h, yp, F, 65, 4, 4, ints(3, 3), 2, 0, 0, 3, 0, 0, 0, op, np_, cp, fp, None)),
                        ("S must be at least 1", (h, yp, F, 65, 4, 4, ip, 0, 0, 0, 3, 0, 0, 0, op, np_, cp, fp, None)),
                        ("64 rows but the graph has 65", (h, yp, F, 64, 4, 4, ip, 2, 0, 0, 3, 0, 0, 0, op, np_, cp, fp, None)),
                        ("first_perm must not be negative", (h, yp, F, 65, 4, 4, ip, 2, 0, -1, 3, 0, 0, 0, op, np_, cp, fp, None)),
                        ("n_perm must not be negative", (h, yp, F, 65, 4, 4, ip, 2, 0, 0, -1, 0, 0, 0, op, np_, cp, fp, None)),
                        ("max_batch must not be negative", (h, yp, F, 65, 4, 4, ip, 2, 0, 0, 3, -1, 0, 0, op, np_, cp, fp, None)),
                        ("max_lds_bytes must not be negative", (h, yp, F, 65, 4, 4, ip, 2, 0, 0, 3, 0, -1, 0, op, np_, cp, fp, None)),
                        ("max_gather_bytes must not be negative", (h, yp, F, 65, 4, 4, ip, 2, 0, 0, 3, 0, 0, -1, op, np_, cp, fp, None))):
        with pytest.raises(_lib.FdxError, match=match):
            _lib.check(lib.fdx_gene_spatial_perm_dev(*args))
    with pytest.raises(_lib.FdxError, match="null argument"):
        _lib.check(lib.fdx_gene_spatial_perm_csr_dev(h, None, ip, 2, 0, 0, 3, 0, 0, 0, op, np_, cp, fp, None))
    torch.cuda.synchronize()
    assert np.all(null.cpu().numpy() == 9.0) and np.all(obs.cpu().numpy() == 9.0)          # a refused call wrote nothing
    # n_perm = 0: the observed planes, no null (a null pointer is accepted), no info
    _lib.check(lib.fdx_gene_spatial_perm_dev(h, yp, F, 65, 4, 4, ip, 2, 0, 0, 0, 0, 0, 0, op, None, cp, None, None))
    torch.cuda.synchronize()
    host = obs.cpu().numpy()
    assert np.array_equal(host[0], [65.0, 65.0]) and np.array_equal(host[5:], np.ones((2, 2))) and counts[0] == 65
    assert np.array_equal(host[2], [float(counts[1])] * 2) and np.array_equal(host[4], host[2])      # y = 1: D = P = W
    _lib.check(lib.fdx_gene_spatial_perm_dev(h, yp, F, 65, 4, 4, ip, 2, 0, 0, 0, 0, 0, 0, op, None, cp, fp, None))
    assert info.tolist() == [4, 0, 2, 1, 0, 0]
    _lib.check(lib.fdx_gene_spatial_perm_dev(h, yp, F, 65, 4, 4, ip, 2, 0, 0, 3, 0, 0, 0, op, np_, cp, fp, None))
    assert info.tolist() == [4, 3, 2, 1, 3, 3]                    # one tile: one workgroup walks the three permutations, a way each
    # n = 0: zeros and NaN, nothing launched
    e = _lib.Graph.from_csr(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), 0)
    counts[:] = 9
    _lib.check(lib.fdx_gene_spatial_perm_dev(e.handle, yp, F, 0, 4, 4, ip, 2, 0, 0, 3, 0, 0, 0, op, np_, cp, fp, None))
    torch.cuda.synchronize()
    host = obs.cpu().numpy()
    assert counts.tolist() == [0, 0, 0] and np.all(null.cpu().numpy() == 0) and np.all(host[:5] == 0) and np.isnan(host[5:]).all()
    e.close()


# ---------------------------------------------------------------- surface
def test_model_method_adds_the_permutation_keys_on_request_only():
    from flashdeconv_amd import FlashDeconv
    from flashdeconv_amd.utils.gene_permutations import STAT_KEYS, spatial_gene_permutation_test
    from flashdeconv_amd.utils.spatial_genes import spatially_variable_genes
    gold = load_golden("fit_counts_100x500x5_d64.npz")
    Y, X, coords = gold["Y"], gold["X"], gold["coords"]
    m = FlashDeconv(sketch_dim=64, max_iter=30, random_state=4).fit(Y, X, coords)

    def same(got, want):
        assert set(got) == set(want)
        for key in want:
            assert np.array_equal(np.asarray(got[key]), np.asarray(want[key]), equal_nan=True), key
    today = spatially_variable_genes(Y, m, n_top=3)
    same(m.get_spatially_variable_genes(Y, n_top=3), today)
    same(m.get_spatially_variable_genes(Y, n_top=3, n_permutations=0, random_state=9, permutation_genes=[1, 2]), today)
    for Yc in (Y, sparse.csr_matrix(Y)):
        got = m.get_spatially_variable_genes(Yc, n_top=3, n_permutations=19)
        assert set(got) == set(today) | set(STAT_KEYS) | {"n_permutations"} and got["n_permutations"] == 19
        same({k: got[k] for k in today}, today)
        direct = spatial_gene_permutation_test(Yc, m, n_permutations=19, random_state=4)          # random_state=None: the model's
        for key in STAT_KEYS:
            assert got[key].shape == (500,) and np.array_equal(got[key], direct[key], equal_nan=True), key
        assert np.array_equal(got["morans_i"], direct["morans_i"], equal_nan=True)
    some = np.array([7, 3, 250])
    got = m.get_spatially_variable_genes(Y, n_permutations=19, random_state=8, permutation_genes=some)
    direct = spatial_gene_permutation_test(Y, m, genes=some, n_permutations=19, random_state=8)
    rest = np.setdiff1d(np.arange(500), some)
    for key in STAT_KEYS:
        assert np.array_equal(got[key][some], direct[key], equal_nan=True) and np.isnan(got[key][rest]).all(), key
    assert not np.isnan(got["p_sim"][some]).all()


def test_deconvolve_writes_the_permutation_columns_on_request_only():
    import flashdeconv_amd as fd
    from flashdeconv_amd.io import prepare_data
    case = datagen.anndata_case()
    kw = dict(cell_type_key="celltype", sketch_dim=64, k_neighbors=4, n_hvg=300, n_markers_per_type=20)
    st, ref1 = datagen.anndata_objects(case)
    for bad in (-1, 2.5, True):
        with pytest.raises(ValueError, match="gene_permutations must be an int >= 0"):
            fd.tl.deconvolve(st, ref1, spatial_genes=True, gene_permutations=bad, **kw)
    with pytest.raises(ValueError, match="needs spatial_genes=True"):
        fd.tl.deconvolve(st, ref1, gene_permutations=19, **kw)
    assert "flashdeconv" not in st.obsm and "flashdeconv_params" not in st.uns                  # refused before the fit
    assert fd.tl.deconvolve(st, ref1, spatial_genes=True, gene_permutations=19, **kw) is None
    st0, ref0 = datagen.anndata_objects(case)
    fd.tl.deconvolve(st0, ref0, spatial_genes=True, **kw)
    assert set(st.uns) == set(st0.uns) and set(st.obsm) == set(st0.obsm)
    assert set(st.uns["flashdeconv_params"]) == set(st0.uns["flashdeconv_params"]) | {"gene_permutations"}
    assert st.uns["flashdeconv_params"]["gene_permutations"] == 19
    frame, frame0 = st.uns["flashdeconv_spatial_genes"], st0.uns["flashdeconv_spatial_genes"]
    assert list(frame.columns) == list(frame0.columns) + ["p_sim", "q_sim", "z_sim"] and frame.shape == (470, 11)
    for column in frame0.columns:
        np.testing.assert_array_equal(frame[column].values, frame0[column].values)
    Y, X, coords, names, genes = prepare_data(st, ref1, cell_type_key="celltype")
    m = fd.FlashDeconv(sketch_dim=64, k_neighbors=4, n_hvg=300, n_markers_per_type=20).fit(Y, X, coords)
    want = m.get_spatially_variable_genes(Y, n_permutations=19, random_state=0)
    for column in ("p_sim", "q_sim", "z_sim"):
        np.testing.assert_array_equal(frame[column].values, want[column])
    live = ~np.isnan(want["p_sim"])
    assert live.any() and np.all((want["p_sim"][live] >= 0.05) & (want["p_sim"][live] <= 1)) and np.all(want["q_sim"][live] >= want["p_sim"][live])
