"""Device graphs of the per-element GPU tests (tests/test_gpu_fit_tail.py, tests/test_gpu_sweep.py) and their upload helper.

Every graph comes with its truth - the oracle's adjacency of the same coordinates (or the CSR handed in), never the device graph's
own export -, the graph's own spot order (perm[p] = caller's id at solver position p) and what fdx_graph_tile_info says about the
traversal it takes.  Built once per process and shared.
"""
import ctypes

import numpy as np
from scipy import sparse

import fdx_oracle as orc
import fit_tail_ref as ref


class _G:
    def __init__(self, g, A, perm, n):
        self.g, self.A, self.perm, self.n = g, sparse.csr_matrix(A), perm, n
        self.tile = g.tile_info()
        _, self.nnz, self.max_deg = g.info()
        assert self.nnz == self.A.nnz, ("the device graph and the oracle's adjacency differ", self.nnz, self.A.nnz)


_cache = {}


def _device_graph(coords, method, k=6, radius=0.0):
    import torch
    from flashdeconv_amd import _lib
    coords = np.ascontiguousarray(coords, dtype=np.float64)
    n = coords.shape[0]
    cd = torch.as_tensor(coords, device="cuda:0")
    h = ctypes.c_void_p()
    _lib.check(_lib.load().fdx_graph_build_dev(ctypes.c_void_p(cd.data_ptr()), n, coords.shape[1], method, int(k), float(radius), None,
                                               ctypes.byref(h)))
    g = _lib.Graph(h.value)
    g.info()
    torch.cuda.synchronize()
    perm_d = torch.empty(n, dtype=torch.int32, device="cuda:0")
    _lib.check(_lib.load().fdx_graph_perm_dev(g.handle, ctypes.c_void_p(perm_d.data_ptr()), None))
    torch.cuda.synchronize()
    return g, perm_d.cpu().numpy().astype(np.int64)


def _knn(n, k=6, dim=2, seed=11):
    """Device-built k-NN graph on tie-free coordinates; truth: the oracle's cKDTree graph.  n = 1: no k-NN build (it needs two
    spots) - the empty graph from CSR."""
    key = ("knn", n, k, dim, seed)
    if key not in _cache:
        from flashdeconv_amd import _lib
        if n == 1:
            _cache[key] = _csr(sparse.csr_matrix((1, 1)), key)
        else:
            coords = ref.tie_free_coords(n, dim, seed)
            g, perm = _device_graph(coords, _lib.GRAPH_KNN, k)
            assert g.knn_ties() == 0
            _cache[key] = _G(g, orc.knn_graph_kdtree(coords, k), perm, n)
    return _cache[key]


def _csr(A, key):
    """A graph from the host CSR: the caller's order, no tile tables."""
    if key not in _cache or _cache[key] is None:
        from flashdeconv_amd import _lib
        A = sparse.csr_matrix(A)
        A.sort_indices()
        n = A.shape[0]
        G = _G(_lib.Graph.from_csr(A.indptr, A.indices, n), A, None, n)
        assert G.tile[2] is False and G.tile[0] == 0
        _cache[key] = G
    return _cache[key]


def _knn_untiled(n, k=6, seed=11):
    """The oracle's k-NN adjacency of the same coordinates as _knn, handed in as CSR."""
    key = ("csr_knn", n, k, seed)
    if key in _cache:
        return _cache[key]
    return _csr(orc.knn_graph_kdtree(ref.tie_free_coords(n, 2, seed), k) if n > 1 else sparse.csr_matrix((1, 1)), key)


def _hub(n):
    return _csr(ref.hub_and_spoke(n), ("hub", n))


def _radius_isolated():
    """A radius graph over a dense patch and 200 spots far from everything: degree 0, and whole slices of width 0."""
    key = ("radius",)
    if key not in _cache:
        from flashdeconv_amd import _lib
        rs = np.random.RandomState(5)
        dense = rs.rand(400, 2) * 20.0
        far = np.stack([200.0 + 10.0 * (np.arange(200) % 15) + rs.rand(200), 200.0 + 10.0 * (np.arange(200) // 15) + rs.rand(200)], 1)
        coords = np.concatenate([dense, far])[rs.permutation(600)]
        g, perm = _device_graph(coords, _lib.GRAPH_RADIUS, radius=1.6)
        _cache[key] = _G(g, orc.radius_graph(coords, 1.6), perm, 600)
    return _cache[key]


def _grid():
    key = ("grid",)
    if key not in _cache:
        from flashdeconv_amd import _lib
        yy, xx = np.mgrid[0:25, 0:24]
        coords = np.stack([xx.ravel(), yy.ravel()], 1).astype(np.float64)
        g, perm = _device_graph(coords, _lib.GRAPH_RADIUS, radius=1.5)      # what method="grid" builds: 1.5 x the lattice spacing
        _cache[key] = _G(g, orc.grid_graph(coords), perm, 600)
    return _cache[key]


def _assert_tiled(G, min_halo=None):
    n_tiles, halo_max, tiled = G.tile
    assert tiled and n_tiles == (G.n + 255) // 256, ("this graph was meant to take the tiled traversal", G.tile)
    assert 8 * (256 + halo_max + 1) * 8 <= 64 * 1024, ("the halo does not fit the tiled kernel's LDS", G.tile)
    if min_halo is not None:
        assert halo_max > min_halo, G.tile
    if G.n > 2:
        assert G.perm is not None and not np.array_equal(G.perm, np.arange(G.n)), "Morton order is the identity: nothing permuted"


def _assert_untiled(G):
    assert G.tile == (0, 0, False), ("this graph was meant to take the generic kernel", G.tile)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
