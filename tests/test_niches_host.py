"""CPU-only tests of the spatial-niches surface (utils.niches): the host half of the k-means++ draw (``pick_row``), the argument
checks that come before anything touches the GPU, and the C entries' declaration, export and binding."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
from scipy import sparse

from conftest import ROOT


def _weights(rs, n):
    """Non-negative weights with runs of zeros; multiples of 2^-20, so every partial sum below is exact whatever its order."""
    d2 = rs.randint(0, 1 << 20, n).astype(np.float64) / (1 << 20)
    for _ in range(max(1, n // 40)):
        a = rs.randint(n)
        d2[a:a + rs.randint(1, 30)] = 0.0
    return d2


@pytest.mark.parametrize("n,R", [(1, 256), (255, 256), (256, 256), (257, 256), (1000, 256), (3000, 512), (5000, 1024)])
def test_pick_row_against_searchsorted(n, R):
    from flashdeconv_amd.utils.niches import pick_row
    rs = np.random.RandomState(n)
    d2 = _weights(rs, n)
    if n == 1:
        d2[0] = 0.5
    nb = -(-n // R)
    if n > R:
        d2[R - 1] = d2[R] = 0.0                                # zeros on both sides of a block edge
    block_sums = np.array([d2[b * R:(b + 1) * R].sum() for b in range(nb)])
    cum = np.cumsum(d2)
    total = cum[-1]
    assert total > 0
    fetched = []

    def fetch_block(b):
        fetched.append(b)
        return b * R, d2[b * R:(b + 1) * R]

    draws = list(rs.random_sample(200) * total)
    draws += [0.0, np.nextafter(total, 0.0)]
    draws += [cum[j] for j in (0, R - 1, R, n - 2) if 0 <= j < n and cum[j] < total]           # exactly on a running sum
    draws += [np.nextafter(cum[j], 0.0) for j in (R - 1, R) if j < n and cum[j] > 0]
    for t in draws:
        del fetched[:]
        row = pick_row(block_sums, fetch_block, t)
        want = int(np.searchsorted(cum, t, side="right"))
        assert row == want and d2[row] > 0, (t, row, want)
        assert fetched == [row // R]                            # one block is read back, the one the draw falls in


def test_pick_row_edges():
    from flashdeconv_amd.utils.niches import pick_row
    d2 = np.array([0.0, 0.25, 0.0, 0.5, 0.0, 0.0, 0.125, 0.0])

    def fetch(b):
        return 4 * b, d2[4 * b:4 * b + 4]

    sums = np.array([0.75, 0.125])
    assert pick_row(sums, fetch, 0.0) == 1 and pick_row(sums, fetch, 0.25) == 3 and pick_row(sums, fetch, 0.75) == 6
    with pytest.raises(ValueError, match="not below the total"):
        pick_row(sums, fetch, 0.875)
    # a block sum that the device rounded up past the block's own running sum: the block's last row of positive weight
    assert pick_row(np.array([0.75, 0.25]), fetch, 0.9) == 6
    # leading blocks without weight are passed over
    assert pick_row(np.array([0.0, 0.125]), lambda b: (4 * b, d2[4:] if b else np.zeros(4)), 0.0) == 6


def test_argument_checks_come_before_the_gpu(monkeypatch):
    from flashdeconv_amd import _lib
    from flashdeconv_amd.utils import niches

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_gpu)
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    rs = np.random.RandomState(0)
    n, K = 6, 3
    V = rs.rand(n, K)
    i = np.arange(n)
    ring = sparse.csr_matrix((np.ones(2 * n), (np.r_[i, i], np.r_[(i + 1) % n, (i - 1) % n])), shape=(n, n))

    for call in (lambda v: niches.kmeans(v, V[:2]), lambda v: niches.kmeans_plusplus(v, 2), lambda v: niches.spatial_niches(v, 2)):
        with pytest.raises(ValueError, match="must be a 2-D"):
            call(V[:, 0])
        with pytest.raises(ValueError, match="must not be empty"):
            call(V[:, :0])
    # kmeans
    with pytest.raises(ValueError, match="init must be a 2-D"):
        niches.kmeans(V, V[0])
    with pytest.raises(ValueError, match="init must have the features' 3 columns"):
        niches.kmeans(V, V[:2, :2])
    with pytest.raises(ValueError, match="must not exceed the number of spots"):
        niches.kmeans(V, rs.rand(n + 1, K))
    with pytest.raises(ValueError, match="between 1 and 64"):
        niches.kmeans(rs.rand(100, K), rs.rand(65, K))
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="max_iter must be a positive integer"):
            niches.kmeans(V, V[:2], max_iter=bad)
    # kmeans_plusplus and spatial_niches: the number of niches
    for fn in (niches.kmeans_plusplus, niches.spatial_niches):
        with pytest.raises(ValueError, match="between 1 and 64"):
            fn(V, 0)
        with pytest.raises(ValueError, match="between 1 and 64"):
            fn(rs.rand(100, K), 65)
        with pytest.raises(ValueError, match="must not exceed the number of spots"):
            fn(V, n + 1)
        with pytest.raises(ValueError, match="n_niches must be an integer"):
            fn(V, 2.0)
    with pytest.raises(ValueError, match="cannot be used to seed"):
        niches.kmeans_plusplus(V, 2, random_state="x")
    # spatial_niches
    with pytest.raises(ValueError, match="Unknown features"):
        niches.spatial_niches(V, 2, features="nope")
    for mode in ("neighborhood", "both"):
        with pytest.raises(ValueError, match="needs a graph"):
            niches.spatial_niches(V, 2, features=mode)
    with pytest.raises(ValueError, match="neighbor_weight must be finite"):
        niches.spatial_niches(V, 2, ring, features="both", neighbor_weight=np.inf)
    with pytest.raises(ValueError, match="Unknown init"):
        niches.spatial_niches(V, 2, init="random")
    with pytest.raises(ValueError, match="init must hold n_niches = 2 centres"):
        niches.spatial_niches(V, 2, init=V[:3])
    with pytest.raises(ValueError, match="init must have the features' 6 columns"):
        niches.spatial_niches(V, 2, ring, features="both", init=V[:2])
    with pytest.raises(ValueError, match="max_iter must be a positive integer"):
        niches.spatial_niches(V, 2, max_iter=0)
    with pytest.raises(ValueError, match="cannot be used to seed"):
        niches.spatial_niches(V, 2, random_state="x")
    # the graph's own checks (_device.resolve_graph) are host-side too
    with pytest.raises(ValueError, match="5 rows but the graph has 6 spots"):
        niches.spatial_niches(V[:5], 2, ring, features="both")
    asym = ring.tolil()
    asym[0, 3] = 1.0
    with pytest.raises(ValueError, match="must be symmetric"):
        niches.spatial_niches(V, 2, asym.tocsr(), features="neighborhood")
    with pytest.raises(TypeError, match="graph must be"):
        niches.spatial_niches(V, 2, np.eye(n), features="neighborhood")


def test_model_method_needs_a_fit():
    from flashdeconv_amd import FlashDeconv
    m = FlashDeconv()
    for kw in ({}, {"what": "abundances"}, {"features": "composition"}, {"what": "nope"}):
        with pytest.raises(RuntimeError, match=r"Model has not been fitted\. Call fit\(\) first\."):
            m.get_spatial_niches(3, **kw)


def test_entries_are_declared_exported_and_bound():
    from flashdeconv_amd import _lib, tl, utils
    text = open(os.path.join(ROOT, "include", "fdx.h")).read()
    lib = _lib.load()
    for name, n_args in (("fdx_kmeans_assign_dev", 11), ("fdx_label_sums_dev", 9), ("fdx_kmeans_seed_dist_dev", 10),
                         ("fdx_kmeans_dev", 13)):
        decl = re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert decl is not None, name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(decl.group(1).split(",")) == n_args, name
        assert args[1] is ctypes.c_int64 and args[2] is ctypes.c_int64 and args[3] is ctypes.c_int32, name     # ldf, n, D
        assert callable(getattr(lib, name))
    for name in ("spatial_niches", "kmeans", "kmeans_plusplus"):
        assert name in utils.__all__ and callable(getattr(utils, name))
    assert inspect.signature(tl.deconvolve).parameters["n_niches"].default is None
    sig = inspect.signature(utils.spatial_niches).parameters
    assert list(sig) == ["values", "n_niches", "graph", "features", "neighbor_weight", "init", "max_iter", "random_state"]
    assert sig["max_iter"].default == 100 and sig["random_state"].default == 0 and sig["init"].default == "k-means++"
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("fdx_kmeans_assign_dev", "fdx_label_sums_dev", "fdx_kmeans_seed_dist_dev", "fdx_kmeans_dev"):
        assert name + "(" in guide, name
