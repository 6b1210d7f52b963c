#!/usr/bin/env python3
"""Everything the C ABI can read back of the graphs of a fixed list of cases, in one .npz: for comparing two builds of the library
bit for bit (run once per build, then `graph_dump.py --compare a.npz b.npz`).

Cases: 2-D uniform n = 257 / 1000 / 20000 (k = 6), 1-D n = 3000 (k = 4), 3-D n = 9000 (k = 6), 8-D n = 5000 (k = 12), a shuffled
70 x 70 lattice (k = 6), radius graphs on the 2-D sets.  Every k-NN case is built whole (default, FDX_GRAPH_SYNC=1, FDX_GRAPH_WCAP=1,
FDX_GRAPH_TWO_ELL_KERNELS=1) and, for W = 3 and 5 ranks, by the four shard routes of tests/test_gpu_sharded.py (replicated, sharded,
band, pipeline; pipeline once more with FDX_GRAPH_WCAP=1).  A call the library refuses (the queued pipeline takes 1-3 coordinates) is
recorded by its return code."""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("FDX_GRAPH_SYNC", "FDX_GRAPH_WCAP", "FDX_GRAPH_WCAP_RANK", "FDX_GRAPH_TWO_ELL_KERNELS")


def cases():
    rs = np.random.RandomState(5)
    out = []
    for n in (257, 1000, 20000):
        out.append((f"u2_{n}", rs.rand(n, 2) * np.sqrt(n), 6))
    out.append(("u1_3000", rs.rand(3000, 1) * 3000.0, 4))
    out.append(("u3_9000", rs.rand(9000, 3) * 9000 ** (1 / 3), 6))
    out.append(("u8_5000", rs.rand(5000, 8), 12))
    gx, gy = np.meshgrid(np.arange(70.0), np.arange(70.0))
    lat = np.stack([gx.ravel(), gy.ravel()], 1)
    out.append(("lattice70", np.ascontiguousarray(lat[rs.permutation(len(lat))]), 6))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.compare:
        a, b = (np.load(p) for p in args.compare)
        bad = [k for k in sorted(set(a.files) | set(b.files)) if k not in a.files or k not in b.files or not np.array_equal(a[k], b[k])]
        print(f"{len(a.files)} / {len(b.files)} arrays, {len(bad)} differ" + (": " + ", ".join(bad[:20]) if bad else ""))
        return 1 if bad or not a.files else 0

    sys.path.insert(0, ROOT)
    import torch
    from flashdeconv_amd import _lib
    from flashdeconv_amd.distributed import shard_bounds
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731
    dump = {}

    def switches(env):
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)
        _lib.env_reload()

    def whole(tag, g, lo=0, hi=None):
        # [lo, hi): the rows the graph was built for - a band shard lays its order out only where it looks, the rest of perm is not data
        n, nnz, md = g.info()
        indptr, indices = g.to_csr_arrays()
        perm = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        _lib.check(lib.fdx_graph_perm_dev(g.handle, ctypes.c_void_p(perm.data_ptr()), st()))
        torch.cuda.synchronize()
        dump[tag + "/info"] = np.array([n, nnz, md, g.knn_ties(), g.knn_far()], dtype=np.int64)
        dump[tag + "/indptr"], dump[tag + "/indices"], dump[tag + "/perm"] = indptr, indices, perm.cpu().numpy()[lo:n if hi is None else hi]

    def local(tag, g, n_own, W):
        nnz, ties, far, over = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_int32(0)
        rc_status = lib.fdx_graph_shard_status(g.handle, ctypes.byref(nnz), ctypes.byref(ties), ctypes.byref(far), ctypes.byref(over))
        dump[tag + "/status"] = np.array([rc_status, nnz.value, ties.value, far.value, over.value], dtype=np.int64)
        if over.value:                      # a bound of the queued pipeline was too small: the caller rebuilds, the arrays are not data
            return
        perm = torch.empty(max(n_own, 1), dtype=torch.int32, device=dev)
        _lib.check(lib.fdx_graph_perm_dev(g.handle, ctypes.c_void_p(perm.data_ptr()), st()))
        nh = ctypes.c_int64(0)
        sc, rc = np.zeros(W, dtype=np.int32), np.zeros(W, dtype=np.int32)
        _lib.check(lib.fdx_graph_halo_info(g.handle, ctypes.byref(nh), _lib.ptr_i32(sc), _lib.ptr_i32(rc)))
        sidx = torch.empty(max(int(sc.sum()), 1), dtype=torch.int32, device=dev)
        _lib.check(lib.fdx_graph_send_indices_dev(g.handle, ctypes.c_void_p(sidx.data_ptr()), st()))
        torch.cuda.synchronize()
        _, nnz_i, md = g.info()
        dump[tag + "/info"] = np.array([n_own, nnz_i, md, nh.value], dtype=np.int64)
        dump[tag + "/perm"], dump[tag + "/send_counts"], dump[tag + "/recv_counts"] = perm.cpu().numpy()[:n_own], sc, rc
        dump[tag + "/send_idx"] = sidx.cpu().numpy()[:int(sc.sum())]
        buf, deg = np.zeros(max(md, 1), dtype=np.int32), ctypes.c_int32(0)
        degs, rows = np.zeros(n_own, dtype=np.int32), []
        for r in range(n_own):
            _lib.check(lib.fdx_graph_row_indices(g.handle, r, _lib.ptr_i32(buf), len(buf), ctypes.byref(deg)))
            degs[r] = deg.value
            rows.append(buf[:deg.value].copy())
        dump[tag + "/deg"] = degs
        dump[tag + "/rows"] = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int32)

    def shard_route(tag, cd, n, dim, k, W, route):
        """The local graphs of all W ranks by one route; a refused call leaves its return code instead."""
        bounds = shard_bounds(n, W)
        kk = min(k, n - 1) + 1
        fulls = None
        if route == "replicated":
            h = ctypes.c_void_p()
            _lib.check(lib.fdx_graph_build_dev(ctypes.c_void_p(cd.data_ptr()), n, dim, _lib.GRAPH_KNN, k, 0.0, st(), ctypes.byref(h)))
            fulls = [_lib.Graph(h.value)] * W
        elif route in ("sharded", "band"):
            lists = lib.fdx_graph_knn_lists_band_dev if route == "band" else lib.fdx_graph_knn_lists_dev
            nbrs = [torch.full((n, kk), -7, dtype=torch.int32, device=dev) for _ in range(W)]
            cnts = [torch.full((n,), -7, dtype=torch.int32, device=dev) for _ in range(W)]
            plans = []
            for r in range(W):
                pl = ctypes.c_void_p()
                _lib.check(lists(ctypes.c_void_p(cd.data_ptr()), n, dim, k, int(bounds[r]), int(bounds[r + 1]),
                                 ctypes.c_void_p(nbrs[r].data_ptr()), ctypes.c_void_p(cnts[r].data_ptr()), st(), ctypes.byref(pl)))
                plans.append(pl)
            if route == "sharded":
                for r in range(W):
                    for q in range(W):
                        if q != r:
                            a, b = int(bounds[q]), int(bounds[q + 1])
                            nbrs[r][a:b], cnts[r][a:b] = nbrs[q][a:b], cnts[q][a:b]
            fulls = []
            for r in range(W):
                h = ctypes.c_void_p()
                _lib.check(lib.fdx_graph_from_knn_lists_dev(plans[r], ctypes.c_void_p(nbrs[r].data_ptr()), ctypes.c_void_p(cnts[r].data_ptr()),
                                                            int(bounds[r]), int(bounds[r + 1]), st(), ctypes.byref(h)))
                fulls.append(_lib.Graph(h.value))
                whole(f"{tag}/full{r}", fulls[-1], int(bounds[r]), int(bounds[r + 1]))
        for r in range(W):
            hl = ctypes.c_void_p()
            if fulls is None:
                rc = lib.fdx_graph_shard_knn_dev(ctypes.c_void_p(cd.data_ptr()), n, dim, k, W, _lib.ptr_i64(bounds), r, st(), ctypes.byref(hl))
            else:
                rc = lib.fdx_graph_localize(fulls[r].handle, W, _lib.ptr_i64(bounds), r, st(), ctypes.byref(hl))
            dump[f"{tag}/rank{r}/rc"] = np.array([rc], dtype=np.int64)
            if rc == 0:
                local(f"{tag}/rank{r}", _lib.Graph(hl.value), int(bounds[r + 1] - bounds[r]), W)

    for name, coords, k in cases():
        n, dim = coords.shape
        for env in ({}, {"FDX_GRAPH_SYNC": "1"}, {"FDX_GRAPH_WCAP": "1"}, {"FDX_GRAPH_TWO_ELL_KERNELS": "1"}):
            switches(env)
            whole(f"{name}/knn/" + ("+".join(env) or "default"), _lib.Graph.from_coords_knn(coords, k))
        switches({})
        if dim == 2:
            for radius in (1.1, 2.0):
                whole(f"{name}/radius{radius}", _lib.Graph.from_coords_radius(coords, radius))
        cd = torch.from_numpy(np.ascontiguousarray(coords)).to(dev)
        for W in (3, 5):
            for route in ("replicated", "sharded", "band", "pipeline"):
                shard_route(f"{name}/W{W}/{route}", cd, n, dim, k, W, route)
            switches({"FDX_GRAPH_WCAP": "1"})
            shard_route(f"{name}/W{W}/pipeline+FDX_GRAPH_WCAP", cd, n, dim, k, W, "pipeline")
            switches({})
        print(f"{name}: {len(dump)} arrays so far", flush=True)
    np.savez_compressed(args.out, **dump)
    print(f"wrote {args.out}: {len(dump)} arrays")
    return 0


if __name__ == "__main__":
    sys.exit(main())
