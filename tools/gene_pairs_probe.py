#!/usr/bin/env python3
"""Wall time of utils.gene_pairs - ``gene_pair_sums`` and ``spatial_gene_pairs(local=True, output="torch")`` - for P random pairs,
listed as drawn and listed sorted by (a, b), beside ``gene_spatial_sums`` of all the columns (what one walk over the matrix costs) and
the route torch offers to ONE of the seventeen sums: gather the pairs' distinct columns to float64, ``torch.sparse.mm(A, .)``,
products and column sums for ``Xab``.  Host clock around calls that end in a device synchronise, 2 warm-up calls, the median of 8
(torch: 1 and 4).  Dense float32 and float64 at 1M x 2,000 on the device-built 6-NN graph of a jittered 1,000 x 1,000 lattice with
P = 100 and 1,000; CSR float32 100k x 20,000 (7.2 % stored) with P = 1,000, torch on the densified matrix.  Checks the agreement of
``Xab`` with torch's float64 result as a fraction of the largest entry.  Prints one ``key value`` line per figure and, at the end,
one JSON line of all of them.

usage: gene_pairs_probe.py [--side 1000] [--genes 2000] [--csr-spots 100000] [--csr-genes 20000]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

res = {}


def timed(fn, warm=2, reps=8):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def note(key, val):
    res[key] = val
    print(key, val, flush=True)


def torch_adjacency(g, n):
    import torch
    indptr, indices = g.to_csr_arrays()
    return torch.sparse_csr_tensor(torch.as_tensor(indptr), torch.as_tensor(indices.astype(np.int64)),
                                   torch.ones(indices.size, dtype=torch.float64), size=(n, n)).cuda()


def torch_xab(Y, A, pairs):
    import torch
    genes, inv = np.unique(pairs.ravel(), return_inverse=True)
    inv = torch.as_tensor(inv.reshape(-1, 2)).cuda()
    Yg = Y[:, torch.as_tensor(genes).cuda()].to(torch.float64)
    L = torch.sparse.mm(A, Yg)
    return (Yg[:, inv[:, 0]] * L[:, inv[:, 1]]).sum(0)


def dense_block(dtype, tag, g, A, n, G):
    import torch
    from flashdeconv_amd.utils.gene_pairs import gene_pair_sums, spatial_gene_pairs
    from flashdeconv_amd.utils.spatial_genes import gene_spatial_sums
    Y = torch.empty((n, G), dtype=dtype, device="cuda").log_normal_(0.0, 1.0)
    note(f"{tag} gene_spatial_sums ms", timed(lambda: gene_spatial_sums(Y, g)))
    rs = np.random.RandomState(1)
    for P in (100, 1000):
        pairs = rs.randint(0, G, size=(P, 2))
        by_a = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]
        note(f"{tag} P={P} sums ms", timed(lambda: gene_pair_sums(Y, g, pairs)))
        note(f"{tag} P={P} sums, pairs listed sorted ms", timed(lambda: gene_pair_sums(Y, g, by_a)))
        note(f"{tag} P={P} sums+stats+local ms", timed(lambda: spatial_gene_pairs(Y, g, pairs, local=True, output="torch")))
        note(f"{tag} P={P} sums+stats+local, pairs listed sorted ms",
             timed(lambda: spatial_gene_pairs(Y, g, by_a, local=True, output="torch")))
        note(f"{tag} P={P} torch Xab ms", timed(lambda: torch_xab(Y, A, pairs), warm=1, reps=4))
        want = torch_xab(Y, A, pairs).cpu().numpy()
        got = gene_pair_sums(Y, g, pairs)["Xab"]
        note(f"{tag} P={P} Xab disagreement / largest entry", float(np.abs(got - want).max() / np.abs(want).max()))
    del Y
    torch.cuda.empty_cache()


def main():
    import torch
    from flashdeconv_amd import _lib
    from flashdeconv_amd.utils.gene_pairs import gene_pair_sums, spatial_gene_pairs
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=1000)
    ap.add_argument("--genes", type=int, default=2000)
    ap.add_argument("--csr-spots", type=int, default=100000)
    ap.add_argument("--csr-genes", type=int, default=20000)
    args = ap.parse_args()
    _lib.require_gpu()
    side, n = args.side, args.side * args.side
    yy, xx = np.mgrid[0:side, 0:side]
    coords = np.stack([xx.ravel(), yy.ravel()], 1).astype(np.float64) + np.random.RandomState(0).uniform(-0.3, 0.3, size=(n, 2))
    g = _lib.Graph.from_coords_knn(coords, 6)
    note("graph n, directed edges, max degree", list(g.info()))
    A = torch_adjacency(g, n)
    dense_block(torch.float32, f"f32 {n}x{args.genes}", g, A, n, args.genes)
    dense_block(torch.float64, f"f64 {n}x{args.genes}", g, A, n, args.genes)
    g.close()
    del A
    n, G = args.csr_spots, args.csr_genes
    g = _lib.Graph.from_coords_knn(np.random.RandomState(2).rand(n, 2) * np.sqrt(n), 6)
    A = torch_adjacency(g, n)
    D = torch.empty((n, G), dtype=torch.float32, device="cuda").log_normal_(0.0, 1.0)
    D *= torch.rand((n, G), device="cuda") < 0.072
    Yc = D.to_sparse_csr()
    tag = f"csr f32 {n}x{G}"
    note(f"{tag} stored entries", int(Yc.values().numel()))
    pairs = np.random.RandomState(3).randint(0, G, size=(1000, 2))
    note(f"{tag} P=1000 sums ms", timed(lambda: gene_pair_sums(Yc, g, pairs)))
    note(f"{tag} P=1000 sums+stats+local ms", timed(lambda: spatial_gene_pairs(Yc, g, pairs, local=True, output="torch")))
    note(f"{tag} P=1000 torch Xab on the densified matrix ms", timed(lambda: torch_xab(D, A, pairs), warm=1, reps=4))
    want = torch_xab(D, A, pairs).cpu().numpy()
    got = gene_pair_sums(Yc, g, pairs)["Xab"]
    note(f"{tag} Xab disagreement / largest entry", float(np.abs(got - want).max() / np.abs(want).max()))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
