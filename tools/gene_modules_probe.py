#!/usr/bin/env python3
"""Wall time of utils.gene_modules - ``gene_coexpression_sums`` and the whole ``spatial_gene_modules(genes=..., output="torch")``
call - for S random genes, beside the two other routes to the same matrices: ``gene_pair_sums`` on all S (S + 1) / 2 pairs (S = 256
only) and the torch float64 composition ``Yg = Y[:, genes].double(); L = torch.sparse.mm(A, Yg); X = Yg.T @ L; Sm = Yg.T @ Yg``
(time and peak extra memory).  Host clock around calls that end in a device synchronise, 2 warm-up calls, the median of 8 (the pair
entry and torch: 1 and 3).  Dense float32 and float64 at 1M x 2,000 on the device-built 6-NN graph of a jittered 1,000 x 1,000
lattice with S = 256 and 1,024; CSR float32 100k x 20,000 (7.2 % stored) with S = 512.  Checks the agreement of ``X`` with torch's
float64 result as a fraction of the largest entry.  Prints one ``key value`` line per figure and, at the end, one JSON line of all
of them.  ``--stage S`` instead runs ``gene_coexpression_sums`` on the float32 matrix three times and nothing else: the run to put
under a kernel trace for the share of each kernel.

usage: gene_modules_probe.py [--side 1000] [--genes 2000] [--csr-spots 100000] [--csr-genes 20000] [--stage S]"""
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


def torch_matrices(Y, A, genes):
    import torch
    Yg = Y[:, torch.as_tensor(genes).cuda()].to(torch.float64)
    L = torch.sparse.mm(A, Yg)
    return Yg.T @ L, Yg.T @ Yg


def compare(tag, Y, Yt, g, A, S, rs, with_pairs):
    """One S on one matrix: Y as the entries take it, Yt the dense CUDA tensor torch indexes."""
    import torch
    from flashdeconv_amd.utils.gene_modules import gene_coexpression_sums, spatial_gene_modules
    from flashdeconv_amd.utils.gene_pairs import gene_pair_sums
    n = Yt.shape[0]
    genes = rs.permutation(Yt.shape[1])[:S]
    ms = timed(lambda: gene_coexpression_sums(Y, g, genes))
    note(f"{tag} S={S} sums ms", ms)
    note(f"{tag} S={S} sums TFLOP/s of 2*2*n*S^2 over the whole call", 4.0 * n * S * S / (ms * 1e-3) / 1e12)
    note(f"{tag} S={S} modules (sums+stats+clustering+scores) ms", timed(lambda: spatial_gene_modules(Y, g, genes=genes, output="torch")))
    if with_pairs:
        ia, ib = np.triu_indices(S)
        pairs = np.stack([genes[ia], genes[ib]], axis=1)
        note(f"{tag} S={S} gene_pair_sums on all {pairs.shape[0]} pairs ms", timed(lambda: gene_pair_sums(Y, g, pairs), warm=1, reps=3))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    note(f"{tag} S={S} torch float64 composition ms", timed(lambda: torch_matrices(Yt, A, genes), warm=1, reps=3))
    note(f"{tag} S={S} torch peak extra memory MB", (torch.cuda.max_memory_allocated() - before) / 2 ** 20)
    want = torch_matrices(Yt, A, genes)[0].cpu().numpy()
    got = gene_coexpression_sums(Y, g, genes)["X"]
    note(f"{tag} S={S} X disagreement / largest entry", float(np.abs(got - want).max() / np.abs(want).max()))


def main():
    import torch
    from flashdeconv_amd import _lib
    from flashdeconv_amd.utils.gene_modules import gene_coexpression_sums
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=1000)
    ap.add_argument("--genes", type=int, default=2000)
    ap.add_argument("--csr-spots", type=int, default=100000)
    ap.add_argument("--csr-genes", type=int, default=20000)
    ap.add_argument("--stage", type=int, default=0)
    args = ap.parse_args()
    _lib.require_gpu()
    side, n = args.side, args.side * args.side
    yy, xx = np.mgrid[0:side, 0:side]
    coords = np.stack([xx.ravel(), yy.ravel()], 1).astype(np.float64) + np.random.RandomState(0).uniform(-0.3, 0.3, size=(n, 2))
    g = _lib.Graph.from_coords_knn(coords, 6)
    note("graph n, directed edges, max degree", list(g.info()))
    rs = np.random.RandomState(1)
    if args.stage:
        Y = torch.empty((n, args.genes), dtype=torch.float32, device="cuda").log_normal_(0.0, 1.0)
        genes = rs.permutation(args.genes)[:args.stage]
        for _ in range(3):
            gene_coexpression_sums(Y, g, genes)
        torch.cuda.synchronize()
        return
    A = torch_adjacency(g, n)
    for dtype, name in ((torch.float32, "f32"), (torch.float64, "f64")):
        Y = torch.empty((n, args.genes), dtype=dtype, device="cuda").log_normal_(0.0, 1.0)
        for S in (256, 1024):
            compare(f"{name} {n}x{args.genes}", Y, Y, g, A, min(S, args.genes), rs, with_pairs=S == 256)
        del Y
        torch.cuda.empty_cache()
    g.close()
    del A
    n, G = args.csr_spots, args.csr_genes
    g = _lib.Graph.from_coords_knn(np.random.RandomState(2).rand(n, 2) * np.sqrt(n), 6)
    A = torch_adjacency(g, n)
    D = torch.empty((n, G), dtype=torch.float32, device="cuda").log_normal_(0.0, 1.0)
    D *= torch.rand((n, G), device="cuda") < 0.072
    Yc = D.to_sparse_csr()
    note(f"csr f32 {n}x{G} stored entries", int(Yc.values().numel()))
    compare(f"csr f32 {n}x{G}", Yc, D, g, A, min(512, G), rs, with_pairs=False)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
