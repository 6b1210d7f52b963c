#!/usr/bin/env python3
"""Wall time of utils.group_genes - ``gene_group_sums`` and the whole ``rank_genes_groups`` call - on a mostly-zero spot-by-gene matrix
(Poisson counts kept with probability ``--density``) with C random groups, beside scipy on a slice of it: ``rankdata`` per gene
column (the ranking alone) and ``mannwhitneyu`` + ``ttest_ind`` per group and gene (what ``rank_genes_groups`` replaces), both scaled
to all genes.  Host clock around calls that end in a device synchronise, 2 warm-up calls, the median of 8.  Dense float32, dense
float64 and CSR float32 on the device.  Reports the stripes and the ranking workspace of each call, and the memory the library's pool
took from the driver over the float32 call.  Prints one ``key value`` line per figure and, at the end, one JSON line of all of them.
``--stage`` instead runs ``gene_group_sums`` on the float32 matrix three times and nothing else: the run to put under a kernel trace.

usage: group_genes_probe.py [--spots 100000] [--genes 2000] [--groups 10] [--density 0.1] [--slice 8] [--stage]"""
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


def main():
    import torch
    from scipy import stats
    from flashdeconv_amd import _lib
    from flashdeconv_amd.utils.group_genes import gene_group_sums, rank_genes_groups
    ap = argparse.ArgumentParser()
    ap.add_argument("--spots", type=int, default=100000)
    ap.add_argument("--genes", type=int, default=2000)
    ap.add_argument("--groups", type=int, default=10)
    ap.add_argument("--density", type=float, default=0.1)
    ap.add_argument("--slice", type=int, default=8)
    ap.add_argument("--stage", action="store_true")
    args = ap.parse_args()
    _lib.require_gpu()
    n, G, C = args.spots, args.genes, args.groups
    torch.manual_seed(0)
    Y = torch.poisson(torch.full((n, G), 3.0, device="cuda")) * (torch.rand((n, G), device="cuda") < args.density)
    labels = torch.randint(0, C, (n,), device="cuda")
    if args.stage:
        for _ in range(3):
            gene_group_sums(Y, labels, n_groups=C)
        torch.cuda.synchronize()
        return
    note("share of zeros", float((Y == 0).double().mean().item()))
    tag = f"{n}x{G} C={C}"
    free0 = torch.cuda.mem_get_info()[0]
    s = gene_group_sums(Y, labels, n_groups=C)
    torch.cuda.synchronize()
    note(f"f32 {tag} memory taken from the driver over the first call MB", (free0 - torch.cuda.mem_get_info()[0]) / 2 ** 20)
    for name, M in (("f32", Y), ("f64", Y.double()), ("csr f32", Y.to_sparse_csr())):
        s = gene_group_sums(M, labels, n_groups=C)
        note(f"{name} {tag} stripes, entries, ranking workspace MB", [s["stripes"], s["stripe_entries"], s["workspace_bytes"] / 2 ** 20])
        note(f"{name} {tag} gene_group_sums ms", timed(lambda: gene_group_sums(M, labels, n_groups=C)))
        note(f"{name} {tag} rank_genes_groups ms", timed(lambda: rank_genes_groups(M, labels, n_groups=C)))
        del M
    small = gene_group_sums(Y, labels, n_groups=C, max_sort_bytes=64 << 20)
    note(f"f32 {tag} 64 MiB budget: stripes, entries, ranking workspace MB",
         [small["stripes"], small["stripe_entries"], small["workspace_bytes"] / 2 ** 20])
    note(f"f32 {tag} 64 MiB budget gene_group_sums ms", timed(lambda: gene_group_sums(Y, labels, n_groups=C, max_sort_bytes=64 << 20)))
    # scipy on a slice of the genes, scaled to all of them
    k = min(args.slice, G)
    Yh, lab = Y[:, :k].cpu().numpy().astype(np.float64), labels.cpu().numpy()
    t0 = time.perf_counter()
    ranks = [stats.rankdata(Yh[:, j], method="average") for j in range(k)]
    note(f"scipy rankdata, {k} genes scaled to {G}, s", (time.perf_counter() - t0) * G / k)
    twice = np.rint(2 * np.stack(ranks, axis=1)).astype(np.int64)
    want = np.stack([twice[lab == c].sum(axis=0) for c in range(C)])
    note("R2 of the slice equals scipy's", bool(np.array_equal(want, s["R2"][:, :k])))
    t0 = time.perf_counter()
    for c in range(C):
        x, y = Yh[lab == c], Yh[lab != c]
        for j in range(k):
            stats.mannwhitneyu(x[:, j], y[:, j], method="asymptotic", use_continuity=False)
            stats.ttest_ind(x[:, j], y[:, j], equal_var=False)
    note(f"scipy mannwhitneyu + ttest_ind, {C} groups x {k} genes scaled to {G}, s", (time.perf_counter() - t0) * G / k)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
