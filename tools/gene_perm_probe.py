#!/usr/bin/env python3
"""Wall time of utils.gene_permutations - ``gene_permutation_sums`` (the device half: gather, tables, the null kernel, the null
copied to the host and counted) - on a grid of spots with its 8-neighbour graph and a mostly-zero float32 spot-by-gene matrix
(Poisson counts kept with probability ``--density``):
  (a) ``--spots-lds`` x ``--genes``, R = ``--perms-lds``, every gene: the LDS route (columns and table in LDS);
  (b) ``--spots-global`` x ``--genes``, R = ``--perms-global``: the global route (columns and table through L2);
  (a') case (a) forced onto the global route (``max_lds_bytes=1``).
Beside (a): ``spatial_permutation_test`` on blocks of 256 of the same columns - the only way to these numbers before this module -
timed on ``--blocks`` blocks and scaled to all genes; and one permutation as a torch composition (``V = Y[pi]``, ``sparse.mm(A, V)``,
three column sums in float64) scaled to R.  "The C entry alone" leaves the null on the device: no copy to the host, no
counting.  Host clock around calls that end in a device synchronise, 2 warm-up calls, the median of 8 (1 and 3 for the slower
comparisons).  Reports the achieved gather rate: R * S * (n + nnz(A)) values of 4 bytes per second.  Prints one ``key value`` line per
figure and, at the end, one JSON line of all of them.  ``--stage`` instead runs case (a) three times and nothing else: the run to
put under a kernel trace.

usage: gene_perm_probe.py [--spots-lds 5000] [--spots-global 100000] [--genes 2000] [--perms-lds 999] [--perms-global 99]
                          [--density 0.1] [--blocks 1] [--stage]"""
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


def device_ms(Y, g, R, max_lds=0, reps=8):
    """The C entry alone (gather, tables, observed and null sums left on the device), all genes: ms, median of ``reps``."""
    import torch
    from flashdeconv_amd import _lib
    from flashdeconv_amd.utils import gene_permutations as gp
    from flashdeconv_amd.utils._device import matrix_on_device
    n, G = Y.shape
    genes = np.arange(G, dtype=np.int32)
    lib, stream = _lib.load(), _lib.current_stream(Y.device)
    obs = torch.empty((7, G), dtype=torch.float64, device=Y.device)
    null = torch.empty((R, 3, G), dtype=torch.float64, device=Y.device)
    with matrix_on_device(Y, Y.device) as m:
        return timed(lambda: gp._one_call(lib, g, m, n, G, genes, 0, 0, R, 0, max_lds, 0, obs, null, stream), warm=1, reps=reps)


def grid_case(n, G, density, seed):
    """(Y float32 CUDA (n, G), graph, scipy adjacency): spots on a near-square lattice, the 8-neighbour graph the model builds."""
    import torch
    from flashdeconv_amd import _lib
    from flashdeconv_amd.utils.graph import coords_to_adjacency
    cols = int(np.ceil(np.sqrt(n)))
    i = np.arange(n)
    coords = np.stack([i % cols, i // cols], 1).astype(np.float64)
    A = coords_to_adjacency(coords, method="radius", radius=1.5).tocsr()
    A.sort_indices()
    g = _lib.Graph.from_csr(A.indptr.astype(np.int64), A.indices.astype(np.int32), n)
    torch.manual_seed(seed)
    Y = (torch.poisson(torch.full((n, G), 3.0, device="cuda")) * (torch.rand((n, G), device="cuda") < density)).float()
    return Y, g, A


def main():
    import torch
    from flashdeconv_amd import _lib
    from flashdeconv_amd.utils.gene_permutations import gene_permutation_sums
    from flashdeconv_amd.utils.spatial_stats import permutation_indices, spatial_permutation_test
    ap = argparse.ArgumentParser()
    ap.add_argument("--spots-lds", type=int, default=5000)
    ap.add_argument("--spots-global", type=int, default=100000)
    ap.add_argument("--genes", type=int, default=2000)
    ap.add_argument("--perms-lds", type=int, default=999)
    ap.add_argument("--perms-global", type=int, default=99)
    ap.add_argument("--density", type=float, default=0.1)
    ap.add_argument("--blocks", type=int, default=1)
    ap.add_argument("--stage", action="store_true")
    args = ap.parse_args()
    _lib.require_gpu()
    G = args.genes
    n, R = args.spots_lds, args.perms_lds
    Y, g, A = grid_case(n, G, args.density, 0)
    if args.stage:
        for _ in range(3):
            gene_permutation_sums(Y, g, n_permutations=R, return_null=False)
        torch.cuda.synchronize()
        return

    def rate(ms, n, nnz, R):
        return R * G * (n + nnz) * 4.0 / (ms * 1e-3) / 1e12

    s = gene_permutation_sums(Y, g, n_permutations=R, return_null=False)
    tag = f"(a) {n}x{G} R={R}"
    note(f"{tag} tile, route, batch, stripes, ways, chunk", [s["tile"], s["route"], s["batch"], s["stripes"], s["ways"], s["chunk"]])
    ms = timed(lambda: gene_permutation_sums(Y, g, n_permutations=R, return_null=False))
    note(f"{tag} gene_permutation_sums ms", ms)
    note(f"{tag} gathered values TB/s", rate(ms, n, A.nnz, R))
    dev = device_ms(Y, g, R)
    note(f"{tag} the C entry alone ms", dev)
    note(f"{tag} the C entry alone: gathered values TB/s", rate(dev, n, A.nnz, R))
    ms0 = timed(lambda: gene_permutation_sums(Y, g, n_permutations=0, return_null=False))
    note(f"{tag} the same call without permutations (gather, observed sums) ms", ms0)
    s1 = gene_permutation_sums(Y, g, n_permutations=R, return_null=False, max_lds_bytes=1)
    note(f"(a') {n}x{G} R={R} tile, route, ways, chunk", [s1["tile"], s1["route"], s1["ways"], s1["chunk"]])
    ms = timed(lambda: gene_permutation_sums(Y, g, n_permutations=R, return_null=False, max_lds_bytes=1), warm=1, reps=3)
    note(f"(a') {n}x{G} R={R} global route ms", ms)
    note(f"(a') {n}x{G} R={R} gathered values TB/s", rate(ms, n, A.nnz, R))
    dev = device_ms(Y, g, R, max_lds=1, reps=3)
    note(f"(a') {n}x{G} R={R} the C entry alone ms", dev)
    note(f"(a') {n}x{G} R={R} the C entry alone: gathered values TB/s", rate(dev, n, A.nnz, R))
    for key in ("count_ge", "sum_i"):
        note(f"(a') {key} equals (a)", bool(np.array_equal(s["counts"][key], s1["counts"][key], equal_nan=True)))
    # the way to these numbers before: the K x K permutation test on blocks of 256 columns
    nb = max(1, min(args.blocks, G // 256))
    cols = [Y[:, 256 * b:256 * (b + 1)].double() for b in range(nb)]
    ms = timed(lambda: [spatial_permutation_test(c, g, n_permutations=R, random_state=0) for c in cols], warm=1, reps=3)
    note(f"{tag} spatial_permutation_test on {nb} block(s) of 256 columns ms", ms)
    note(f"{tag} spatial_permutation_test scaled to {G} genes ms", ms * G / (256.0 * nb))
    # one permutation as a torch composition, scaled to R
    At = torch.sparse_csr_tensor(torch.as_tensor(A.indptr.astype(np.int64)), torch.as_tensor(A.indices.astype(np.int64)),
                                 torch.ones(A.nnz, dtype=torch.float32), size=A.shape).cuda()
    deg = torch.as_tensor(np.diff(A.indptr).astype(np.float64)).cuda()
    pis = [torch.as_tensor(permutation_indices(0, r, n)).cuda() for r in range(4)]

    def torch_perm():
        for pi in pis:
            V = Y[pi]
            L = torch.sparse.mm(At, V)
            Vd = V.double()
            (Vd * L.double()).sum(0), deg @ Vd, deg @ (Vd * Vd)
    ms = timed(torch_perm)
    note(f"{tag} torch gather + sparse.mm + sums, one permutation ms", ms / len(pis))
    note(f"{tag} torch composition scaled to R ms", ms / len(pis) * R)
    del Y, g, cols, At
    # (b) the global route
    n, R = args.spots_global, args.perms_global
    Y, g, A = grid_case(n, G, args.density, 1)
    s = gene_permutation_sums(Y, g, n_permutations=R, return_null=False)
    tag = f"(b) {n}x{G} R={R}"
    note(f"{tag} tile, route, batch, stripes, ways, chunk", [s["tile"], s["route"], s["batch"], s["stripes"], s["ways"], s["chunk"]])
    ms = timed(lambda: gene_permutation_sums(Y, g, n_permutations=R, return_null=False), warm=1, reps=8)
    note(f"{tag} gene_permutation_sums ms", ms)
    note(f"{tag} gathered values TB/s", rate(ms, n, A.nnz, R))
    dev = device_ms(Y, g, R)
    note(f"{tag} the C entry alone ms", dev)
    note(f"{tag} the C entry alone: gathered values TB/s", rate(dev, n, A.nnz, R))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
