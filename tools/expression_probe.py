#!/usr/bin/env python3
"""Wall time of utils.expression.celltype_expression - the weighted gene sums (one pass over Y in HBM) and the per-gene NNLS solves,
timed apart - against the route torch offers to the same numbers: ``W.T @ Y.double()`` (a float64 copy of Y for float32 input;
for CSR ``torch.sparse.mm`` where this build has it, otherwise reported as unsupported), ``W.T @ W``, the two moment sums, and the
solves on the host (scipy.optimize.nnls on the K x K Cholesky form of each gene's problem).  Host clock around a device
synchronise, one warm-up of each route, the routes alternating, medians of the repeats.  Checks that both routes give the same
sums within 1e-10 relative to the largest entry.  The bytes and operations the algorithm needs are computed here from the shapes:

    bytes  = passes * n * G * itemsize(Y) + n * Kpad * 8 + 2 * segments * (Kpad + 2) * G * 8      (CSR: nnz * (4 + itemsize) per pass)
    flops  = 2 * n * G * K  (+ 3 per entry for the moments)                                         (CSR: nnz in place of n * G)

with passes = chunks of 32 types (CSR: of 8), Kpad = K rounded up to 16, segments = rows / 2048.  Prints one JSON line; the GPU
clock torch reports before and after is in it.  For a kernel trace run it on its own under

    rocprofv3 --kernel-trace --stats -d <dir> -- python3 tools/expression_probe.py --shapes f32:1000000x2000x30 --reps 2 --no-torch

usage: expression_probe.py [--shapes f32:1000000x2000x30,f64:1000000x2000x30,csr:1000000x20000x30,f32:5000x2000x30,f32g8:1000000x2000x30]
                           [--reps 5] [--no-torch]     (kind f32 / f64 / csr, an optional g<C> for C groups of spots)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK, FP64_PEAK = 8.0e12, 78.6e12          # bytes / s and float64 FLOP / s (vector: half the float32 vector rate)
SEG = 2048


def clock():
    import torch
    try:
        return int(torch.cuda.clock_rate())
    except Exception:
        return None


def timed(fns, reps):
    """Median and all times (ms) of every callable, the callables alternating."""
    import torch
    out = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out[i].append((time.perf_counter() - t0) * 1e3)
    return [(sorted(t)[len(t) // 2], t) for t in out]


def make_Y(torch, kind, n, G, dev, gen):
    """Poisson counts: dense (mean 1.5) or CSR with about 7 % of the entries stored, built in blocks of rows."""
    if kind != "csr":
        Y = torch.empty((n, G), dtype=torch.float32 if kind == "f32" else torch.float64, device=dev)
        for r0 in range(0, n, 1 << 16):
            r1 = min(n, r0 + (1 << 16))
            Y[r0:r1] = torch.poisson(torch.full((r1 - r0, G), 1.5, device=dev), generator=gen).to(Y.dtype)
        return Y, n * G
    crow, col, val, nnz = [torch.zeros(1, dtype=torch.int64, device=dev)], [], [], 0
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for r0 in range(0, n, 1 << 15):
            r1 = min(n, r0 + (1 << 15))
            Yc = torch.poisson(torch.full((r1 - r0, G), 0.0726, device=dev), generator=gen).to_sparse_csr()
            crow.append(Yc.crow_indices()[1:] + nnz)
            col.append(Yc.col_indices().to(torch.int32))
            val.append(Yc.values())
            nnz += int(Yc.values().numel())
        Y = torch.sparse_csr_tensor(torch.cat(crow), torch.cat(col), torch.cat(val), size=(n, G), device=dev)
    return Y, nnz


def host_nnls(A, B):
    """Every gene's NNLS on the host from the Gram form: A = R'R, min |R s - R^-T b| over s >= 0 (scipy.optimize.nnls)."""
    import numpy as np
    from scipy.linalg import cholesky, solve_triangular
    from scipy.optimize import nnls
    R = cholesky(A + 1e-12 * np.trace(A) / A.shape[0] * np.eye(A.shape[0]))
    Z = solve_triangular(R, B, trans="T")
    return np.stack([nnls(R, Z[:, g], maxiter=30 * A.shape[0])[0] for g in range(B.shape[1])], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="f32:1000000x2000x30,f64:1000000x2000x30,csr:1000000x20000x30,f32:5000x2000x30,f32g8:1000000x2000x30")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    from flashdeconv_amd import _lib
    from flashdeconv_amd.utils import expression as ex
    dev = torch.device("cuda", 0)
    res = {"metric": "celltype_expression_ms", "reps": a.reps, "clock_mhz_before": clock(), "shapes": {}}
    for spec in a.shapes.split(","):
        kind, shape = spec.split(":")
        C = 1
        if "g" in kind:
            kind, c = kind.split("g")
            C = int(c)
        n, G, K = (int(v) for v in shape.split("x"))
        gen = torch.Generator(device=dev).manual_seed(1)
        Y, entries = make_Y(torch, kind, n, G, dev, gen)
        W = torch.rand((n, K), generator=gen, device=dev, dtype=torch.float64) ** 4
        W = (W / W.sum(1, keepdim=True)).contiguous()
        groups = torch.randint(0, C, (n,), generator=gen, device=dev) if C > 1 else None
        labels, Cc = ex._check_groups(groups, n, C if C > 1 else None)
        torch.cuda.synchronize()
        item = 4 if kind != "f64" else 8
        Kpad = -(-K // 16) * 16
        passes = -(-Kpad // 32) if kind != "csr" else Kpad // 8
        segs = -(-n // SEG) + C
        y_bytes = entries * (item if kind != "csr" else item + 4)
        alg_bytes = passes * y_bytes + n * Kpad * 8 + 2 * segs * (Kpad + 2) * G * 8
        flops = 2 * entries * K + 3 * entries
        bound_s = max(alg_bytes / HBM_PEAK, flops / FP64_PEAK)
        row = {"kind": kind, "n": n, "G": G, "K": K, "C": C, "entries": entries, "alg_bytes": alg_bytes, "flops": flops,
               "bound_ms": bound_s * 1e3, "bound_by": "bytes" if alg_bytes / HBM_PEAK >= flops / FP64_PEAK else "flops"}
        keep = {}

        def sums():
            keep["s"] = ex._sums_device(Y, W, labels, Cc, n, G, K)

        def solve():
            A, B, q, _, _ = keep["s"]
            keep["x"] = ex._solve_device(A, B, q, 0.0, 10000, 1e-10)

        def whole():
            keep["w"] = ex.celltype_expression(Y, W, groups=groups, n_groups=C if C > 1 else None, output="torch")

        def torch_sums():
            Yd = Y if kind == "f64" else (Y.to(torch.float64) if kind != "csr" else Y)
            if kind == "csr":
                Bt = torch.sparse.mm(Yd.to(torch.float64).t().to_sparse_csr(), W).t().contiguous()
                q = u = None
            else:
                Bt = W.t() @ Yd
                q, u = (Yd * Yd).sum(0), Yd.sum(0)
            keep["t"] = (W.t() @ W, Bt, q, u)

        sums()
        solve()
        whole()                                                   # warm-up: code objects, pool blocks
        n_iter = keep["x"][1]
        row["n_iter_max"], row["n_iter_mean"] = int(n_iter.max().item()), float(n_iter.double().mean().item())
        row["converged_all"] = bool(keep["x"][2].all().item())
        fns, names = [sums, solve, whole], ["sums_ms", "solve_ms", "whole_ms"]
        if not a.no_torch and C == 1:
            try:
                torch_sums()
                At, Bt = keep["t"][0], keep["t"][1]
                A, B = keep["s"][0][0], keep["s"][1][0]
                row["B_max_rel_diff"] = float(((B - Bt).abs().max() / Bt.abs().max()).item())
                row["A_max_rel_diff"] = float(((A - At).abs().max() / At.abs().max()).item())
                assert row["B_max_rel_diff"] < 1e-10 and row["A_max_rel_diff"] < 1e-10, row
                fns.append(torch_sums)
                names.append("torch_sums_ms")
                t0 = time.perf_counter()
                S_host = host_nnls(_lib.tensor_to_host(At), _lib.tensor_to_host(Bt))
                row["host_nnls_ms"] = (time.perf_counter() - t0) * 1e3
                S = _lib.tensor_to_host(keep["x"][0][0])
                row["S_max_rel_diff_to_host_nnls"] = float(np.abs(S - S_host).max() / np.abs(S_host).max())
            except (RuntimeError, NotImplementedError) as e:
                row["torch_route"] = f"unsupported: {type(e).__name__}: {str(e)[:160]}"
        elif C > 1:
            row["torch_route"] = "not run: torch has no grouped form of the contraction short of C masked copies"
        for name, (med, all_ms) in zip(names, timed(fns, a.reps)):
            row[name], row[name.replace("_ms", "_all_ms")] = med, all_ms
        row["sums_share_of_bound"] = row["bound_ms"] / row["sums_ms"]
        if "torch_sums_ms" in row:
            row["torch_sums_over_sums"] = row["torch_sums_ms"] / row["sums_ms"]
        res["shapes"][spec] = row
        keep.clear()
        del Y, W
        torch.cuda.empty_cache()
        _lib.load().fdx_trim()
    res["clock_mhz_after"] = clock()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
