#!/usr/bin/env python3
"""Wall time of utils.metrics.evaluate_deconvolution on simulated proportions built on the device (~85 % exact-zero truth):
from device tensors and from numpy arrays (upload included), host clock around a device synchronise, median of the repeats.
Prints one JSON line.  For a kernel trace run it on its own under

    rocprofv3 --kernel-trace --stats -d <dir> -- python3 tools/metrics_probe.py --reps 3

usage: metrics_probe.py [--sizes 1000000x30,10000000x50] [--reps 10] [--no-numpy]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def simulate(n, K, seed, dev):
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    t = torch.distributions.Gamma(torch.full((K,), 0.3, device=dev, dtype=torch.float64), 1.0).sample((n,))
    t = t / t.sum(1, keepdim=True).clamp_min(1e-300)
    t = torch.round(t * 1000) / 1000 * (torch.rand((n, K), generator=g, device=dev, dtype=torch.float64) > 0.85)
    p = (t + 0.02 * torch.randn((n, K), generator=g, device=dev, dtype=torch.float64)).clamp_min(0.0)
    p = p * (torch.rand((n, K), generator=g, device=dev, dtype=torch.float64) > 0.5)
    return p.contiguous(), t.contiguous()


def timed(fn, reps):
    import torch
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    out.sort()
    return out[len(out) // 2], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000x30,10000000x50")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()
    import torch
    from flashdeconv_amd.utils.metrics import evaluate_deconvolution
    dev = torch.device("cuda", 0)
    res = {"metric": "evaluate_deconvolution_ms", "reps": a.reps, "sizes": {}}
    for spec in a.sizes.split(","):
        n, K = (int(v) for v in spec.split("x"))
        P, T = simulate(n, K, 1, dev)
        torch.cuda.synchronize()
        evaluate_deconvolution(P, T)                      # warm-up: code objects, pool blocks
        row = {}
        row["device_ms"], row["device_all_ms"] = timed(lambda: evaluate_deconvolution(P, T), a.reps)
        if not a.no_numpy:
            p, t = P.cpu().numpy(), T.cpu().numpy()
            evaluate_deconvolution(p, t)
            row["numpy_ms"], row["numpy_all_ms"] = timed(lambda: evaluate_deconvolution(p, t), a.reps)
            del p, t
        row["input_bytes"] = 2 * n * K * 8
        res["sizes"][spec] = row
        del P, T
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
