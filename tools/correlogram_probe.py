#!/usr/bin/env python3
"""Wall time of utils.correlogram.correlogram_sums (one walk over the pairs, no graph) against the composed route to the same
numbers - per radius a radius graph built on the device from the resident coordinates and spatial_sums on it, then differences of
neighbouring radii - on a hexagonal slide with HBM-resident float64 values and coordinates.  Host clock around a device
synchronise, one warm-up of each route, the two routes alternating, medians of the repeats.  The graph cache is switched off for
the process (FDX_NO_PLAN_CACHE=1): a composed call on a new slide builds its graphs.  Checks that both routes give the same
counts and, within 1e-9 relative to the largest entry, the same C per band.  Prints one JSON line; the GPU clock torch reports
before and after is in it.  For a kernel trace run it on its own under

    rocprofv3 --kernel-trace --stats -d <dir> -- python3 tools/correlogram_probe.py --shapes 1000000x30x6 --reps 2 --no-composed

usage: correlogram_probe.py [--shapes 5000x30x10,1000000x30x6] [--reps 7] [--no-composed]"""
import argparse
import ctypes
import json
import os
import sys
import time

os.environ.setdefault("FDX_NO_PLAN_CACHE", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def hex_slide(n):
    """About n spots of a hexagonal lattice with unit spacing (rows sqrt(3) / 2 apart, every other row shifted by 1 / 2)."""
    import numpy as np
    m = int(round(n ** 0.5))
    r, c = np.divmod(np.arange(m * m), m)
    return np.stack([c + 0.5 * (r & 1), r * (3 ** 0.5 / 2)], axis=1)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="5000x30x10,1000000x30x6")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-composed", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    from flashdeconv_amd import _lib
    from flashdeconv_amd.utils.correlogram import correlogram_sums
    from flashdeconv_amd.utils.graph import grid_radius
    from flashdeconv_amd.utils.spatial_stats import spatial_sums
    dev = torch.device("cuda", 0)
    res = {"metric": "correlogram_ms", "reps": a.reps, "clock_mhz_before": clock(), "shapes": {}}
    for spec in a.shapes.split(","):
        n, K, B = (int(v) for v in spec.split("x"))
        xy = hex_slide(n)
        n = xy.shape[0]
        radii = grid_radius(xy[:min(n, 20000)]) * np.arange(1, B + 1)
        g = torch.Generator(device=dev).manual_seed(1)
        V = torch.rand((n, K), generator=g, device=dev, dtype=torch.float64)
        V = (V / V.sum(1, keepdim=True)).contiguous()
        xy_d = torch.as_tensor(xy, device=dev)
        torch.cuda.synchronize()

        def single():
            return correlogram_sums(V, xy_d, radii)

        def composed():
            out = []
            for r in radii:
                h = ctypes.c_void_p()
                _lib.check(_lib.load().fdx_graph_build_dev(ctypes.c_void_p(xy_d.data_ptr()), n, 2, _lib.GRAPH_RADIUS, 0, float(r),
                                                           None, ctypes.byref(h)))
                graph = _lib.Graph(h.value)
                try:
                    out.append(spatial_sums(V, graph))
                finally:
                    graph.close()
            return out

        s = single()                                             # warm-up: code objects, pool blocks
        row = {"n": n, "K": K, "B": B, "radii_over_spacing": [float(r) for r in radii], "candidates": s["candidates"],
               "pairs": int(s["W"].sum()), "bands_per_pass": s["bands_per_pass"]}
        fns = [single]
        if not a.no_composed:
            c = composed()
            W = np.diff(np.array([0] + [x["W"] for x in c]))
            C = np.diff(np.stack([np.zeros((K, K))] + [x["C"] for x in c]), axis=0)
            row["same_counts"] = bool(np.array_equal(W, s["W"]))
            row["C_max_rel_diff"] = float(np.abs(C - s["C"]).max() / np.abs(s["C"]).max())
            assert row["same_counts"] and row["C_max_rel_diff"] < 1e-9, row
            fns.append(composed)
        t = timed(fns, a.reps)
        row["single_ms"], row["single_all_ms"] = t[0]
        row["candidates_per_s"] = s["candidates"] / (t[0][0] * 1e-3)
        if not a.no_composed:
            row["composed_ms"], row["composed_all_ms"] = t[1]
            row["composed_over_single"] = t[1][0] / t[0][0]
        res["shapes"][spec] = row
        del V, xy_d
        torch.cuda.empty_cache()
    res["clock_mhz_after"] = clock()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
