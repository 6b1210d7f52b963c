#!/usr/bin/env python3
"""Capture golden vectors of the reference's evaluation metrics (flashdeconv/utils/metrics.py) into metrics.npz.

The module needs only numpy and scipy, so it is loaded from its file (the package's __init__ would import numba).  Every case
is a seeded (pred, true) pair; the file holds the inputs and, per case, every function and flag of the module:

  <case>__pred, <case>__true                       inputs (float32 for the f32 case: the reference runs on astype(float64))
  <case>__rmse / __rmse_per, __mae / __mae_per     compute_rmse / compute_mae
  <case>__{pearson,spearman,kendall}[_per]         compute_correlation (method="kendall" is Pearson in the reference)
  <case>__jsd, <case>__jsd_e3                      compute_jsd, epsilon 1e-10 and 1e-3
  <case>__rare_t05, <case>__rare_t20               compute_rare_cell_detection, threshold 0.05 and 0.2
  <case>__eval_overall                             evaluate_deconvolution: [rmse, mae, pearson, spearman, mean_jsd]
  <case>__eval_per                                 (K, 6): rmse, mae, pearson, spearman, mean_proportion_true / _pred
  names / named__eval_*                            the "dirichlet" case evaluated with cell_type_names

Run:  FDX_REFERENCE=<checkout> python tests/golden/make_metrics_golden.py
"""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("FDX_REFERENCE")
PER_KEYS = ["rmse", "mae", "pearson", "spearman", "mean_proportion_true", "mean_proportion_pred"]
OVERALL_KEYS = ["rmse", "mae", "pearson", "spearman", "mean_jsd"]


def _load_metrics():
    path = os.path.join(REF or "", "flashdeconv", "utils", "metrics.py")
    if not REF or not os.path.isfile(path):
        raise SystemExit("make_metrics_golden.py: set FDX_REFERENCE to a checkout of the reference (the directory holding flashdeconv/)")
    spec = importlib.util.spec_from_file_location("reference_metrics", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cases():
    rng = np.random.default_rng(20261015)
    out = {}
    t = rng.dirichlet(np.ones(6) * 0.7, size=300)
    p = 0.7 * t + 0.3 * rng.dirichlet(np.ones(6), size=300)
    out["dirichlet"] = (p, t)
    # heavily tied: quantised values, ~80 % exact-zero truth
    t = np.round(rng.dirichlet(np.ones(5) * 0.3, size=400), 2) * (rng.random((400, 5)) > 0.8)
    p = np.round(np.clip(t + rng.normal(0, 0.05, t.shape), 0, None), 2)
    out["tied"] = (p, t)
    # mixed -0.0 / +0.0 (one tie for the ranks)
    t = np.round(rng.random((200, 4)), 1) * (rng.random((200, 4)) > 0.5)
    t[rng.random(t.shape) < 0.25] = -0.0
    p = np.round(rng.random((200, 4)), 1) * (rng.random((200, 4)) > 0.5)
    p[rng.random(p.shape) < 0.25] = -0.0
    out["negzero"] = (p, t)
    t = rng.dirichlet(np.ones(5), size=120)
    p = t + rng.normal(0, 0.02, t.shape)
    p[:, 2] = 0.25
    out["constcol"] = (p, t)
    out["allconst"] = (np.full((50, 3), 0.2), np.full((50, 3), 0.2))
    t = rng.dirichlet(np.ones(4), size=100)
    p = t + rng.normal(0, 0.05, t.shape)
    p[17, 1] = np.nan
    out["nan"] = (p, t)
    t = rng.dirichlet(np.ones(5), size=100)
    p = rng.dirichlet(np.ones(5), size=100)
    p[[3, 40, 77]] = 0.0
    t[[3, 41]] = 0.0
    out["zerorows"] = (p, t)
    t = rng.random((50, 1))
    out["k1"] = (t + rng.normal(0, 0.1, t.shape), t)
    out["n1"] = (rng.dirichlet(np.ones(7), size=1), rng.dirichlet(np.ones(7), size=1))
    t = rng.dirichlet(np.ones(8), size=250).astype(np.float32)
    out["f32"] = ((t + rng.normal(0, 0.03, t.shape)).astype(np.float32), t)
    # near-constant column: the centred sums must hold at 1e-7 spread
    t = rng.dirichlet(np.ones(4), size=300)
    p = t + rng.normal(0, 0.05, t.shape)
    p[:, 0] = 0.5 + 1e-7 * rng.normal(size=300)
    t[:, 1] = 0.5 + 1e-7 * rng.normal(size=300)
    out["nearconst"] = (p, t)
    # no rare entry at either threshold
    t = np.where(rng.random((80, 4)) < 0.5, 0.0, 0.2 + 0.8 * rng.random((80, 4)))
    out["norare"] = (rng.random((80, 4)), t)
    return out


def main():
    m = _load_metrics()
    data = {}
    for name, (p, t) in cases().items():
        data[f"{name}__pred"], data[f"{name}__true"] = p, t
        P, T = p.astype(np.float64), t.astype(np.float64)
        for per in (False, True):
            sfx = "_per" if per else ""
            data[f"{name}__rmse{sfx}"] = np.asarray(m.compute_rmse(P, T, per_cell_type=per), dtype=np.float64)
            data[f"{name}__mae{sfx}"] = np.asarray(m.compute_mae(P, T, per_cell_type=per), dtype=np.float64)
            for meth in ("pearson", "spearman", "kendall"):
                data[f"{name}__{meth}{sfx}"] = np.asarray(m.compute_correlation(P, T, method=meth, per_cell_type=per), dtype=np.float64)
        data[f"{name}__jsd"] = m.compute_jsd(P, T)
        data[f"{name}__jsd_e3"] = m.compute_jsd(P, T, epsilon=1e-3)
        data[f"{name}__rare_t05"] = np.asarray(m.compute_rare_cell_detection(P, T), dtype=np.float64)
        data[f"{name}__rare_t20"] = np.asarray(m.compute_rare_cell_detection(P, T, threshold=0.2), dtype=np.float64)
        ev = m.evaluate_deconvolution(P, T)
        data[f"{name}__eval_overall"] = np.array([ev["overall"][k] for k in OVERALL_KEYS])
        data[f"{name}__eval_per"] = np.array([[ev["per_cell_type"][f"CellType_{k}"][f] for f in PER_KEYS] for k in range(P.shape[1])])
        if name == "dirichlet":
            names = np.array([f"type_{chr(65 + k)}" for k in range(P.shape[1])])
            ev = m.evaluate_deconvolution(P, T, cell_type_names=names)
            data["names"] = names
            data["named__eval_overall"] = np.array([ev["overall"][k] for k in OVERALL_KEYS])
            data["named__eval_per"] = np.array([[ev["per_cell_type"][nm][f] for f in PER_KEYS] for nm in names])
    out = os.path.join(HERE, "metrics.npz")
    np.savez_compressed(out, **data)
    print(f"wrote {out}: {len(data)} arrays, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    with np.errstate(invalid="ignore", divide="ignore"):
        main()
