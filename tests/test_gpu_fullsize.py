"""-m gpu: BASELINE.json's full single-GPU size (1M spots x 2000 genes x 30 types, d=512): against the CPU oracle at that
very size (test_config3_at_one_million_spots_against_the_oracle: 16 GB of host float64, ~30-45 s of CPU per family) and through
size-independent properties.  Synthetic inputs are generated on the device (bench.py generators)."""
import hashlib
import os
import sys

import numpy as np
import pytest
from scipy import sparse

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def big():
    import torch
    sys.path.insert(0, ROOT)
    import bench
    free, _ = torch.cuda.mem_get_info()
    if free < 40 * 2**30:
        pytest.skip("BASELINE configs[2] needs 40 GB of free HBM (1M x 2000 float32 and the fit's buffers)")
    n = 1_000_000
    Y, X, coords = bench.gen_gaussian(torch, n, 2000, 30, torch.device("cuda", 0), seed=7)
    return n, Y, X, coords


def test_full_size_fit_properties(big):
    import torch
    from flashdeconv_amd import FlashDeconv
    n, Y, X, coords = big
    m = FlashDeconv(sketch_dim=512, preprocess="raw", n_hvg=2000)
    P = m.fit_transform(Y, X, coords, output="torch")
    assert P.shape == (n, 30) and m.beta_.shape == (n, 30)
    assert bool(torch.all(m.beta_ >= 0)) and bool(torch.isfinite(P).all())
    assert float((P.sum(dim=1) - 1).abs().max()) < 1e-12                      # rows of proportions sum to one
    assert m.info_["converged"] and 3 <= m.info_["n_iterations"] <= 15           # well-conditioned family: 5-7 sweeps
    assert np.isfinite(m.info_["final_objective"]) and m.lambda_used_ > 0
    h1 = hashlib.sha256(m.beta_.cpu().numpy().tobytes()).hexdigest()
    P2 = FlashDeconv(sketch_dim=512, preprocess="raw", n_hvg=2000).fit_transform(Y, X, coords, output="torch")
    assert torch.equal(P, P2)                                                    # run-to-run bit determinism
    # spot order independence: permuting the spots permutes the result (graph, hash and solve are order-free)
    perm = torch.randperm(n, device=Y.device, generator=torch.Generator(device=Y.device).manual_seed(1))
    P3 = FlashDeconv(sketch_dim=512, preprocess="raw", n_hvg=2000).fit_transform(Y[perm], X, coords[perm], output="torch")
    assert float((P3 - P[perm]).abs().max()) < 1e-9
    # adjacency: symmetric, binary, no self loops, k <= degree
    A = m.adjacency_
    assert A.shape == (n, n) and (A != A.T).nnz == 0 and A.diagonal().sum() == 0 and np.all(A.data == 1.0)
    deg = np.diff(A.indptr)
    assert deg.min() >= 6 and 6.5 < deg.mean() < 7.6
    assert h1 == hashlib.sha256(m.beta_.cpu().numpy().tobytes()).hexdigest()


def test_full_size_sketch_linearity_and_solver_fixed_point(big):
    import torch
    from flashdeconv_amd import FlashDeconv
    n, Y, X, coords = big
    # scaling Y and X by 2 (raw mode) scales the sketches by 2 and leaves the NNLS solution beta unchanged up to the
    # regularisers' scale: with rho = 0 and lambda = 0 the abundances are exactly scale invariant
    kw = dict(sketch_dim=512, preprocess="raw", n_hvg=2000, rho_sparsity=0.0, lambda_spatial=0.0, max_iter=8, tol=1e-30)
    b1 = FlashDeconv(**kw).fit(Y, X, coords, output="torch").beta_
    b2 = FlashDeconv(**kw).fit(Y * 2.0, X * 2.0, coords, output="torch").beta_
    assert float((b1 - b2).abs().max()) < 1e-9 * float(b1.abs().max())


@pytest.mark.parametrize("n,K,family", [(10_000, 10, "gaussian"), (100_000, 20, "gaussian"), (30_000, 20, "counts"),
                                        (100_000, 20, "counts_f32")])
def test_baseline_configs_at_full_size_against_the_oracle(n, K, family):
    """BASELINE.json configs[0] (10k x 2000 x 10) and configs[1] (100k x 2000 x 20, d = 512) at their full sizes, plus a
    count-like / log-CPM case, against the CPU oracle (the pinned restatement of the reference): same selected genes, same
    iteration count, abundances within 1e-8 relative Frobenius (contract: 1e-4).  counts_f32: the configs[1] shape with the
    counts stored as FLOAT32 - the reference then computes log-CPM in float32 (numpy dtype rules, core/deconv.py:190-191)
    and the device a float32-class log1p (csrc/tile_device.h); the oracle is fed the same float32 array, tolerance 1e-5."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import datagen
    import fdx_oracle as orc
    from conftest import rel_fro
    from flashdeconv_amd import FlashDeconv
    if family == "gaussian":
        Y, X, coords, _ = datagen.gaussian_raw(n, 2000, K, seed=n % 97)
        pre, max_iter = "raw", 100
    else:
        Y, X, coords, _ = datagen.count_like(n, 2000, K, 0.1, 5)
        pre, max_iter = "log_cpm", 12
        if family == "counts_f32":
            Y = Y.astype(np.float32)
    tol = 1e-5 if family == "counts_f32" else 1e-8
    m = FlashDeconv(sketch_dim=512, preprocess=pre, n_hvg=2000, max_iter=max_iter).fit(Y, X, coords)
    want = orc.fit(Y, X, coords, sketch_dim=512, preprocess_method=pre, n_hvg=2000, max_iter=max_iter, graph="kdtree")
    assert np.array_equal(m.gene_idx_, want["gene_idx"])
    A, B = m.adjacency_, want["adjacency"].tocsr()
    assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
    assert m.info_["n_iterations"] == want["info"]["n_iterations"] and m.info_["converged"] == want["info"]["converged"]
    np.testing.assert_allclose(m.lambda_used_, want["lambda_used"], rtol=1e-10)
    assert rel_fro(m.beta_, want["beta"]) < tol
    assert rel_fro(m.proportions_, want["proportions"]) < tol


@pytest.mark.parametrize("family", ["gaussian", "counts_f32"])
def test_config3_at_one_million_spots_against_the_oracle(family):
    """BASELINE.json configs[2] ITSELF - 1M spots x 2000 genes x 30 types, d = 512, the inputs of bench.py - against the CPU
    oracle (the pinned restatement of core/deconv.py:305-398, core/solver.py:385-413) on the same rows: same genes, the same
    adjacency index for index, the same iteration count and stopping verdict, abundances and proportions within 1e-8 relative
    Frobenius (contract 1e-4).  What the 10k / 100k cases above cannot see: a defect that only appears past 100k rows (32-bit
    offsets, tile counts, Morton cells).  counts_f32: the count-like family of the bench (log-CPM, float32 rows: the reference
    computes float32, the device a float32-class log1p - tolerance 1e-5 as above), 10 sweeps."""
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bench
    import fdx_oracle as orc
    from conftest import rel_fro
    from flashdeconv_amd import FlashDeconv, _lib
    free, _ = torch.cuda.mem_get_info()
    if free < 40 * 2**30:
        pytest.skip("BASELINE configs[2] needs 40 GB of free HBM")
    n, dev = 1_000_000, torch.device("cuda", 0)
    if family == "gaussian":
        Y, X, coords = bench.gen_gaussian(torch, n, 2000, 30, dev, seed=3)
        pre, max_iter, tol = "raw", 100, 1e-8
    else:
        Y, X, coords = bench.gen_counts(torch, n, 2000, 30, dev, seed=3)
        pre, max_iter, tol = "log_cpm", 10, 1e-5
    m = FlashDeconv(sketch_dim=512, preprocess=pre, n_hvg=2000, max_iter=max_iter).fit(Y, X, coords)
    Yh = _lib.tensor_to_host(Y)                               # the float32 rows the device read
    ch = _lib.tensor_to_host(coords)
    del Y, coords
    torch.cuda.empty_cache()
    if family == "gaussian":
        Yh = Yh.astype(np.float64)                            # raw: the reference's astype(float64) of the same values
    want = orc.fit(Yh, X, ch, sketch_dim=512, preprocess_method=pre, n_hvg=2000, max_iter=max_iter, graph="kdtree")
    del Yh
    assert np.array_equal(m.gene_idx_, want["gene_idx"]) and len(m.gene_idx_) == 2000
    A, B = m.adjacency_, want["adjacency"].tocsr()
    assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
    assert m.info_["n_iterations"] == want["info"]["n_iterations"] and m.info_["converged"] == want["info"]["converged"]
    np.testing.assert_allclose(m.lambda_used_, want["lambda_used"], rtol=1e-10 if family == "gaussian" else 1e-6)
    np.testing.assert_allclose(m.info_["final_objective"], want["info"]["final_objective"], rtol=1e-9 if family == "gaussian" else 1e-5)
    assert rel_fro(m.beta_, want["beta"]) < tol
    assert rel_fro(m.proportions_, want["proportions"]) < tol


# ---- BASELINE.json configs[4]: 10M spots x 5000 genes x 50 types, sketch_dim 1024, lambda auto, 8 GPUs -> 1.25M spots per GPU
def test_config5_shape_against_the_oracle():
    """configs[4]'s per-spot shape (5000 genes, 50 types, d = 1024, lambda auto) at a spot count the CPU oracle reaches:
    same adjacency, same iteration count, abundances within 1e-8 relative Frobenius (contract 1e-4)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import datagen
    import fdx_oracle as orc
    from conftest import rel_fro
    from flashdeconv_amd import FlashDeconv
    for family, pre, max_iter in (("gaussian", "raw", 100), ("counts", "log_cpm", 15)):
        if family == "gaussian":
            Y, X, coords, _ = datagen.gaussian_raw(3000, 5000, 50, seed=5)
        else:
            Y, X, coords, _ = datagen.count_like(2000, 5000, 50, 0.1, 6)
        m = FlashDeconv(sketch_dim=1024, preprocess=pre, n_hvg=5000, max_iter=max_iter).fit(Y, X, coords)
        want = orc.fit(Y, X, coords, sketch_dim=1024, preprocess_method=pre, n_hvg=5000, max_iter=max_iter, graph="kdtree")
        assert np.array_equal(m.gene_idx_, want["gene_idx"]) and len(m.gene_idx_) == 5000
        A, B = m.adjacency_, want["adjacency"].tocsr()
        assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
        assert m.info_["n_iterations"] == want["info"]["n_iterations"] and m.info_["converged"] == want["info"]["converged"]
        np.testing.assert_allclose(m.lambda_used_, want["lambda_used"], rtol=1e-10)
        assert rel_fro(m.beta_, want["beta"]) < 1e-8 and rel_fro(m.proportions_, want["proportions"]) < 1e-8


def test_config5_full_shard_properties_and_sharding():
    """One rank's share of configs[4] at full size: 1.25M spots x 5000 genes x 50 types, d = 1024, lambda auto, on one
    GPU.  Size-independent properties (the oracle cannot run here), run-to-run determinism, and the sharded path itself:
    the same problem cut into 4 shards driven by the native loop (thread ranks) must give the single-GPU bits."""
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bench
    import test_gpu_sharded as tsh
    from flashdeconv_amd import FlashDeconv, _lib
    from flashdeconv_amd.distributed import diag_mean
    free, _ = torch.cuda.mem_get_info()
    if free < 90 * 2**30:
        pytest.skip("a configs[4] shard needs 90 GB of free HBM (1.25M x 5000 float32 = 25 GB, the fit, four shard copies)")
    dev = torch.device("cuda", 0)
    n, G, K, d = 1_250_000, 5000, 50, 1024
    Y, X, coords = bench.gen_gaussian(torch, n, G, K, dev, seed=11)
    m = FlashDeconv(sketch_dim=d, preprocess="raw", n_hvg=G)
    P = m.fit_transform(Y, X, coords, output="torch")
    assert P.shape == (n, K) and bool(torch.all(m.beta_ >= 0)) and bool(torch.isfinite(P).all())
    assert float((P.sum(dim=1) - 1).abs().max()) < 1e-12
    assert m.info_["converged"] and 3 <= m.info_["n_iterations"] <= 20 and m.lambda_used_ > 0
    P2 = FlashDeconv(sketch_dim=d, preprocess="raw", n_hvg=G).fit_transform(Y, X, coords, output="torch")
    assert torch.equal(P, P2)
    W = 4
    full, shards = tsh._native_shards(torch, coords, Y, X, W, d, K, _lib.PRE_RAW)
    lam, rho_eff = m.lambda_used_, 0.01 * diag_mean(shards[0]["XtX_h"])
    results = tsh._run_native_threads(torch, shards, K, lam, rho_eff, 1e-4, 100)
    assert all(res[0] == m.info_["n_iterations"] and res[1] for res in results)
    assert torch.equal(tsh._assemble(torch, shards, results, n, K), m.beta_)


def test_config4_ten_million_spots_eight_virtual_ranks():
    """BASELINE configs[4] at its real size on ONE GPU: 10M spots x 5000 genes x 50 types, sketch_dim 1024, lambda auto,
    8 ranks (tools/virtual_ranks.py: the sharded plan as 8 processes would run it - every rank bins all 10M points and
    finds the lists of its own 1.25M rows, the 320 MB of list rows are all-gathered, every rank symmetrises and localises
    its rows -, each rank's 1.25M x 5000 float32 shard generated, sketched into H by fdx_prepare_dev and freed, then the
    native iteration loop with 8 thread ranks).  No oracle reaches this size: size-independent properties, run-to-run bit
    determinism of the loop, and the 8-rank result equal to the 4-rank result bit for bit (the Jacobi sweep of
    core/solver.py:157-166 is partition-independent)."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import virtual_ranks as vr
    free, _ = torch.cuda.mem_get_info()
    if free < 120 * 2**30:
        pytest.skip("configs[4] on one GPU needs 120 GB of free HBM (a 4-rank shard of Y alone is 50 GB)")
    torch.cuda.set_device(0)
    n, G, K, d = 10_000_000, 5000, 50, 1024
    keep = {}
    beta8, prop8, info8 = vr.run_config5(torch, 8, n=n, G=G, K=K, d=d, seed=11, keep=keep)
    print("configs[4] / 8 virtual ranks:", info8)
    its = info8["n_iterations"]
    assert len(set(its)) == 1 and 3 <= its[0] <= 20 and all(info8["converged"])       # every rank stops at the same sweep
    assert info8["knn_ties"] == 0 and info8["lambda_used"] > 0
    assert sum(info8["n_own"]) == n and min(info8["n_halo"]) > 0
    assert 6 * n <= info8["nnz"] <= 9 * n                                              # mean degree of a k = 6 union graph ~ 7.06
    assert bool((beta8 >= 0).all()) and bool(torch.isfinite(beta8).all())
    assert float((prop8.sum(dim=1) - 1).abs().max()) < 1e-12
    # the iteration loop again on the same shards: same bits
    res2 = vr.virtual_solve(torch, keep["ranks"], K, keep["lam"], keep["rho_eff"], 1e-4, 100)
    again, _ = vr.assemble(torch, keep["ranks"], res2, n, K, want_props=False)
    assert torch.equal(again, beta8)
    del again, prop8
    coords = keep["coords"]
    for R in keep["ranks"]:
        R["g"].close()
    keep.clear()
    torch.cuda.empty_cache()
    # the same job cut into 4 shards of 2.5M spots
    beta4, _, info4 = vr.run_config5(torch, 4, n=n, G=G, K=K, d=d, seed=11, coords=coords)
    print("configs[4] / 4 virtual ranks:", info4)
    assert info4["n_iterations"][0] == its[0] and info4["nnz"] == info8["nnz"]
    np.testing.assert_allclose(info4["lambda_used"], info8["lambda_used"], rtol=1e-14)
    assert torch.equal(beta4, beta8)


def test_bench_inputs_repeat_and_dump_outputs_of_the_timed_fits(tmp_path, monkeypatch, capsys):
    """bench.py's generators give the same inputs for the same seed (every draw from the seeded generator), and --dump-outputs
    writes what each family's last timed fit returned: float64 files within bench.DUMP_BYTES, taken from the model that ran
    exactly --warmup + --steps fits (not the cold fit's own model) after its last fit."""
    import json
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from flashdeconv_amd import FlashDeconv
    dev = torch.device("cuda", 0)
    for gen, G in ((bench.gen_gaussian, 300), (bench.gen_counts, 300), (bench.gen_sparse, 2000)):
        (Y1, X1, c1), (Y2, X2, c2) = gen(torch, 20000, G, 8, dev, 5), gen(torch, 20000, G, 8, dev, 5)
        parts = (lambda Y: (Y.crow_indices(), Y.col_indices(), Y.values())) if Y1.layout == torch.sparse_csr else (lambda Y: (Y,))
        assert all(torch.equal(u, v) for u, v in zip(parts(Y1), parts(Y2))), gen.__name__
        assert np.array_equal(X1, X2) and torch.equal(c1, c2), gen.__name__
    fits, models, dumped_from = {}, [], []       # fit calls per model (models kept alive so that ids stay unique); per dump:
    fit0, outputs0 = FlashDeconv.fit, bench.fit_outputs    # (model id, its fit calls when the dump was taken)

    def counting_fit(self, *args, **kwargs):
        if id(self) not in fits:
            models.append(self)
        fits[id(self)] = fits.get(id(self), 0) + 1
        return fit0(self, *args, **kwargs)

    def recording_outputs(torch_, model, rows):
        dumped_from.append((id(model), fits.get(id(model))))
        return outputs0(torch_, model, rows)

    monkeypatch.setattr(FlashDeconv, "fit", counting_fit)
    monkeypatch.setattr(bench, "fit_outputs", recording_outputs)
    out = tmp_path / "dump"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--family", "all", "--spots", "20000", "--genes", "300", "--types", "8",
                                      "--sketch-dim", "64", "--sparse-genes", "2000", "--steps", "3", "--warmup", "1",
                                      "--no-cpu-baseline", "--no-live-pmc", "--no-host-arrays", "--dump-outputs", str(out)])
    bench.main()
    line = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1])
    # five dumps (gaussian, its float64-Y twin, counts, sparse, lattice), each of a model with 1 warm-up + 3 timed fits and none after
    assert len(dumped_from) == 5 and all(n == 4 and fits[m] == 4 for m, n in dumped_from), (dumped_from, fits)
    assert len({m for m, _ in dumped_from}) == 5
    models.clear()
    recs = {"gaussian": dict(line["config"], steps=line["steps"]), "gaussian_y_f64": line["y_f64"], "counts": line["count_like"],
            "sparse": line["sparse_csr"], "lattice": line["lattice"]}
    files = {p.name: np.load(p) for p in out.iterdir()}
    assert sum(p.stat().st_size for p in out.iterdir()) <= bench.DUMP_BYTES
    assert all(v.dtype == np.float64 for v in files.values())
    assert np.array_equal(files["sample_rows.npy"], np.arange(20000))
    for fam, rec in recs.items():
        assert rec["steps"] == 3, fam
        beta, prop, info = files[f"{fam}_beta.npy"], files[f"{fam}_proportions.npy"], files[f"{fam}_info.npy"]
        assert beta.shape == prop.shape == (20000, 8) and bool((beta >= 0).all()), fam
        np.testing.assert_allclose(prop.sum(axis=1), 1.0, atol=1e-12)
        assert info[0] == rec["n_iterations"] and info[1] == float(rec["converged"]), fam
        assert files[f"{fam}_gene_idx.npy"].ndim == 1
    assert set(files) == {"sample_rows.npy"} | {f"{f}_{k}.npy" for f in recs for k in ("beta", "proportions", "info", "gene_idx")}


def test_bench_plain_run_times_the_headline_alone_and_full_adds_the_rest(monkeypatch, capsys):
    """A plain run fits the gaussian/raw family alone - one model, exactly --warmup + --steps fits - and starts no CPU baseline,
    host_arrays record or PMC child runs; its line carries the contract keys and nothing of another family.  --full at the same
    size: every family's record, one cold fit per family, and the three extra measurements (stubbed here: they are the slow part)."""
    import json
    sys.path.insert(0, ROOT)
    import bench
    from flashdeconv_amd import FlashDeconv
    fits, models, called = {}, [], []
    fit0 = FlashDeconv.fit

    def counting_fit(self, *args, **kwargs):
        if id(self) not in fits:
            models.append(self)                  # kept alive so that ids stay unique
        fits[id(self)] = fits.get(id(self), 0) + 1
        return fit0(self, *args, **kwargs)

    monkeypatch.setattr(FlashDeconv, "fit", counting_fit)
    for name, stub in (("cpu_baseline", {"value": 1.0}), ("host_arrays_record", {}), ("live_pmc_traffic", {})):
        monkeypatch.setattr(bench, name, lambda *a, _name=name, _stub=stub, **k: called.append(_name) or _stub)
    small = ["--spots", "20000", "--genes", "300", "--types", "8", "--sketch-dim", "64", "--sparse-genes", "2000",
             "--steps", "3", "--warmup", "1"]

    def run(extra):
        monkeypatch.setattr(sys, "argv", ["bench.py"] + small + extra)
        bench.main()
        return json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1])

    line = run([])
    assert list(fits.values()) == [4] and called == [], (fits, called)
    assert line["metric"] == bench.METRIC and line["unit"] == "spots/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["steps"] == 3 and line["warmup"] == 1 and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["config"]["n_iterations"] >= 1 and line["roofline"]["ms_per_launch"] > 0
    assert not set(line) & {"count_like", "y_f64", "sparse_csr", "lattice", "cold_ms", "host_arrays", "cpu_baseline"}, sorted(line)
    fits.clear()
    models.clear()
    line = run(["--full"])
    assert sorted(called) == ["cpu_baseline", "host_arrays_record", "live_pmc_traffic"], called
    # five families (gaussian, its float64-Y twin, counts, sparse, lattice): 1 warm-up + 3 timed fits each, then one cold fit each
    assert sorted(fits.values()) == [1] * 5 + [4] * 5, fits
    recs = [line, line["y_f64"], line["count_like"], line["sparse_csr"], line["lattice"]]
    assert all(r["cold_ms"] > 0 and r["steps"] == 3 for r in recs)
    assert line["cpu_baseline"] == {"value": 1.0} and line["host_arrays"] == {}
