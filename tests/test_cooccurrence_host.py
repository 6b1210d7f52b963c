"""CPU-only tests of the label co-occurrence by distance band (utils.cooccurrence): the host assembly entry by entry with every NaN
rule, the ratio on a hand case, the per-band moments against enumeration of all permutations, the request and argument checks
that come before anything touches the GPU, the C entry's declaration, export and binding, the public signatures, and the
precondition that makes the bit-for-bit comparison of the float64 null sums in tests/test_gpu_cooccurrence.py legitimate."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import cooccurrence_ref as ref
import nhood_ref


def _by_hand(count, na, n, W, sds, ge=None, le=None, sd=None, sq=None, R=0):
    """assemble_cooccurrence for one mode's arrays, entry by entry in Python floats."""
    B, C = count.shape[0], count.shape[1]
    keys = ["expected", "variance", "z_score", "interaction", "ratio"]
    if R:
        keys += ["p_greater", "p_less", "p_value", "null_mean", "null_std", "z_sim"]
    out = {k: np.full((B, C, C), np.nan) for k in keys}
    for b in range(B):
        E, V = nhood_ref.moments(n, int(W[b]), int(sds[b]), na)
        total = float(count[b].sum())
        for a in range(C):
            row = float(count[b, a].sum())
            for c in range(C):
                col = float(count[b, :, c].sum())
                N = float(count[b, a, c])
                out["expected"][b, a, c], out["variance"][b, a, c] = E[a, c], V[a, c]
                if V[a, c] > 0:
                    out["z_score"][b, a, c] = (N - E[a, c]) / math.sqrt(V[a, c])
                if row > 0:
                    out["interaction"][b, a, c] = N / row
                if row > 0 and col > 0:
                    out["ratio"][b, a, c] = N * total / (row * col)
                if R:
                    pg, pl = (1.0 + ge[b, a, c]) / (R + 1.0), (1.0 + le[b, a, c]) / (R + 1.0)
                    mean = sd[b, a, c] / R
                    std = math.sqrt(max(sq[b, a, c] / R - mean * mean, 0.0))
                    out["p_greater"][b, a, c], out["p_less"][b, a, c] = pg, pl
                    out["p_value"][b, a, c] = min(1.0, 2.0 * min(pg, pl))
                    out["null_mean"][b, a, c], out["null_std"][b, a, c] = N + mean, std
                    if std > 0:
                        out["z_sim"][b, a, c] = -mean / std
    return out


def _tiny_case(seed, n=9, C=3, leave_out=True):
    """A tiny point set with two bands, labels, the reference's counts, degrees and a null of 6 permutations."""
    import correlogram_ref as cr
    rs = np.random.RandomState(seed)
    coords = rs.randint(0, 4, size=(n, 2)).astype(np.float64)
    radii = np.array([1.0, 2.5])
    labels = rs.randint(0, C, n)
    if leave_out:
        labels[0] = -1
    g = cr.band_reference(np.zeros((n, 1)), coords, radii)
    deg = g["deg"]
    cum = np.cumsum(deg, axis=1)
    obs = ref.band_counts(g["A"], labels, C)
    null = ref.null_counts(g["A"], labels, C, 3, 0, 6)
    return {"coords": coords, "radii": radii, "labels": labels, "A": g["A"], "obs": obs, "null": null, "n": n, "C": C,
            "na": nhood_ref.label_counts(labels, C), "W": deg.sum(0), "sds": (deg * deg).sum(0), "sds_cum": (cum * cum).sum(0),
            "acc": ref.accumulate(null, obs)}


# ---------------------------------------------------------------- the assembly
@pytest.mark.parametrize("mode", ["band", "cumulative"])
def test_assemble_entry_by_entry(mode):
    from flashdeconv_amd.utils.cooccurrence import assemble_cooccurrence
    t = _tiny_case(1)
    tail = "_cum" if mode == "cumulative" else ""
    perm = [t["acc"][k + tail] for k in ("count_ge", "count_le", "sum_d", "sumsq_d")]
    for R in (0, 6):
        got = assemble_cooccurrence(t["obs"], t["na"], t["n"], t["W"], t["sds"], t["sds_cum"], *(perm if R else [None] * 4),
                                    n_permutations=R, mode=mode)
        count = np.cumsum(t["obs"], axis=0) if mode == "cumulative" else t["obs"]
        W = np.cumsum(t["W"]) if mode == "cumulative" else t["W"]
        sds = t["sds_cum"] if mode == "cumulative" else t["sds"]
        want = _by_hand(count, t["na"], t["n"], W, sds, *[p.astype(np.float64) for p in perm], R=R)
        assert np.array_equal(got["count"], count) and got["count"].dtype == np.int64
        assert np.array_equal(got["W"], W) and np.array_equal(got["label_counts"], t["na"])
        assert ("p_value" in got) == (R > 0) and ("n_permutations" in got) == (R > 0)
        for k, v in want.items():
            assert got[k].shape == v.shape and got[k].dtype == np.float64, k
            assert np.array_equal(np.isnan(got[k]), np.isnan(v)), (mode, R, k)
            np.testing.assert_allclose(got[k], v, rtol=1e-12, atol=0, err_msg=f"{mode} {R} {k}")
    # the cumulative count of the last band is the count of the radius graph of r_B
    A_all = t["A"][0] + t["A"][1]
    assert np.array_equal(np.cumsum(t["obs"], axis=0)[-1], nhood_ref.pair_counts(A_all, t["labels"], t["C"]))


def test_assemble_nan_rules_and_checks():
    from flashdeconv_amd.utils.cooccurrence import assemble_cooccurrence
    C = 3
    # band 0: an ordinary band; band 1: empty (W = 0); label 2 never occurs
    count = np.zeros((2, C, C), dtype=np.int64)
    count[0, :2, :2] = [[2, 3], [3, 0]]
    na = np.array([3, 3, 0])
    zeros = np.zeros((2, C, C))
    got = assemble_cooccurrence(count, na, 8, [8, 0], [12, 0], [12, 12], zeros.astype(np.int64) + 4, zeros.astype(np.int64) + 4, zeros,
                                zeros, n_permutations=4)
    assert np.isnan(got["z_score"][1]).all() and np.isnan(got["expected"][1]).all()          # an empty band: no moments
    assert np.isnan(got["interaction"][1]).all() and np.isnan(got["ratio"][1]).all()          # ... no rows, no columns
    assert np.isfinite(got["z_score"][0, :2, :2]).all()
    assert np.isnan(got["interaction"][0, 2]).all() and np.isfinite(got["interaction"][0, :2]).all()      # the empty row only
    assert np.isnan(got["ratio"][0, 2]).all() and np.isnan(got["ratio"][0, :, 2]).all() and np.isfinite(got["ratio"][0, :2, :2]).all()
    assert np.isnan(got["z_score"][0, 2]).all() and np.isnan(got["z_score"][0, :, 2]).all()  # a label without spots cannot vary
    assert np.isnan(got["z_sim"]).all() and np.all(got["null_std"] == 0)                       # a null that does not vary
    assert np.all(got["p_value"] == 1.0) and np.array_equal(got["null_mean"], count.astype(np.float64))
    # n < 4: no moments, nothing raises
    small = assemble_cooccurrence(count[:1, :2, :2], np.array([2, 1]), 3, [4], [6])
    assert np.isnan(small["z_score"]).all() and np.isfinite(small["ratio"]).all()
    # cumulative: the running sums, and sum_deg_sq_cum in the place of sum_deg_sq
    cum = assemble_cooccurrence(count, na, 8, [8, 0], [12, 0], [12, 12], mode="cumulative")
    assert np.array_equal(cum["count"][1], count[0]) and np.array_equal(cum["W"], [8, 8])
    np.testing.assert_array_equal(cum["z_score"][1], cum["z_score"][0])
    for bad, match in ((dict(count=count[0]), "count must be"), (dict(count=count.astype(np.float64)), "integer array"),
                       (dict(label_counts=na[:2]), "count must be"), (dict(W=[8]), "must be \\(B,\\)"),
                       (dict(mode="ring"), "Unknown mode"), (dict(mode="cumulative"), "sum_deg_sq_cum is needed"),
                       (dict(n_permutations=3), "are needed when n_permutations >= 1"),
                       (dict(n_permutations=3, count_ge=zeros[0], count_le=zeros, sum_d=zeros, sumsq_d=zeros), "must be \\(B, C, C\\)")):
        kw = dict(count=count, label_counts=na, n=8, W=[8, 0], sum_deg_sq=[12, 0])
        kw.update(bad)
        with pytest.raises(ValueError, match=match):
            assemble_cooccurrence(**kw)


def test_ratio_on_a_hand_case():
    from flashdeconv_amd.utils.cooccurrence import assemble_cooccurrence
    # one band, two labels: a's neighbours are 2 a and 6 b, b's are 6 a and 10 b - 24 pair ends, 8 of them at a, 16 at b
    count = np.array([[[2, 6], [6, 10]]], dtype=np.int64)
    got = assemble_cooccurrence(count, np.array([3, 5]), 8, [24], [80])
    want = np.array([[[(2 / 8) / (8 / 24), (6 / 8) / (16 / 24)], [(6 / 16) / (8 / 24), (10 / 16) / (16 / 24)]]])
    np.testing.assert_allclose(got["ratio"], want, rtol=1e-15)
    np.testing.assert_array_equal(got["interaction"], np.array([[[0.25, 0.75], [0.375, 0.625]]]))
    # a label without pairs: its row and its column have no ratio
    count = np.array([[[4, 0], [0, 0]]], dtype=np.int64)
    r = assemble_cooccurrence(count, np.array([4, 4]), 8, [4], [4])["ratio"]
    assert r[0, 0, 0] == 1.0 and np.isnan(r[0, 0, 1]) and np.isnan(r[0, 1]).all()


# ---------------------------------------------------------------- moments per band against enumeration
@pytest.mark.parametrize("seed,n,C", [(2, 7, 2), (3, 8, 2), (4, 7, 3)])
def test_band_moments_against_enumeration(seed, n, C):
    from flashdeconv_amd.utils.cooccurrence import assemble_cooccurrence
    t = _tiny_case(seed, n=n, C=C, leave_out=seed == 4)
    for mode in ("band", "cumulative"):
        got = assemble_cooccurrence(t["obs"], t["na"], n, t["W"], t["sds"], t["sds_cum"], mode=mode)
        for b in range(2):
            A = t["A"][b] if mode == "band" or b == 0 else t["A"][0] + t["A"][1]
            if A.nnz == 0:
                assert np.isnan(got["expected"][b]).all()
                continue
            E0, V0 = nhood_ref.moments_by_enumeration(A, t["labels"], C)
            assert np.all(np.abs(got["expected"][b] - E0) <= 1e-12 * np.maximum(1.0, np.abs(E0))), (mode, b)
            assert np.all(np.abs(got["variance"][b] - V0) <= 1e-12 * np.maximum(1.0, np.abs(V0))), (mode, b)


# ---------------------------------------------------------------- requests and argument checks
def test_request():
    from flashdeconv_amd.utils.cooccurrence import cooccurrence_request
    assert cooccurrence_request(False) is None and cooccurrence_request(None) is None and cooccurrence_request(np.bool_(False)) is None
    assert cooccurrence_request(True) == {} and cooccurrence_request(3) == {"n_bands": 3} and cooccurrence_request(np.int64(32)) == {"n_bands": 32}
    assert cooccurrence_request([1, 2.5]) == {"radii": [1.0, 2.5]} and cooccurrence_request(np.array([0.5])) == {"radii": [0.5]}
    for bad in (0, 33, -1):
        with pytest.raises(ValueError, match="n_bands"):
            cooccurrence_request(bad)
    for bad in ("3", 2.5, b"x"):
        with pytest.raises(ValueError, match="co_occurrence must be a bool, a number of bands or a sequence of radii"):
            cooccurrence_request(bad)
    for bad, match in (([], "non-empty"), ([2.0, 1.0], "strictly ascending"), ([0.0, 1.0], "positive"), ([1.0, np.inf], "finite"),
                       (list(range(1, 34)), "at most 32")):
        with pytest.raises(ValueError, match=match):
            cooccurrence_request(bad)


def test_argument_checks_come_before_the_gpu(monkeypatch):
    from flashdeconv_amd import _lib
    from flashdeconv_amd.utils import cooccurrence as co

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_gpu)
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    n = 6
    coords = np.arange(2.0 * n).reshape(n, 2)
    labels = np.array([0, 1, 0, 1, -1, 2])
    radii = [1.0, 2.0]
    calls = (lambda l, c=coords, **kw: co.label_cooccurrence(l, c, radii, **kw), lambda l, c=coords, **kw: co.label_band_counts(l, c, radii, **kw))
    for call in calls:
        with pytest.raises(ValueError, match="labels has 5 rows but coords has 6"):
            call(labels[:5])
        with pytest.raises(ValueError, match="non-empty 1-D"):
            call(labels.reshape(2, 3))
        for bad in (labels.astype(np.float64), labels > 0):
            with pytest.raises(TypeError, match="labels must be integers"):
                call(bad)
        with pytest.raises(ValueError, match=r"labels must lie in \[-1, 2\)"):
            call(labels, n_labels=2)
        with pytest.raises(ValueError, match="at most 64 labels"):
            call(np.array([0, 1, 0, 1, 0, 64]))
        for bad in (0, 65, True):
            with pytest.raises(ValueError, match="n_labels must be an int from 1 to 64"):
                call(labels, n_labels=bad)
        with pytest.raises(ValueError, match="coords must be 2D"):
            call(labels, np.arange(6.0))
        with pytest.raises(ValueError, match="built for 1 to 3 coordinate dimensions"):
            call(labels, np.zeros((n, 4)))
        for bad in (-1, 2.5, True):
            with pytest.raises(ValueError, match="n_permutations must be an int >= 0"):
                call(labels, n_permutations=bad)
        for bad in (0, -3, 1.5):
            with pytest.raises(ValueError, match="max_candidates must be an int >= 1"):
                call(labels, max_candidates=bad)
        for bad in (1, "yes", None):
            with pytest.raises(ValueError, match="return_null must be True or False"):
                call(labels, return_null=bad)
    for bad, match in (([], "non-empty"), ([2.0, 1.0], "strictly ascending"), ([-1.0], "positive"), (list(range(1, 34)), "at most 32")):
        for fn in (co.label_cooccurrence, co.label_band_counts):
            with pytest.raises(ValueError, match=match):
                fn(labels, coords, bad)
    with pytest.raises(ValueError, match="Unknown mode"):
        co.label_cooccurrence(labels, coords, radii, mode="ring")
    with pytest.raises(ValueError, match="n_bands"):
        co.label_cooccurrence(labels, coords, n_bands=0)
    with pytest.raises(ValueError, match="random_state must be in"):
        co.label_cooccurrence(labels, coords, radii, random_state=-1)
    for name in ("first_perm", "max_batch", "max_bands_per_pass", "max_blocks"):
        with pytest.raises(ValueError, match=name + " must be an int >= 0"):
            co.label_band_counts(labels, coords, radii, **{name: -1})
    with pytest.raises(ValueError, match="degree must be True or False"):
        co.label_band_counts(labels, coords, radii, degree=1)


def test_model_and_deconvolve_checks():
    from flashdeconv_amd import FlashDeconv, tl
    m = FlashDeconv()
    coords = np.zeros((4, 2))
    for kw in ({}, {"n_niches": 3}, {"labels": np.zeros(4, dtype=np.int64)}):
        with pytest.raises(RuntimeError, match=r"Model has not been fitted\. Call fit\(\) first\."):
            m.get_co_occurrence(coords, **kw)
    for bad in ("3", 2.5, 0, 33, [2.0, 1.0], []):
        with pytest.raises(ValueError):                                                        # before the data is looked at
            tl.deconvolve(None, None, co_occurrence=bad)


# ---------------------------------------------------------------- the entry and the signatures
def test_entry_is_declared_exported_and_bound():
    from flashdeconv_amd import FlashDeconv, _lib, tl, utils
    text = open(os.path.join(ROOT, "include", "fdx.h")).read()
    name = "fdx_label_cooccurrence_dev"
    decl = re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert decl is not None
    res, args = _lib.SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == len(decl.group(1).split(",")) == 27
    assert args[1] is ctypes.c_int64 and args[4] is ctypes.c_int32 and args[7] is ctypes.c_uint64 and args[13] is ctypes.c_int64
    assert callable(getattr(_lib.load(), name))
    assert name + "(" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    makefile = open(os.path.join(ROOT, "flashdeconv_amd", "csrc", "Makefile")).read()
    light = re.search(r"^LIGHT = (.*)$", makefile, re.M).group(1).split()
    assert "label_band_kernels.cpp" in light
    for fn in ("label_cooccurrence", "label_band_counts", "assemble_cooccurrence"):
        assert fn in utils.__all__ and callable(getattr(utils, fn)) and fn in utils.__doc__
    sig = inspect.signature(utils.label_cooccurrence).parameters
    assert list(sig) == ["labels", "coords", "radii", "n_bands", "n_labels", "n_permutations", "random_state", "mode", "max_candidates",
                         "return_null"]
    assert (sig["radii"].default is None and sig["n_bands"].default == 10 and sig["n_permutations"].default == 999
            and sig["random_state"].default == 0 and sig["mode"].default == "band" and sig["return_null"].default is False)
    sig = inspect.signature(utils.label_band_counts).parameters
    assert list(sig) == ["labels", "coords", "radii", "n_labels", "seed", "first_perm", "n_permutations", "max_batch",
                         "max_bands_per_pass", "max_blocks", "max_candidates", "degree", "return_null"]
    assert all(sig[k].default == 0 for k in ("seed", "first_perm", "n_permutations", "max_batch", "max_bands_per_pass", "max_blocks"))
    assert "mode" in inspect.signature(utils.assemble_cooccurrence).parameters
    sig = inspect.signature(FlashDeconv.get_co_occurrence).parameters
    assert list(sig)[:8] == ["self", "coords", "labels", "n_niches", "radii", "n_bands", "n_permutations", "random_state"]
    assert sig["n_bands"].default == 10 and sig["n_permutations"].default == 999 and sig["random_state"].default is None
    params = list(inspect.signature(tl.deconvolve).parameters)
    assert params[-1] == "co_occurrence" and inspect.signature(tl.deconvolve).parameters["co_occurrence"].default is False


def test_entry_without_spots_and_its_refusals_need_no_gpu():
    """n = 0 returns zeros (every N^r equals N = 0: count_ge = count_le = n_perm) before anything is queued, and the argument checks
    of the C entry come before its first launch: both run on a machine without a GPU."""
    from flashdeconv_amd import _lib
    lib = _lib.load()
    C, B, R = 3, 2, 5
    X = B * C * C

    def call(n=0, dim=2, C=C, radii=(1.0, 2.0), first=0, n_perm=R, caps=(0, 0, 0), max_candidates=0):
        r = np.asarray(radii, dtype=np.float64)
        na, pair, deg = np.full(C, -1, dtype=np.int64), np.full(X, -1, dtype=np.int64), np.full(3 * B, -1, dtype=np.int64)
        ge, le = np.full(2 * X, -1, dtype=np.int64), np.full(2 * X, -1, dtype=np.int64)
        sd, sq = np.full(2 * X, -1.0), np.full(2 * X, -1.0)
        batch, bpp, cand = np.full(1, -1, dtype=np.int32), np.full(1, -1, dtype=np.int32), np.full(1, -1, dtype=np.int64)
        rc = lib.fdx_label_cooccurrence_dev(None, n, dim, None, C, _lib.ptr_f64(r), r.size, ctypes.c_uint64(1), first, n_perm, caps[0],
                                            caps[1], caps[2], max_candidates, None, None, _lib.ptr_i64(na), _lib.ptr_i64(pair),
                                            _lib.ptr_i64(deg), _lib.ptr_i64(ge), _lib.ptr_i64(le), _lib.ptr_f64(sd), _lib.ptr_f64(sq),
                                            _lib.ptr_i32(batch), _lib.ptr_i32(bpp), _lib.ptr_i64(cand), None)
        return rc, (na, pair, deg, ge, le, sd, sq, batch, bpp, cand)

    rc, (na, pair, deg, ge, le, sd, sq, batch, bpp, cand) = call()
    assert rc == 0
    assert not na.any() and not pair.any() and not deg.any() and not sd.any() and not sq.any()
    assert np.all(ge == R) and np.all(le == R)
    assert batch[0] == 0 and bpp[0] == 0 and cand[0] == 0
    for kw, msg in ((dict(n=-1), "n must be between 0 and 2\\^31 - 129"), (dict(n=(1 << 31) - 128), "n must be between"),
                    (dict(n=4), "null argument"), (dict(dim=0), "dimension must be 1, 2 or 3"), (dict(dim=4), "dimension must be"),
                    (dict(radii=()), "between 1 and 32 radii"),
                    (dict(radii=tuple(range(1, 34))), "between 1 and 32 radii"), (dict(radii=(2.0, 1.0)), "strictly ascending"),
                    (dict(radii=(0.0, 1.0)), "strictly ascending"), (dict(radii=(1.0, np.inf)), "strictly ascending"),
                    (dict(first=-1), "must not be negative"), (dict(n_perm=-1), "must not be negative"),
                    (dict(caps=(-1, 0, 0)), "must not be negative"), (dict(caps=(0, -1, 0)), "must not be negative"),
                    (dict(caps=(0, 0, -1)), "must not be negative"), (dict(max_candidates=-1), "must not be negative")):
        rc, _ = call(**kw)
        assert rc != 0, kw
        with pytest.raises(_lib.FdxError, match="fdx_label_cooccurrence_dev: .*" + msg):
            _lib.check(rc)
    for bad in (0, 65):                                            # (apart: the output arrays are sized by C)
        r = np.array([1.0])
        big = np.zeros(2 * 65 * 65, dtype=np.int64)
        rc = lib.fdx_label_cooccurrence_dev(None, 0, 2, None, bad, _lib.ptr_f64(r), 1, ctypes.c_uint64(1), 0, 0, 0, 0, 0, 0, None, None,
                                            _lib.ptr_i64(big), _lib.ptr_i64(big), _lib.ptr_i64(big), _lib.ptr_i64(big), _lib.ptr_i64(big),
                                            _lib.ptr_f64(big.astype(np.float64)), _lib.ptr_f64(big.astype(np.float64)), None, None, None, None)
        with pytest.raises(_lib.FdxError, match="the number of labels must be between 1 and 64"):
            _lib.check(rc)


# ---------------------------------------------------------------- the precondition of the bit-for-bit null sums
def test_null_sums_of_the_gpu_cases_are_exact_in_any_order():
    """Every d = N^r - N is an integer with |d| <= max Wcum, so R terms of d^2 sum to at most R max(Wcum)^2: below 2^53 every
    partial sum is an exactly representable integer, the float64 sums do not depend on their order, and comparing them bit for
    bit with the reference's is legitimate."""
    cases = [(name, max(ref.NULL_R)) for name in ref.NULL_SETS] + [(ref.LONG_CASE[0], ref.LONG_CASE[2])]
    cases += [(name, R) for name, _, R in ref.CAPS_CASES]
    for name, R in cases:
        wcum = ref.null_case_wcum(name)
        print(f"{name}: R = {R}, max Wcum = {wcum}, R Wcum^2 = {R * wcum * wcum:.3g}")
        assert R * wcum * wcum < 2 ** 53, (name, R, wcum)
