"""CPU-only tests of the neighbourhood enrichment (utils.neighborhoods): the exact join-count moments against enumeration of all
permutations, the quality of the keyed-bijection null against those moments (on the NumPy reference alone), the host assembly, the
argument checks that come before anything touches the GPU, and the C entry's declaration, export and binding."""
import ctypes
import functools
import inspect
import os
import re

import numpy as np
import pytest
from scipy import sparse

from conftest import ROOT

import nhood_ref as ref


# ---------------------------------------------------------------- moments against enumeration
# (n, C, labels): one case has a label of count 1 (n = 7, C = 3), one leaves a spot out (-1)
ENUM_CASES = [(7, 1, [0] * 7), (7, 2, [0, 1, 0, 0, 1, 1, 0]), (7, 3, [0, 1, 2, 0, 1, 0, 1]), (7, 4, [0, 1, 2, 3, 0, 1, 2]),
              (8, 2, [0, 1, 1, 0, 1, 0, 0, 1]), (7, 2, [0, 1, -1, 0, 1, 1, 0])]


@pytest.mark.parametrize("n,C,labels", ENUM_CASES)
def test_moments_against_enumeration(n, C, labels):
    from flashdeconv_amd.utils.neighborhoods import join_count_moments
    rs = np.random.RandomState(10 * n + C)
    A = ref.random_graph(rs, n)
    labels = np.array(labels)
    n_, W, sdeg2 = ref.graph_counts(A)
    E, V = join_count_moments(n_, W, sdeg2, ref.label_counts(labels, C))
    E0, V0 = ref.moments_by_enumeration(A, labels, C)
    Er, Vr = ref.moments(n_, W, sdeg2, ref.label_counts(labels, C))
    print(f"n {n} C {C}: max |E - enum| {np.abs(E - E0).max():.3g}, max |Var - enum| {np.abs(V - V0).max():.3g}")
    assert np.all(np.abs(E - E0) <= 1e-12 * np.maximum(1.0, np.abs(E0)))
    assert np.all(np.abs(V - V0) <= 1e-12 * np.maximum(1.0, np.abs(V0)))
    assert np.all(np.abs(E - Er) <= 1e-12 * np.maximum(1.0, np.abs(Er))) and np.all(np.abs(V - Vr) <= 1e-12 * np.maximum(1.0, np.abs(Vr)))
    # a count that cannot vary has variance exactly 0: no z score from rounding noise
    assert np.all(V[V0 == 0] == 0)


def test_moments_nan_rules_and_checks():
    from flashdeconv_amd.utils.neighborhoods import join_count_moments
    for n, W, na in ((3, 4, [1, 2]), (2, 2, [1, 1]), (0, 0, [0, 0]), (10, 0, [4, 6])):
        E, V = join_count_moments(n, W, 8, np.array(na))
        assert E.shape == V.shape == (2, 2) and np.isnan(E).all() and np.isnan(V).all()
    E, V = join_count_moments(4, 6, 10, np.array([2, 2]))
    assert np.isfinite(E).all() and np.isfinite(V).all()
    with pytest.raises(ValueError, match="label_counts must be a non-empty 1-D integer array"):
        join_count_moments(10, 4, 8, np.array([0.5, 1.0]))
    with pytest.raises(ValueError, match="sum to at most n"):
        join_count_moments(5, 4, 8, np.array([3, 3]))


# ---------------------------------------------------------------- the null against the exact moments (reference alone)
@functools.lru_cache(maxsize=None)
def _slide():
    rs = np.random.RandomState(0)
    n = 1000
    coords = rs.rand(n, 2)
    A = ref.knn_graph(coords, 6)
    labels = rs.randint(0, 5, n)
    return coords, A, labels


def test_null_matches_the_exact_moments():
    _, A, labels = _slide()
    C, R = 5, 999
    n, W, sdeg2 = ref.graph_counts(A)
    E, V = ref.moments(n, W, sdeg2, ref.label_counts(labels, C))
    null = ref.null_counts(A, labels, C, 7, 0, R).astype(np.float64)
    mean, var = null.mean(0), null.var(0)
    dev = np.abs(mean - E) / np.sqrt(V / R)
    ratio = var / V
    print(f"max |null_mean - E| / sqrt(Var / R) = {dev.max():.3f}; null_var / Var in [{ratio.min():.4f}, {ratio.max():.4f}]")
    assert np.all(dev <= 5.0)
    assert np.all((ratio >= 0.8) & (ratio <= 1.25))


def test_striped_labels_are_enriched_on_the_diagonal():
    from flashdeconv_amd.utils.neighborhoods import assemble_enrichment
    coords, A, _ = _slide()
    C = 5
    labels = np.minimum((coords[:, 0] * C).astype(np.int64), C - 1)
    n, W, sdeg2 = ref.graph_counts(A)
    out = assemble_enrichment(ref.pair_counts(A, labels, C), ref.label_counts(labels, C), n, W, sdeg2)
    z = np.diagonal(out["z_score"])
    print("analytic z of the diagonal:", np.round(z, 1))
    assert np.all(z > 10)


# ---------------------------------------------------------------- assembly
def test_assemble_enrichment():
    from flashdeconv_amd.utils.neighborhoods import assemble_enrichment
    rs = np.random.RandomState(3)
    n, C, R = 60, 4, 23
    A = ref.random_graph(rs, n, 0.1)
    labels = rs.randint(0, 3, n)                      # label 3 never occurs
    n_, W, sdeg2 = ref.graph_counts(A)
    obs, na = ref.pair_counts(A, labels, C), ref.label_counts(labels, C)
    null = ref.null_counts(A, labels, C, 5, 0, R)
    ge, le, sd, sq = ref.accumulate(null, obs)
    out = assemble_enrichment(obs, na, n_, W, sdeg2, ge, le, sd, sq, R)
    assert set(out) == {"count", "label_counts", "expected", "variance", "z_score", "interaction", "p_greater", "p_less", "p_value",
                        "null_mean", "null_std", "z_sim", "n_permutations"}
    assert out["n_permutations"] == R and np.array_equal(out["count"], obs) and np.array_equal(out["label_counts"], na)
    np.testing.assert_array_equal(out["p_greater"], (1.0 + (null >= obs).sum(0)) / (R + 1.0))
    np.testing.assert_array_equal(out["p_less"], (1.0 + (null <= obs).sum(0)) / (R + 1.0))
    np.testing.assert_array_equal(out["p_value"], np.minimum(1.0, 2.0 * np.minimum(out["p_greater"], out["p_less"])))
    np.testing.assert_allclose(out["null_mean"], null.mean(0), rtol=1e-13, atol=1e-12)
    np.testing.assert_allclose(out["null_std"], null.std(0), rtol=1e-9, atol=1e-9)
    E, V = ref.moments(n_, W, sdeg2, na)
    live = V > 1e-9
    np.testing.assert_allclose(out["z_score"][live], ((obs - E) / np.sqrt(np.where(live, V, 1.0)))[live], rtol=1e-10)
    # the label that never occurs: counts 0, variance 0, no z score of either kind, a p value of 1, no interaction row
    assert np.all(obs[3] == 0) and np.all(obs[:, 3] == 0)
    assert np.all(out["variance"][3] == 0) and np.all(out["variance"][:, 3] == 0)
    assert np.isnan(out["z_score"][3]).all() and np.isnan(out["z_score"][:, 3]).all()
    assert np.isnan(out["z_sim"][3]).all() and np.isnan(out["z_sim"][:, 3]).all() and np.all(out["null_std"][3] == 0)
    assert np.all(out["p_value"][3] == 1.0) and np.isnan(out["interaction"][3]).all()
    assert np.isfinite(out["z_sim"][:3, :3]).all() and np.isfinite(out["z_score"][:3, :3]).all()
    # interaction rows sum to 1 where the row has edges and nobody is labelled -1
    np.testing.assert_allclose(out["interaction"][:3].sum(1), 1.0, rtol=1e-14)
    np.testing.assert_array_equal(out["interaction"][:3], obs[:3] / obs[:3].sum(1, keepdims=True))
    # without permutations: the observed keys alone; the sums are then not needed
    plain = assemble_enrichment(obs, na, n_, W, sdeg2)
    assert set(plain) == {"count", "label_counts", "expected", "variance", "z_score", "interaction"}
    for k in plain:
        np.testing.assert_array_equal(plain[k], out[k])
    # every spot in one label: N_00 = W whatever the permutation - variance 0, NaN z scores, p = 1
    one = np.zeros(n, dtype=np.int64)
    obs1 = ref.pair_counts(A, one, 1)
    z = np.zeros((1, 1))
    out1 = assemble_enrichment(obs1, [n], n_, W, sdeg2, z + R, z + R, z, z, R)
    assert obs1[0, 0] == W and out1["variance"][0, 0] == 0 and np.isnan(out1["z_score"][0, 0]) and np.isnan(out1["z_sim"][0, 0])
    assert out1["p_value"][0, 0] == 1.0 and out1["interaction"][0, 0] == 1.0
    # shape and type checks
    with pytest.raises(ValueError, match=r"count must be \(C, C\)"):
        assemble_enrichment(obs[:, :3], na, n_, W, sdeg2)
    with pytest.raises(ValueError, match="integer array"):
        assemble_enrichment(obs.astype(np.float64), na, n_, W, sdeg2)
    with pytest.raises(ValueError, match="are needed when n_permutations >= 1"):
        assemble_enrichment(obs, na, n_, W, sdeg2, n_permutations=3)
    with pytest.raises(ValueError, match=r"must be \(C, C\)"):
        assemble_enrichment(obs, na, n_, W, sdeg2, ge[:2], le, sd, sq, R)


# ---------------------------------------------------------------- argument checks
def test_argument_checks_come_before_the_gpu(monkeypatch):
    from flashdeconv_amd import _lib
    from flashdeconv_amd.utils import neighborhoods as nh

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_gpu)
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    n = 6
    i = np.arange(n)
    ring = sparse.csr_matrix((np.ones(2 * n), (np.r_[i, i], np.r_[(i + 1) % n, (i - 1) % n])), shape=(n, n))
    labels = np.array([0, 1, 0, 1, -1, 2])
    calls = (lambda l, **kw: nh.neighborhood_enrichment(l, ring, **kw), lambda l, **kw: nh.label_pair_counts(l, ring, **kw))
    for call in calls:
        with pytest.raises(ValueError, match="5 rows but the graph has 6 spots"):             # wrong length
            call(labels[:5])
        with pytest.raises(ValueError, match="non-empty 1-D"):
            call(labels.reshape(2, 3))
        with pytest.raises(ValueError, match="non-empty 1-D"):
            call(labels[:0])
        for bad in (labels.astype(np.float64), labels.astype(np.float32), labels > 0, [0.5] * n):
            with pytest.raises(TypeError, match="labels must be integers"):                     # float (and bool) labels
                call(bad)
        with pytest.raises(ValueError, match=r"labels must lie in \[-1, 2\)"):                 # a label >= n_labels
            call(labels, n_labels=2)
        with pytest.raises(ValueError, match=r"labels must lie in \[-1, 3\)"):                 # a label < -1
            call(np.array([0, 1, 0, 1, -2, 2]))
        with pytest.raises(ValueError, match="at most 64 labels"):
            call(np.array([0, 1, 0, 1, 0, 64]))
        for bad in (0, 65, -1, 2.0, True, "3"):
            with pytest.raises(ValueError, match="n_labels must be an int from 1 to 64"):      # n_labels outside 1 .. 64
                call(labels, n_labels=bad)
        for bad in (-1, 2.5, True):
            with pytest.raises(ValueError, match="n_permutations must be an int >= 0"):
                call(labels, n_permutations=bad)
        for bad in (1, 0, "yes", None):
            with pytest.raises(ValueError, match="return_null must be True or False"):        # non-bool flags
                call(labels, return_null=bad)
    # the graph's own checks (_device.resolve_graph) are host-side too
    asym = ring.tolil()
    asym[0, 3] = 1.0
    with pytest.raises(ValueError, match="must be symmetric"):
        nh.label_pair_counts(labels, asym.tocsr())
    with pytest.raises(TypeError, match="graph must be"):
        nh.neighborhood_enrichment(labels, np.eye(n))
    with pytest.raises(ValueError, match="first_perm must be an int >= 0"):
        nh.label_pair_counts(labels, ring, first_perm=-1)
    with pytest.raises(ValueError, match="max_batch must be an int >= 0"):
        nh.label_pair_counts(labels, ring, max_batch=-1)
    with pytest.raises(ValueError, match="random_state must be in"):
        nh.neighborhood_enrichment(labels, ring, random_state=-1)
    # host labels of any integer dtype, lists among them, pass the checks as int32
    for good in (labels.astype(np.int8), labels.astype(np.int64), labels.astype(np.uint8) % 3, labels.tolist()):
        got_n, lab, C = nh.check_labels(good)
        assert got_n == n and lab.dtype == np.int32 and C == 3


def test_model_and_deconvolve_checks():
    from flashdeconv_amd import FlashDeconv, tl
    m = FlashDeconv()
    for kw in ({}, {"n_niches": 3}, {"labels": np.zeros(4, dtype=np.int64)}):
        with pytest.raises(RuntimeError, match=r"Model has not been fitted\. Call fit\(\) first\."):
            m.get_neighborhood_enrichment(**kw)
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="nhood_enrichment must be True or False"):        # before the data is looked at
            tl.deconvolve(None, None, nhood_enrichment=bad)


def test_entry_is_declared_exported_and_bound():
    from flashdeconv_amd import _lib, tl, utils
    text = open(os.path.join(ROOT, "include", "fdx.h")).read()
    name = "fdx_label_pair_counts_dev"
    decl = re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert decl is not None
    res, args = _lib.SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == len(decl.group(1).split(",")) == 17
    assert args[2] is ctypes.c_int32 and args[3] is ctypes.c_uint64 and args[4] is ctypes.c_int64 and args[6] is ctypes.c_int32
    assert callable(getattr(_lib.load(), name))
    for fn in ("neighborhood_enrichment", "label_pair_counts", "join_count_moments", "assemble_enrichment"):
        assert fn in utils.__all__ and callable(getattr(utils, fn))
    sig = inspect.signature(utils.neighborhood_enrichment).parameters
    assert list(sig) == ["labels", "graph", "n_labels", "n_permutations", "random_state", "return_null"]
    assert sig["n_permutations"].default == 999 and sig["random_state"].default == 0 and sig["return_null"].default is False
    sig = inspect.signature(utils.label_pair_counts).parameters
    assert list(sig) == ["labels", "graph", "n_labels", "seed", "first_perm", "n_permutations", "max_batch", "return_null"]
    assert inspect.signature(tl.deconvolve).parameters["nhood_enrichment"].default is False
    from flashdeconv_amd import FlashDeconv
    sig = inspect.signature(FlashDeconv.get_neighborhood_enrichment).parameters
    assert list(sig)[:5] == ["self", "labels", "n_niches", "n_permutations", "random_state"] and sig["n_permutations"].default == 999
    assert name + "(" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    makefile = open(os.path.join(ROOT, "flashdeconv_amd", "csrc", "Makefile")).read()
    light = re.search(r"^LIGHT = (.*)$", makefile, re.M).group(1).split()
    assert "label_pair_kernels.cpp" in light
