"""NumPy reference of the label co-occurrence by distance band (utils.cooccurrence, csrc/label_band_kernels.cpp), shared by
tests/test_cooccurrence_host.py and tests/test_gpu_cooccurrence.py.

    the band adjacencies A_b   correlogram_ref.band_reference(...)["A"] (brute force over all ordered pairs, the device's distance)
    N_b                        nhood_ref.pair_counts(A_b, labels, C);  Ncum_b = sum_{b' <= b} N_{b'}
    the null                   the same of labels[permutation_indices(seed, r, n)], r = first .. first + R - 1
    the accumulation           nhood_ref.accumulate per band, of the band counts and of the cumulative counts, in permutation order
    the degrees                deg (n, B) of the band adjacencies; sum_deg_sq_cum from the cumulative degree
"""
import functools

import numpy as np

import correlogram_ref as cr
import nhood_ref

C_LIST = (1, 2, 16, 17, 32, 33, 64)
KINDS = ("random", "minus", "missing", "one", "none")

# the GPU null cases: (coordinate set, C, R) - every R of a set shares the longest null
NULL_SETS = ("square23", "ragged2", "cube8")
NULL_C = (5, 64)
NULL_R = (7, 8, 9, 15, 16, 17, 64)
NULL_SEED = 7
LONG_CASE = ("square23", 5, 999)
CAPS_CASES = (("square32_B10", 5, 40), ("cloud257", 5, 40), ("ragged2", 5, 40), ("ragged2", 64, 40))


def make_labels(n, C, kind, seed=0):
    """The label kinds of tests/test_gpu_nhood.py (_labels), restated."""
    rs = np.random.RandomState(1000 * C + seed)
    if kind == "random":
        lab = rs.randint(0, C, n)
    elif kind == "minus":                                  # about 10 % left out
        lab = rs.randint(0, C, n)
        lab[rs.rand(n) < 0.1] = -1
    elif kind == "missing":                                # label C // 2 never occurs (C = 1: nobody is labelled)
        lab = rs.randint(0, C, n)
        lab[lab == C // 2] = (C // 2 + 1) % C if C > 1 else -1
    elif kind == "one":                                    # every spot in the last label
        lab = np.full(n, C - 1)
    else:                                                  # every spot left out
        lab = np.full(n, -1)
    return lab.astype(np.int64)


@functools.lru_cache(maxsize=None)
def _sets():
    return cr.coord_sets()


@functools.lru_cache(maxsize=None)
def geometry(name):
    """Of a coordinate set of correlogram_ref.coord_sets(): coords, radii, the band adjacencies A (list of B CSR), deg (n, B) int64,
    W, sum_deg_sq, sum_deg_sq_cum (B,) int64.  Computed once and shared; the arrays are read-only."""
    coords, radii = _sets()[name]
    n = coords.shape[0]
    ref = cr.band_reference(np.zeros((n, 1)), coords, radii)
    deg = ref["deg"]
    cum = np.cumsum(deg, axis=1)
    out = {"coords": coords, "radii": radii, "n": n, "A": ref["A"], "deg": deg, "W": ref["W"].astype(np.int64),
           "sum_deg_sq": ref["sum_deg_sq"].astype(np.int64), "sum_deg_sq_cum": (cum * cum).sum(0).astype(np.int64)}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def band_counts(A, labels, C):
    """(B, C, C) int64: N_b for every band adjacency of A."""
    return np.stack([nhood_ref.pair_counts(a, labels, C) for a in A])


def null_counts(A, labels, C, seed, first, R):
    """(R, B, C, C) int64: N^r_b for r = first .. first + R - 1."""
    from flashdeconv_amd.utils.spatial_stats import permutation_indices
    labels = np.asarray(labels)
    n = labels.shape[0]
    out = np.zeros((R, len(A), C, C), dtype=np.int64)
    for j in range(R):
        out[j] = band_counts(A, labels[permutation_indices(seed, first + j, n)], C)
    return out


@functools.lru_cache(maxsize=None)
def shared_null(name, C, kind, seed, first, R):
    """null_counts of a coordinate set with make_labels(n, C, kind), computed once; read-only."""
    g = geometry(name)
    null = null_counts(g["A"], make_labels(g["n"], C, kind), C, seed, first, R)
    null.setflags(write=False)
    return null


def accumulate(null, obs):
    """{count_ge, count_le, sum_d, sumsq_d, and the four with _cum} (B, C, C) of a null (R, B, C, C) against obs (B, C, C): per band
    nhood_ref.accumulate of the band counts and of the running sums over bands, in permutation order."""
    B = obs.shape[0]
    out = {}
    for tail, nl, ob in (("", null, obs), ("_cum", np.cumsum(null, axis=1), np.cumsum(obs, axis=0))):
        per_band = [nhood_ref.accumulate(nl[:, b], ob[b]) for b in range(B)]
        for k, key in enumerate(("count_ge", "count_le", "sum_d", "sumsq_d")):
            out[key + tail] = np.stack([per_band[b][k] for b in range(B)])
    return out


def null_case_wcum(name):
    """max_b Wcum_b of a coordinate set: what the exactness of the float64 sums of a null case depends on."""
    return int(np.cumsum(geometry(name)["W"]).max())
