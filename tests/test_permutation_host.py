"""CPU-only tests of what the four permutation tests share (utils._permutation): that the four assemblers rank an observed
statistic against its null by one rule, bit for bit; that the rule gives the same bits in NumPy and in torch; the one spelling of
a permutation's key; and the splitting of R permutations into calls."""
import numpy as np
import pytest

R_LIST = [1, 2, 99, 999]
RANK_KEYS = ("p_greater", "p_less", "p_value", "z_sim")
RANK_NAMES = ("p_greater", "p_less", "p_value", "mean_d", "std_d", "z_sim")      # what rank_against_null returns, in order
M = 18                                                          # cases per R: two (3, 3) blocks


def _mix64_py(x):
    """The splitmix64 finaliser in Python integers."""
    m = (1 << 64) - 1
    x &= m
    x ^= x >> 30
    x = (x * 0xbf58476d1ce4e5b9) & m
    x ^= x >> 27
    x = (x * 0x94d049bb133111eb) & m
    return x ^ (x >> 31)


def _cases(R):
    """(count_ge, count_le, sum_d, sumsq_d), float64 (M,): three hand-picked rows - all ties, never reached, a variance that rounds
    below zero - then random counts in [0, R] with sums of a null that varies."""
    rng = np.random.RandomState(1000 + R)
    ge = rng.randint(0, R + 1, size=M).astype(np.float64)
    le = rng.randint(0, R + 1, size=M).astype(np.float64)
    sd = rng.standard_normal(M) * R
    sq = sd * sd / R + R * rng.uniform(0.1, 2.0, size=M)
    ge[0], le[0], sd[0], sq[0] = R, R, 0.0, 0.0
    ge[1], le[1], sd[1], sq[1] = 0, R, -2.0 * R, 5.0 * R
    sd[2] = 0.3 * R
    mean = sd[2] / np.float64(R)
    sq[2] = mean * mean * R
    while not sq[2] / np.float64(R) - mean * mean < 0:
        sq[2] = np.nextafter(sq[2], 0.0)
    return ge, le, sd, sq


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


@pytest.fixture(scope="module", params=R_LIST)
def ranked(request):
    """(R, the four inputs, what ``rank_against_null`` makes of them in NumPy)."""
    from flashdeconv_amd.utils._permutation import rank_against_null
    R = request.param
    cases = _cases(R)
    with np.errstate(divide="ignore", invalid="ignore"):
        want = rank_against_null(np, *cases, R)
    return R, cases, dict(zip(RANK_KEYS, want[:3] + want[5:]))


def test_the_cases_hold_the_degenerate_rows(ranked):
    R, (ge, le, sd, sq), want = ranked
    assert want["p_greater"][0] == 1.0 and want["p_less"][0] == 1.0 and want["p_value"][0] == 1.0 and np.isnan(want["z_sim"][0])
    assert want["p_greater"][1] == 1.0 / (R + 1.0) and want["p_value"][1] == min(1.0, 2.0 / (R + 1.0)) and want["z_sim"][1] == 2.0
    assert sq[2] / np.float64(R) - (sd[2] / np.float64(R)) ** 2 < 0 and np.isnan(want["z_sim"][2])
    assert np.all(np.isfinite(want["z_sim"][3:])) and np.all((want["p_value"] > 0) & (want["p_value"] <= 1))


@pytest.mark.parametrize("K", [1, 3])
def test_assemble_permutation_applies_the_shared_rule(ranked, K):
    from flashdeconv_amd.utils.spatial_stats import assemble_permutation
    R, cases, want = ranked
    KK = K * K
    m2 = np.linspace(1.0, 2.0, K)                               # no dead column: the module's own mask is off everywhere
    C = np.arange(KK, dtype=np.float64).reshape(K, K) - 1.0
    for at in range(0, M, KK):
        got = assemble_permutation(10, 20, m2, C, *(a[at:at + KK].reshape(K, K) for a in cases), R)
        for key in RANK_KEYS:
            assert _same(got["cross_" + key], want[key][at:at + KK].reshape(K, K)), (key, at)
            assert _same(got[key], np.diagonal(got["cross_" + key])), key


def test_assemble_local_applies_the_shared_rule(ranked):
    from flashdeconv_amd.utils.local_stats import assemble_local
    R, cases, want = ranked
    rng = np.random.RandomState(5)
    V = rng.standard_normal((M, 1))
    S = rng.standard_normal((M, 1))
    deg = np.full(M, 2, dtype=np.int32)                         # no isolated spot: the module's own mask is off everywhere
    got = assemble_local(V, S, deg, V.mean(0), ((V - V.mean(0)) ** 2).sum(0), M, 2 * M, *(a.reshape(M, 1) for a in cases),
                         n_permutations=R)
    for key in RANK_KEYS:
        assert _same(got[key], want[key].reshape(M, 1)), key
    Z = V - V.mean(0)
    own = np.where(Z > 0, got["p_greater"], np.where(Z < 0, got["p_less"], 1.0))
    assert _same(got["local_i_p_greater"], own)


def test_assemble_enrichment_applies_the_shared_rule(ranked):
    from flashdeconv_amd.utils.neighborhoods import assemble_enrichment
    R, cases, want = ranked
    count = np.arange(9, dtype=np.int64).reshape(3, 3)
    for at in range(0, M, 9):
        got = assemble_enrichment(count, np.array([4, 5, 6]), 20, 60, 200, *(a[at:at + 9].reshape(3, 3) for a in cases), R)
        for key in RANK_KEYS:
            assert _same(got[key], want[key][at:at + 9].reshape(3, 3)), (key, at)
        assert _same(got["null_mean"], count + cases[2][at:at + 9].reshape(3, 3) / np.float64(R))


def test_the_gene_assembler_uses_the_shared_p_and_moments(ranked):
    from flashdeconv_amd.utils._permutation import null_moments, p_from_count
    from flashdeconv_amd.utils.gene_permutations import assemble_gene_permutation
    R, (ge, le, s, sq), _ = ranked
    rng = np.random.RandomState(6)
    n, W = 50, 200
    y = rng.standard_normal((n, M))                             # no constant gene: nothing is dead
    u, q = y.sum(0), (y * y).sum(0)
    D, H, P = 4.0 * u, 4.0 * q, rng.standard_normal(M)
    counts = {"count_ge": ge.astype(np.int64), "count_le": le.astype(np.int64), "count_c_le": le[::-1].astype(np.int64),
              "sum_i": s, "sumsq_i": sq, "n_permutations": R}
    got = assemble_gene_permutation(n, W, u, q, D, H, P, y.min(0), y.max(0), counts=counts)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean, std = null_moments(np, s, sq, R)
    assert _same(got["p_sim"], p_from_count(np, ge, R)) and _same(got["p_sim_less"], p_from_count(np, le, R))
    assert _same(got["gearys_p_sim"], p_from_count(np, le[::-1].copy(), R))
    assert _same(got["null_mean"], mean) and _same(got["null_std"], std)
    assert np.array_equal(np.isnan(got["z_sim"]), ~(std > 0))


def _bits_differ(a, b):
    return np.ascontiguousarray(a).view(np.int64) != np.ascontiguousarray(b).view(np.int64)


def _both_namespaces(R, cases):
    import torch
    from flashdeconv_amd.utils._permutation import rank_against_null
    with np.errstate(divide="ignore", invalid="ignore"):
        want = rank_against_null(np, *cases, R)
    got = rank_against_null(torch, *(torch.from_numpy(a.copy()) for a in cases), R)
    assert len(got) == len(want) == 6 and all(g.dtype == torch.float64 and g.shape == w.shape for w, g in zip(want, got))
    return dict(zip(RANK_NAMES, want)), {k: g.numpy() for k, g in zip(RANK_NAMES, got)}


def test_rank_against_null_gives_the_same_bits_in_numpy_and_torch(ranked):
    """All six outputs, NumPy against torch on CPU float64 tensors, bit for bit."""
    R, cases, _ = ranked
    want, got = _both_namespaces(R, cases)
    differing = {k: int(_bits_differ(want[k], got[k]).sum()) for k in RANK_NAMES}
    assert not any(differing.values()), differing


def test_the_square_root_is_numpys_for_cpu_tensors():
    """Enough arguments that torch's own CPU square root differs from NumPy's on some of them, whatever the vector path."""
    import torch
    from flashdeconv_amd.utils._permutation import _sqrt
    v = np.random.RandomState(0).uniform(0.0, 3.0, 100003)
    v[:3] = 0.0, np.inf, np.nan
    for arr in (v, v[:18], v[::3]):
        got = _sqrt(torch, torch.from_numpy(arr))
        assert got.dtype == torch.float64 and not _bits_differ(got.numpy(), np.sqrt(arr)).any()
    assert not _bits_differ(_sqrt(np, v), np.sqrt(v)).any()


def test_the_rule_equals_its_plain_python_evaluation(ranked):
    import math
    from flashdeconv_amd.utils._permutation import rank_against_null
    R, (ge, le, sd, sq), _ = ranked
    with np.errstate(divide="ignore", invalid="ignore"):
        got = dict(zip(RANK_NAMES, rank_against_null(np, ge, le, sd, sq, R)))
    for i in range(M):
        greater, less = (1.0 + float(ge[i])) / (R + 1.0), (1.0 + float(le[i])) / (R + 1.0)
        mean = float(sd[i]) / R
        std = math.sqrt(max(float(sq[i]) / R - mean * mean, 0.0))
        row = {"p_greater": greater, "p_less": less, "p_value": min(1.0, 2.0 * min(greater, less)), "mean_d": mean, "std_d": std,
               "z_sim": -mean / std if std > 0 else math.nan}
        for k in RANK_NAMES:
            assert not _bits_differ(np.float64(row[k]), got[k][i]).any(), (k, i)


@pytest.mark.parametrize("seed", [0, 17, 2 ** 64 - 1])
@pytest.mark.parametrize("r", [0, 1, 2 ** 40])
def test_permutation_key_is_the_key_behind_permutation_indices(seed, r):
    from flashdeconv_amd.utils._permutation import _keyed_bijection, permutation_indices, permutation_key
    key = permutation_key(seed, r)
    assert key == _mix64_py(_mix64_py(seed) + (r + 1) * 0x9e3779b97f4a7c15)
    for n in (5, 257):
        assert np.array_equal(permutation_indices(seed, r, n), _keyed_bijection(key, np.arange(n, dtype=np.uint64), n))


def test_conditional_indices_derives_its_key_from_permutation_key():
    from flashdeconv_amd.utils._permutation import _keyed_bijection, permutation_key
    from flashdeconv_amd.utils.local_stats import conditional_indices
    seed, r, spot, n, count = 17, 3, 4, 100, 9
    key = _mix64_py(permutation_key(seed, r) + (spot + 1) * 0x9e3779b97f4a7c15)
    c = _keyed_bijection(key, np.arange(count + 1, dtype=np.uint64), n)
    assert np.array_equal(conditional_indices(seed, r, spot, n, count), c[c != spot][:count])


@pytest.mark.parametrize("R, chunk", [(0, 5), (1, 1), (10, 3), (10, 10), (10, 99)])
def test_permutation_chunks_are_ordered_and_sum_to_R(R, chunk):
    from flashdeconv_amd.utils._permutation import permutation_chunks
    calls = list(permutation_chunks(R, chunk))
    if R == 0:
        assert calls == [(0, 0)]
        return
    assert sum(cnt for _, cnt in calls) == R and len(calls) == -(-R // chunk)
    at = 0
    for done, cnt in calls:
        assert done == at and 1 <= cnt <= chunk
        at += cnt
    assert all(cnt == chunk for _, cnt in calls[:-1]) and calls[-1][1] == R - chunk * (len(calls) - 1)   # only the last is ragged


def test_check_permutation_counts_speaks_as_check_count():
    from flashdeconv_amd.utils._device import check_count
    from flashdeconv_amd.utils._permutation import check_permutation_counts
    assert check_permutation_counts(np.int64(5)) == (5, 0, 0) and check_permutation_counts(0, 3, 7) == (0, 3, 7)
    for name, args in (("n_permutations", (-1, 0, 0)), ("first_perm", (1, 2.0, 0)), ("max_batch", (1, 0, True))):
        with pytest.raises(ValueError) as ours:
            check_permutation_counts(*args)
        with pytest.raises(ValueError) as theirs:
            check_count(name, args[("n_permutations", "first_perm", "max_batch").index(name)])
        assert str(ours.value) == str(theirs.value)


def test_the_definition_has_one_home():
    from flashdeconv_amd import utils
    from flashdeconv_amd.utils import _permutation, spatial_stats
    assert spatial_stats.permutation_indices is _permutation.permutation_indices
    assert utils.permutation_indices is _permutation.permutation_indices
    assert spatial_stats._permutation_seed is _permutation._permutation_seed
    assert spatial_stats._NULL_CALL_BYTES == _permutation._NULL_CALL_BYTES
