"""Reference of the local spatial statistics (tests/test_local_stats_host.py, tests/test_gpu_local_stats.py).  It imports nothing
from the package.

The draw, restated in plain Python integers from the docstring of flashdeconv_amd/utils/local_stats.py:
    mix64            the splitmix64 finaliser, modulo 2^64
    key_r            mix64(mix64(seed) + (r + 1) * GOLDEN)
    key              mix64(key_r + (spot + 1) * GOLDEN)
    F_key            8 rounds of an unbalanced Feistel network on b = max(2, bit_length(n - 1)) bits: x = (L << wr) | R with
                     wl = b // 2, wr = b - wl; a round sends (L, R) to (R, L ^ (mix64(key ^ (round << 32 | R)) mod 2^width(L))) and
                     swaps the widths; a value >= n goes through again
    conditional_indices(seed, r, spot, n, count)
                     the first `count` values other than `spot` among F_key(0), ..., F_key(count)

and a loop-level NumPy reference of what the device keeps: S, and over the permutations S_r (added in slot order), the counts of
S_r >= S and S_r <= S and the sums of d = S_r - S and d^2, added in permutation order.
"""
import functools

import numpy as np

MASK = (1 << 64) - 1
GOLDEN = 0x9e3779b97f4a7c15


def mix64(x):
    x &= MASK
    x ^= x >> 30
    x = (x * 0xbf58476d1ce4e5b9) & MASK
    x ^= x >> 27
    x = (x * 0x94d049bb133111eb) & MASK
    return x ^ (x >> 31)


def feistel(key, x, n):
    b = max(2, (n - 1).bit_length())
    wl0 = b // 2
    wr0 = b - wl0
    while True:
        L, R = x >> wr0, x & ((1 << wr0) - 1)
        wl, wr = wl0, wr0
        for rnd in range(8):
            f = mix64(key ^ ((rnd << 32) | R)) & ((1 << wl) - 1)
            L, R = R, L ^ f
            wl, wr = wr, wl
        x = (L << wr0) | R
        if x < n:
            return x


def conditional_key(seed, r, spot):
    key_r = mix64(mix64(seed) + (r + 1) * GOLDEN)
    return mix64(key_r + (spot + 1) * GOLDEN)


@functools.lru_cache(maxsize=None)
def conditional_indices(seed, r, spot, n, count):
    """A tuple of `count` Python ints."""
    assert 0 <= spot < n and 0 <= count <= n - 1 and r >= 0 and seed >= 0
    key = conditional_key(seed, r, spot)
    out = []
    for t in range(count + 1):
        c = feistel(key, t, n)
        if c != spot and len(out) < count:
            out.append(c)
    assert len(out) == count
    return tuple(out)


def neighbor_sums(V, A):
    """(S (n, K), deg (n,)) of a scipy CSR adjacency: the rows of the neighbours added one by one in list order."""
    V = np.asarray(V, dtype=np.float64)
    n, K = V.shape
    S = np.zeros((n, K))
    deg = np.zeros(n, dtype=np.int64)
    for i in range(n):
        nb = A.indices[A.indptr[i]:A.indptr[i + 1]]
        deg[i] = len(nb)
        for j in nb:
            S[i] += V[j]
    return S, deg


def local_reference(V, A, seed, first, R):
    """dict of S, deg and, over conditional permutations first .. first + R - 1, count_ge, count_le (int64) and sum_d, sumsq_d."""
    V = np.asarray(V, dtype=np.float64)
    n, K = V.shape
    S, deg = neighbor_sums(V, A)
    ge, le = np.zeros((n, K), dtype=np.int64), np.zeros((n, K), dtype=np.int64)
    sd, sq = np.zeros((n, K)), np.zeros((n, K))
    for i in range(n):
        for r in range(first, first + R):
            Sr = np.zeros(K)
            for c in conditional_indices(int(seed), r, i, n, int(deg[i])):
                Sr += V[c]
            d = Sr - S[i]
            ge[i] += Sr >= S[i]
            le[i] += Sr <= S[i]
            sd[i] += d
            sq[i] += d * d
    return {"S": S, "deg": deg, "count_ge": ge, "count_le": le, "sum_d": sd, "sumsq_d": sq}


def _mix64_np(x):
    x = x ^ (x >> np.uint64(30))
    x = x * np.uint64(0xbf58476d1ce4e5b9)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(0x94d049bb133111eb)
    return x ^ (x >> np.uint64(31))


def conditional_indices_batch(seed, r_first, R, spot, n, count):
    """(R, count) int64: row j is conditional_indices(seed, r_first + j, spot, n, count), all R keys walked at once in NumPy uint64
    arithmetic (for the null-distribution tests, where a Python loop per draw is too slow; tested against the loop above)."""
    keys = np.array([conditional_key(seed, r_first + j, spot) for j in range(R)], dtype=np.uint64)[:, None]
    b = max(2, (n - 1).bit_length())
    wl0 = b // 2
    wr0 = b - wl0
    x = np.broadcast_to(np.arange(count + 1, dtype=np.uint64), (R, count + 1)).copy()
    todo = np.ones(x.shape, dtype=bool)
    with np.errstate(over="ignore"):
        while todo.any():
            L, Rh = x >> np.uint64(wr0), x & np.uint64((1 << wr0) - 1)
            wl, wr = wl0, wr0
            for rnd in range(8):
                f = _mix64_np(keys ^ (np.uint64(rnd << 32) | Rh)) & np.uint64((1 << wl) - 1)
                L, Rh = Rh, L ^ f
                wl, wr = wr, wl
            x = np.where(todo, (L << np.uint64(wr0)) | Rh, x)
            todo = todo & (x >= np.uint64(n))
    x = x.astype(np.int64)
    out = np.empty((R, count), dtype=np.int64)
    for j in range(R):
        row = x[j][x[j] != spot]
        out[j] = row[:count]
    return out
