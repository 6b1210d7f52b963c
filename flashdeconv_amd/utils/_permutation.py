"""What the four permutation tests share (``spatial_stats``, ``local_stats``, ``gene_permutations``, ``neighborhoods``): the
definition of the permutation of a seed (``permutation_indices``; the kernels evaluate it in place, csrc/perm_device.h) with the one
spelling of its key, the checks and the splitting of a request, and the rule that ranks an observed statistic against its null.
Private: the public names are re-exported by the modules that document them.

The ranking functions take the array namespace ``xp`` (numpy or torch) and float64 arrays, run the same expressions in the same
order in both and give the same bits, on CPU and on device tensors.  Constants are 0-d values of the namespace, never Python
scalars: torch divides by a host scalar through its reciprocal, which is not the quotient NumPy forms.  Nothing is masked here:
what counts as dead or isolated is the caller's.
"""
import numpy as np

from ._device import check_count

_MASK64 = (1 << 64) - 1
_GOLDEN = 0x9e3779b97f4a7c15
_FEISTEL_ROUNDS = 8
_NULL_CALL_BYTES = 256 << 20          # return_null on host arrays: the device holds this much of the null per call


def _mix64(x):
    """The splitmix64 finaliser on a uint64 array (arithmetic modulo 2^64)."""
    x = x ^ (x >> np.uint64(30))
    x = x * np.uint64(0xbf58476d1ce4e5b9)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(0x94d049bb133111eb)
    return x ^ (x >> np.uint64(31))


def _mix64_int(x):
    return int(_mix64(np.array([x & _MASK64], dtype=np.uint64))[0])


def permutation_key(seed, r):
    """The key of permutation ``r`` of ``seed``, a Python int below 2^64: ``mix64(mix64(seed) + (r + 1) * 0x9e3779b97f4a7c15)``."""
    return _mix64_int(_mix64_int(seed) + (r + 1) * _GOLDEN)


def permutation_indices(seed, r, n):
    """``pi_r(0 .. n - 1)`` of ``seed`` as an int64 array: the permutation ``fdx_spatial_perm_dev`` applies to the rows of V
    (``V_pi[i] = V[pi_r(i)]``), defined here in NumPy uint64 arithmetic; the device matches it bit for bit.

    An unbalanced Feistel network on ``b = max(2, bit_length(n - 1))`` bits: ``x = (L << wr) | R`` with ``wl = b // 2`` bits of L
    and ``wr = b - wl`` of R; each of 8 rounds sends ``(L, R)`` to ``(R, L ^ (F(R) mod 2^width(L)))`` and swaps the two widths,
    with ``F(R) = mix64(key ^ (round << 32 | R))``, ``mix64`` the splitmix64 finaliser and
    ``key = mix64(mix64(seed) + (r + 1) * 0x9e3779b97f4a7c15)``.  That is a bijection of [0, 2^b); a value >= n is sent through it
    again until it falls below n (cycle-walking: a start below n lies on a cycle that returns below n), which makes it a
    bijection of [0, n).  ``2^b < 2 n`` for n >= 3, so a walk takes under two steps on average."""
    seed, r, n = int(seed), int(r), int(n)
    if r < 0 or n < 0 or n >= (1 << 31) - 128:
        raise ValueError(f"r must not be negative and n must be in [0, 2^31 - 128), got r = {r}, n = {n}")
    return _keyed_bijection(permutation_key(seed, r), np.arange(n, dtype=np.uint64), n)


def _keyed_bijection(key, x, n):
    """``F_key(x)`` for a uint64 array ``x`` of values below ``n``: the Feistel network of ``permutation_indices`` under ``key``
    (a Python int below 2^64), cycle-walked below ``n``; int64."""
    b = max(2, (n - 1).bit_length()) if n > 0 else 2
    wl0, wr0 = b // 2, b - b // 2
    key = np.uint64(key)
    out = np.array(x, dtype=np.uint64)
    todo = np.arange(out.size)
    with np.errstate(over="ignore"):
        while todo.size:
            x = out[todo]
            L, R = x >> np.uint64(wr0), x & np.uint64((1 << wr0) - 1)
            wl, wr = wl0, wr0
            for rnd in range(_FEISTEL_ROUNDS):
                f = _mix64(key ^ (np.uint64(rnd << 32) | R)) & np.uint64((1 << wl) - 1)
                L, R = R, L ^ f
                wl, wr = wr, wl
            x = (L << np.uint64(wr0)) | R
            out[todo] = x
            todo = todo[x >= np.uint64(n)]
    return out.astype(np.int64)


def _permutation_seed(random_state):
    """A uint64 seed: a non-negative int as it stands, else one 63-bit draw from the ``RandomState`` that
    ``utils.check_random_state`` makes of the argument."""
    if isinstance(random_state, (int, np.integer)) and not isinstance(random_state, (bool, np.bool_)):
        if not 0 <= int(random_state) <= _MASK64:
            raise ValueError(f"random_state must be in [0, 2^64) when it is an int, got {random_state}")
        return int(random_state)
    from .random import check_random_state
    rs = check_random_state(random_state)
    return (int(rs.randint(0, 1 << 31)) << 32) | int(rs.randint(0, 1 << 32, dtype=np.int64))


def check_permutation_counts(n_permutations, first_perm=0, max_batch=0):
    """``(n_permutations, first_perm, max_batch)`` as ints >= 0 (``ValueError`` on the first that is not)."""
    return (check_count("n_permutations", n_permutations), check_count("first_perm", first_perm),
            check_count("max_batch", max_batch))


def permutation_chunks(R, chunk):
    """``(done, cnt)`` of the calls that run R permutations at most ``chunk`` at a time, in order; the one call ``(0, 0)`` for
    R = 0 (the observed sums still need it)."""
    done = 0
    while True:
        cnt = min(chunk, R - done)
        yield done, cnt
        done += cnt
        if done >= R:
            return


def _const(xp, like, v):
    """``v`` as a 0-d float64 of ``xp``: a NumPy scalar, or a tensor on the device of the float64 tensor ``like``."""
    return np.float64(v) if xp is np else like.new_full((), v)


def _sqrt(xp, v):
    """The correctly rounded square root in both namespaces.  torch's own is that on the device but not on the CPU (the last bit
    of about one argument in a hundred differs, which ones depends on the vector path), so a CPU tensor goes through NumPy on its
    own memory."""
    if xp is np or v.device.type != "cpu":
        return xp.sqrt(v)
    return xp.from_numpy(np.sqrt(v.numpy()))


def p_from_count(xp, count, R):
    """``(1 + count) / (R + 1)``."""
    return (1.0 + count) / _const(xp, count, float(R) + 1.0)


def two_sided(xp, greater, less):
    """``min(1, 2 min(greater, less))``."""
    return xp.minimum(_const(xp, greater, 1.0), 2.0 * xp.minimum(greater, less))


def null_moments(xp, s, sq, R):
    """``(mean, std)`` of R null values with sum ``s`` and sum of squares ``sq``: ``std = sqrt(max(sq / R - mean * mean, 0))``.
    The clamp is against a plain 0: an infinite ``sq`` gives an infinite ``std``, not NaN."""
    Rc = _const(xp, s, float(R))
    mean = s / Rc
    return mean, _sqrt(xp, xp.maximum(sq / Rc - mean * mean, _const(xp, sq, 0.0)))


def rank_against_null(xp, count_ge, count_le, sum_d, sumsq_d, R):
    """``(p_greater, p_less, p_value, mean_d, std_d, z_sim)`` of an observed statistic against R >= 1 null values, from the counts
    of null values ``>=`` / ``<=`` it and the sums of ``d = null - observed`` and ``d^2``: ``z_sim = -mean_d / std_d``, NaN where
    the null does not vary."""
    greater, less = p_from_count(xp, count_ge, R), p_from_count(xp, count_le, R)
    mean_d, std_d = null_moments(xp, sum_d, sumsq_d, R)
    spread = std_d > 0
    z_sim = xp.where(spread, -mean_d / xp.where(spread, std_d, _const(xp, std_d, 1.0)), float("nan"))
    return greater, less, two_sided(xp, greater, less), mean_d, std_d, z_sim
