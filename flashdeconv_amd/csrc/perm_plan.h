// The host arithmetic the four permutation entries share: the widths of the Feistel halves, the clamp of a permutation batch and
// the layout of the four null arrays.  Plain host code (no HIP): tested by hosttest/plan_asan.cpp.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace fdx {

// b = max(2, bit_length(n - 1)), split into the Feistel halves
inline void ss_feistel_widths(long long n, int* wl, int* wr) {
    int b = 0;
    for (long long v = n - 1; v > 0; v >>= 1) ++b;
    b = b < 2 ? 2 : b;
    *wl = b / 2;
    *wr = b - b / 2;
}

// The permutations of one launch chain: what the scratch budget holds (fit), a hard cap (a grid dimension), max_batch when
// positive, n_perm, and one at the least.
inline long long perm_batch(long long fit, long long cap, long long max_batch, long long n_perm) {
    long long b = std::min(fit, cap);
    if (max_batch > 0) b = std::min(b, max_batch);
    return std::max<long long>(1, std::min(b, std::max<long long>(1, n_perm)));
}

// [count_ge X int64 | count_le X int64 | sum_d X | sumsq_d X] inside a packed result of 64-bit words, for X statistics: the
// offsets are in words from the start of the block, the first at `base`, `end` one past the last.
struct NullSumsLayout {
    size_t X, count_ge, count_le, sum_d, sumsq_d, end;
    explicit NullSumsLayout(size_t x = 0, size_t base = 0)
        : X(x), count_ge(base), count_le(base + x), sum_d(base + 2 * x), sumsq_d(base + 3 * x), end(base + 4 * x) {}
    // a downloaded block into the caller's arrays
    void unpack(const void* block, int64_t* count_ge_out, int64_t* count_le_out, double* sum_d_out, double* sumsq_d_out) const {
        const char* h = static_cast<const char*>(block);
        std::memcpy(count_ge_out, h + 8 * count_ge, 8 * X);
        std::memcpy(count_le_out, h + 8 * count_le, 8 * X);
        std::memcpy(sum_d_out, h + 8 * sum_d, 8 * X);
        std::memcpy(sumsq_d_out, h + 8 * sumsq_d, 8 * X);
    }
    // the answers without spots: every null value equals the observed one
    void fill_empty(int64_t n_perm, int64_t* count_ge_out, int64_t* count_le_out, double* sum_d_out, double* sumsq_d_out) const {
        std::fill(count_ge_out, count_ge_out + X, n_perm);
        std::fill(count_le_out, count_le_out + X, n_perm);
        std::fill(sum_d_out, sum_d_out + X, 0.0);
        std::fill(sumsq_d_out, sumsq_d_out + X, 0.0);
    }
};

}  // namespace fdx
