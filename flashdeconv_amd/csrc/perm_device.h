// The keyed bijection of [0, n) that the permutation kernels evaluate instead of reading an index array, and the keys of a
// launch's permutations (internal; the one copy of what a kernel evaluates - the host arithmetic beside it is perm_plan.h's).
// utils/_permutation.py:permutation_indices is its definition: an unbalanced Feistel network of 8 rounds on
// b = max(2, bit_length(n - 1)) bits (left half b / 2 bits, right half the rest, the widths swap every round), the round function
// the splitmix64 finaliser, values >= n walked along their cycle until they fall below n.
#pragma once
#include <hip/hip_runtime.h>

#include "perm_plan.h"

namespace fdx {

// the splitmix64 finaliser
__host__ __device__ __forceinline__ unsigned long long ss_mix64(unsigned long long x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ULL;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebULL;
    x ^= x >> 31;
    return x;
}

// permutation r of a seed has the key mix64(seed_mixed + (r + 1) * golden), seed_mixed = mix64(seed)
__host__ __device__ __forceinline__ unsigned long long ss_perm_key(unsigned long long seed_mixed, long long r) {
    return ss_mix64(seed_mixed + ((unsigned long long)r + 1ULL) * 0x9e3779b97f4a7c15ULL);
}

// What identifies the permutations of a launch: element j is permutation r = first + j of the seed.
struct PermKeys {
    unsigned long long seed_mixed;   // mix64(seed)
    long long first;                 // r of element 0
    int wl, wr;                      // widths of the Feistel halves of [0, n): wl = b / 2, wr = b - wl
};

inline PermKeys perm_keys(unsigned long long seed, long long first, long long n) {
    PermKeys k{ss_mix64(seed), first, 0, 0};
    ss_feistel_widths(n, &k.wl, &k.wr);
    return k;
}

__host__ __device__ __forceinline__ unsigned long long perm_key_at(const PermKeys& k, long long j) {
    return ss_perm_key(k.seed_mixed, k.first + j);
}

// pi(i) for i < n < 2^31: x = (L << wr) | R; a round sends (L, R) to (R, L ^ F(R)) and swaps the widths; 8 rounds restore them
__device__ __forceinline__ int ss_permute_index(unsigned long long key, int i, int n, int wl, int wr) {
    unsigned x = (unsigned)i;
    do {
        unsigned L = x >> wr, R = x & ((1u << wr) - 1u);
        int a = wl, c = wr;
#pragma unroll
        for (unsigned round = 0; round < 8; ++round) {
            const unsigned f = (unsigned)ss_mix64(key ^ (((unsigned long long)round << 32) | R)) & ((1u << a) - 1u);
            const unsigned nr = L ^ f;
            L = R;
            R = nr;
            const int t = a;
            a = c;
            c = t;
        }
        x = (L << wr) | R;
    } while (x >= (unsigned)n);
    return (int)x;
}

}  // namespace fdx
