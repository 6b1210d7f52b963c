// What the label permutation entries share on the device (label_pair_kernels.cpp: join counts over the graph; label_gene_kernels.cpp:
// per-label gene sums): labels as one byte per spot with the range check, and the bytes of a group of B permutations staged
// interleaved per position, so that one 8- or 16-byte load returns a position's label under every permutation of its group.
#pragma once
#include <hip/hip_runtime.h>

#include "perm_device.h"

namespace fdx {

constexpr int LP_MAX_LABELS = 64;
constexpr unsigned LP_NONE = 0xffu;      // the byte of a spot that is not counted (labels are below 64: bit 7 marks it)

struct LpPermArgs {
    PermKeys keys;
    int batch;                           // permutations of this launch (the last group may be ragged)
};

// codes[i] = the byte of label i; *flag |= 1 where a label is outside [-1, C); label_counts[a] = n_a; WITH_DEG: deg_sums = {sum deg,
// sum deg^2} (else deg and deg_sums are not read)
template <bool WITH_DEG>
__global__ __launch_bounds__(256) void lp_prepare_kernel(const int* __restrict__ labels, const int* __restrict__ deg, int n, int C,
                                                         unsigned char* __restrict__ codes,
                                                         unsigned long long* __restrict__ label_counts,
                                                         unsigned long long* __restrict__ deg_sums, int* __restrict__ flag) {
    __shared__ unsigned hist[LP_MAX_LABELS];
    __shared__ unsigned long long red[4][2];
    if (threadIdx.x < LP_MAX_LABELS) hist[threadIdx.x] = 0u;
    __syncthreads();
    unsigned long long sd = 0, sd2 = 0;
    bool bad = false;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int l = labels[i];
        bad |= l < -1 || l >= C;
        const bool counted = l >= 0 && l < C;
        codes[i] = counted ? (unsigned char)l : (unsigned char)LP_NONE;
        if (counted) atomicAdd(&hist[l], 1u);
        if constexpr (WITH_DEG) {
            const unsigned long long dg = (unsigned long long)deg[i];
            sd += dg;
            sd2 += dg * dg;
        }
    }
    if (bad) atomicOr(flag, 1);
    if constexpr (WITH_DEG) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            sd += __shfl_xor(sd, off, 64);
            sd2 += __shfl_xor(sd2, off, 64);
        }
        if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = sd; red[threadIdx.x >> 6][1] = sd2; }
    }
    __syncthreads();
    if ((int)threadIdx.x < C && hist[threadIdx.x]) atomicAdd(&label_counts[threadIdx.x], (unsigned long long)hist[threadIdx.x]);
    if constexpr (WITH_DEG) {
        if (threadIdx.x < 2) {
            const unsigned long long s = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
            if (s) atomicAdd(&deg_sums[threadIdx.x], s);
        }
    }
}

// Lr[blockIdx.y][q][j] = byte of l[pi_r(perm[q])], r = first + blockIdx.y * B + j, for q < ld (perm null: the caller's spot order):
// LP_NONE for -1, for positions n .. ld - 1 and for permutations past the batch.  IDENTITY: permutation 0 of the one group is the
// identity, the rest LP_NONE.
template <int B, bool IDENTITY>
__global__ __launch_bounds__(256) void lp_stage_kernel(const unsigned char* __restrict__ codes, const int* __restrict__ perm, int n,
                                                       long long ld, unsigned char* __restrict__ Lr, LpPermArgs pa) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= ld) return;
    unsigned w[B / 4];
#pragma unroll
    for (int k = 0; k < B / 4; ++k) w[k] = 0xffffffffu;
    if (q < n) {
        const int row = perm ? perm[q] : (int)q;
        if constexpr (IDENTITY) {
            w[0] = 0xffffff00u | codes[row];
        } else {
            const int j0 = blockIdx.y * B;
#pragma unroll
            for (int j = 0; j < B; ++j)
                if (j0 + j < pa.batch) {
                    const unsigned c = codes[ss_permute_index(perm_key_at(pa.keys, j0 + j), row, n, pa.keys.wl, pa.keys.wr)];
                    w[j / 4] = (w[j / 4] & ~(0xffu << (8 * (j % 4)))) | (c << (8 * (j % 4)));
                }
        }
    }
    unsigned* out = reinterpret_cast<unsigned*>(Lr + ((size_t)blockIdx.y * ld + q) * B);
    if constexpr (B == 8) *reinterpret_cast<uint2*>(out) = make_uint2(w[0], w[1]);
    else *reinterpret_cast<uint4*>(out) = make_uint4(w[0], w[1], w[2], w[3]);
}

}  // namespace fdx
