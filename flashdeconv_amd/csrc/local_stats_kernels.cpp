// Local indicators of spatial association (not in the reference): per spot i and column a of V (n, K) the neighbour sum
//   S_ia = sum_{j in N(i)} V_ja
// over the model's graph, and its conditional-permutation null: spot i keeps its value and its deg_i neighbours are replaced by
// deg_i other spots drawn without replacement, S_ia,r their sum, for r = first_perm .. first_perm + n_perm - 1.  Kept per (i, a):
//   count_ge = #{S_r >= S}    count_le = #{S_r <= S}    sum_d, sumsq_d of d = S_r - S
// Local Moran's I, Gi*, the quadrants and the p values are assembled from these (flashdeconv_amd/utils/local_stats.py).
// Everything is ranked on the raw sums: with deg_i fixed S_r >= S is the event lag_r >= lag, zeros add exactly (the ties of
// zero-inflated data stay ties), and the device's rounding of the mean does not enter.
//
// The draw is a function, as the permutations of spatial_stats_kernels.cpp are (perm_device.h): with F_key the keyed bijection of
// [0, n), key = mix64(key_r + (i + 1) * golden) and key_r the key of permutation r, the drawn spots are the first deg_i values
// other than i among F_key(0), ..., F_key(deg_i) - a bijection meets i at most once, so deg_i + 1 evaluations always suffice.
// utils/local_stats.py:conditional_indices is the definition; ls_draw below is the one device copy, which the kernel and
// fdx_conditional_indices_dev both call.
//
// Two kernels behind the observed pass of spatial_stats_kernels.cpp (which gives mean, m2 and the degree sums):
//   neighbour sums   one lane per position of the sliced ELL, LS_KC columns of register accumulators per walk of the list; rows of
//                    V are read in the caller's order through perm, S and deg are written in the caller's order
//   conditional null one wave per spot, the lanes take 64 permutations at a time: deg_i is uniform across the wave, so the draw
//                    loop is, and each lane reads whole row segments of V (LS_KC contiguous doubles).  Columns go in chunks of
//                    LS_KC (the draws are evaluated again per chunk: a few hundred integer operations against a row gather); a lane keeps
//                    its running sum_d / sumsq_d over its permutations r = first + lane, first + lane + 64, ... in ascending
//                    order and the 64 lanes are added by a fixed butterfly at the end; the comparisons against the broadcast S
//                    are counted by ballot and popcount.  No floating-point atomics, no LDS, no per-lane array indexed at run
//                    time, any degree (a hub of degree n - 1 just loops longer).  The grid is a function of n only and no
//                    result depends on it.
#include "fdx_graph.h"
#include "fdx_internal.h"
#include "fdx_kernels.h"
#include "perm_device.h"

#include <algorithm>
#include <vector>

namespace fdx {

constexpr int LS_KC = 8;                 // columns per walk of a list / per evaluation of the draws
constexpr int LS_CAP_BLOCKS = 1 << 18;   // cap of the null kernel's grid (4 spots per workgroup per stride)

// the conditional permutations of a launch: the first n_perm of keys
struct LsPermArgs {
    PermKeys keys;
    int n_perm;
};

__host__ __device__ __forceinline__ unsigned long long ls_cond_key(unsigned long long key_r, int spot) {
    return ss_mix64(key_r + ((unsigned long long)spot + 1ULL) * 0x9e3779b97f4a7c15ULL);
}

// take(slot, c) for the `count` spots c drawn for `spot`, slot = 0 .. count - 1 in order; 0 <= count <= n - 1
template <class Take>
__device__ __forceinline__ void ls_draw(unsigned long long key, int spot, int n, int count, int wl, int wr, Take&& take) {
    if (count <= 0) return;
    bool skipped = false;
    for (int t = 0; t <= count; ++t) {
        const int c = ss_permute_index(key, t, n, wl, wr);
        const bool self = c == spot;
        if (!self && (skipped || t < count)) take(skipped ? t - 1 : t, c);
        skipped = skipped || self;
    }
}

// nbr_sum[perm[p]][k] = sum over the ELL entries j of position p of V[perm[j]][k] (pad entries skipped), in list order;
// deg_out[perm[p]] = deg[p]
__global__ __launch_bounds__(256) void ls_nbr_sum_kernel(const double* __restrict__ V, long long ldv,
                                                         const int* __restrict__ ell_base, const int* __restrict__ slice_off,
                                                         const int* __restrict__ deg, const int* __restrict__ perm, int n,
                                                         int n_slices, int K, double* __restrict__ nbr_sum,
                                                         int* __restrict__ deg_out) {
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int slice = blockIdx.x * 4 + wib; slice < n_slices; slice += gridDim.x * 4) {
        const long long p = (long long)slice * 64 + lane;
        const bool active = p < n;
        const int w0 = slice_off[slice];
        const int w = slice_off[slice + 1] - w0;
        const int* ell = ell_base + (size_t)w0 * 64 + lane;
        const size_t orow = active ? (perm ? (size_t)perm[p] : (size_t)p) : 0;
        if (active) deg_out[orow] = deg[p];
        for (int k0 = 0; k0 < K; k0 += LS_KC) {
            double acc[LS_KC];
#pragma unroll
            for (int kk = 0; kk < LS_KC; ++kk) acc[kk] = 0.0;
            for (int m = 0; m < w; ++m) {
                const int j = active ? ell[(size_t)m * 64] : n;
                if (j >= 0 && j < n) {
                    const double* row = V + (size_t)(perm ? perm[j] : j) * ldv;
#pragma unroll
                    for (int kk = 0; kk < LS_KC; ++kk) acc[kk] += row[k0 + kk < K ? k0 + kk : K - 1];   // past K - 1: loaded, not kept
                }
            }
            if (active) {
#pragma unroll
                for (int kk = 0; kk < LS_KC; ++kk)
                    if (k0 + kk < K) nbr_sum[orow * K + k0 + kk] = acc[kk];
            }
        }
    }
}

// the conditional null of spot blockIdx.x * 4 + wave (grid-stride), in the caller's order: deg_out and nbr_sum as written above
__global__ __launch_bounds__(256) void ls_cond_null_kernel(const double* __restrict__ V, long long ldv, int n, int K,
                                                           const int* __restrict__ deg_out, const double* __restrict__ nbr_sum,
                                                           LsPermArgs pa, int* __restrict__ count_ge, int* __restrict__ count_le,
                                                           double* __restrict__ sum_d, double* __restrict__ sumsq_d) {
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (long long sp = (long long)blockIdx.x * 4 + wib; sp < n; sp += (long long)gridDim.x * 4) {
        const int spot = (int)sp;
        const int dg = __builtin_amdgcn_readfirstlane(deg_out[spot]);
        const size_t obase = (size_t)spot * K;
        for (int k0 = 0; k0 < K; k0 += LS_KC) {
            double s_obs[LS_KC], sd[LS_KC], sq[LS_KC];
            int ge[LS_KC], le[LS_KC];
#pragma unroll
            for (int kk = 0; kk < LS_KC; ++kk) {
                s_obs[kk] = nbr_sum[obase + (k0 + kk < K ? k0 + kk : K - 1)];
                sd[kk] = sq[kk] = 0.0;
                ge[kk] = le[kk] = 0;
            }
            for (long long r0 = 0; r0 < pa.n_perm; r0 += 64) {                     // 64-bit: n_perm may be 2^31 - 1
                const bool valid = r0 + lane < pa.n_perm;
                PermKeys pass = pa.keys;                                           // the 64 permutations of this pass: their first
                pass.first += r0;                                                  // is uniform, one scalar addition
                double acc[LS_KC];
#pragma unroll
                for (int kk = 0; kk < LS_KC; ++kk) acc[kk] = 0.0;
                if (valid) {
                    const unsigned long long key = ls_cond_key(perm_key_at(pass, lane), spot);
                    ls_draw(key, spot, n, dg, pa.keys.wl, pa.keys.wr, [&](int, int c) {
                        const double* row = V + (size_t)c * ldv;
#pragma unroll
                        for (int kk = 0; kk < LS_KC; ++kk) acc[kk] += row[k0 + kk < K ? k0 + kk : K - 1];
                    });
                }
#pragma unroll
                for (int kk = 0; kk < LS_KC; ++kk) {
                    const double d = acc[kk] - s_obs[kk];
                    ge[kk] += __popcll(__ballot(valid && acc[kk] >= s_obs[kk]));
                    le[kk] += __popcll(__ballot(valid && acc[kk] <= s_obs[kk]));
                    if (valid) {
                        sd[kk] += d;
                        sq[kk] = fma(d, d, sq[kk]);
                    }
                }
            }
#pragma unroll
            for (int kk = 0; kk < LS_KC; ++kk) {
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    sd[kk] += __shfl_xor(sd[kk], off, 64);
                    sq[kk] += __shfl_xor(sq[kk], off, 64);
                }
                if (lane == 0 && k0 + kk < K) {
                    count_ge[obase + k0 + kk] = ge[kk];
                    count_le[obase + k0 + kk] = le[kk];
                    sum_d[obase + k0 + kk] = sd[kk];
                    sumsq_d[obase + k0 + kk] = sq[kk];
                }
            }
        }
    }
}

// out[slot] = the slot-th spot drawn for `spot` under `key`: one lane runs the kernel's own draw
__global__ __launch_bounds__(64) void ls_cond_indices_kernel(unsigned long long key, int spot, int n, int count, int wl, int wr,
                                                             int* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    ls_draw(key, spot, n, count, wl, wr, [&](int slot, int c) { out[slot] = c; });
}

}  // namespace fdx

using namespace fdx;

extern "C" {

// Behind the observed pass of launch_spatial_stats (mean, m2 and the counts are that pass's): nbr_sum (n, K) float64 and deg (n)
// int32 in the caller's spot order; with n_perm > 0 count_ge, count_le (n, K) int32 and sum_d, sumsq_d (n, K) float64 over
// conditional permutations first_perm .. first_perm + n_perm - 1 of `seed`, overwritten.
int fdx_local_stats_dev(const fdx_graph* g, const double* V_dev, int64_t ldv, int32_t K, uint64_t seed, int64_t first_perm,
                        int64_t n_perm, double* nbr_sum_dev, int32_t* deg_dev, int32_t* count_ge_dev, int32_t* count_le_dev,
                        double* sum_d_dev, double* sumsq_d_dev, double* mean_out, double* m2_out, int64_t* counts_out,
                        void* stream) {
    FDX_REQUIRE(g && V_dev && nbr_sum_dev && deg_dev && mean_out && m2_out && counts_out, "fdx_local_stats_dev: null argument");
    FDX_REQUIRE(K >= 1 && ldv >= K, "fdx_local_stats_dev: K must be positive and ldv at least K");
    FDX_REQUIRE(first_perm >= 0 && n_perm >= 0, "fdx_local_stats_dev: first_perm and n_perm must not be negative");
    FDX_REQUIRE(n_perm < (1LL << 31), "fdx_local_stats_dev: n_perm must be below 2^31");
    FDX_REQUIRE(n_perm == 0 || (count_ge_dev && count_le_dev && sum_d_dev && sumsq_d_dev),
                "fdx_local_stats_dev: null argument (the permutation outputs may be null only with n_perm == 0)");
    GraphTables t;
    FDX_TRY(whole_graph_tables(g, "fdx_local_stats_dev", &t));
    hipStream_t st = (hipStream_t)stream;
    PoolStream pool_stream(st);
    counts_out[0] = t.n;
    counts_out[1] = counts_out[2] = 0;
    if (t.n == 0) {                                     // no row to write
        SpatialSumsLayout(K).fill_empty(mean_out, m2_out, nullptr);
        return 0;
    }
    const SpatialStatsPlan plan = spatial_stats_plan(t.n, K);
    DevBuf scratch, out;
    FDX_TRY(scratch.alloc(plan.scratch_doubles * sizeof(double)));
    FDX_TRY(out.alloc(plan.sums.observed_doubles * sizeof(double)));
    FDX_TRY(launch_spatial_stats(plan, V_dev, ldv, K, t, scratch.as<double>(), 1, out.as<double>(), nullptr, nullptr, st));
    hipLaunchKernelGGL(ls_nbr_sum_kernel, dim3(plan.lag_blocks), dim3(256), 0, st, V_dev, ldv, t.ell, t.slice_off, t.deg, t.perm, t.n,
                       plan.n_slices, K, nbr_sum_dev, deg_dev);
    FDX_CHECK_LAUNCH();
    if (n_perm > 0) {
        const LsPermArgs pa{perm_keys(seed, first_perm, t.n), (int)n_perm};
        hipLaunchKernelGGL(ls_cond_null_kernel, dim3(std::min(LS_CAP_BLOCKS, ceil_div(t.n, 4))), dim3(256), 0, st, V_dev, ldv, t.n, K,
                           deg_dev, nbr_sum_dev, pa, count_ge_dev, count_le_dev, sum_d_dev, sumsq_d_dev);
        FDX_CHECK_LAUNCH();
    }
    std::vector<double> host(plan.sums.observed_doubles);
    FDX_TRY(copy_d2h(host.data(), out.p, host.size() * sizeof(double), st));   // the call's one host synchronisation
    plan.sums.unpack(host.data(), mean_out, m2_out, nullptr, counts_out + 1);
    return 0;
}

// out_dev[t] = the t-th of the `count` spots drawn for `spot` in conditional permutation r
int fdx_conditional_indices_dev(uint64_t seed, int64_t r, int64_t spot, int64_t n, int64_t count, int32_t* out_dev, void* stream) {
    FDX_REQUIRE(n >= 1 && n < (1LL << 31) - 128, "fdx_conditional_indices_dev: n must be between 1 and 2^31 - 129");
    FDX_REQUIRE(r >= 0, "fdx_conditional_indices_dev: r must not be negative");
    FDX_REQUIRE(spot >= 0 && spot < n, "fdx_conditional_indices_dev: spot must be in [0, n)");
    FDX_REQUIRE(count >= 0 && count <= n - 1, "fdx_conditional_indices_dev: count must be between 0 and n - 1");
    FDX_REQUIRE(count == 0 || out_dev, "fdx_conditional_indices_dev: null argument");
    if (count == 0) return 0;
    const PermKeys keys = perm_keys(seed, r, n);
    hipLaunchKernelGGL(ls_cond_indices_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream,
                       ls_cond_key(perm_key_at(keys, 0), (int)spot), (int)spot, (int)n, (int)count, keys.wl, keys.wr, out_dev);
    FDX_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
