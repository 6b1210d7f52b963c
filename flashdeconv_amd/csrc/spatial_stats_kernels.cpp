// Spatial autocorrelation of per-spot values V (n, K) over the model's graph (not in the reference): with A the symmetric binary
// adjacency held as the sliced ELL, mean_a = (1/n) sum_i V_ia, Z = V - mean, the kernels produce
//   m2_a = sum_i Z_ia^2,   lag = A Z,   C = Z' lag (K, K),   sum_i deg_i and sum_i deg_i^2,
// and on request the neighbour-averaged values (A V)_ia / deg_i in the caller's spot order.  Moran's I, the bivariate Moran matrix
// and the z scores are assembled from these on the host (flashdeconv_amd/utils/spatial_stats.py).
//
// Four passes, each a grid-stride kernel on at most SS_CAP_BLOCKS workgroups that leaves per-workgroup partials, and one
// fixed-order reduction of the partials behind each: no floating-point atomics, the grid depends on (n, K) only, so two calls on the
// same inputs add the same numbers in the same order.
//   column sums   V row-major in the caller's order -> mean
//   centre        Z = V - mean, transposed into type-major planes (K, ld) in the graph's solver order (position p holds spot
//                 perm[p]: the layout beta has in the solver), through a [spot][type] LDS tile of 32 types at a time; positions
//                 n .. ld - 1 are written as zeros, so the ELL pad index (n) gathers zeros and needs no mask; m2 partials
//   lag           one lane per spot, one wave per 64-spot slice: ONE index per ELL entry, then KC gathers into KC register
//                 accumulators (KC a template parameter: 8, 16 or 32 types per walk of the slice's list - more types walk the list
//                 again); lag planes (K, ld), the degree sums, neighbor_mean = lag / deg + mean
//   cross         C = Z' lag as a skinny float64 product: a workgroup owns a 32 x 32 tile of the pair space (blockIdx.y; any K),
//                 stages 64 positions of the 32 + 32 planes in LDS and keeps a 2 x 2 block of C per thread in registers
// The two-pass centred form is what makes near-constant columns (proportions) safe: sum V^2 - n mean^2 is never formed.
//
// Permutation null (fdx_spatial_perm_dev): after the observed pass above, and m4 = sum Z^4 from its planes, B permutations per
// launch chain recompute C_r = Zpi' (A Zpi) with Zpi[k][p] = V[pi_r(perm[p])][k] - mean[k]: the centre kernel with the row index
// sent through pi_r (evaluated in the kernel: no index array), the lag and cross kernels as they are, each with the batch as one
// more grid dimension and per-batch plane offsets.  mean and m2 do not change under a permutation.  One kernel then reduces every
// C_r in block order and one adds them to the counts and sums against C_obs in permutation order.
//
// The spatial correlogram (correlogram_kernels.cpp) runs the column-sum, centre, m4, cross and reduce kernels of this file on its
// own binning and lag planes: launch_spatial_moments, launch_spatial_cross_batch and launch_reduce_i64 are what crosses.
//
// pi_r is a keyed bijection of [0, n): an unbalanced Feistel network of 8 rounds on b = max(2, bit_length(n - 1)) bits (left half
// b / 2 bits, right half the rest, the widths swap every round), the round function the splitmix64 finaliser, values >= n walked
// along their cycle until they fall below n (perm_device.h).  utils/_permutation.py:permutation_indices is its definition.
#include "fdx_graph.h"
#include "fdx_internal.h"
#include "fdx_kernels.h"
#include "gene_pass.h"
#include "perm_device.h"

#include <algorithm>
#include <vector>

namespace fdx {

constexpr int SS_CAP_BLOCKS = 1024;      // cap of every grid here: partials do not grow with n
constexpr int SS_KT = 32;                // centre: types staged at a time
constexpr int SS_KS = SS_KT + 1;         //         odd row stride of the [spot][type] tile (column reads hit 64 banks)
constexpr int SS_CT = 32;                // cross: edge of a pair-space tile
constexpr int SS_CP = 64;                //        positions staged at a time (one slice)
constexpr int SS_PERM_MAX_BATCH = 512;   // permutation batches: SCRATCH_BUDGET_BYTES sizes B (one at the least), this caps it (a grid dimension)

// same-wave LDS hand-off: a wave's ds operations execute in order; this keeps the compiler from moving them across
__device__ __forceinline__ void wave_lds_handoff() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// the permutations of a centre launch (batch element j is keys' element j) and where their planes go
struct SsPermArgs {
    PermKeys keys;
    long long plane_stride;          // doubles between the planes of two batch elements (K * ld)
};

// partials[b][c] = sum of V[r][c] over block b's rows [b * rows_per_block, ...): 256 / K rows in flight per pass (consecutive
// threads read consecutive addresses of a row), their running sums added in a fixed order at the end
__global__ __launch_bounds__(256) void ss_colsum_kernel(const double* __restrict__ V, long long ldv, int n, int K,
                                                        int rows_per_block, double* __restrict__ partials) {
    __shared__ double red[256];
    const long long r0 = (long long)blockIdx.x * rows_per_block;
    const long long r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
    for (int c0 = 0; c0 < K; c0 += 256) {
        const int Kc = K - c0 < 256 ? K - c0 : 256;
        const int rpp = 256 / Kc;
        const int c = threadIdx.x % Kc, rs = threadIdx.x / Kc;
        double s = 0.0;
        if (rs < rpp)
            for (long long r = r0 + rs; r < r1; r += rpp) s += V[(size_t)r * ldv + c0 + c];
        red[threadIdx.x] = s;
        __syncthreads();
        if ((int)threadIdx.x < Kc) {
            double t = 0.0;
            for (int j = 0; j < rpp; ++j) t += red[j * Kc + threadIdx.x];
            partials[(size_t)blockIdx.x * K + c0 + threadIdx.x] = t;
        }
        __syncthreads();
    }
}

// out[i] = (partials[0][i] + partials[1][i] + ...) / div, in that order
template <class T>
__global__ __launch_bounds__(256) void ss_reduce_kernel(const T* __restrict__ partials, int nparts, long long width, T div,
                                                        T* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= width) return;
    T s = 0;
    for (int b = 0; b < nparts; ++b) s += partials[(size_t)b * width + i];
    out[i] = s / div;
}

// Z[k][p] = V[perm[p]][k] - mean[k] for p < n, 0 for n <= p < ld (n_slices_ld = ld / 64 slices are written);
// m2_partials[block][k] = the block's share of sum_p Z[k][p]^2.
// PERMUTED: batch element blockIdx.y reads row pi_r(perm[p]) instead, r = pa.keys.first + blockIdx.y, into its own planes; whole rows of
// V are still read as segments (the type-major planes are never gathered from); no m2 (it does not change) and no m2 tile.
template <bool PERMUTED>
__global__ __launch_bounds__(256) void ss_centre_kernel(const double* __restrict__ V, long long ldv, const double* __restrict__ mean,
                                                        const int* __restrict__ perm, int n, int n_slices_ld, int K,
                                                        double* __restrict__ Z, long long ld, double* __restrict__ m2_partials,
                                                        SsPermArgs pa) {
    extern __shared__ __attribute__((aligned(16))) double smem[];   // 4 tiles [64][SS_KS], then m2 [4][K]
    __shared__ int row_s[4][64];
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double* tile = smem + (size_t)wib * 64 * SS_KS;
    double* m2_all = smem + (size_t)4 * 64 * SS_KS;
    double* m2w = m2_all + (size_t)wib * K;
    unsigned long long key = 0;
    if constexpr (PERMUTED) {
        key = perm_key_at(pa.keys, blockIdx.y);
        Z += (size_t)blockIdx.y * pa.plane_stride;
    } else {
        for (int k = lane; k < K; k += 64) m2w[k] = 0.0;
    }
    for (int slice = blockIdx.x * 4 + wib; slice < n_slices_ld; slice += gridDim.x * 4) {
        const long long p = (long long)slice * 64 + lane;
        wave_lds_handoff();                                        // the previous slice's readers of row_s are done
        int row = p < n ? (perm ? perm[p] : (int)p) : -1;
        if constexpr (PERMUTED)
            if (row >= 0) row = ss_permute_index(key, row, n, pa.keys.wl, pa.keys.wr);
        row_s[wib][lane] = row;
        for (int k0 = 0; k0 < K; k0 += SS_KT) {
            const int kc = K - k0 < SS_KT ? K - k0 : SS_KT;
            wave_lds_handoff();
            // element f = lane + 64 j of the wave's 64 x kc block: (spot, type) advance by (64 / kc, 64 % kc) with a carry; the
            // lanes of one load cover whole row segments of kc doubles
            const int total = 64 * kc;
            const int ds = 64 / kc, dk = 64 - ds * kc;
            int sp = lane / kc, k = lane - sp * kc;
#pragma unroll 4
            for (int f = lane; f < total; f += 64) {
                const int src = row_s[wib][sp];
                tile[sp * SS_KS + k] = src >= 0 ? V[(size_t)src * ldv + k0 + k] - mean[k0 + k] : 0.0;
                sp += ds;
                k += dk;
                if (k >= kc) { k -= kc; ++sp; }
            }
            wave_lds_handoff();
            for (int kk = 0; kk < kc; ++kk) Z[(size_t)(k0 + kk) * ld + p] = tile[lane * SS_KS + kk];
            if constexpr (!PERMUTED)
                if (lane < kc) {                                   // lane owns type k0 + lane: its 64 squares in spot order
                    double s = 0.0;
                    for (int q = 0; q < 64; ++q) {
                        const double z = tile[q * SS_KS + lane];
                        s = fma(z, z, s);
                    }
                    m2w[k0 + lane] += s;
                }
        }
    }
    if constexpr (!PERMUTED) {
        __syncthreads();
        for (int k = threadIdx.x; k < K; k += 256)
            m2_partials[(size_t)blockIdx.x * K + k] =
                ((m2_all[k] + m2_all[K + k]) + m2_all[2 * K + k]) + m2_all[3 * (size_t)K + k];
    }
}

// lag[k][p] = sum over the ELL entries of position p of Z[k][entry] (pad entries read the zero column n); positions of the last
// slice past n get 0.  deg_partials[block] = {sum deg, sum deg^2}.  nbr_mean (may be null): row perm[p] of an (n, K) row-major
// matrix, lag / deg + mean (the mean of the neighbours' V), 0 without neighbours.  Batch element blockIdx.y works on the planes
// batch_stride doubles further on; deg_partials may be null (the permuted passes: the degrees are the observed pass's).
template <int KC>
__global__ __launch_bounds__(256) void ss_lag_kernel(const double* __restrict__ Z, long long ld, const int* __restrict__ ell_base,
                                                     const int* __restrict__ slice_off, const int* __restrict__ deg,
                                                     const int* __restrict__ perm, const double* __restrict__ mean, int n,
                                                     int n_slices, int K, double* __restrict__ lag, double* __restrict__ nbr_mean,
                                                     long long* __restrict__ deg_partials, long long batch_stride) {
    __shared__ long long red[4][2];
    Z += (size_t)blockIdx.y * batch_stride;
    lag += (size_t)blockIdx.y * batch_stride;
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    long long sd = 0, sd2 = 0;
    for (int slice = blockIdx.x * 4 + wib; slice < n_slices; slice += gridDim.x * 4) {
        const long long p = (long long)slice * 64 + lane;
        const bool active = p < n;
        const int w0 = slice_off[slice];
        const int w = slice_off[slice + 1] - w0;
        const int* ell = ell_base + (size_t)w0 * 64 + lane;
        const int dg = active ? deg[p] : 0;
        sd += dg;
        sd2 += (long long)dg * dg;
        const size_t orow = active ? (perm ? (size_t)perm[p] : (size_t)p) : 0;
        for (int k0 = 0; k0 < K; k0 += KC) {
            const double* zp[KC];                                  // planes past K - 1 repeat the last one: loaded, not kept
#pragma unroll
            for (int kk = 0; kk < KC; ++kk) zp[kk] = Z + (size_t)(k0 + kk < K ? k0 + kk : K - 1) * ld;
            double acc[KC];
#pragma unroll
            for (int kk = 0; kk < KC; ++kk) acc[kk] = 0.0;
            int j_next = (w > 0 && active) ? ell[0] : n;
            for (int m = 0; m < w; ++m) {
                const int j = j_next;
                if (m + 1 < w) j_next = active ? ell[(size_t)(m + 1) * 64] : n;
#pragma unroll
                for (int kk = 0; kk < KC; ++kk) acc[kk] += zp[kk][j];
            }
#pragma unroll
            for (int kk = 0; kk < KC; ++kk)
                if (k0 + kk < K) {
                    lag[(size_t)(k0 + kk) * ld + p] = active ? acc[kk] : 0.0;
                    if (nbr_mean && active)
                        nbr_mean[orow * K + k0 + kk] = dg > 0 ? acc[kk] / (double)dg + mean[k0 + kk] : 0.0;
                }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sd += __shfl_xor(sd, off, 64);
        sd2 += __shfl_xor(sd2, off, 64);
    }
    if (!deg_partials) return;
    if (lane == 0) { red[wib][0] = sd; red[wib][1] = sd2; }
    __syncthreads();
    if (threadIdx.x < 2)
        deg_partials[(size_t)blockIdx.x * 2 + threadIdx.x] =
            red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// partials[blockIdx.x][a][b] = sum over the block's 64-position chunks of Z[a][p] * lag[b][p], for the (a, b) of pair-space tile
// blockIdx.y = tile_a * ntb + tile_b.  Thread (ta, tb) of 16 x 16 owns a in {ta, ta + 16}, b in {tb, tb + 16} of the tile: per
// position two LDS reads of each operand (the ta reads broadcast) feed four FMAs; the row stride of 65 doubles puts the 16 lag
// rows a half-wave reads on 16 different bank pairs.  Batch element blockIdx.z: Z planes z_stride and lag planes lag_stride doubles
// further on (z_stride 0: every element's lag against the same Z - the bands of a correlogram), partials gridDim.x * K * K further on.
__global__ __launch_bounds__(256) void ss_cross_kernel(const double* __restrict__ Z, const double* __restrict__ lag, long long ld,
                                                       int n_chunks, int K, int ntb, double* __restrict__ partials,
                                                       long long z_stride, long long lag_stride) {
    __shared__ double zs[SS_CT][SS_CP + 1], ls[SS_CT][SS_CP + 1];
    Z += (size_t)blockIdx.z * z_stride;
    lag += (size_t)blockIdx.z * lag_stride;
    partials += (size_t)blockIdx.z * gridDim.x * K * K;
    const int a_base = (blockIdx.y / ntb) * SS_CT, b_base = (blockIdx.y % ntb) * SS_CT;
    const int ta = threadIdx.x >> 4, tb = threadIdx.x & 15;
    const int sr = threadIdx.x >> 6, sc = threadIdx.x & 63;
    double c00 = 0.0, c01 = 0.0, c10 = 0.0, c11 = 0.0;
    for (int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const size_t p = (size_t)chunk * SS_CP + sc;
#pragma unroll
        for (int i = 0; i < SS_CT / 4; ++i) {
            const int r = sr + 4 * i;
            zs[r][sc] = a_base + r < K ? Z[(size_t)(a_base + r) * ld + p] : 0.0;
            ls[r][sc] = b_base + r < K ? lag[(size_t)(b_base + r) * ld + p] : 0.0;
        }
        __syncthreads();
#pragma unroll 8
        for (int q = 0; q < SS_CP; ++q) {
            const double z0 = zs[ta][q], z1 = zs[ta + 16][q];
            const double l0 = ls[tb][q], l1 = ls[tb + 16][q];
            c00 = fma(z0, l0, c00);
            c01 = fma(z0, l1, c01);
            c10 = fma(z1, l0, c10);
            c11 = fma(z1, l1, c11);
        }
        __syncthreads();
    }
    double* out = partials + (size_t)blockIdx.x * K * K;
    const int a0 = a_base + ta, a1 = a0 + 16, b0 = b_base + tb, b1 = b0 + 16;
    if (a0 < K && b0 < K) out[(size_t)a0 * K + b0] = c00;
    if (a0 < K && b1 < K) out[(size_t)a0 * K + b1] = c01;
    if (a1 < K && b0 < K) out[(size_t)a1 * K + b0] = c10;
    if (a1 < K && b1 < K) out[(size_t)a1 * K + b1] = c11;
}

// partials[blockIdx.x][k] = the block's share of sum_p Z[k][p]^4 for plane k = blockIdx.y: 256 positions at a time, each thread's
// running sum, then a fixed tree over the 256 threads
__global__ __launch_bounds__(256) void ss_m4_kernel(const double* __restrict__ Z, long long ld, int K, double* __restrict__ partials) {
    __shared__ double red[256];
    const double* z = Z + (size_t)blockIdx.y * ld;
    double s = 0.0;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < ld; p += (long long)gridDim.x * 256) {
        const double v = z[p], v2 = v * v;
        s = fma(v2, v2, s);
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[(size_t)blockIdx.x * K + blockIdx.y] = red[0];
}

// out[j][i] = partials[j][0][i] + partials[j][1][i] + ... for batch element j = blockIdx.y: the order of ss_reduce_kernel, and a
// permutation's C_r does not depend on the batch it ran in (at 1M spots 1024 partials per output and few threads: latency-bound)
__global__ __launch_bounds__(256) void ss_reduce_batch_kernel(const double* __restrict__ partials, int nparts, long long width,
                                                              double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= width) return;
    const double* pj = partials + (size_t)blockIdx.y * nparts * width;
    double s = 0;
#pragma unroll 16                                                  // sixteen loads in flight; the additions keep their order
    for (int b = 0; b < nparts; ++b) s += pj[(size_t)b * width + i];
    out[(size_t)blockIdx.y * width + i] = s;
}

// the batch's C_r against C_obs, one thread per pair, in permutation order: d = C_r - C_obs
__global__ __launch_bounds__(256) void ss_perm_accum_kernel(const double* __restrict__ Cr, int B, long long KK,
                                                            const double* __restrict__ C_obs, long long* __restrict__ count_ge,
                                                            long long* __restrict__ count_le, double* __restrict__ sum_d,
                                                            double* __restrict__ sumsq_d) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= KK) return;
    const double c0 = C_obs[i];
    long long ge = count_ge[i], le = count_le[i];
    double s = sum_d[i], q = sumsq_d[i];
    for (int j = 0; j < B; ++j) {
        const double c = Cr[(size_t)j * KK + i];
        const double d = c - c0;
        ge += c >= c0 ? 1 : 0;
        le += c <= c0 ? 1 : 0;
        s += d;
        q = fma(d, d, q);
    }
    count_ge[i] = ge;
    count_le[i] = le;
    sum_d[i] = s;
    sumsq_d[i] = q;
}

// out[i] = pi_r(i)
__global__ __launch_bounds__(256) void ss_perm_indices_kernel(unsigned long long key, int n, int wl, int wr, int* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = ss_permute_index(key, (int)i, n, wl, wr);
}

SpatialStatsPlan spatial_stats_plan(long long n, int K) {
    SpatialStatsPlan s;
    s.ld = round_up(n + 1, 64);
    s.n_slices = ceil_div(n, 64);
    s.colsum_blocks = (int)std::min<long long>(SS_CAP_BLOCKS, std::max<long long>(1, ceil_div(n, 1024)));
    s.rows_per_block = ceil_div(n, s.colsum_blocks);
    s.colsum_blocks = ceil_div(n, s.rows_per_block);
    s.centre_blocks = (int)std::min<long long>(SS_CAP_BLOCKS, ceil_div(s.ld / 64, 4));
    s.lag_blocks = std::min(SS_CAP_BLOCKS, ceil_div(s.n_slices, 4));
    s.pair_tiles_1d = ceil_div(K, SS_CT);
    const int tiles = s.pair_tiles_1d * s.pair_tiles_1d;
    // the product runs over the positions the lag pass wrote: n_slices chunks of 64 (Z is 0 from n on)
    s.cross_blocks = (int)std::max<long long>(1, std::min<long long>(s.n_slices, SS_CAP_BLOCKS / tiles));
    const size_t KK = (size_t)K * K;
    s.partials_doubles = std::max({(size_t)s.colsum_blocks * K, (size_t)s.centre_blocks * K, (size_t)s.cross_blocks * KK,
                                   (size_t)s.lag_blocks * 2});
    s.scratch_doubles = 2 * (size_t)K * s.ld + s.partials_doubles;
    s.sums = SpatialSumsLayout(K);
    return s;
}

template <int KC>
static void launch_lag(const SpatialStatsPlan& s, int batch, long long batch_stride, const double* Z, const GraphTables& g,
                       const double* mean, int K, double* lag, double* nbr_mean, long long* deg_part, hipStream_t st) {
    hipLaunchKernelGGL(ss_lag_kernel<KC>, dim3(s.lag_blocks, batch), dim3(256), 0, st, Z, s.ld, g.ell, g.slice_off, g.deg, g.perm, mean,
                       g.n, s.n_slices, K, lag, nbr_mean, deg_part, batch_stride);
}

static void launch_lag_for(const SpatialStatsPlan& s, int batch, long long batch_stride, const double* Z, const GraphTables& g,
                           const double* mean, int K, double* lag, double* nbr_mean, long long* deg_part, hipStream_t st) {
    if (K <= 8) launch_lag<8>(s, batch, batch_stride, Z, g, mean, K, lag, nbr_mean, deg_part, st);
    else if (K <= 16) launch_lag<16>(s, batch, batch_stride, Z, g, mean, K, lag, nbr_mean, deg_part, st);
    else launch_lag<32>(s, batch, batch_stride, Z, g, mean, K, lag, nbr_mean, deg_part, st);
}

// the passes that do not look at the graph: mean, Z in the order of `perm`, m2 and (m4 != null) m4
int launch_spatial_moments(const SpatialStatsPlan& s, const double* V, long long ldv, int n, int K, const int* perm, double* Z,
                           double* part, double* mean, double* m2, double* m4, hipStream_t st) {
    hipLaunchKernelGGL(ss_colsum_kernel, dim3(s.colsum_blocks), dim3(256), 0, st, V, ldv, n, K, s.rows_per_block, part);
    FDX_CHECK_LAUNCH();
    hipLaunchKernelGGL(ss_reduce_kernel<double>, dim3(ceil_div(K, 256)), dim3(256), 0, st, part, s.colsum_blocks, (long long)K,
                       (double)n, mean);
    FDX_CHECK_LAUNCH();
    const size_t lds = ((size_t)4 * 64 * SS_KS + (size_t)4 * K) * sizeof(double);
    if (lds > 64 * 1024)
        FDX_HIP(hipFuncSetAttribute((const void*)ss_centre_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(ss_centre_kernel<false>, dim3(s.centre_blocks), dim3(256), lds, st, V, ldv, mean, perm, n, (int)(s.ld / 64),
                       K, Z, s.ld, part, SsPermArgs{});
    FDX_CHECK_LAUNCH();
    hipLaunchKernelGGL(ss_reduce_kernel<double>, dim3(ceil_div(K, 256)), dim3(256), 0, st, part, s.centre_blocks, (long long)K, 1.0,
                       m2);
    FDX_CHECK_LAUNCH();

    if (m4) {
        hipLaunchKernelGGL(ss_m4_kernel, dim3(s.centre_blocks, K), dim3(256), 0, st, Z, s.ld, K, part);
        FDX_CHECK_LAUNCH();
        hipLaunchKernelGGL(ss_reduce_kernel<double>, dim3(ceil_div(K, 256)), dim3(256), 0, st, part, s.centre_blocks, (long long)K,
                           1.0, m4);
        FDX_CHECK_LAUNCH();
    }
    return 0;
}

int launch_spatial_cross_batch(const SpatialStatsPlan& s, const double* Z, const double* lag, long long lag_stride, int batch, int K,
                               double* part, double* C, hipStream_t st) {
    const long long KK = (long long)K * K;
    hipLaunchKernelGGL(ss_cross_kernel, dim3(s.cross_blocks, s.pair_tiles_1d * s.pair_tiles_1d, batch), dim3(256), 0, st, Z, lag, s.ld,
                       s.n_slices, K, s.pair_tiles_1d, part, 0LL, lag_stride);
    FDX_CHECK_LAUNCH();
    hipLaunchKernelGGL(ss_reduce_batch_kernel, dim3(ceil_div(KK, 256), batch), dim3(256), 0, st, part, s.cross_blocks, KK, C);
    FDX_CHECK_LAUNCH();
    return 0;
}

int launch_reduce_i64(const long long* partials, int nparts, long long width, long long* out, hipStream_t st) {
    hipLaunchKernelGGL(ss_reduce_kernel<long long>, dim3(ceil_div(width, 256)), dim3(256), 0, st, partials, nparts, width, 1LL, out);
    FDX_CHECK_LAUNCH();
    return 0;
}

// The four passes of the observed statistics.  scratch: Z planes (K, ld) for `batch` elements, as many lag planes - the first of
// each are used - then s.partials_doubles of partials; m4 (may be null) = sum Z^4.
int launch_spatial_stats(const SpatialStatsPlan& s, const double* V, long long ldv, int K, const GraphTables& g, double* scratch,
                         int batch, double* out, double* nbr_mean, double* m4, hipStream_t st) {
    if (g.n <= 0) return 0;
    double* Z = scratch;
    double* lag = Z + (size_t)batch * K * s.ld;
    double* part = lag + (size_t)batch * K * s.ld;
    double* mean = out + s.sums.mean;
    double* C = out + s.sums.C;
    long long* counts = reinterpret_cast<long long*>(out + s.sums.deg_sums);
    const size_t KK = s.sums.KK;

    FDX_TRY(launch_spatial_moments(s, V, ldv, g.n, K, g.perm, Z, part, mean, out + s.sums.m2, m4, st));

    long long* deg_part = reinterpret_cast<long long*>(part);
    launch_lag_for(s, 1, 0, Z, g, mean, K, lag, nbr_mean, deg_part, st);
    FDX_CHECK_LAUNCH();
    hipLaunchKernelGGL(ss_reduce_kernel<long long>, dim3(1), dim3(256), 0, st, deg_part, s.lag_blocks, 2LL, 1LL, counts);
    FDX_CHECK_LAUNCH();

    hipLaunchKernelGGL(ss_cross_kernel, dim3(s.cross_blocks, s.pair_tiles_1d * s.pair_tiles_1d), dim3(256), 0, st, Z, lag, s.ld,
                       s.n_slices, K, s.pair_tiles_1d, part, 0LL, 0LL);
    FDX_CHECK_LAUNCH();
    hipLaunchKernelGGL(ss_reduce_kernel<double>, dim3(ceil_div((long long)KK, 256)), dim3(256), 0, st, part, s.cross_blocks,
                       (long long)KK, 1.0, C);
    FDX_CHECK_LAUNCH();
    return 0;
}

// A permutation-null call (fdx_spatial_perm_dev): the observed plan, the batch B of permutations per launch chain - what a scratch
// budget of 1 GiB holds, 512 at the most, capped by max_batch (0: no cap) and n_perm, one at the least - and its buffers.  The
// packed result is s.sums.perm_doubles doubles.
struct SpatialPermPlan {
    SpatialStatsPlan s;
    int batch;
    size_t plane_doubles;        // K * ld: the Z (and lag) planes of one batch element
    size_t cross_part_doubles;   // cross partials of one batch element
    size_t part_doubles;         // partials block: the observed pass's or the batch's cross partials, whichever is larger
    size_t null_doubles;         // B * K * K when the caller keeps no null (own_null), else 0
    size_t scratch_doubles;      // [Z B planes | lag B planes | partials | C_r of a batch]
};

static SpatialPermPlan spatial_perm_plan(long long n, int K, long long n_perm, int max_batch, bool own_null) {
    SpatialPermPlan p;
    p.s = spatial_stats_plan(n, K);
    const size_t KK = (size_t)K * K;
    p.plane_doubles = (size_t)K * p.s.ld;
    p.cross_part_doubles = (size_t)p.s.cross_blocks * KK;
    // per permutation in flight: its Z and lag planes, its cross partials and, where the caller keeps no null, its C_r
    const size_t per_perm = (2 * p.plane_doubles + p.cross_part_doubles + KK) * sizeof(double);
    const long long B = perm_batch((long long)(SCRATCH_BUDGET_BYTES / per_perm), SS_PERM_MAX_BATCH, max_batch, n_perm);
    p.batch = (int)B;
    p.part_doubles = std::max(p.s.partials_doubles, (size_t)B * p.cross_part_doubles);
    p.null_doubles = own_null ? (size_t)B * KK : 0;
    p.scratch_doubles = 2 * (size_t)B * p.plane_doubles + p.part_doubles + p.null_doubles;
    return p;
}

// The observed pass, m4, then permutations first_perm .. first_perm + n_perm - 1 of `seed` in batches; null_dev (n_perm, K, K)
// device or null.  Everything is left in out (device) as p.s.sums lays it out.
static int launch_spatial_perm(const SpatialPermPlan& p, const double* V, long long ldv, int K, const GraphTables& g,
                               unsigned long long seed, long long first_perm, long long n_perm, double* null_dev, double* scratch,
                               double* out, hipStream_t st) {
    const int n = g.n;
    if (n <= 0) return 0;
    const SpatialStatsPlan& s = p.s;
    const size_t KK = s.sums.KK;
    const int B = p.batch;
    double* Zall = scratch;
    double* lagall = Zall + (size_t)B * p.plane_doubles;
    double* part = lagall + (size_t)B * p.plane_doubles;
    double* own_null = part + p.part_doubles;
    double* mean = out + s.sums.mean;
    double* C_obs = out + s.sums.C;
    long long* count_ge = reinterpret_cast<long long*>(out + s.sums.count_ge);
    long long* count_le = reinterpret_cast<long long*>(out + s.sums.count_le);
    double* sum_d = out + s.sums.sum_d;
    double* sumsq_d = out + s.sums.sumsq_d;

    // the observed statistics in batch element 0's planes, m4 from its Z among them (the permutations overwrite it)
    FDX_TRY(launch_spatial_stats(s, V, ldv, K, g, scratch, B, out, nullptr, out + s.sums.m4, st));
    FDX_HIP(hipMemsetAsync(count_ge, 0, (s.sums.perm_doubles - s.sums.count_ge) * sizeof(double), st));   // the counts and the sums of d
    if (n_perm <= 0) return 0;

    SsPermArgs pa{perm_keys(seed, first_perm, n), (long long)p.plane_doubles};
    const size_t lds = (size_t)4 * 64 * SS_KS * sizeof(double);
    FDX_HIP(hipFuncSetAttribute((const void*)ss_centre_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int tiles = s.pair_tiles_1d * s.pair_tiles_1d;
    for (long long done = 0; done < n_perm; done += B) {
        const int b = (int)std::min<long long>(B, n_perm - done);       // the last batch may be ragged
        pa.keys.first = first_perm + done;
        hipLaunchKernelGGL(ss_centre_kernel<true>, dim3(s.centre_blocks, b), dim3(256), lds, st, V, ldv, mean, g.perm, n,
                           (int)(s.ld / 64), K, Zall, s.ld, (double*)nullptr, pa);
        FDX_CHECK_LAUNCH();
        launch_lag_for(s, b, pa.plane_stride, Zall, g, mean, K, lagall, nullptr, nullptr, st);
        FDX_CHECK_LAUNCH();
        hipLaunchKernelGGL(ss_cross_kernel, dim3(s.cross_blocks, tiles, b), dim3(256), 0, st, Zall, lagall, s.ld, s.n_slices, K,
                           s.pair_tiles_1d, part, pa.plane_stride, pa.plane_stride);
        FDX_CHECK_LAUNCH();
        double* Cr = null_dev ? null_dev + (size_t)done * KK : own_null;
        hipLaunchKernelGGL(ss_reduce_batch_kernel, dim3(ceil_div((long long)KK, 256), b), dim3(256), 0, st, part, s.cross_blocks,
                           (long long)KK, Cr);
        FDX_CHECK_LAUNCH();
        hipLaunchKernelGGL(ss_perm_accum_kernel, dim3(ceil_div((long long)KK, 256)), dim3(256), 0, st, Cr, b, (long long)KK, C_obs,
                           count_ge, count_le, sum_d, sumsq_d);
        FDX_CHECK_LAUNCH();
    }
    return 0;
}

}  // namespace fdx

using namespace fdx;

extern "C" {

int fdx_spatial_autocorr_dev(const fdx_graph* g, const double* V_dev, int64_t ldv, int32_t K, double* mean_out, double* m2_out,
                             double* C_out, int64_t* counts_out, double* neighbor_mean_dev, void* stream) {
    FDX_REQUIRE(g && V_dev && mean_out && m2_out && C_out && counts_out, "fdx_spatial_autocorr_dev: null argument");
    FDX_REQUIRE(K >= 1 && ldv >= K, "fdx_spatial_autocorr_dev: K must be positive and ldv at least K");
    GraphTables t;
    FDX_TRY(whole_graph_tables(g, "fdx_spatial_autocorr_dev", &t));
    hipStream_t st = (hipStream_t)stream;
    PoolStream pool_stream(st);
    counts_out[0] = t.n;
    counts_out[1] = counts_out[2] = 0;
    if (t.n == 0) {
        SpatialSumsLayout(K).fill_empty(mean_out, m2_out, C_out);
        return 0;
    }
    const SpatialStatsPlan plan = spatial_stats_plan(t.n, K);
    DevBuf scratch, out;
    FDX_TRY(scratch.alloc(plan.scratch_doubles * sizeof(double)));
    FDX_TRY(out.alloc(plan.sums.observed_doubles * sizeof(double)));
    FDX_TRY(launch_spatial_stats(plan, V_dev, ldv, K, t, scratch.as<double>(), 1, out.as<double>(), neighbor_mean_dev, nullptr, st));
    std::vector<double> host(plan.sums.observed_doubles);
    FDX_TRY(copy_d2h(host.data(), out.p, host.size() * sizeof(double), st));   // the call's one host synchronisation
    plan.sums.unpack(host.data(), mean_out, m2_out, C_out, counts_out + 1);
    return 0;
}

int fdx_spatial_perm_dev(const fdx_graph* g, const double* V_dev, int64_t ldv, int32_t K, uint64_t seed, int64_t first_perm,
                         int64_t n_perm, int32_t max_batch, double* null_dev, double* mean_out, double* m2_out, double* C_out,
                         int64_t* counts_out, double* m4_out, int64_t* count_ge_out, int64_t* count_le_out, double* sum_d_out,
                         double* sumsq_d_out, int32_t* batch_out, void* stream) {
    FDX_REQUIRE(g && V_dev && mean_out && m2_out && C_out && counts_out && m4_out && count_ge_out && count_le_out && sum_d_out &&
                    sumsq_d_out,
                "fdx_spatial_perm_dev: null argument");
    FDX_REQUIRE(K >= 1 && ldv >= K, "fdx_spatial_perm_dev: K must be positive and ldv at least K");
    FDX_REQUIRE(first_perm >= 0 && n_perm >= 0 && max_batch >= 0,
                "fdx_spatial_perm_dev: first_perm, n_perm and max_batch must not be negative");
    GraphTables t;
    FDX_TRY(whole_graph_tables(g, "fdx_spatial_perm_dev", &t));
    hipStream_t st = (hipStream_t)stream;
    PoolStream pool_stream(st);
    const size_t KK = (size_t)K * K;
    counts_out[0] = t.n;
    counts_out[1] = counts_out[2] = 0;
    if (batch_out) *batch_out = 0;
    if (t.n == 0) {                                     // nothing to permute: every C_r equals C_obs = 0
        const SpatialSumsLayout empty(K);
        empty.fill_empty(mean_out, m2_out, C_out, m4_out);
        empty.NullSumsLayout::fill_empty(n_perm, count_ge_out, count_le_out, sum_d_out, sumsq_d_out);
        if (null_dev && n_perm > 0) FDX_HIP(hipMemsetAsync(null_dev, 0, (size_t)n_perm * KK * sizeof(double), st));
        return 0;
    }
    const SpatialPermPlan plan = spatial_perm_plan(t.n, K, n_perm, max_batch, null_dev == nullptr);
    if (batch_out) *batch_out = n_perm > 0 ? plan.batch : 0;
    DevBuf scratch, out;
    FDX_TRY(scratch.alloc(plan.scratch_doubles * sizeof(double)));
    FDX_TRY(out.alloc(plan.s.sums.perm_doubles * sizeof(double)));
    FDX_TRY(launch_spatial_perm(plan, V_dev, ldv, K, t, seed, first_perm, n_perm, null_dev, scratch.as<double>(), out.as<double>(), st));
    std::vector<double> host(plan.s.sums.perm_doubles);
    FDX_TRY(copy_d2h(host.data(), out.p, host.size() * sizeof(double), st));   // the call's one host synchronisation
    plan.s.sums.unpack(host.data(), mean_out, m2_out, C_out, counts_out + 1, m4_out, count_ge_out, count_le_out, sum_d_out,
                       sumsq_d_out);
    return 0;
}

// out_dev[i] = pi_r(i), i < n: the permutation the kernels above apply
int fdx_permutation_indices_dev(uint64_t seed, int64_t r, int64_t n, int32_t* out_dev, void* stream) {
    FDX_REQUIRE(n >= 0 && n < (1LL << 31) - 128, "fdx_permutation_indices_dev: n must be between 0 and 2^31 - 129");
    FDX_REQUIRE(r >= 0, "fdx_permutation_indices_dev: r must not be negative");
    FDX_REQUIRE(n == 0 || out_dev, "fdx_permutation_indices_dev: null argument");
    if (n == 0) return 0;
    const PermKeys keys = perm_keys(seed, r, n);
    hipLaunchKernelGGL(ss_perm_indices_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, perm_key_at(keys, 0), (int)n,
                       keys.wl, keys.wr, out_dev);
    FDX_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
