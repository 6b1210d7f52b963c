// k-means of per-spot feature rows (spatial niches; not in the reference).  F is the (n, D) row-major feature matrix with row
// stride ldf >= D (columns D .. ldf - 1 are never read), M the (C, D) centres, 1 <= C <= 64.  Everywhere
//   d2(i, c) = sum_k (F_ik - M_ck)^2,   the difference formed first, accumulated by fma in ascending k from 0
// (the expanded form |v|^2 - 2 v.m + |m|^2 cancels on nearly collinear proportions and is not used).
//
// Three kernels, float64 throughout, no floating-point atomics; every grid is a function of the shapes only and every sum is taken
// in a fixed order, so two calls on the same inputs return the same bits.
//   distance     (assign and seed distance: one template)  a workgroup owns 256 consecutive rows, one 64-row slice per wave, lane =
//                row.  The slice is staged 32 columns at a time through a [64][33] LDS tile (rows of F are read as whole segments,
//                the odd stride makes the per-row reads conflict free); the CC centres of the walk sit beside it in LDS and are read
//                as broadcasts into CC register accumulators per lane (CC = 8 or 16 from C; more centres walk the columns again -
//                centres past C - 1 repeat the last one: computed, not kept).  assign: label = the smallest c attaining the minimum,
//                the rows whose label changed (int64) and sum_i d2(i, label_i) per workgroup.  seed distance (CC = 1):
//                d2_i = min(d2_i, d2(i, m)) and its sum per workgroup.  Workgroup partials are added in index order by one
//                workgroup (assign) or per fixed block of R rows (seed distance; R a multiple of 256 and a function of n only).
//   label sums   the thread layout of the column sums of spatial_stats_kernels.cpp (256 / D rows in flight, consecutive threads on
//                consecutive addresses of a row); every thread keeps C private accumulators acc[c][thread] in LDS and adds its rows
//                in ascending order; row slots, then workgroups, are added in index order.  Labels outside 0 .. C - 1 are skipped.
//                Counts are int64 from a second walk over the labels alone.
//   reduce       sums[c][k] and counts[c] from the partials and, on request, centres[c] = sums[c] / counts[c] where counts[c] > 0
//                (an empty niche keeps its centre).
#include "fdx_internal.h"
#include "fdx_kernels.h"

#include <algorithm>
#include <string>
#include <vector>

namespace fdx {

constexpr int KM_DT = 32;                   // distance: columns staged at a time
constexpr int KM_DS = KM_DT + 1;            //           odd row stride of the [row][column] tile
constexpr int KM_ROWS = 256;                //           rows of a workgroup (4 waves x 64)
constexpr int KM_SEED_CAP = 1024;           // seed distance: most blocks of R rows
constexpr int KM_SUMS_CAP = 1024;           // label sums: most workgroups ...
constexpr size_t KM_SUMS_PARTIALS = 1 << 20;   // ... and most doubles of their partials (8 MB)

// Dynamic LDS: 4 tiles [64][KM_DS], then the centres of the walk [CC][KM_DT].
template <int CC, bool SEED>
__global__ __launch_bounds__(256) void km_dist_kernel(const double* __restrict__ F, long long ldf, int n, int D,
                                                      const double* __restrict__ M, int C, int* __restrict__ labels,
                                                      double* __restrict__ min_d2, double* __restrict__ d2_io,
                                                      long long* __restrict__ changed_part, double* __restrict__ sum_part) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    __shared__ double red_s[4];
    __shared__ long long red_c[4];
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double* tile = smem + (size_t)wib * 64 * KM_DS;
    double* ms = smem + (size_t)4 * 64 * KM_DS;
    const long long slice0 = (long long)blockIdx.x * KM_ROWS + wib * 64;
    const long long row = slice0 + lane;
    const bool active = row < n;

    double best = __builtin_inf();
    int best_c = 0;
    for (int c0 = 0; c0 < C; c0 += CC) {
        double acc[CC];
#pragma unroll
        for (int j = 0; j < CC; ++j) acc[j] = 0.0;
        for (int k0 = 0; k0 < D; k0 += KM_DT) {
            const int kc = D - k0 < KM_DT ? D - k0 : KM_DT;
            __syncthreads();                                       // the previous chunk's readers of ms and the tiles are done
            for (int f = threadIdx.x; f < CC * kc; f += 256) {
                const int j = f / kc, k = f - j * kc;
                const int c = c0 + j < C ? c0 + j : C - 1;
                ms[j * KM_DT + k] = M[(size_t)c * D + k0 + k];
            }
            // element f = lane + 64 i of the wave's 64 x kc block: (row, column) advance by (64 / kc, 64 % kc) with a carry; the
            // lanes of one load cover whole row segments of kc doubles
            const int total = 64 * kc;
            const int ds = 64 / kc, dk = 64 - ds * kc;
            int sp = lane / kc, k = lane - sp * kc;
#pragma unroll 4
            for (int f = lane; f < total; f += 64) {
                const long long r = slice0 + sp;
                tile[sp * KM_DS + k] = r < n ? F[(size_t)r * ldf + k0 + k] : 0.0;
                sp += ds;
                k += dk;
                if (k >= kc) { k -= kc; ++sp; }
            }
            __syncthreads();
#pragma unroll 4
            for (int kk = 0; kk < kc; ++kk) {
                const double x = tile[lane * KM_DS + kk];
#pragma unroll
                for (int j = 0; j < CC; ++j) {
                    const double d = x - ms[j * KM_DT + kk];
                    acc[j] = fma(d, d, acc[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < CC; ++j)
            if (c0 + j < C && acc[j] < best) { best = acc[j]; best_c = c0 + j; }
    }

    double s = 0.0;
    long long ch = 0;
    if (active) {
        if (SEED) {
            const double old = d2_io[row];
            s = best < old ? best : old;
            d2_io[row] = s;
        } else {
            ch = labels[row] != best_c;
            labels[row] = best_c;
            if (min_d2) min_d2[row] = best;
            s = best;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_xor(s, off, 64);
        ch += __shfl_xor(ch, off, 64);
    }
    if (lane == 0) { red_s[wib] = s; red_c[wib] = ch; }
    __syncthreads();
    if (threadIdx.x == 0) {
        sum_part[blockIdx.x] = ((red_s[0] + red_s[1]) + red_s[2]) + red_s[3];
        if (!SEED) changed_part[blockIdx.x] = red_c[0] + red_c[1] + red_c[2] + red_c[3];
    }
}

// out_sum[b] = sum_part[b * per] + ... + sum_part[b * per + per - 1] (those below nparts), and the same for the changed counts
// (null: not wanted).  One workgroup per b: thread t adds its parts t, t + 256, ... in ascending order, then thread 0 the 256
// running sums in thread order.
__global__ __launch_bounds__(256) void km_reduce_parts_kernel(const double* __restrict__ sum_part,
                                                              const long long* __restrict__ changed_part, int nparts, int per,
                                                              double* __restrict__ out_sum, long long* __restrict__ out_changed) {
    __shared__ double rs[256];
    __shared__ long long rc[256];
    const long long p0 = (long long)blockIdx.x * per;
    const long long p1 = p0 + per < nparts ? p0 + per : nparts;
    double s = 0.0;
    long long c = 0;
    for (long long p = p0 + threadIdx.x; p < p1; p += 256) {
        s += sum_part[p];
        if (changed_part) c += changed_part[p];
    }
    rs[threadIdx.x] = s;
    rc[threadIdx.x] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        long long tc = 0;
        for (int j = 0; j < 256; ++j) { t += rs[j]; tc += rc[j]; }
        out_sum[blockIdx.x] = t;
        if (out_changed) out_changed[blockIdx.x] = tc;
    }
}

// partials[b][c][k] = sum of F[r][k] over block b's rows r with labels[r] == c; cnt_partials[b][c] = how many.  F null: counts only.
// Dynamic LDS: acc[C][256] doubles (reused as int64 for the counts).
__global__ __launch_bounds__(256) void km_label_sums_kernel(const double* __restrict__ F, long long ldf,
                                                            const int* __restrict__ labels, int n, int D, int C, int rows_per_block,
                                                            double* __restrict__ partials, long long* __restrict__ cnt_partials) {
    extern __shared__ __attribute__((aligned(16))) double acc[];
    const long long r0 = (long long)blockIdx.x * rows_per_block;
    const long long r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
    if (F) {
        for (int c0 = 0; c0 < D; c0 += 256) {
            const int Kc = D - c0 < 256 ? D - c0 : 256;
            const int rpp = 256 / Kc;
            const int c = threadIdx.x % Kc, rs = threadIdx.x / Kc;
            for (int j = 0; j < C; ++j) acc[j * 256 + threadIdx.x] = 0.0;
            if (rs < rpp)
                for (long long r = r0 + rs; r < r1; r += rpp) {
                    const int lab = labels[r];
                    if ((unsigned)lab < (unsigned)C) acc[lab * 256 + threadIdx.x] += F[(size_t)r * ldf + c0 + c];
                }
            __syncthreads();
            for (int o = threadIdx.x; o < C * Kc; o += 256) {
                const int j = o / Kc, cc = o - j * Kc;
                double t = 0.0;
                for (int q = 0; q < rpp; ++q) t += acc[j * 256 + q * Kc + cc];
                partials[((size_t)blockIdx.x * C + j) * D + c0 + cc] = t;
            }
            __syncthreads();
        }
    }
    long long* cnt = reinterpret_cast<long long*>(acc);
    for (int j = 0; j < C; ++j) cnt[j * 256 + threadIdx.x] = 0;
    for (long long r = r0 + threadIdx.x; r < r1; r += 256) {
        const int lab = labels[r];
        if ((unsigned)lab < (unsigned)C) cnt[lab * 256 + threadIdx.x] += 1;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < C; j += 256) {
        long long t = 0;
        for (int q = 0; q < 256; ++q) t += cnt[j * 256 + q];
        cnt_partials[(size_t)blockIdx.x * C + j] = t;
    }
}

// Thread i = (c, k) of C x D (C x 1 when partials is null): counts[c] and sums[c][k] from the partials in block order;
// centres (may be null): centres[c][k] = sums[c][k] / counts[c] where counts[c] > 0.
__global__ __launch_bounds__(256) void km_reduce_sums_kernel(const double* __restrict__ partials,
                                                             const long long* __restrict__ cnt_partials, int nparts, int C, int D,
                                                             double* __restrict__ sums, long long* __restrict__ counts,
                                                             double* __restrict__ centres) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long width = (long long)C * D;
    if (i >= width) return;
    const int c = (int)(i / D), k = (int)(i - (long long)c * D);
    long long cnt = 0;
    for (int b = 0; b < nparts; ++b) cnt += cnt_partials[(size_t)b * C + c];
    if (k == 0) counts[c] = cnt;
    if (!partials) return;
    double s = 0.0;
    for (int b = 0; b < nparts; ++b) s += partials[(size_t)b * width + i];
    sums[i] = s;
    if (centres && cnt > 0) centres[i] = s / (double)cnt;
}

// Grids and scratch of the k-means kernels on n rows, D columns and C centres (functions of the shapes only).
struct KmeansPlan {
    int dist_blocks;             // workgroups of the assign / seed-distance kernel: 256 rows each
    int seed_per, seed_blocks;   // seed distance: workgroups per block of seed_rows rows, and how many such blocks (<= 1024)
    long long seed_rows;
    int sums_blocks, rows_per_block;   // label sums
    size_t dist_part_bytes;      // scratch of an assign / seed-distance launch
    size_t sums_part_bytes;      // scratch of a label-sums launch
};

static KmeansPlan kmeans_plan(long long n, int D, int C) {
    KmeansPlan p;
    p.dist_blocks = std::max(1, ceil_div(n, KM_ROWS));
    p.seed_per = std::max(1, ceil_div(p.dist_blocks, KM_SEED_CAP));
    p.seed_rows = (long long)p.seed_per * KM_ROWS;
    p.seed_blocks = ceil_div(p.dist_blocks, p.seed_per);
    const size_t CD = (size_t)C * D;
    const long long cap = std::min<long long>(KM_SUMS_CAP, std::max<size_t>(1, KM_SUMS_PARTIALS / CD));
    p.sums_blocks = (int)std::min<long long>(cap, std::max<long long>(1, ceil_div(n, 1024)));
    p.rows_per_block = std::max(1, ceil_div(n, p.sums_blocks));
    p.sums_blocks = std::max(1, ceil_div(n, p.rows_per_block));
    p.dist_part_bytes = (size_t)p.dist_blocks * 16;
    p.sums_part_bytes = (size_t)p.sums_blocks * (CD + C) * 8;
    return p;
}

static size_t km_dist_lds_bytes(int cc) { return ((size_t)4 * 64 * KM_DS + (size_t)cc * KM_DT) * sizeof(double); }

template <int CC, bool SEED>
static int launch_dist(const KmeansPlan& p, const double* F, long long ldf, int n, int D, const double* M, int C, int* labels,
                       double* min_d2, double* d2_io, long long* changed_part, double* sum_part, hipStream_t st) {
    const size_t lds = km_dist_lds_bytes(CC);
    FDX_HIP(hipFuncSetAttribute((const void*)km_dist_kernel<CC, SEED>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((km_dist_kernel<CC, SEED>), dim3(p.dist_blocks), dim3(256), lds, st, F, ldf, n, D, M, C, labels, min_d2,
                       d2_io, changed_part, sum_part);
    FDX_CHECK_LAUNCH();
    return 0;
}

// labels[i] = arg-min over c of d2(i, c) (smallest c), min_d2 (may be null); to the device: changed_out[0] = rows whose label
// differs from the previous content of labels, inertia_out[0] = sum_i d2(i, label_i).
static int launch_kmeans_assign(const KmeansPlan& p, const double* F, long long ldf, int n, int D, const double* M, int C,
                                int* labels, double* min_d2, void* dist_part, long long* changed_out, double* inertia_out, hipStream_t st) {
    double* sum_part = reinterpret_cast<double*>(dist_part);
    long long* changed_part = reinterpret_cast<long long*>(sum_part + p.dist_blocks);
    if (C <= 8) FDX_TRY((launch_dist<8, false>(p, F, ldf, n, D, M, C, labels, min_d2, nullptr, changed_part, sum_part, st)));
    else FDX_TRY((launch_dist<16, false>(p, F, ldf, n, D, M, C, labels, min_d2, nullptr, changed_part, sum_part, st)));
    hipLaunchKernelGGL(km_reduce_parts_kernel, dim3(1), dim3(256), 0, st, sum_part, changed_part, p.dist_blocks, p.dist_blocks,
                       inertia_out, changed_out);
    FDX_CHECK_LAUNCH();
    return 0;
}

// d2[i] = min(d2[i], d2(i, m)); block_sums[b] (device, p.seed_blocks of them) = sum of d2 over rows [b * seed_rows, ...).
static int launch_kmeans_seed_dist(const KmeansPlan& p, const double* F, long long ldf, int n, int D, const double* m,
                                   double* d2, void* dist_part, double* block_sums, hipStream_t st) {
    double* sum_part = reinterpret_cast<double*>(dist_part);
    FDX_TRY((launch_dist<1, true>(p, F, ldf, n, D, m, 1, nullptr, nullptr, d2, nullptr, sum_part, st)));
    hipLaunchKernelGGL(km_reduce_parts_kernel, dim3(p.seed_blocks), dim3(256), 0, st, sum_part, (const long long*)nullptr,
                       p.dist_blocks, p.seed_per, block_sums, (long long*)nullptr);
    FDX_CHECK_LAUNCH();
    return 0;
}

// sums (C, D) and counts (C) per label (device); F null: counts only (sums untouched).  centres (may be null): rows with a
// positive count become sums / counts.  The plan's C and D must be the ones passed here.
static int launch_label_sums(const KmeansPlan& p, const double* F, long long ldf, const int* labels, int n, int D, int C,
                             void* sums_part, double* sums, long long* counts, double* centres, hipStream_t st) {
    double* partials = reinterpret_cast<double*>(sums_part);
    long long* cnt_partials = reinterpret_cast<long long*>(partials + (size_t)p.sums_blocks * C * D);
    const size_t lds = (size_t)C * 256 * sizeof(double);
    if (lds > 64 * 1024)
        FDX_HIP(hipFuncSetAttribute((const void*)km_label_sums_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(km_label_sums_kernel, dim3(p.sums_blocks), dim3(256), lds, st, F, ldf, labels, n, D, C, p.rows_per_block,
                       partials, cnt_partials);
    FDX_CHECK_LAUNCH();
    const long long width = F ? (long long)C * D : (long long)C;
    hipLaunchKernelGGL(km_reduce_sums_kernel, dim3(ceil_div(width, 256)), dim3(256), 0, st, F ? partials : (const double*)nullptr,
                       cnt_partials, p.sums_blocks, C, F ? D : 1, sums, counts, centres);
    FDX_CHECK_LAUNCH();
    return 0;
}

}  // namespace fdx

using namespace fdx;

// the shape checks the k-means entries share; `who` names the entry in the message
static int kmeans_check_shape(const char* who, int64_t ldf, int64_t n, int32_t D, int32_t C, bool centres_are_rows) {
    const std::string w(who);
    FDX_REQUIRE(D >= 1, w + ": D must be positive");
    FDX_REQUIRE(ldf >= D, w + ": ldf must be at least D");
    FDX_REQUIRE(C >= 1 && C <= 64, w + ": C must be between 1 and 64");
    FDX_REQUIRE(n >= 0 && n < (1LL << 31) - 128, w + ": too many rows");
    if (centres_are_rows) FDX_REQUIRE(C <= n, w + ": C must not exceed n");
    return 0;
}

extern "C" {

int fdx_kmeans_assign_dev(const double* F_dev, int64_t ldf, int64_t n, int32_t D, const double* centres_dev, int32_t C,
                          int32_t* labels_dev, double* min_d2_dev, int64_t* changed_out, double* inertia_out, void* stream) {
    FDX_REQUIRE(F_dev && centres_dev && labels_dev && changed_out && inertia_out, "fdx_kmeans_assign_dev: null argument");
    FDX_TRY(kmeans_check_shape("fdx_kmeans_assign_dev", ldf, n, D, C, true));
    hipStream_t st = (hipStream_t)stream;
    PoolStream pool_stream(st);
    const KmeansPlan plan = kmeans_plan(n, D, C);
    DevBuf part, out;
    FDX_TRY(part.alloc(plan.dist_part_bytes));
    FDX_TRY(out.alloc(16));
    FDX_TRY(launch_kmeans_assign(plan, F_dev, ldf, (int)n, D, centres_dev, C, labels_dev, min_d2_dev, part.p, out.as<long long>(),
                                 out.as<double>() + 1, st));
    unsigned char host[16];
    FDX_TRY(copy_d2h(host, out.p, 16, st));            // the call's one host synchronisation
    std::memcpy(changed_out, host, 8);
    std::memcpy(inertia_out, host + 8, 8);
    return 0;
}

int fdx_label_sums_dev(const double* F_dev, int64_t ldf, int64_t n, int32_t D, const int32_t* labels_dev, int32_t C,
                       double* sums_out, int64_t* counts_out, void* stream) {
    FDX_REQUIRE(sums_out && counts_out && (n == 0 || (F_dev && labels_dev)), "fdx_label_sums_dev: null argument");
    FDX_TRY(kmeans_check_shape("fdx_label_sums_dev", ldf, n, D, C, false));
    const size_t CD = (size_t)C * D;
    std::fill(sums_out, sums_out + CD, 0.0);
    std::fill(counts_out, counts_out + C, (int64_t)0);
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    PoolStream pool_stream(st);
    const KmeansPlan plan = kmeans_plan(n, D, C);
    DevBuf part, out;
    FDX_TRY(part.alloc(plan.sums_part_bytes));
    FDX_TRY(out.alloc((CD + C) * 8));
    FDX_TRY(launch_label_sums(plan, F_dev, ldf, labels_dev, (int)n, D, C, part.p, out.as<double>(),
                              reinterpret_cast<long long*>(out.as<double>() + CD), nullptr, st));
    std::vector<double> host(CD + C);
    FDX_TRY(copy_d2h(host.data(), out.p, (CD + C) * 8, st));
    std::copy(host.begin(), host.begin() + CD, sums_out);
    std::memcpy(counts_out, host.data() + CD, (size_t)C * 8);
    return 0;
}

int fdx_kmeans_seed_dist_dev(const double* F_dev, int64_t ldf, int64_t n, int32_t D, const double* centre_dev, double* d2_dev,
                             double* block_sums_out, int64_t* block_rows_out, int32_t* n_blocks_out, void* stream) {
    FDX_REQUIRE(F_dev && centre_dev && d2_dev && block_sums_out && block_rows_out && n_blocks_out,
                "fdx_kmeans_seed_dist_dev: null argument");
    FDX_TRY(kmeans_check_shape("fdx_kmeans_seed_dist_dev", ldf, n, D, 1, true));
    hipStream_t st = (hipStream_t)stream;
    PoolStream pool_stream(st);
    const KmeansPlan plan = kmeans_plan(n, D, 1);
    DevBuf part, out;
    FDX_TRY(part.alloc(plan.dist_part_bytes));
    FDX_TRY(out.alloc((size_t)plan.seed_blocks * 8));
    FDX_TRY(launch_kmeans_seed_dist(plan, F_dev, ldf, (int)n, D, centre_dev, d2_dev, part.p, out.as<double>(), st));
    FDX_TRY(copy_d2h(block_sums_out, out.p, (size_t)plan.seed_blocks * 8, st));
    *block_rows_out = plan.seed_rows;
    *n_blocks_out = plan.seed_blocks;
    return 0;
}

int fdx_kmeans_dev(const double* F_dev, int64_t ldf, int64_t n, int32_t D, int32_t C, int32_t max_iter, double* centres_dev,
                   int32_t* labels_dev, int64_t* counts_out, double* inertia_out, int32_t* n_iter_out, int32_t* converged_out,
                   void* stream) {
    FDX_REQUIRE(F_dev && centres_dev && labels_dev && counts_out && inertia_out && n_iter_out && converged_out,
                "fdx_kmeans_dev: null argument");
    FDX_TRY(kmeans_check_shape("fdx_kmeans_dev", ldf, n, D, C, true));
    FDX_REQUIRE(max_iter >= 1, "fdx_kmeans_dev: max_iter must be positive");
    hipStream_t st = (hipStream_t)stream;
    PoolStream pool_stream(st);
    const KmeansPlan plan = kmeans_plan(n, D, C);
    const size_t CD = (size_t)C * D;
    DevBuf dist_part, sums_part, out;
    FDX_TRY(dist_part.alloc(plan.dist_part_bytes));
    FDX_TRY(sums_part.alloc(plan.sums_part_bytes));
    FDX_TRY(out.alloc(16 + (CD + C) * 8));               // [changed | inertia | sums C*D | counts C]
    long long* changed_d = out.as<long long>();
    double* inertia_d = out.as<double>() + 1;
    double* sums_d = out.as<double>() + 2;
    long long* counts_d = reinterpret_cast<long long*>(sums_d + CD);
    FDX_HIP(hipMemsetAsync(labels_dev, 0xFF, (size_t)n * sizeof(int32_t), st));      // every label -1
    int it = 0, converged = 0;
    unsigned char host[16];
    for (;;) {
        ++it;
        FDX_TRY(launch_kmeans_assign(plan, F_dev, ldf, (int)n, D, centres_dev, C, labels_dev, nullptr, dist_part.p, changed_d,
                                     inertia_d, st));
        FDX_TRY(copy_d2h(host, out.p, 16, st));          // 16 bytes per iteration: the loop's only host synchronisation
        int64_t changed;
        std::memcpy(&changed, host, 8);
        if (changed == 0) { converged = 1; break; }
        if (it == max_iter) break;
        FDX_TRY(launch_label_sums(plan, F_dev, ldf, labels_dev, (int)n, D, C, sums_part.p, sums_d, counts_d, centres_dev, st));
    }
    FDX_TRY(launch_label_sums(plan, nullptr, ldf, labels_dev, (int)n, D, C, sums_part.p, sums_d, counts_d, nullptr, st));
    FDX_TRY(copy_d2h(counts_out, counts_d, (size_t)C * 8, st));
    std::memcpy(inertia_out, host + 8, 8);
    *n_iter_out = it;
    *converged_out = converged;
    return 0;
}

}  // extern "C"
