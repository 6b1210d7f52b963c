// Permutation test per gene for Moran's I and Geary's C (additive, not in the reference): for S distinct columns `genes` of a
// spot-by-gene matrix Y (n, G) over the model's graph - A its symmetric binary adjacency, deg_i = sum_j A_ij - and the permutations
// pi_r = permutation_indices(seed, r, n), r = first_perm .. first_perm + n_perm - 1 (perm_device.h), with v_i = y[pi_r(i)] in the
// caller's spot order, everything float64 on the value converted from storage:
//   null (n_perm, 3, S):   0 P_r = sum_i v_i sum_{j in N(i)} v_j      1 D_r = sum_i deg_i v_i      2 H_r = sum_i deg_i v_i^2
//   obs (7, S):            u = sum y, q = sum y^2, D, H, P (the identity in place of pi_r), ymin, ymax
// The statistics and the counting are the host's (flashdeconv_amd/utils/gene_permutations.py); include/fdx.h has the definitions.
//
// Stages.
//   gather   Yt = the wanted columns in the graph's POSITION order (position p holds the caller's spot perm[p]) in the storage type,
//            in tiles of TG genes, position-major inside a tile: Yt[tile][p][g] = Y[perm[p], genes[tile * TG + g]], 0 past S.  One
//            position's TG values are one 16-byte (float32, TG = 4) read, and a tile is one contiguous block, which is what the
//            LDS route copies.  CSR: the copy zeroed, then the stored entries scattered through a column-to-slot map (a wave per
//            position, a lane per stored entry).  A copy above max_gather_bytes (default SCRATCH_BUDGET_BYTES) goes in STRIPES of whole
//            tiles, one tile at the least.
//   tables   per permutation of a batch T_r[p] = inv[pi_r(perm[p])], the position whose value lands at position p (int32, inv the
//            inverse of perm): one Feistel evaluation (about 100 integer operations) per (r, p), shared by every gene.  The observed
//            sums use the identity table through the same null kernel, so they share its summation order.
//   null     a workgroup of 256 threads owns a tile of TG genes and a range of the batch's permutations.  Thread t walks the
//            positions p = t, t + 256, ... in ascending order; a wave therefore walks one ELL slice of 64 positions at a time and
//            its neighbour reads are coalesced.  Per position: i0 = T[p], the neighbours j of p from the sliced ELL exactly as
//            gs_stage_segment / gs_neighbour_row read them (dg = min(deg, slice width), pad and out-of-range indices skipped;
//            a hub simply loops longer, a slice of width 0 not at all), T[j], and the TG values at i0 and at every T[j].
//              route 2  (LDS, LDS table)  the tile's columns AND the permutation's table are in LDS: TG * elem * n + 4 n bytes.
//                       Every one of the R * n * (1 + deg) value gathers and index gathers is an LDS read; global memory serves
//                       the coalesced ELL reads and one coalesced copy of the table per permutation.
//              route 1  (LDS, global table)  n too large for the table to fit beside one column: the column in LDS (TG = 1), the
//                       table gathered through L2.
//              route 0  (global)  any n: the same loop reads Yt and the table through L2, TG = 4 (float64: 2).
//            TG is the largest of 4, 2, 1 (float64: of 2, 1) whose tile fits max_lds_bytes (the device's LDS per workgroup by
//            default): a position's values are at most 16 bytes.
//
// Choices, and why (DESIGN.md section 3 has the measurements):
//   * position-major tiles: the index T[j] is the expensive part of a gather (one LDS / L2 read per neighbour), and one index then
//     serves TG genes with a single wide read (ds_read_b128 moves twice the bytes per LDS cycle of ds_read_b32).
//   * the table in LDS: without it every neighbour costs a random 4-byte L2 read per TG genes, an order of magnitude more L2
//     requests than the pass has LDS reads; with it the tile is 20 n bytes (float32, TG = 4): n <= 8,100 spots keeps four genes
//     resident, n <= 13,600 two, n <= 20,400 one, and up to 40,000 the column alone (route 1).
//   * 256 threads a permutation, up to four permutations (WAYS) a workgroup: a workgroup that declares more than half of the
//     160 KiB runs alone on its CU, and 256 threads are one wave per SIMD - too few to hide the latency of the chain ELL read ->
//     table read -> value read, although a thread keeps 1 + 8 independent gathers in flight.  More threads on ONE permutation
//     would shorten each thread's walk (20 positions at n = 5,000) against a reduction of 3 TG values that does not shrink, and
//     would change the order; instead the LDS left beside the tile holds further tables (4 n bytes each) and every 256 threads
//     walk a permutation of their own over the shared columns: n = 5,000 runs 4 ways (16 waves a CU) in 161.5 KB.  A workgroup
//     never has more ways than permutations to walk.
//
//   * the grid runs the permutation ranges fastest and the tiles slowest, and the global route gives every workgroup ONE
//     permutation (it loads nothing of its own): the workgroups in flight together share a few tiles and find them in L2 /
//     Infinity Cache.  Tiles fastest: 513 ms for 99 permutations of 100,000 x 2,000 float32; this way: 385 ms.
//
// Order: no floating-point atomics.  Thread t adds its positions in ascending order with explicit fma, a neighbour sum in the
// stored neighbour order; the 256 partial sums are combined by a fixed tree (xor butterfly over the 64 lanes, then the four waves
// in order).  So EVERY (gene, permutation) SUM DEPENDS ONLY ON THE GRAPH, THE COLUMN AND THE PERMUTATION - not on the tile, the batch,
// the stripe, the route, the other genes or max_batch; two calls, a range of permutations split into calls and all routes return
// the same bits.
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "fdx_graph.h"
#include "fdx_internal.h"
#include "gene_gather.h"
#include "gene_pass.h"
#include "gene_walk.h"
#include "perm_device.h"

namespace fdx {
namespace {

constexpr int GP_THREADS = 256;
constexpr int GP_MAX_TILE = 4;                                            // genes of a tile: 16 bytes a position, so 4 float32 or 2 float64
// (four float64 genes would stage 8 neighbours x 32 bytes = 64 registers under the 128 of a 1024-thread workgroup, and spill)
constexpr int gp_max_tile(size_t elem) { return elem == sizeof(double) ? GP_MAX_TILE / 2 : GP_MAX_TILE; }
constexpr int GP_MAX_WAYS = 4;                                            // permutations a workgroup walks at a time, 256 threads each
constexpr int GP_WAY_RED_BYTES = 4 * 3 * GP_MAX_TILE * (int)sizeof(double);   // a way's four wave sums
constexpr int GP_RED_BYTES = GP_MAX_WAYS * GP_WAY_RED_BYTES;
constexpr int GP_ROUTE_GLOBAL = 0, GP_ROUTE_LDS = 1, GP_ROUTE_LDS_TABLE = 2;
constexpr size_t GP_DEVICE_LDS = 160 * 1024;                              // LDS a workgroup may declare on gfx950
constexpr int GP_TARGET_GROUPS = 2048;                                    // workgroups a launch aims at (8 per CU)

template <typename T, int TG>
struct alignas(sizeof(T) * TG) GpVec { T v[TG]; };

// (gene_gather.h: the gather kernels, shared with the label gene sums)

__global__ __launch_bounds__(256) void gp_inverse_kernel(const int* __restrict__ perm, int n, int* __restrict__ inv) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < n) inv[perm[p]] = p;
}

// tables[b][p] = inv[pi_r(perm[p])], r = keys' element b, for b < nb (identity: tables[0][p] = p); perm / inv null: the caller's order
__global__ __launch_bounds__(256) void gp_tables_kernel(const int* __restrict__ perm, const int* __restrict__ inv, int n, PermKeys keys,
                                                        bool identity, int* __restrict__ tables) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    int at = p;
    if (!identity) {
        const int src = ss_permute_index(perm_key_at(keys, blockIdx.y), perm ? perm[p] : p, n, keys.wl, keys.wr);
        at = inv ? inv[src] : src;
    }
    tables[(size_t)blockIdx.y * n + p] = at;
}

// p += step for a loop over p < n, in 32 bits although n may lie within `step` of 2^31: false where the loop ends.
__device__ __forceinline__ bool gp_step(int& p, int step, int n) {
    if (p >= n - step) return false;
    p += step;
    return true;
}

// The fixed tree of the file header over the 256 values (threads t = 0 .. 255 of one way) of each of CNT sums; the result in the v[]
// of the way's thread 0.  Every thread of the workgroup calls it (two barriers).
template <int CNT>
__device__ __forceinline__ void gp_block_sum(double (&v)[CNT], double* red, int t) {
#pragma unroll
    for (int k = 0; k < CNT; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);
    }
    const int w = t >> 6;
    __syncthreads();                                            // red's readers of the round before
    if ((t & 63) == 0) {
#pragma unroll
        for (int k = 0; k < CNT; ++k) red[w * CNT + k] = v[k];
    }
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int k = 0; k < CNT; ++k) v[k] = ((red[k] + red[CNT + k]) + red[2 * CNT + k]) + red[3 * CNT + k];
    }
}

// One permutation's sums of one tile: thread t of 256 over p = t, t + 256, ...; acc[3 g + {0, 1, 2}] = P, D, H of gene g.
template <typename T, int TG>
__device__ __forceinline__ void gp_walk(const GpVec<T, TG>* cols, const int* tab, const GraphTables& g, int t, double (&acc)[3 * TG]) {
    constexpr int NB = GS_NB;                                   // neighbours whose loads are in flight together, added in the stored order
    for (int p = t; p < g.n;) {
        const int w0 = g.slice_off[p >> 6];
        const int dg = min(g.deg[p], g.slice_off[(p >> 6) + 1] - w0);
        const GpVec<T, TG> own = cols[tab[p]];
        const int* row = g.ell + (size_t)w0 * 64 + (p & 63);
        double lag[TG];
#pragma unroll
        for (int k = 0; k < TG; ++k) lag[k] = 0.0;
        for (int m0 = 0; m0 < dg; m0 += NB) {
            GpVec<T, TG> nb[NB];
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const int j = m0 + i < dg ? row[(size_t)(m0 + i) * 64] : -1;
                if (j >= 0 && j < g.n) {
                    nb[i] = cols[tab[j]];
                } else {
#pragma unroll
                    for (int k = 0; k < TG; ++k) nb[i].v[k] = (T)0;
                }
            }
#pragma unroll
            for (int i = 0; i < NB; ++i) {
#pragma unroll
                for (int k = 0; k < TG; ++k) lag[k] += (double)nb[i].v[k];      // (x + 0 = x: an empty slot changes nothing)
            }
        }
        const double d = (double)dg;
#pragma unroll
        for (int k = 0; k < TG; ++k) {
            const double y = (double)own.v[k];
            acc[3 * k] = fma(y, lag[k], acc[3 * k]);
            acc[3 * k + 1] = fma(d, y, acc[3 * k + 1]);
            acc[3 * k + 2] = fma(d * y, y, acc[3 * k + 2]);
        }
        if (!gp_step(p, GP_THREADS, g.n)) break;
    }
}

// Workgroup (x, y): tile y of the stripe (genes s0 + y * TG ..), permutations [x * chunk, min(nb, (x + 1) * chunk)) of the batch
// (x runs fastest: the workgroups in flight together share few tiles, which the global route then finds in L2 / Infinity Cache),
// blockDim.x / 256 WAYS of them at a time: the 256 threads of way w walk permutation b + w with a table of their own, so the order
// of a (gene, permutation) sum does not know how many ways there are.  outP / outD / outH: element (b, s) at out[b * row_stride + s].
template <typename T, int TG, bool COLS_LDS, bool TAB_LDS>
__global__ __launch_bounds__(GP_THREADS * GP_MAX_WAYS) void gp_null_kernel(const T* __restrict__ Yt, const int* __restrict__ tables,
                                                                           GraphTables g, int s0, int S, int nb, int chunk,
                                                                           double* __restrict__ outP, double* __restrict__ outD,
                                                                           double* __restrict__ outH, long long row_stride) {
    extern __shared__ __attribute__((aligned(32))) unsigned char gp_smem[];
    typedef GpVec<T, TG> Vec;
    const int way = threadIdx.x >> 8, t = threadIdx.x & (GP_THREADS - 1), ways = blockDim.x >> 8;
    double* red = reinterpret_cast<double*>(gp_smem + way * GP_WAY_RED_BYTES);
    Vec* cols_sh = reinterpret_cast<Vec*>(gp_smem + GP_RED_BYTES);
    int* tab_sh = reinterpret_cast<int*>(gp_smem + GP_RED_BYTES + (COLS_LDS ? (size_t)g.n * sizeof(Vec) : 0)) + (size_t)way * g.n;
    const Vec* tile = reinterpret_cast<const Vec*>(Yt) + (size_t)blockIdx.y * g.n;
    if (COLS_LDS) {
        for (int p = threadIdx.x; p < g.n;) {
            cols_sh[p] = tile[p];
            if (!gp_step(p, (int)blockDim.x, g.n)) break;
        }
    }
    const int b0 = blockIdx.x * chunk, b1 = min(nb, b0 + chunk);
    const int gene0 = s0 + (int)blockIdx.y * TG;
    for (int bb = b0; bb < b1; bb += ways) {                    // (uniform over the workgroup: every thread meets every barrier)
        const int b = bb + way;
        const bool active = b < b1;
        const int* tab = tables + (size_t)(active ? b : b0) * g.n;
        double acc[3 * TG];
#pragma unroll
        for (int k = 0; k < 3 * TG; ++k) acc[k] = 0.0;
        if (TAB_LDS && active) {                                // (the way's walkers of the table before have passed gp_block_sum's barriers)
            for (int p = t; p < g.n;) {
                tab_sh[p] = tab[p];
                if (!gp_step(p, GP_THREADS, g.n)) break;
            }
        }
        if (COLS_LDS || TAB_LDS) __syncthreads();
        if (active) {
            if (COLS_LDS && TAB_LDS) gp_walk<T, TG>(cols_sh, tab_sh, g, t, acc);
            else if (COLS_LDS) gp_walk<T, TG>(cols_sh, tab, g, t, acc);
            else gp_walk<T, TG>(tile, tab, g, t, acc);
        }
        gp_block_sum<3 * TG>(acc, red, t);
        if (t == 0 && active) {
#pragma unroll
            for (int k = 0; k < TG; ++k) {
                if (gene0 + k < S) {
                    const size_t at = (size_t)b * row_stride + gene0 + k;
                    outP[at] = acc[3 * k];
                    outD[at] = acc[3 * k + 1];
                    outH[at] = acc[3 * k + 2];
                }
            }
        }
    }
}

// u, q, ymin, ymax of the stripe's genes from Yt in the null kernel's order (thread t over p = t, t + 256, ...; the fixed tree, min
// and max by the same tree); a workgroup per tile.  obs: the (7, S) planes.
template <typename T, int TG>
__global__ __launch_bounds__(GP_THREADS) void gp_moments_kernel(const T* __restrict__ Yt, int n, int s0, int S, double* __restrict__ obs) {
    __shared__ double red[4 * 2 * TG];
    __shared__ double ext[4][2 * TG];
    typedef GpVec<T, TG> Vec;
    const Vec* tile = reinterpret_cast<const Vec*>(Yt) + (size_t)blockIdx.x * n;
    double acc[2 * TG], mn[TG], mx[TG];
#pragma unroll
    for (int k = 0; k < TG; ++k) {
        acc[2 * k] = acc[2 * k + 1] = 0.0;
        mn[k] = INFINITY;
        mx[k] = -INFINITY;
    }
    for (long long p = threadIdx.x; p < n; p += GP_THREADS) {
        const Vec c = tile[p];
#pragma unroll
        for (int k = 0; k < TG; ++k) {
            const double y = (double)c.v[k];
            acc[2 * k] += y;
            acc[2 * k + 1] = fma(y, y, acc[2 * k + 1]);
            mn[k] = fmin(mn[k], y);
            mx[k] = fmax(mx[k], y);
        }
    }
#pragma unroll
    for (int k = 0; k < TG; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            mn[k] = fmin(mn[k], __shfl_xor(mn[k], off, 64));
            mx[k] = fmax(mx[k], __shfl_xor(mx[k], off, 64));
        }
        if ((threadIdx.x & 63) == 0) {
            ext[threadIdx.x >> 6][2 * k] = mn[k];
            ext[threadIdx.x >> 6][2 * k + 1] = mx[k];
        }
    }
    gp_block_sum<2 * TG>(acc, red, (int)threadIdx.x);           // (its barriers publish ext as well)
    if (threadIdx.x == 0) {
        const int gene0 = s0 + (int)blockIdx.x * TG;
#pragma unroll
        for (int k = 0; k < TG; ++k) {
            if (gene0 + k < S) {
                obs[gene0 + k] = acc[2 * k];
                obs[(size_t)S + gene0 + k] = acc[2 * k + 1];
                obs[5 * (size_t)S + gene0 + k] = fmin(fmin(ext[0][2 * k], ext[1][2 * k]), fmin(ext[2][2 * k], ext[3][2 * k]));
                obs[6 * (size_t)S + gene0 + k] = fmax(fmax(ext[0][2 * k + 1], ext[1][2 * k + 1]), fmax(ext[2][2 * k + 1], ext[3][2 * k + 1]));
            }
        }
    }
}

// counts[0 .. 1] = {sum dg, sum dg^2}, dg = min(deg, slice width) as the walk reads it: one workgroup, integers
__global__ __launch_bounds__(256) void gp_counts_kernel(GraphTables g, long long* __restrict__ counts) {
    __shared__ long long red[2][256];
    long long sd = 0, sd2 = 0;
    for (long long pp = threadIdx.x; pp < g.n; pp += 256) {
        const int p = (int)pp;
        const int w0 = g.slice_off[p >> 6];
        const long long dg = min(g.deg[p], g.slice_off[(p >> 6) + 1] - w0);
        sd += dg;
        sd2 += dg * dg;
    }
    red[0][threadIdx.x] = sd;
    red[1][threadIdx.x] = sd2;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            red[0][threadIdx.x] += red[0][threadIdx.x + off];
            red[1][threadIdx.x] += red[1][threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x < 2) counts[threadIdx.x] = red[threadIdx.x][0];
}

// How a call runs: the gene tile, the route, the permutations a workgroup walks at a time and the dynamic LDS of the null kernel.
struct GpPlan { int tile, route, ways; size_t lds; };
// What a launch of the null kernel ran with: permutations a workgroup walks at a time, permutations of a workgroup.
struct GpLaunch { int ways = 0, chunk = 0; };

// The largest tile of 4, 2, 1 genes whose columns and table fit `cap` bytes of LDS; else the column alone; else global memory.
GpPlan gp_plan(long long n, size_t elem, size_t cap) {
    for (int tg = gp_max_tile(elem); tg >= 1; tg >>= 1) {
        const size_t need = GP_RED_BYTES + (size_t)n * (tg * elem + sizeof(int));
        if (need > cap) continue;
        int ways = 1;                                           // further tables, while they fit: more waves to hide the gathers' latency
        while (ways < GP_MAX_WAYS && need + (size_t)ways * n * sizeof(int) <= cap) ++ways;
        return {tg, GP_ROUTE_LDS_TABLE, ways, need + (size_t)(ways - 1) * n * sizeof(int)};
    }
    const size_t need = GP_RED_BYTES + (size_t)n * elem;
    if (need <= cap) return {1, GP_ROUTE_LDS, GP_MAX_WAYS, need};
    return {gp_max_tile(elem), GP_ROUTE_GLOBAL, 1, (size_t)GP_RED_BYTES};
}

template <typename T, int TG, bool COLS_LDS, bool TAB_LDS>
int gp_launch_null_as(const GpPlan& plan, const T* Yt, const int* tables, const GraphTables& pos, int s0, int tiles, int S, int nb,
                      double* outP, double* outD, double* outH, long long row_stride, GpLaunch* ran, hipStream_t st) {
    auto* kernel = gp_null_kernel<T, TG, COLS_LDS, TAB_LDS>;
    if (plan.lds > 64 * 1024) FDX_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));
    // which permutations share a workgroup changes no bit: on the LDS routes enough workgroups to fill the chip, each loading its
    // tile once for many permutations; on the global route, where a workgroup loads nothing, one permutation each
    // - never fewer permutations a workgroup than it has ways: no 256 threads that only meet barriers
    const int ways_fit = std::min(plan.ways, nb);
    const int groups = COLS_LDS ? std::max(1, std::min(ceil_div(nb, ways_fit), ceil_div(GP_TARGET_GROUPS, tiles))) : nb;
    const int chunk = ceil_div(nb, groups);
    const int ways = std::min(ways_fit, chunk);
    hipLaunchKernelGGL(kernel, dim3((unsigned)ceil_div(nb, chunk), (unsigned)tiles), dim3(GP_THREADS * ways), plan.lds, st, Yt, tables, pos,
                       s0, S, nb, chunk, outP, outD, outH, row_stride);
    FDX_CHECK_LAUNCH();
    if (ran) *ran = GpLaunch{ways, chunk};
    return 0;
}

template <typename T>
int gp_launch_null(const GpPlan& plan, const T* Yt, const int* tables, const GraphTables& pos, int s0, int tiles, int S, int nb,
                   double* outP, double* outD, double* outH, long long row_stride, GpLaunch* ran, hipStream_t st) {
#define GP_CASE(TG, C, TB) return gp_launch_null_as<T, TG, C, TB>(plan, Yt, tables, pos, s0, tiles, S, nb, outP, outD, outH, row_stride, ran, st)
    if (plan.route == GP_ROUTE_GLOBAL) GP_CASE(gp_max_tile(sizeof(T)), false, false);
    if (plan.route == GP_ROUTE_LDS) GP_CASE(1, true, false);
    if constexpr (gp_max_tile(sizeof(T)) == 4) {
        if (plan.tile == 4) GP_CASE(4, true, true);
    }
    if (plan.tile == 2) GP_CASE(2, true, true);
    GP_CASE(1, true, true);
#undef GP_CASE
}

template <typename T, int TG>
int gp_gather_as(const GraphTables& t, const GeneMatrix& y, const T* data, const int* genes_dev, const int* slot_dev, int S, int s0,
                 int tiles, T* Yt, hipStream_t st) {
    return gather_gene_tiles<T, TG>(t.perm, t.n, y, data, genes_dev, slot_dev, S, s0, tiles, Yt, st);
}

template <typename T>
int gp_moments(int tg, const T* Yt, int n, int s0, int tiles, int S, double* obs, hipStream_t st) {
    if (tg == 4 && gp_max_tile(sizeof(T)) == 4)
        hipLaunchKernelGGL((gp_moments_kernel<T, gp_max_tile(sizeof(T))>), dim3((unsigned)tiles), dim3(GP_THREADS), 0, st, Yt, n, s0, S, obs);
    else if (tg == 2) hipLaunchKernelGGL((gp_moments_kernel<T, 2>), dim3((unsigned)tiles), dim3(GP_THREADS), 0, st, Yt, n, s0, S, obs);
    else hipLaunchKernelGGL((gp_moments_kernel<T, 1>), dim3((unsigned)tiles), dim3(GP_THREADS), 0, st, Yt, n, s0, S, obs);
    FDX_CHECK_LAUNCH();
    return 0;
}

struct GpRequest {
    const int32_t* genes;
    int S;
    unsigned long long seed;
    long long first_perm, n_perm, max_batch;
    size_t gather_bytes;                                        // what the gathered copy of a stripe may take
    double *obs, *null;
};
// What a call ran with (info_out): batch, stripes, and the first permutation launch's ways and chunk.
struct GpRan { int batch = 0, stripes = 0; GpLaunch first; };

// Everything of a call with t.n >= 1 spots, queued on st.  *batch_out / *stripes_out: what ran.
template <typename T>
int gp_run(const GraphTables& t, const GeneMatrix& y, const T* data, const GpRequest& q, const GpPlan& plan, GpRan* ran, hipStream_t st) {
    const int n = t.n, S = q.S, tg = plan.tile;
    const int tiles_all = ceil_div(S, tg);
    const size_t tile_bytes = (size_t)n * tg * sizeof(T);
    // grid y of the null kernel and the copy's budget bound a stripe's tiles, one tile at the least
    const int stripe_tiles = (int)std::max<size_t>(1, std::min<size_t>({(size_t)tiles_all, (size_t)65535, q.gather_bytes / tile_bytes}));
    // a table of n positions per permutation in flight; 65535: grid y of the tables kernel
    const long long batch = perm_batch((long long)(SCRATCH_BUDGET_BYTES / ((size_t)n * sizeof(int))), 65535, q.max_batch, q.n_perm);
    ran->batch = (int)batch;
    ran->stripes = ceil_div(tiles_all, stripe_tiles);

    DevBuf yt_buf, tab_buf, inv_buf, list_buf;
    FDX_TRY(yt_buf.alloc((size_t)stripe_tiles * tile_bytes));
    FDX_TRY(tab_buf.alloc((size_t)batch * n * sizeof(int)));
    std::vector<int> list;                                      // dense: the genes; CSR: the column-to-slot map
    if (y.sparse) {
        list.assign((size_t)y.G, -1);
        for (int s = 0; s < S; ++s) list[q.genes[s]] = s;
    } else {
        list.assign(q.genes, q.genes + S);
    }
    FDX_TRY(list_buf.alloc(list.size() * sizeof(int)));
    FDX_TRY(copy_h2d(list_buf.p, list.data(), list.size() * sizeof(int), st));
    const int* inv = nullptr;
    if (t.perm) {
        FDX_TRY(inv_buf.alloc((size_t)n * sizeof(int)));
        hipLaunchKernelGGL(gp_inverse_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, t.perm, n, inv_buf.as<int>());
        FDX_CHECK_LAUNCH();
        inv = inv_buf.as<int>();
    }
    GraphTables pos = t;
    pos.perm = nullptr;                                         // Yt is in the graph's order: rows are positions
    PermKeys keys = perm_keys(q.seed, q.first_perm, n);
    T* Yt = yt_buf.as<T>();
    int* tables = tab_buf.as<int>();
    for (int t0 = 0; t0 < tiles_all; t0 += stripe_tiles) {
        const int tiles = std::min(stripe_tiles, tiles_all - t0), s0 = t0 * tg;
        const int *genes_dev = y.sparse ? nullptr : list_buf.as<int>(), *slot_dev = y.sparse ? list_buf.as<int>() : nullptr;
        if (tg == 4 && gp_max_tile(sizeof(T)) == 4) FDX_TRY((gp_gather_as<T, gp_max_tile(sizeof(T))>(t, y, data, genes_dev, slot_dev, S, s0, tiles, Yt, st)));
        else if (tg == 2) FDX_TRY((gp_gather_as<T, 2>(t, y, data, genes_dev, slot_dev, S, s0, tiles, Yt, st)));
        else FDX_TRY((gp_gather_as<T, 1>(t, y, data, genes_dev, slot_dev, S, s0, tiles, Yt, st)));
        FDX_TRY(gp_moments(tg, Yt, n, s0, tiles, S, q.obs, st));
        // the observed sums: the identity table through the null kernel
        hipLaunchKernelGGL(gp_tables_kernel, dim3((unsigned)ceil_div(n, 256), 1), dim3(256), 0, st, t.perm, inv, n, keys, true,
                           tables);
        FDX_CHECK_LAUNCH();
        FDX_TRY(gp_launch_null(plan, Yt, tables, pos, s0, tiles, S, 1, q.obs + 4 * (size_t)S, q.obs + 2 * (size_t)S, q.obs + 3 * (size_t)S,
                               0LL, nullptr, st));
        for (long long done = 0; done < q.n_perm; done += batch) {
            const int nb = (int)std::min<long long>(batch, q.n_perm - done);
            keys.first = q.first_perm + done;
            hipLaunchKernelGGL(gp_tables_kernel, dim3((unsigned)ceil_div(n, 256), (unsigned)nb), dim3(256), 0, st, t.perm, inv, n, keys, false,
                               tables);
            FDX_CHECK_LAUNCH();
            double* row = q.null + (size_t)done * 3 * S;
            FDX_TRY(gp_launch_null(plan, Yt, tables, pos, s0, tiles, S, nb, row, row + S, row + 2 * (size_t)S, 3LL * S,
                                   t0 == 0 && done == 0 ? &ran->first : nullptr, st));
        }
    }
    return 0;
}

int gene_perm_entry(const char* who, const fdx_graph* g, const GeneMatrix& y, const int32_t* genes, int32_t S, uint64_t seed,
                    int64_t first_perm, int64_t n_perm, int64_t max_batch, int64_t max_lds_bytes, int64_t max_gather_bytes, double* obs_dev,
                    double* null_dev, int64_t* counts_out, int64_t* info_out, void* stream) {
    const std::string w(who);
    hipStream_t st = (hipStream_t)stream;
    FDX_TRY(check_gene_matrix(who, y, g && genes && obs_dev && counts_out && (null_dev || n_perm <= 0), false, "ldy < G"));
    FDX_REQUIRE(y.G >= 1, w + ": G must be at least 1");
    FDX_REQUIRE(y.n >= 0 && y.n < (1LL << 31) - 128, w + ": n must be between 0 and 2^31 - 129");
    GraphTables t;
    FDX_TRY(whole_graph_tables(g, who, &t));
    FDX_REQUIRE(y.n == t.n, w + ": Y has " + std::to_string(y.n) + " rows but the graph has " + std::to_string(t.n) + " spots");
    FDX_REQUIRE(S >= 1, w + ": S must be at least 1");
    for (int s = 0; s < S; ++s) FDX_REQUIRE(genes[s] >= 0 && genes[s] < y.G, w + ": gene index out of range");
    {
        std::vector<int32_t> sorted(genes, genes + S);
        std::sort(sorted.begin(), sorted.end());
        FDX_REQUIRE(std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end(), w + ": gene listed twice");
    }
    FDX_REQUIRE(first_perm >= 0, w + ": first_perm must not be negative");
    FDX_REQUIRE(n_perm >= 0, w + ": n_perm must not be negative");
    FDX_REQUIRE(first_perm <= (1LL << 62) && n_perm <= (1LL << 40), w + ": too many permutations");
    FDX_REQUIRE(max_batch >= 0, w + ": max_batch must not be negative");
    FDX_REQUIRE(max_lds_bytes >= 0, w + ": max_lds_bytes must not be negative");
    FDX_REQUIRE(max_gather_bytes >= 0, w + ": max_gather_bytes must not be negative");
    const size_t cap = std::min<size_t>(GP_DEVICE_LDS, max_lds_bytes > 0 ? (size_t)max_lds_bytes : GP_DEVICE_LDS);
    const GpPlan plan = gp_plan(t.n, y.dtype == FDX_F32 ? sizeof(float) : sizeof(double), cap);
    PoolStream pool_stream(st);
    counts_out[0] = t.n;
    counts_out[1] = counts_out[2] = 0;
    if (info_out) {
        info_out[0] = plan.tile;
        info_out[1] = 0;
        info_out[2] = plan.route;
        info_out[3] = info_out[4] = info_out[5] = 0;
    }
    if (t.n == 0) {                                 // empty sums; no value to be the smallest or the largest; no permutation kernel
        std::vector<double> h((size_t)7 * S, 0.0);
        std::fill(h.begin() + (size_t)5 * S, h.end(), std::numeric_limits<double>::quiet_NaN());
        FDX_TRY(copy_h2d(obs_dev, h.data(), h.size() * sizeof(double), st));
        if (n_perm > 0) FDX_HIP(hipMemsetAsync(null_dev, 0, (size_t)n_perm * 3 * S * sizeof(double), st));
        FDX_HIP(hipStreamSynchronize(st));
        return 0;
    }
    const GpRequest q{genes, S, (unsigned long long)seed, first_perm, n_perm, max_batch,
                      max_gather_bytes > 0 ? (size_t)max_gather_bytes : SCRATCH_BUDGET_BYTES, obs_dev, null_dev};
    GpRan ran;
    FDX_TRY(dispatch_gene_matrix(
        y, [&](auto* Yd) { return gp_run(t, y, Yd, q, plan, &ran, st); },
        [&](auto* values) { return gp_run(t, y, values, q, plan, &ran, st); }));
    DevBuf counts;
    FDX_TRY(counts.alloc(2 * sizeof(long long)));
    hipLaunchKernelGGL(gp_counts_kernel, dim3(1), dim3(256), 0, st, t, counts.as<long long>());
    FDX_CHECK_LAUNCH();
    long long host[2];
    FDX_TRY(copy_d2h(host, counts.p, sizeof(host), st));         // the call's one host synchronisation
    counts_out[1] = host[0];
    counts_out[2] = host[1];
    if (info_out) {
        info_out[1] = n_perm > 0 ? ran.batch : 0;
        info_out[3] = ran.stripes;
        info_out[4] = ran.first.ways;
        info_out[5] = ran.first.chunk;
    }
    return 0;
}

}  // namespace
}  // namespace fdx

using namespace fdx;

extern "C" {

int fdx_gene_spatial_perm_dev(const fdx_graph* g, const void* Y_dev, int32_t dtype, int64_t n, int32_t G, int64_t ldy, const int32_t* genes,
                              int32_t S, uint64_t seed, int64_t first_perm, int64_t n_perm, int64_t max_batch, int64_t max_lds_bytes,
                              int64_t max_gather_bytes, double* obs_dev, double* null_dev, int64_t* counts_out, int64_t* info_out,
                              void* stream) {
    return gene_perm_entry("fdx_gene_spatial_perm_dev", g, GeneMatrix(Y_dev, dtype, n, G, ldy), genes, S, seed, first_perm, n_perm,
                           max_batch, max_lds_bytes, max_gather_bytes, obs_dev, null_dev, counts_out, info_out, stream);
}

int fdx_gene_spatial_perm_csr_dev(const fdx_graph* g, const fdx_csr_view* Y, const int32_t* genes, int32_t S, uint64_t seed,
                                  int64_t first_perm, int64_t n_perm, int64_t max_batch, int64_t max_lds_bytes, int64_t max_gather_bytes,
                                  double* obs_dev, double* null_dev, int64_t* counts_out, int64_t* info_out, void* stream) {
    return gene_perm_entry("fdx_gene_spatial_perm_csr_dev", g, GeneMatrix(Y), genes, S, seed, first_perm, n_perm, max_batch, max_lds_bytes,
                           max_gather_bytes, obs_dev, null_dev, counts_out, info_out, stream);
}

}  // extern "C"
