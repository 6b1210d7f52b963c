// Spatial gene modules (additive, not in the reference): for a list of S distinct columns of a spot-by-gene matrix Y (n, G) the
// whole S x S spatial co-expression matrix over the model's graph - A its symmetric binary adjacency, deg_i = sum_j A_ij,
// lag_g,i = sum_{j in N(i)} y_jg in the graph's stored neighbour order - as raw sums, everything float64 on the value converted
// from storage, and the module scores of the spots.  What the device leaves (include/fdx.h has the definitions):
//   per gene (6, S):    0 u = sum y    1 D = sum deg y    2 L = sum lag^2    3 DL = sum deg lag    4 ymin    5 ymax
//   matrices (2, S, S): 0 S_ab = sum_i y_a,i y_b,i        1 X_ab = sum_i y_a,i lag_b,i
// The statistics are assembled on the host (flashdeconv_amd/utils/gene_modules.py).
//
// Three stages, one path for every S:
//   gather   Yg[p, s] = Y[perm[p], genes[s]] in the STORAGE type, S padded with zero columns to S_pad, a multiple of GM_TILE
//            (dense: a thread per element; CSR: the matrix zeroed, then a wave per position and a lane per stored entry through a
//            G-sized column-to-slot map).  After it every read is contiguous and neighbour indices are positions - the ELL stores
//            positions - so the walk of gene_walk.h runs on Yg with the identity order.
//   lag      per SPLIT of split_segments segments (a segment: FDX_GENE_SPATIAL_SEGMENT_POSITIONS positions): a workgroup owns 64
//            columns, wave w the rows [64 w, 64 w + 64) of every segment; a lane walks them in ascending order, writes
//            Lg[p, s] = sum_m Yg[nbr_m(p), s] (float64, stored neighbour order, hubs through the ELL) to the split's scratch and
//            accumulates the six per-gene sums; the four quarter sums of a column are added in the order w = 0, 1, 2, 3.
//   contract a workgroup owns one GM_TILE x GM_TILE tile (genes a x genes b) of one split and accumulates S and X over the split's
//            positions in ascending order on the f64 matrix cores (v_mfma_f64_16x16x4_f64; operand comment: gram_kernels.cpp).
//            Genes a (the MFMA's A operand, rows of D) come from Yg, genes b (B operand, columns of D) from Yg for S and from Lg
//            for X, staged through LDS as doubles in sub-blocks of GM_KB positions; wave w owns rows 16 w .. 16 w + 15 of the tile
//            and all four 16-column blocks.  S is computed for tiles with block_a <= block_b only; the finish kernel writes
//            S_ab = S_ba = the entry whose slot pair is (min, max).
// The split sums are folded in ascending split order (gene_pass.h: launch_gene_fold under for_segment_batches - a block of scratch
// holds a split's two padded matrices, its six planes and its lag rows).
//
// Order: no floating-point atomics; neither the tile shape nor the split depends on S, four lanes of the lag kernel own a column
// and an MFMA accumulator element its pair, so EVERY NUMBER DEPENDS ONLY ON THE GRAPH, THE ONE OR TWO COLUMNS AND split_segments -
// not on the other genes of the list, their order, or the number of blocks in flight.  split_segments moves the boundaries at which
// the sums are reassociated: other roundings, no change in an exact case.
//
// Scores: one kernel over Yg, a thread per (position, module): out[perm[p] * ldo + c] = sum over the module's genes, in their order
// in `genes`, of y * scale - shift.
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "fdx_graph.h"
#include "fdx_internal.h"
#include "fdx_kernels.h"
#include "gene_pass.h"
#include "gene_walk.h"

namespace fdx {
namespace {

typedef double gm_double4 __attribute__((ext_vector_type(4)));

constexpr int GM_TILE = 64;                                  // genes of a tile's side; S is padded to a multiple of it
constexpr int GM_KB = 32;                                    // positions of an LDS sub-block
constexpr int GM_LD = GM_TILE + 16;                          // row stride (doubles) in LDS: = 16 mod 32, the two k rows that a
                                                             // 32-lane half of ds_read_b64 touches fall on disjoint banks
constexpr int GM_S_MAX = 4096;
constexpr int GM_GENE_PLANES = 6, GM_MIN = 4, GM_MAX = 5;
constexpr int GM_LAG_GENES = 64;                             // columns of a workgroup of the lag kernel, one per lane of a wave
constexpr int GM_DEFAULT_SPLIT = 16;
constexpr size_t GM_DEFAULT_GATHER = (size_t)16 << 30;

// doubles of a split's block: the two padded matrices, the six planes, the lag rows of its positions
inline size_t gm_block_doubles(int S_pad, int split_pos) {
    return 2 * (size_t)S_pad * S_pad + (size_t)GM_GENE_PLANES * S_pad + (size_t)split_pos * S_pad;
}

// Yg[p, s] = Y[perm[p], genes[s]] for s < S, 0 for S <= s < S_pad; a thread per element, s fastest
template <typename T>
__global__ __launch_bounds__(256) void gm_gather_dense_kernel(const T* __restrict__ Y, long long ldy, const int* __restrict__ perm,
                                                              long long n, const int* __restrict__ genes, int S, int S_pad,
                                                              T* __restrict__ Yg) {
    const long long total = n * S_pad;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long p = e / S_pad;
        const int s = (int)(e - p * S_pad);
        const long long row = perm ? perm[p] : p;
        Yg[e] = s < S ? Y[row * ldy + genes[s]] : (T)0;
    }
}

// Yg (zeroed) takes the stored entries of the wanted columns: a wave per position, a lane per stored entry of its row; the entries
// of a row have distinct columns, so every element has one writer
template <typename T>
__global__ __launch_bounds__(256) void gm_gather_csr_kernel(const long long* __restrict__ indptr, const int* __restrict__ indices,
                                                            const T* __restrict__ values, const int* __restrict__ perm, long long n,
                                                            int G, const int* __restrict__ slot_of, int S_pad, T* __restrict__ Yg) {
    const int lane = threadIdx.x & 63;
    for (long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); p < n; p += (long long)gridDim.x * 4) {
        const long long row = perm ? perm[p] : p;
        const long long e1 = indptr[row + 1];
        for (long long e = indptr[row] + lane; e < e1; e += 64) {
            const int c = indices[e];
            const int slot = (unsigned)c < (unsigned)G ? slot_of[c] : -1;
            if (slot >= 0) Yg[p * S_pad + slot] = values[e];
        }
    }
}

// gs_walk_segment of gene_walk.h for ONE column and the rows [r_lo, r_hi) of the staged segment: use(r, dg, y, lag) per row in order,
// the next row's 1 + GS_NB loads issued before this row's are consumed, a hub's further neighbours from the ELL.
template <typename T, class Use>
__device__ __forceinline__ void gm_walk_rows(const T* yp, long long ld, const GraphTables& g, int p0, int r_lo, int r_hi,
                                             const GsSegmentTables& sh, Use&& use) {
    if (r_lo >= r_hi) return;
    T c[1 + GS_NB], nx[1 + GS_NB];                           // [0]: the row itself, [1 + m]: neighbour m (0 where none)
    auto load = [&](int r, T (&a)[1 + GS_NB]) {
        a[0] = yp[(long long)sh.row[r] * ld];
#pragma unroll
        for (int m = 0; m < GS_NB; ++m) {
            const long long nr = sh.nbr[m * GS_SEG + r];
            a[1 + m] = nr >= 0 ? yp[nr * ld] : (T)0;
        }
    };
    load(r_lo, c);
    for (int r = r_lo; r < r_hi; ++r) {
        if (r + 1 < r_hi) load(r + 1, nx);
        const int dg = sh.deg[r];
        double lag = 0.0;
#pragma unroll
        for (int m = 0; m < GS_NB; ++m) lag += (double)c[1 + m];     // (x + 0 = x: the slots past the degree change nothing)
        if (dg > GS_NB) {
            const int p = p0 + r, w0 = g.slice_off[p >> 6];
            for (int m0 = GS_NB; m0 < dg; m0 += 8) {
                T e[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const long long nr = m0 + k < dg ? gs_neighbour_row(g, w0, p, m0 + k) : -1;
                    e[k] = nr >= 0 ? yp[nr * ld] : (T)0;
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) lag += (double)e[k];
            }
        }
        use(r, dg, (double)c[0], lag);
#pragma unroll
        for (int k = 0; k < 1 + GS_NB; ++k) c[k] = nx[k];
    }
}

// Workgroup x: split x of this launch (the call's split split0 + x, segments [.. * sps, .. + sps)); workgroup row y: the columns
// [64 y, 64 y + 64) of Yg.  Lane l of wave w owns column 64 y + l over QUARTER w - rows [64 w, 64 w + 64) - of every segment of
// the split: it writes those rows' lags and adds them, segment after segment, into its six sums; the four quarters of a column are
// then added in the order w = 0, 1, 2, 3.  g: the graph's tables with perm = null (Yg is in the graph's order).  The lag rows and
// the six planes go into the split's block; deg_part (row 0): the segments' degree sums.
template <typename T>
__global__ __launch_bounds__(256) void gm_lag_kernel(const T* __restrict__ Yg, int S_pad, GraphTables g, int split0, int sps,
                                                     double* __restrict__ part, long long block_doubles,
                                                     long long* __restrict__ deg_part) {
    __shared__ GsSegmentTables sh;
    __shared__ long long red[2][4];
    __shared__ double quarter[3][GM_GENE_PLANES][GM_LAG_GENES];
    const int tid = threadIdx.x, w = tid >> 6;
    const int j = blockIdx.y * GM_LAG_GENES + (tid & 63);       // (< S_pad: a multiple of 64)
    const T* yp = Yg + j;
    const int n_seg = (g.n + GS_SEG - 1) / GS_SEG;
    const int seg_lo = (split0 + (int)blockIdx.x) * sps, seg_hi = min(n_seg, seg_lo + sps);
    double* block = part + (size_t)blockIdx.x * block_doubles;
    double* lag_rows = block + 2 * (size_t)S_pad * S_pad + (size_t)GM_GENE_PLANES * S_pad;
    const bool owner = blockIdx.y == 0;
    double u = 0.0, D = 0.0, L = 0.0, DL = 0.0, mn = INFINITY, mx = -INFINITY;
    for (int seg = seg_lo; seg < seg_hi; ++seg) {
        const int p0 = seg * GS_SEG;
        const int cnt = min(GS_SEG, g.n - p0);
        gs_stage_segment(g, p0, p0 + cnt, sh, red, owner, nullptr, owner ? deg_part + 2 * (size_t)seg : nullptr);
        double* rows = lag_rows + (size_t)(seg - seg_lo) * GS_SEG * S_pad + j;
        gm_walk_rows(yp, (long long)S_pad, g, p0, 64 * w, min(cnt, 64 * w + 64), sh, [&](int r, int dg, double y, double lag) {
            const double d = (double)dg;
            rows[(size_t)r * S_pad] = lag;
            u += y;
            D += d * y;
            L += lag * lag;
            DL += d * lag;
            mn = fmin(mn, y);
            mx = fmax(mx, y);
        });
    }
    const double v[GM_GENE_PLANES] = {u, D, L, DL, mn, mx};
    if (w > 0) {
#pragma unroll
        for (int k = 0; k < GM_GENE_PLANES; ++k) quarter[w - 1][k][tid & 63] = v[k];
    }
    __syncthreads();
    if (w == 0) {
        double* planes = block + 2 * (size_t)S_pad * S_pad + j;
#pragma unroll
        for (int k = 0; k < GM_GENE_PLANES; ++k) {
            double acc = v[k];
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                const double o = quarter[x][k][tid & 63];
                acc = k == GM_MIN ? fmin(acc, o) : k == GM_MAX ? fmax(acc, o) : acc + o;
            }
            planes[(size_t)k * S_pad] = acc;
        }
    }
}

// One workgroup per (split of this launch, tile): S (ta <= tb only) and X of the tile (ta, tb) over the split's positions in
// ascending order, written into the split's block.  Which workgroup takes which tile changes no bit, so the 1-D grid is laid out
// for the caches: xcd_remap hands every XCD a contiguous range of the logical order - split after split, within a split panels of
// 8 tile columns, a panel row after row - so that the ~64 workgroups an XCD runs at a time read the same 32 positions of 8 x 8
// tiles' operands through its L2.  The next sub-block's global loads are issued before this one's MFMAs and wait in registers.
template <typename T>
__global__ __launch_bounds__(256) void gm_contract_kernel(const T* __restrict__ Yg, int S_pad, int n, int split0, int split_pos,
                                                          double* __restrict__ part, long long block_doubles) {
    __shared__ double As[GM_KB * GM_LD], By[GM_KB * GM_LD], Bl[GM_KB * GM_LD];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tiles = S_pad / GM_TILE, per_split = tiles * tiles;
    const int logical = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    const int z = logical / per_split, tile = logical - z * per_split;
    const int panel = tile / (8 * tiles), width = min(8, tiles - 8 * panel), rem = tile - panel * 8 * tiles;
    const int ta = rem / width, tb = 8 * panel + rem - ta * width;
    const bool with_s = ta <= tb;                               // (uniform over the workgroup)
    const long long p_lo = (long long)(split0 + z) * split_pos;
    const int cnt = (int)min((long long)split_pos, (long long)n - p_lo);
    double* block = part + (size_t)z * block_doubles;
    const double* lag_rows = block + 2 * (size_t)S_pad * S_pad + (size_t)GM_GENE_PLANES * S_pad;
    const int a0 = ta * GM_TILE, b0 = tb * GM_TILE;
    const int lg = tid & 63, lr = tid >> 6;                     // staging: column lg of rows lr, lr + 4, ...
    const int i = lane & 15, q = lane >> 4;                     // MFMA: A[i][k = q], B[k = q][j = i], D[q + 4 r][i]
    gm_double4 accS[4], accX[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) accS[t] = accX[t] = gm_double4{0.0, 0.0, 0.0, 0.0};
    T ra[GM_KB / 4], rb[GM_KB / 4];
    double rl[GM_KB / 4];
    auto fetch = [&](int r0) {                                  // the sub-block at r0, zeros past the split's end
#pragma unroll
        for (int rr = 0; rr < GM_KB / 4; ++rr) {
            const int r = r0 + lr + 4 * rr;
            const bool in = r < cnt;
            const size_t src = (size_t)(p_lo + r) * S_pad;
            ra[rr] = in ? Yg[src + a0 + lg] : (T)0;
            rb[rr] = in && with_s ? Yg[src + b0 + lg] : (T)0;
            rl[rr] = in ? lag_rows[(size_t)r * S_pad + b0 + lg] : 0.0;
        }
    };
    fetch(0);
    for (int r0 = 0; r0 < cnt; r0 += GM_KB) {
        __syncthreads();                                        // the readers of the sub-block before
#pragma unroll
        for (int rr = 0; rr < GM_KB / 4; ++rr) {
            const int at = (lr + 4 * rr) * GM_LD + lg;
            As[at] = (double)ra[rr];
            if (with_s) By[at] = (double)rb[rr];
            Bl[at] = rl[rr];
        }
        __syncthreads();
        if (r0 + GM_KB < cnt) fetch(r0 + GM_KB);
#pragma unroll
        for (int step = 0; step < GM_KB / 4; ++step) {
            const int row = (4 * step + q) * GM_LD;
            const double a = As[row + 16 * wave + i];
#pragma unroll
            for (int t = 0; t < 4; ++t) accX[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Bl[row + 16 * t + i], accX[t], 0, 0, 0);
            if (with_s) {
#pragma unroll
                for (int t = 0; t < 4; ++t) accS[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, By[row + 16 * t + i], accS[t], 0, 0, 0);
            }
        }
    }
    double* Sm = block;
    double* Xm = block + (size_t)S_pad * S_pad;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const size_t at = (size_t)(a0 + 16 * wave + q + 4 * r) * S_pad + b0 + 16 * t + i;
            Xm[at] = accX[t][r];
            if (with_s) Sm[at] = accS[t][r];
        }
    }
}

// cross (2, S, S) and gene_sums (6, S) from the folded padded block: S_ab = S_ba = the entry of the slots (min, max)
__global__ __launch_bounds__(256) void gm_finish_kernel(const double* __restrict__ folded, int S, int S_pad, double* __restrict__ cross,
                                                        double* __restrict__ gene_sums) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long SS = (long long)S * S;
    if (e < SS) {
        const int a = (int)(e / S), b = (int)(e - (long long)a * S);
        cross[e] = folded[(size_t)min(a, b) * S_pad + max(a, b)];
        cross[SS + e] = folded[(size_t)S_pad * S_pad + (size_t)a * S_pad + b];
    }
    if (e < (long long)GM_GENE_PLANES * S) {
        const int k = (int)(e / S), j = (int)(e - (long long)k * S);
        gene_sums[e] = folded[2 * (size_t)S_pad * S_pad + (size_t)k * S_pad + j];
    }
}

// out[row(p) * ldo + c] = sum over the members m of module c (member[off[c] .. off[c + 1]), slots in the order of `genes`) of
// Yg[p, m] * scale[m] - shift[m]; a thread per (position, module)
template <typename T>
__global__ __launch_bounds__(256) void gm_scores_kernel(const T* __restrict__ Yg, int S_pad, const int* __restrict__ perm, long long n,
                                                        int C, const int* __restrict__ off, const int* __restrict__ member,
                                                        const double* __restrict__ scale, const double* __restrict__ shift,
                                                        double* __restrict__ out, long long ldo) {
    const long long total = n * C;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long p = e / C;
        const int c = (int)(e - p * C);
        const T* y = Yg + p * S_pad;
        double acc = 0.0;
        for (int k = off[c]; k < off[c + 1]; ++k) {
            const int m = member[k];
            acc += (double)y[m] * scale[m] - shift[m];
        }
        const long long row = perm ? perm[p] : p;
        out[row * ldo + c] = acc;
    }
}

// Stage 1 for either form of Y: Yg (n, S_pad) of the storage type, queued on st.
template <typename T>
int gm_gather(const GraphTables& t, const GeneMatrix& y, const T* data, const int32_t* genes, int S, int S_pad, T* Yg, hipStream_t st) {
    const long long n = t.n;
    if (y.sparse) {
        std::vector<int> slot_of((size_t)y.G, -1);
        for (int s = 0; s < S; ++s) slot_of[genes[s]] = s;
        DevBuf map_buf;
        FDX_TRY(map_buf.alloc(slot_of.size() * sizeof(int)));
        FDX_TRY(copy_h2d(map_buf.p, slot_of.data(), slot_of.size() * sizeof(int), st));
        FDX_HIP(hipMemsetAsync(Yg, 0, (size_t)n * S_pad * sizeof(T), st));
        hipLaunchKernelGGL(gm_gather_csr_kernel, dim3((unsigned)std::min<long long>(ceil_div(n, 4), 1 << 16)), dim3(256), 0, st,
                           (const long long*)y.csr->indptr, y.csr->indices, data, t.perm, n, y.G, map_buf.as<int>(), S_pad, Yg);
        FDX_CHECK_LAUNCH();
        return 0;
    }
    DevBuf genes_buf;
    FDX_TRY(genes_buf.alloc((size_t)S * sizeof(int)));
    FDX_TRY(copy_h2d(genes_buf.p, genes, (size_t)S * sizeof(int), st));
    const long long blocks = std::min<long long>(((long long)n * S_pad + 255) / 256, 1 << 20);
    hipLaunchKernelGGL(gm_gather_dense_kernel, dim3((unsigned)blocks), dim3(256), 0, st, data, y.ldy, t.perm, n, genes_buf.as<int>(), S,
                       S_pad, Yg);
    FDX_CHECK_LAUNCH();
    return 0;
}

template <typename T>
int gm_run_sums(const GraphTables& t, const GeneMatrix& y, const T* data, const int32_t* genes, int S, int S_pad, int sps,
                double* gene_sums, double* cross, long long* deg_part, hipStream_t st) {
    DevBuf yg_buf, folded;
    FDX_TRY(yg_buf.alloc((size_t)t.n * S_pad * sizeof(T)));
    FDX_TRY(gm_gather(t, y, data, genes, S, S_pad, yg_buf.as<T>(), st));
    const T* Yg = yg_buf.as<T>();
    GraphTables pos = t;
    pos.perm = nullptr;                                         // Yg is in the graph's order: rows are positions
    const int n_seg = ceil_div(t.n, GS_SEG), n_splits = ceil_div(n_seg, sps), split_pos = sps * GS_SEG;
    const size_t block = gm_block_doubles(S_pad, split_pos);
    const int tiles = S_pad / GM_TILE;
    const long long SP2 = (long long)S_pad * S_pad;
    FDX_TRY(folded.alloc((2 * (size_t)SP2 + (size_t)GM_GENE_PLANES * S_pad) * sizeof(double)));
    const size_t seg_bytes = block * sizeof(double);             // (68 KB at the least: a launch never has 65,536 splits)
    FDX_TRY(for_segment_batches(n_splits, seg_bytes, [&](int sb0, int nb, double* part) {
        const long long stride = (long long)(seg_bytes / sizeof(double));
        hipLaunchKernelGGL(gm_lag_kernel, dim3((unsigned)nb, (unsigned)ceil_div(S_pad, GM_LAG_GENES)), dim3(256), 0, st, Yg, S_pad, pos, sb0,
                           sps, part, stride, deg_part);
        FDX_CHECK_LAUNCH();
        hipLaunchKernelGGL(gm_contract_kernel, dim3((unsigned)(tiles * tiles * nb)), dim3(256), 0, st, Yg, S_pad, t.n, sb0,
                           split_pos, part, stride);
        FDX_CHECK_LAUNCH();
        // the two matrices as two planes of S_pad^2 "genes"; then the six planes
        const SegmentBlocks m{part, stride, SP2, 1LL, sb0, nb};
        FDX_TRY(launch_gene_fold(m, 0, 2, (int)SP2, nullptr, 1, folded.as<double>(), 0, SP2, -1, -1, st));
        const SegmentBlocks p{part + 2 * (size_t)SP2, stride, (long long)S_pad, 1LL, sb0, nb};
        return launch_gene_fold(p, 0, GM_GENE_PLANES, S_pad, nullptr, 1, folded.as<double>() + 2 * (size_t)SP2, 0, (long long)S_pad, GM_MIN,
                                GM_MAX, st);
    }));
    const long long cells = std::max<long long>((long long)S * S, (long long)GM_GENE_PLANES * S);
    hipLaunchKernelGGL(gm_finish_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, folded.as<double>(), S, S_pad, cross,
                       gene_sums);
    FDX_CHECK_LAUNCH();
    return 0;
}

template <typename T>
int gm_run_scores(const GraphTables& t, const GeneMatrix& y, const T* data, const int32_t* genes, const int32_t* label, int S, int S_pad,
                  int C, const double* scale, const double* shift, double* out, long long ldo, hipStream_t st) {
    DevBuf yg_buf, lists;
    FDX_TRY(yg_buf.alloc((size_t)t.n * S_pad * sizeof(T)));
    FDX_TRY(gm_gather(t, y, data, genes, S, S_pad, yg_buf.as<T>(), st));
    std::vector<int> host((size_t)C + 1 + S, 0);                 // off (C + 1), then the members in the order of `genes`
    for (int s = 0; s < S; ++s)
        if (label[s] >= 0) ++host[(size_t)label[s] + 1];
    for (int c = 0; c < C; ++c) host[(size_t)c + 1] += host[c];
    std::vector<int> fill(host.begin(), host.begin() + C);
    for (int s = 0; s < S; ++s)
        if (label[s] >= 0) host[(size_t)C + 1 + fill[label[s]]++] = s;
    FDX_TRY(lists.alloc(host.size() * sizeof(int)));
    FDX_TRY(copy_h2d(lists.p, host.data(), host.size() * sizeof(int), st));
    const long long blocks = std::min<long long>(((long long)t.n * C + 255) / 256, 1 << 20);
    hipLaunchKernelGGL(gm_scores_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const T*)yg_buf.as<T>(), S_pad, t.perm, (long long)t.n,
                       C, lists.as<int>(), lists.as<int>() + C + 1, scale, shift, out, ldo);
    FDX_CHECK_LAUNCH();
    return 0;
}

// What a call leaves behind: the sums (scores == false) or the module scores.
struct ModuleOutput {
    bool scores = false;
    int split_segments = 0;
    double *gene_sums = nullptr, *cross = nullptr;           // (6, S), (2, S, S) device
    int64_t* counts_out = nullptr;                           // host
    const int32_t* label = nullptr;                          // S, host
    int C = 0;
    const double *scale = nullptr, *shift = nullptr;         // S each, device
    double* out = nullptr;                                   // (n, ldo) device
    long long ldo = 0;
};

int gene_module_entry(const char* who, const fdx_graph* g, const GeneMatrix& y, const int32_t* genes, int32_t S, int64_t max_gather_bytes,
                      const ModuleOutput& o, void* stream) {
    const std::string w(who);
    hipStream_t st = (hipStream_t)stream;
    const bool outputs = o.scores ? (o.label && o.scale && o.shift && o.out) : (o.gene_sums && o.cross && o.counts_out);
    FDX_TRY(check_gene_matrix(who, y, g && genes && outputs, false, "ldy < G"));
    FDX_REQUIRE(y.G >= 1, w + ": G must be at least 1");
    FDX_REQUIRE(y.n >= 0 && y.n < (1LL << 31) - 128, w + ": n must be between 0 and 2^31 - 129");
    GraphTables t;
    FDX_TRY(whole_graph_tables(g, who, &t));
    FDX_REQUIRE(y.n == t.n, w + ": Y has " + std::to_string(y.n) + " rows but the graph has " + std::to_string(t.n) + " spots");
    FDX_REQUIRE(S >= 1 && S <= GM_S_MAX, w + ": S must be in [1, 4096]");
    for (int s = 0; s < S; ++s) FDX_REQUIRE(genes[s] >= 0 && genes[s] < y.G, w + ": gene index out of range");
    {
        std::vector<int32_t> sorted(genes, genes + S);
        std::sort(sorted.begin(), sorted.end());
        FDX_REQUIRE(std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end(), w + ": gene listed twice");
    }
    const int S_pad = (int)round_up(S, GM_TILE);
    const size_t elem = y.dtype == FDX_F32 ? sizeof(float) : sizeof(double);
    const unsigned long long need = (unsigned long long)t.n * S_pad * elem;
    const unsigned long long cap = max_gather_bytes > 0 ? (unsigned long long)max_gather_bytes : GM_DEFAULT_GATHER;
    FDX_REQUIRE(need <= cap, w + ": gathered matrix needs " + std::to_string(need) + " bytes, max_gather_bytes is " + std::to_string(cap));
    if (o.scores) {
        FDX_REQUIRE(o.ldo >= o.C, w + ": ldo < C");
        FDX_REQUIRE(o.C >= 1, w + ": C must be at least 1");
        for (int s = 0; s < S; ++s) FDX_REQUIRE(o.label[s] >= -1 && o.label[s] < o.C, w + ": label outside [-1, C)");
    } else {
        FDX_REQUIRE(o.split_segments >= 0, w + ": split_segments must not be negative");
    }
    PoolStream pool_stream(st);
    if (!o.scores) {
        o.counts_out[0] = t.n;
        o.counts_out[1] = o.counts_out[2] = 0;
    }
    if (t.n == 0) {                                 // empty sums; no value to be the smallest or the largest; no row to score
        if (o.scores) return 0;
        std::vector<double> h((size_t)GM_GENE_PLANES * S, 0.0);
        std::fill(h.begin() + (size_t)GM_MIN * S, h.end(), std::numeric_limits<double>::quiet_NaN());
        FDX_TRY(copy_h2d(o.gene_sums, h.data(), h.size() * sizeof(double), st));
        FDX_HIP(hipMemsetAsync(o.cross, 0, 2 * (size_t)S * S * sizeof(double), st));
        FDX_HIP(hipStreamSynchronize(st));
        return 0;
    }
    if (o.scores)
        return dispatch_gene_matrix(
            y,
            [&](auto* Yd) { return gm_run_scores(t, y, Yd, genes, o.label, S, S_pad, o.C, o.scale, o.shift, o.out, o.ldo, st); },
            [&](auto* values) { return gm_run_scores(t, y, values, genes, o.label, S, S_pad, o.C, o.scale, o.shift, o.out, o.ldo, st); });
    const int n_seg = ceil_div(t.n, GS_SEG);
    const int sps = std::min(o.split_segments > 0 ? o.split_segments : GM_DEFAULT_SPLIT, n_seg);
    DevBuf deg_buf, counts;
    FDX_TRY(deg_buf.alloc((size_t)n_seg * 2 * sizeof(long long)));
    FDX_TRY(counts.alloc(2 * sizeof(long long)));
    long long* deg_part = deg_buf.as<long long>();
    FDX_TRY(dispatch_gene_matrix(
        y, [&](auto* Yd) { return gm_run_sums(t, y, Yd, genes, S, S_pad, sps, o.gene_sums, o.cross, deg_part, st); },
        [&](auto* values) { return gm_run_sums(t, y, values, genes, S, S_pad, sps, o.gene_sums, o.cross, deg_part, st); }));
    FDX_TRY(launch_segment_degree_counts(deg_part, n_seg, counts.as<long long>(), st));
    long long host[2];
    FDX_TRY(copy_d2h(host, counts.p, sizeof(host), st));         // the call's last host synchronisation
    o.counts_out[1] = host[0];
    o.counts_out[2] = host[1];
    return 0;
}

ModuleOutput sums_output(int split_segments, double* gene_sums_dev, double* cross_dev, int64_t* counts_out) {
    ModuleOutput o;
    o.split_segments = split_segments;
    o.gene_sums = gene_sums_dev;
    o.cross = cross_dev;
    o.counts_out = counts_out;
    return o;
}

ModuleOutput scores_output(const int32_t* label, int C, const double* scale, const double* shift, double* out_dev, int64_t ldo) {
    ModuleOutput o;
    o.scores = true;
    o.label = label;
    o.C = C;
    o.scale = scale;
    o.shift = shift;
    o.out = out_dev;
    o.ldo = ldo;
    return o;
}

}  // namespace
}  // namespace fdx

using namespace fdx;

extern "C" {

int fdx_gene_coexpr_sums_dev(const fdx_graph* g, const void* Y_dev, int32_t dtype, int64_t n, int32_t G, int64_t ldy, const int32_t* genes,
                             int32_t S, int32_t split_segments, int64_t max_gather_bytes, double* gene_sums_dev, double* cross_dev,
                             int64_t* counts_out, void* stream) {
    return gene_module_entry("fdx_gene_coexpr_sums_dev", g, GeneMatrix(Y_dev, dtype, n, G, ldy), genes, S, max_gather_bytes,
                             sums_output(split_segments, gene_sums_dev, cross_dev, counts_out), stream);
}

int fdx_gene_coexpr_sums_csr_dev(const fdx_graph* g, const fdx_csr_view* Y, const int32_t* genes, int32_t S, int32_t split_segments,
                                 int64_t max_gather_bytes, double* gene_sums_dev, double* cross_dev, int64_t* counts_out, void* stream) {
    return gene_module_entry("fdx_gene_coexpr_sums_csr_dev", g, GeneMatrix(Y), genes, S, max_gather_bytes,
                             sums_output(split_segments, gene_sums_dev, cross_dev, counts_out), stream);
}

int fdx_gene_module_scores_dev(const fdx_graph* g, const void* Y_dev, int32_t dtype, int64_t n, int32_t G, int64_t ldy, const int32_t* genes,
                               const int32_t* label, int32_t S, int32_t C, const double* scale_dev, const double* shift_dev,
                               double* out_dev, int64_t ldo, void* stream) {
    return gene_module_entry("fdx_gene_module_scores_dev", g, GeneMatrix(Y_dev, dtype, n, G, ldy), genes, S, 0,
                             scores_output(label, C, scale_dev, shift_dev, out_dev, ldo), stream);
}

int fdx_gene_module_scores_csr_dev(const fdx_graph* g, const fdx_csr_view* Y, const int32_t* genes, const int32_t* label, int32_t S,
                                   int32_t C, int64_t max_gather_bytes, const double* scale_dev, const double* shift_dev, double* out_dev,
                                   int64_t ldo, void* stream) {
    return gene_module_entry("fdx_gene_module_scores_csr_dev", g, GeneMatrix(Y), genes, S, max_gather_bytes,
                             scores_output(label, C, scale_dev, shift_dev, out_dev, ldo), stream);
}

}  // extern "C"
