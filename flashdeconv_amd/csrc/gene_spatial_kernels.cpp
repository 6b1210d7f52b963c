// Spatially variable genes (additive, not in the reference): per gene g of a spot-by-gene matrix Y (n, G) the nine sums from which
// Moran's I, Geary's C and their moments are assembled on the host (flashdeconv_amd/utils/spatial_genes.py), over the model's
// graph - A its symmetric binary adjacency, deg_i = sum_j A_ij - from one pass over Y as it lies in HBM (float32 / float64 dense
// with any row stride, or CSR kept sparse).  Planes of the (9, G) result, everything float64 on the value converted from storage:
//   0 u = sum y      1 q = sum y^2      2 c3 = sum y^3      3 c4 = sum y^4      4 D = sum deg y      5 H = sum deg y^2
//   6 P = sum_i y_i lag_i, lag_i = sum_{j in N(i)} y_j in the graph's stored neighbour order      7 min y      8 max y
// include/fdx.h has the definitions.
//
// Order of the sums.  The graph's positions 0 .. n - 1 (position p holds the caller's spot perm[p]) are cut into SEGMENTS of
// FDX_GENE_SPATIAL_SEGMENT_POSITIONS positions; a segment is summed position after position into zeroed accumulators, its sums go
// to a scratch block, and the fold adds the segment sums in ascending order (planes 7 and 8: keeps the smaller / larger).  That
// order is a function of the graph alone; gene_pass.h has the rule for what changes no bit of it (stripe, batches of segments)
// and the fold.
//
// A workgroup first stages its segment's index tables in LDS, one thread per position: the caller's row, the degree and the caller's
// rows of the first GS_NB neighbours (the chain perm[p], deg[p], slice_off, ell, perm[j] is walked by 256 threads at once, not
// once per row; gene_walk.h, shared with the gene-pair sums).  Walking in the graph's order keeps the neighbours' rows close for
// device-built (Morton-ordered) graphs: the 1 + deg reads of a row are then served by L2 / Infinity Cache.
//   dense  a thread owns two gene columns (j, j + 256: rows are read coalesced), a workgroup 512; row and neighbour indices are
//          read from LDS by broadcast; the 1 + GS_NB loads of the next position are issued before this position's are consumed.
//          Neighbours past GS_NB (a hub) are read from the ELL, eight loads at a time.
//   CSR    a workgroup per segment walks its positions in order, a barrier after each; a thread owns an entry (i, c) of the row,
//          looks column c up in the rows of N(i) (binary search in sorted rows, a scan otherwise) and adds into the segment's block
//          [plane][gene] in global memory - the entries of a row have distinct columns, so no two threads meet between barriers.  A
//          tenth plane counts the stored entries of a column: with fewer than n of them the implicit 0 takes part in min / max.
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

constexpr int GS_GENES = 512;                                // genes of a dense workgroup, two per thread
constexpr int GS_PLANES = 9, GS_CSR_PLANES = 10;             // CSR: plane 9 counts the stored entries
constexpr int GS_MIN = 7, GS_MAX = 8;

// part[s][plane][j] for the segments seg0 + s, s < n_seg, of this launch; workgroup x takes segments [x * stripe, (x + 1) * stripe),
// workgroup row y the genes [512 y, 512 y + 512).
template <typename T>
__global__ __launch_bounds__(256) void gs_dense_kernel(const T* __restrict__ Y, long long ldy, GraphTables g, int seg0, int n_seg,
                                                       int stripe, int G, double* __restrict__ part, int* __restrict__ deg_out,
                                                       long long* __restrict__ deg_part) {
    __shared__ GsSegmentTables sh;
    __shared__ long long red[2][4];
    const int tid = threadIdx.x;
    const int j0 = blockIdx.y * GS_GENES + tid, j1 = j0 + 256;
    const bool ok0 = j0 < G, ok1 = j1 < G;
    const T* y0p = Y + (ok0 ? j0 : 0);
    const T* y1p = Y + (ok1 ? j1 : 0);
    const int s0 = blockIdx.x * stripe, s1 = min(n_seg, s0 + stripe);
    for (int s = s0; s < s1; ++s) {
        const int p0 = (seg0 + s) * GS_SEG;
        const int cnt = min(GS_SEG, g.n - p0);
        gs_stage_segment(g, p0, p0 + cnt, sh, red, blockIdx.y == 0, deg_out, deg_part + 2 * (size_t)(seg0 + s));
        double u0 = 0.0, q0 = 0.0, t0 = 0.0, f0 = 0.0, D0 = 0.0, H0 = 0.0, P0 = 0.0;
        double u1 = 0.0, q1 = 0.0, t1 = 0.0, f1 = 0.0, D1 = 0.0, H1 = 0.0, P1 = 0.0;
        double mn0 = INFINITY, mx0 = -INFINITY, mn1 = INFINITY, mx1 = -INFINITY;
        gs_walk_segment(y0p, y1p, ldy, g, p0, cnt, sh, [&](int, int dg, double ya, double yb, double lag0, double lag1) {
            const double d = (double)dg;
            const double ya2 = ya * ya, yb2 = yb * yb;
            u0 += ya;                 u1 += yb;
            q0 += ya2;                q1 += yb2;
            t0 += ya2 * ya;           t1 += yb2 * yb;
            f0 += ya2 * ya2;          f1 += yb2 * yb2;
            D0 += d * ya;             D1 += d * yb;
            H0 += d * ya2;            H1 += d * yb2;
            P0 += ya * lag0;          P1 += yb * lag1;
            mn0 = fmin(mn0, ya);      mn1 = fmin(mn1, yb);
            mx0 = fmax(mx0, ya);      mx1 = fmax(mx1, yb);
        });
        double* out = part + (size_t)s * GS_PLANES * G;
        if (ok0) {
            const double v[GS_PLANES] = {u0, q0, t0, f0, D0, H0, P0, mn0, mx0};
#pragma unroll
            for (int k = 0; k < GS_PLANES; ++k) out[(size_t)k * G + j0] = v[k];
        }
        if (ok1) {
            const double v[GS_PLANES] = {u1, q1, t1, f1, D1, H1, P1, mn1, mx1};
#pragma unroll
            for (int k = 0; k < GS_PLANES; ++k) out[(size_t)k * G + j1] = v[k];
        }
    }
}

// The stored value of column c in row `row` as a double, 0 where the row does not store it.
template <typename T, bool SORTED>
__device__ __forceinline__ double gs_csr_lookup(const long long* __restrict__ indptr, const int* __restrict__ indices,
                                                const T* __restrict__ values, long long row, int c) {
    long long lo = indptr[row], hi = indptr[row + 1];
    if (SORTED) {
        const long long end = hi;
        while (lo < hi) {                                        // the first entry whose column is not below c
            const long long mid = lo + ((hi - lo) >> 1);
            if (indices[mid] < c) lo = mid + 1;
            else hi = mid;
        }
        return lo < end && indices[lo] == c ? (double)values[lo] : 0.0;
    }
    for (long long e = lo; e < hi; ++e)                          // distinct columns: at most one entry matches
        if (indices[e] == c) return (double)values[e];
    return 0.0;
}

// part[s][plane][c], 10 planes, for the segments of this launch; one workgroup row.  Between two barriers a workgroup adds the
// entries of ONE row, whose columns differ: every element of the block has one owner.
template <typename T, bool SORTED>
__global__ __launch_bounds__(256) void gs_csr_kernel(const long long* __restrict__ indptr, const int* __restrict__ indices,
                                                     const T* __restrict__ values, GraphTables g, int seg0, int n_seg, int stripe,
                                                     int G, double* part, int* __restrict__ deg_out, long long* __restrict__ deg_part) {
    __shared__ GsSegmentTables sh;
    __shared__ long long red[2][4];
    const int tid = threadIdx.x;
    const int s0 = blockIdx.x * stripe, s1 = min(n_seg, s0 + stripe);
    for (int s = s0; s < s1; ++s) {
        const int p0 = (seg0 + s) * GS_SEG;
        const int cnt = min(GS_SEG, g.n - p0);
        double* P = part + (size_t)s * GS_CSR_PLANES * G;
        for (size_t e = tid; e < (size_t)GS_CSR_PLANES * G; e += 256) {
            const int plane = (int)(e / (size_t)G);
            P[e] = plane == GS_MIN ? INFINITY : plane == GS_MAX ? -INFINITY : 0.0;
        }
        gs_stage_segment(g, p0, p0 + cnt, sh, red, true, deg_out, deg_part + 2 * (size_t)(seg0 + s));
        for (int r = 0; r < cnt; ++r) {
            const long long row = sh.row[r];
            const int dg = sh.deg[r];
            const int p = p0 + r, w0 = g.slice_off[p >> 6];
            const double d = (double)dg;
            const long long e0 = indptr[row], e1 = indptr[row + 1];
            for (long long e = e0 + tid; e < e1; e += 256) {
                const int c = indices[e];
                const double y = (double)values[e];
                double lag = 0.0;
                for (int m = 0; m < dg; ++m) {
                    const int nr = m < GS_NB ? sh.nbr[m * GS_SEG + r] : gs_neighbour_row(g, w0, p, m);
                    if (nr >= 0) lag += gs_csr_lookup<T, SORTED>(indptr, indices, values, nr, c);
                }
                const double y2 = y * y;
                double* o = P + c;
                o[0] += y;
                o[(size_t)G] += y2;
                o[2 * (size_t)G] += y2 * y;
                o[3 * (size_t)G] += y2 * y2;
                o[4 * (size_t)G] += d * y;
                o[5 * (size_t)G] += d * y2;
                o[6 * (size_t)G] += y * lag;
                o[(size_t)GS_MIN * G] = fmin(o[(size_t)GS_MIN * G], y);
                o[(size_t)GS_MAX * G] = fmax(o[(size_t)GS_MAX * G], y);
                o[9 * (size_t)G] += 1.0;
            }
            __syncthreads();                        // the next row adds after this one: fixed order per (plane, gene)
        }
    }
}

// CSR: the nine planes from the ten folded ones; a column that stores fewer than n entries holds an implicit 0
__global__ __launch_bounds__(256) void gs_csr_finish_kernel(const double* __restrict__ folded, int G, double n,
                                                            double* __restrict__ sums) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= G) return;
    const bool implicit_zero = folded[(size_t)9 * G + j] < n;
#pragma unroll
    for (int k = 0; k < GS_PLANES; ++k) {
        double v = folded[(size_t)k * G + j];
        if (implicit_zero && k == GS_MIN) v = fmin(v, 0.0);
        if (implicit_zero && k == GS_MAX) v = fmax(v, 0.0);
        sums[(size_t)k * G + j] = v;
    }
}

// counts[0 .. 1] = {sum deg, sum deg^2} over the n_seg segment pairs: one workgroup, integers (any order gives the same sums)
__global__ __launch_bounds__(256) void gs_counts_kernel(const long long* __restrict__ deg_part, int n_seg, long long* __restrict__ counts) {
    __shared__ long long red[2][256];
    long long sd = 0, sd2 = 0;
    for (int s = threadIdx.x; s < n_seg; s += 256) {
        sd += deg_part[2 * (size_t)s];
        sd2 += deg_part[2 * (size_t)s + 1];
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

template <typename T>
void launch_csr(const fdx_csr_view* Y, const T* values, const GraphTables& t, int sb0, int nb, int stripe, double* part, int* deg_out,
                long long* deg_part, hipStream_t st) {
    auto* kernel = Y->sorted_rows ? gs_csr_kernel<T, true> : gs_csr_kernel<T, false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)ceil_div(nb, stripe)), dim3(256), 0, st, (const long long*)Y->indptr, Y->indices, values, t,
                       sb0, nb, stripe, Y->G, part, deg_out, deg_part);
}

// The nine planes of fdx.h over a whole graph of t.n >= 1 spots.  Everything queued on st: the planes to sums (device), deg_out
// (device, may be null), {sum deg, sum deg^2} to counts (device); the segment sums live in the pool.
int launch_gene_spatial_sums(const GraphTables& t, const GeneMatrix& y, double* sums, int* deg_out, long long* counts, hipStream_t st) {
    const int n_seg = ceil_div(t.n, GS_SEG), G = y.G;
    const int planes = y.sparse ? GS_CSR_PLANES : GS_PLANES;
    const int stripe = stripe_segments();
    const size_t seg_bytes = (size_t)planes * G * sizeof(double);
    DevBuf deg_buf, folded;
    FDX_TRY(deg_buf.alloc((size_t)n_seg * 2 * sizeof(long long)));
    if (y.sparse) FDX_TRY(folded.alloc(seg_bytes));
    long long* deg_part = deg_buf.as<long long>();
    double* fold_out = y.sparse ? folded.as<double>() : sums;
    FDX_TRY(for_segment_batches(n_seg, seg_bytes, [&](int sb0, int nb, double* part) {
        dispatch_gene_matrix(
            y, [&](auto* Yd) {
                hipLaunchKernelGGL(gs_dense_kernel, dim3((unsigned)ceil_div(nb, stripe), (unsigned)ceil_div(G, GS_GENES)), dim3(256), 0,
                                   st, Yd, y.ldy, t, sb0, nb, stripe, G, part, deg_out, deg_part);
                return 0;
            },
            [&](auto* values) { return launch_csr(y.csr, values, t, sb0, nb, stripe, part, deg_out, deg_part, st), 0; });
        FDX_CHECK_LAUNCH();
        const SegmentBlocks b{part, (long long)planes * G, (long long)G, 1LL, sb0, nb};
        return launch_gene_fold(b, 0, planes, G, nullptr, 1, fold_out, 0, (long long)G, GS_MIN, GS_MAX, st);
    }));
    if (y.sparse) {
        hipLaunchKernelGGL(gs_csr_finish_kernel, dim3((unsigned)ceil_div(G, 256)), dim3(256), 0, st, fold_out, G, (double)t.n, sums);
        FDX_CHECK_LAUNCH();
    }
    return launch_segment_degree_counts(deg_part, n_seg, counts, st);
}

int gene_spatial_entry(const char* who, const fdx_graph* g, const GeneMatrix& y, double* sums_dev, int* deg_dev, int64_t* counts_out,
                       void* stream) {
    const std::string w(who);
    hipStream_t st = (hipStream_t)stream;
    FDX_TRY(check_gene_matrix(who, y, g && sums_dev && counts_out, false, "ldy < G"));
    FDX_REQUIRE(y.G >= 1, w + ": G must be at least 1");
    FDX_REQUIRE(y.G <= GS_GENES * 65535, w + ": too many genes for one call");
    FDX_REQUIRE(y.n >= 0 && y.n < (1LL << 31) - 128, w + ": n must be between 0 and 2^31 - 129");
    GraphTables t;
    FDX_TRY(whole_graph_tables(g, who, &t));
    FDX_REQUIRE(y.n == t.n, w + ": Y has " + std::to_string(y.n) + " rows but the graph has " + std::to_string(t.n) + " spots");
    PoolStream pool_stream(st);
    counts_out[0] = t.n;
    counts_out[1] = counts_out[2] = 0;
    if (t.n == 0) {                                 // empty sums; no value to be the smallest or the largest
        std::vector<double> h((size_t)GS_PLANES * y.G, 0.0);
        std::fill(h.begin() + (size_t)GS_MIN * y.G, h.end(), std::numeric_limits<double>::quiet_NaN());
        FDX_TRY(copy_h2d(sums_dev, h.data(), h.size() * sizeof(double), st));
        FDX_HIP(hipStreamSynchronize(st));
        return 0;
    }
    DevBuf counts;
    FDX_TRY(counts.alloc(2 * sizeof(long long)));
    FDX_TRY(launch_gene_spatial_sums(t, y, sums_dev, deg_dev, counts.as<long long>(), st));
    long long host[2];
    FDX_TRY(copy_d2h(host, counts.p, sizeof(host), st));         // the call's one host synchronisation
    counts_out[1] = host[0];
    counts_out[2] = host[1];
    return 0;
}

}  // namespace

int launch_segment_degree_counts(const long long* deg_part, int n_seg, long long* counts, hipStream_t st) {
    hipLaunchKernelGGL(gs_counts_kernel, dim3(1), dim3(256), 0, st, deg_part, n_seg, counts);
    FDX_CHECK_LAUNCH();
    return 0;
}

}  // namespace fdx

using namespace fdx;

extern "C" {

int fdx_gene_spatial_sums_dev(const fdx_graph* g, const void* Y_dev, int32_t dtype, int64_t n, int32_t G, int64_t ldy,
                              double* sums_dev, int32_t* deg_dev, int64_t* counts_out, void* stream) {
    return gene_spatial_entry("fdx_gene_spatial_sums_dev", g, GeneMatrix(Y_dev, dtype, n, G, ldy), sums_dev, deg_dev, counts_out, stream);
}

int fdx_gene_spatial_sums_csr_dev(const fdx_graph* g, const fdx_csr_view* Y, double* sums_dev, int32_t* deg_dev, int64_t* counts_out,
                                  void* stream) {
    return gene_spatial_entry("fdx_gene_spatial_sums_csr_dev", g, GeneMatrix(Y), sums_dev, deg_dev, counts_out, stream);
}

}  // extern "C"
