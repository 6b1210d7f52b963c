// Spatial graph construction on the device: what the four graph sources share (internal).
//
// Replaces flashdeconv/utils/graph.py:
//   build_knn_graph    :25-83   (cKDTree build + query k+1 incl. self, drop self, A + A^T, binary)
//   build_radius_graph :86-133  (cKDTree.query_pairs(r), symmetric)
// and hands the result to the solver in the sliced-ELL layout of fdx_graph.h.
//
// Pipeline (all on the stream, one small D2H for the bounding box):
//   1. bounding box -> uniform grid with ~4 points per cell (k-NN; radius graphs: cell edge >= radius).
//   2. order by (Morton code of the cell, original index) -> perm / rank: count per key, scan, rank within the cell
//      (rocPRIM's stable radix sort above 4M keys; same order either way).  Points inside a cell keep caller order,
//      and any 256 consecutive sorted points form a compact patch (small tile halo in the BCD sweep).
//   3. exact k-NN: one lane per point scans the cells of growing Chebyshev shells until the k+1-th best squared distance
//      is provably inside the scanned block.  Squared distances are evaluated in float64 WITHOUT fma contraction
//      ((dx*dx + dy*dy) + dz*dz, each rounded) and ties are broken by the lower original index.
//   4. union symmetrisation: in-degree count (inside the k-NN kernel for whole-graph builds), reverse lists, per-row sort
//      by original index + unique.
//   5. sliced ELL (slice = 64 consecutive sorted points = one wavefront of the BCD sweep).
//
// graph_bin.cpp: steps 1-2.  graph_knn.cpp: step 3, the band of a spot shard, the plan of a two-phase build.  graph_ell.cpp: steps 4-5,
// the radius graph, export.  graph_shard.cpp: a shard's local graph (graph_localize, the deferred shard build).
// A __global__ function lives in the source that launches it; what another source needs of it crosses as a host function below.
#pragma once
#include <algorithm>
#include <cmath>
#include <functional>
#include <memory>
#include <vector>

#include "fdx_env.h"
#include "fdx_graph.h"
#include "fdx_internal.h"
#include "fdx_kernels.h"
#include "graph_build.h"

namespace fdx {

struct GridParams {
    double mn[3];
    double inv_h[3];
    double h[3];
    int nc[3];       // cells per axis (1 for unused / zero-extent axes)
    int stride[3];   // cell id = sum_a c_a * stride[a]
    int dim;
};

__device__ __forceinline__ int cell_coord(double x, double mn, double inv_h, int nc) {
    int c = (int)floor((x - mn) * inv_h);
    return max(0, min(nc - 1, c));
}

__device__ __forceinline__ double dist2_exact(double dx, double dy, double dz) {
    // sum of squares with every product and sum rounded, as a host float64 loop computes it: no fma contraction (the
    // compiler's default for device code, and __dmul_rn / __dadd_rn are plain operators to it)
#pragma clang fp contract(off)
    const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
    return (xx + yy) + zz;
}

constexpr int FDX_KNN_MAX_DIM = 8;           // k-NN graphs: above three coordinates the search is exhaustive (graph_knn.cpp)
constexpr int BAND_R = 2;                    // the band of a spot shard: rows of cells within BAND_R cells of an own cell (graph_knn.cpp)
constexpr int SLICE_WIDTH_BLOCKS = 1024;     // most blocks of slice_width_kernel: a (sum, max) pair of partials each
constexpr int SHARD_MAX_RANKS = 32;
struct ShardBounds { long long b[SHARD_MAX_RANKS + 1]; };      // range starts of the ranks, by value (no upload to wait for)

struct BinnedPoints {
    GridParams gp;
    DevBuf perm, rank, sc, sc2, cstart;            // sc2: (x, y) pairs of the sorted points, dim <= 2 only; cstart also holds cend, the key counters and the need flags
    int* cend_p = nullptr;                         // cell -> end of its range (inside cstart's block)
    int* count_p = nullptr;                        // counting path: members per key
    unsigned char* need_p = nullptr;               // spot shards: [bins] keys within BAND_R cells of an own key, [bins] within 2 BAND_R
    DevBuf keys, vals, skeys, sort_tmp, start, scan_tmp;   // sort temporaries: kept until the struct dies so that binning needs no final sync
    long long n = 0;
    int n_cells = 0;
    long long bins = 0;            // counting path: size of the Morton key space (start has bins + 1 entries); 0 on the sorting path
};

// A set of rows that have lists: the direct range [first, first + n_direct), then the first min(*n_listed, cap) rows of `listed`
// (NULL: none) - a shard's own rows and its band; all rows of the order are the direct range [0, n).
struct RowSet {
    long long first, n_direct;
    const int* listed;
    const int* n_listed;       // device-side count
    int cap;
    long long threads() const { return n_direct + (listed ? cap : 0); }
};
__device__ __forceinline__ long long row_of_set(const RowSet& rs, long long i) {   // row of thread i, -1: none
    if (i < rs.n_direct) return rs.first + i;
    i -= rs.n_direct;
    if (!rs.listed || i >= rs.cap || i >= *rs.n_listed) return -1;
    return rs.listed[i];
}

// nnz and the widest slice from the blocks' partials of slice_width_kernel: a workgroup of 256 threads, every thread gets both
__device__ __forceinline__ void reduce_width_partials(const long long* __restrict__ part, int n_part, long long* nnz, int* widest) {
    __shared__ long long s_sum[256];
    __shared__ int s_max[256];
    long long tot = 0;
    int wmax = 0;
    for (int b = threadIdx.x; b < n_part; b += 256) { tot += part[2 * b]; wmax = max(wmax, (int)part[2 * b + 1]); }
    s_sum[threadIdx.x] = tot;
    s_max[threadIdx.x] = wmax;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            s_sum[threadIdx.x] += s_sum[threadIdx.x + s];
            s_max[threadIdx.x] = max(s_max[threadIdx.x], s_max[threadIdx.x + s]);
        }
        __syncthreads();
    }
    *nnz = s_sum[0];
    *widest = s_max[0];
}
// the first five words of a queued build's pinned block: [0] ELL rows, [1] nnz, [2] widest slice, [3] largest tile halo |
// failed-tile flag << 32, [4] tied rows
__device__ __forceinline__ void write_meta_head(long long* __restrict__ meta, const int* __restrict__ slice_off, int n_slices,
                                                long long nnz, int widest, const int* __restrict__ summary,
                                                const int* __restrict__ ties) {
    meta[0] = (long long)slice_off[n_slices];
    meta[1] = nnz;
    meta[2] = (long long)widest;
    meta[3] = (long long)(unsigned)summary[0] | ((long long)summary[1] << 32);
    meta[4] = ties ? (long long)ties[0] : 0;
}

inline void trace_host(const char* what) { trace_host(nullptr, what); }   // the steps of a graph build

// rocPRIM's two calls: ask for the size of the temporary storage, grow `tmp` to it, run.  call(void* temp, size_t& bytes) -> hipError_t
template <class Call>
int with_temp(DevBuf& tmp, Call&& call) {
    size_t bytes = 0;
    FDX_HIP(call(nullptr, bytes));
    if (tmp.bytes < bytes) FDX_TRY(tmp.alloc(bytes));
    FDX_HIP(call(tmp.p, bytes));
    return 0;
}

// ---- graph_bin.cpp
// shard_lo < shard_hi: a spot shard's binning - the ranking pass lays out only the cells the shard's build looks at
// (cell_need_kernel; counting path only: the sorting path lays out everything)
int bin_points(const double* d_coords, long long n, int dim, double target_per_cell, double min_h, BinnedPoints* b, hipStream_t st,
               long long shard_lo = 0, long long shard_hi = 0, int shard_R = 0, const std::function<int()>* extra_under_wait = nullptr);

// ---- graph_ell.cpp: the stages the whole-graph builds and the shard builds share
int exclusive_scan_int(const int* in, int* out, long long count, hipStream_t st, DevBuf& tmp);
// Union symmetrisation of rows [lo, hi) (utils/graph.py:80-81), queued on st: in-degrees over the row set -> scan -> reverse lists ->
// merge_rows_kernel.  indeg (count + 1 ints), cursor (count), rev_off (count + 1), ws (segments of capacity kk + in-degree, 2 kk per
// row at most) and deg are indexed by row - base over `count` rows: base 0 and count n for arrays over the whole order, base lo and
// count hi - lo for a shard's local ones.  indeg and cursor arrive zeroed.  arrival != NULL: the k-NN kernel has counted (indeg) and
// drawn the places (arrival) already.  rev_cap: entries of the reverse list, a bound the host knows; < 0: read back behind the scan.
int symmetrise_rows(const int* nbr, const int* cnt, int kk, const RowSet& rs, long long lo, long long hi, long long base, long long count,
                    int* indeg, int* cursor, int* rev_off, const int* arrival, DevBuf& rev, long long rev_cap, const int* perm,
                    const int* rank, int* ws, int* deg, hipStream_t st, DevBuf& scan_tmp);
// width[s] of every slice, the blocks' partials (wblocks of them) and slice_off = the scan of the widths
int queue_slice_offsets(const int* deg, long long n, int n_slices, int wblocks, int* width, long long* part, int* summary_zero,
                        int* slice_off, hipStream_t st, DevBuf& scan_tmp);
// ELL rows per slice a queued build leaves room for: three times the list length, at least 24 (slice widths of a k = 6 graph are
// 9-12), at most 96; forced (tests): what FDX_GRAPH_WCAP says
int ell_w_cap(int list_len, bool forced);
// sliced ELL from the row segments.  hscan == NULL: entries as they are, pad index `pad`.  Else a shard's local indices: own
// neighbour q -> q - lo, outside -> n + hscan[q] (its halo slot), pad -> n + hscan[n_all]
int queue_fill_ell(const int* ws, int seg_stride, const int* seg_extra, const int* deg, const int* slice_off, long long n, int n_slices,
                   int pad, int* ell, long long cap_rows, hipStream_t st, long long lo = 0, const int* hscan = nullptr, long long n_all = 0);
// tile tables of g (n, deg, slice_off, ell set): allocates tile_halo / tile_hcnt / ell_local for cap_rows ELL rows and queues the
// tile kernel - over the ELL, or (ws != NULL) in one pass over the row segments that writes the global-index ELL too
int queue_tile_tables(fdx_graph* g, long long cap_rows, int* summary, hipStream_t st, const int* ws = nullptr, int seg_stride = 0,
                      const int* seg_extra = nullptr);

// ---- graph_shard.cpp
int shard_meta_sync(fdx_graph* g);               // takes over what a queued shard build left in the pinned block

}  // namespace fdx

struct fdx_graph_plan {
    fdx::BinnedPoints b;
    long long n = 0;
    int kk = 0;
    hipStream_t st = nullptr;      // stream the binning / k-NN kernels were queued on
    fdx::DevBuf indeg, arrival;    // whole graph in one piece: in-degrees and reverse-list places from the k-NN kernel
    fdx::DevBuf ties;              // [0] rows of [lo, hi) with a tie at the k-th neighbour, [1] some walk of [lo, hi) left the 3 x 3 block (knn_kernel)
    // spot shard with band recompute (graph_knn_lists, band = true): the rows outside [lo, hi) whose lists were found here,
    // counters = {cells listed, band rows, -, band list overflowed}
    fdx::DevBuf band_rows, band_counters;
    int band_cap = 0;
    bool kernels_done = false;     // set by graph_meta_sync: the graph's meta event (recorded behind every kernel that reads
                                   // the plan) has completed - no stream sync needed, which would also wait for whatever the
                                   // caller queued behind the build (the sketch kernel of the fit)
    ~fdx_graph_plan() { if (!kernels_done) (void)hipStreamSynchronize(st); }   // nothing may still read the buffers when they go back to the pool
};

struct fdx_shard_build {
    fdx_graph_plan* plan = nullptr;
    fdx::DevBuf nbr, cnt, zeros, rev_off, rev, rows, hscan, mask, off_rb, tileflag, tile_counts, scan_tmp;
    // what the second phase (shard_queue_rest) needs; `queued` = it has run
    long long n = 0, lo = 0, hi = 0;
    int kk = 0, n_ranks = 0;
    long long bounds[fdx::SHARD_MAX_RANKS + 1] = {};
    hipStream_t st_first = nullptr;          // stream of the first phase (the caller's)
    hipEvent_t ev_first = nullptr;           // recorded there behind the k-NN lists and the copy of the own rows' ids
    bool queued = false;
    std::shared_ptr<fdx::HelperTicket> ticket;   // the second phase was handed to the helper thread: wait before touching anything it writes
    ~fdx_shard_build() {
        if (plan) fdx::graph_plan_destroy(plan);
        if (ev_first) (void)hipEventDestroy(ev_first);
    }
};
