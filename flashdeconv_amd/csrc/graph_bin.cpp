// Graph build, steps 1-2 (graph_internal.h): bounding box, grid, and the order of the points by (Morton code of the cell, index).
#include <rocprim/device/device_radix_sort.hpp>

#include <cstring>
#include <memory>

#include "graph_build.h"
#include "graph_internal.h"

namespace fdx {

// ------------------------------------------------------------------------------------------------ bbox
__device__ __forceinline__ double wave_min_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}
// (the tree reduction of six 256-entry LDS arrays this kernel used to end with - eight barrier-separated steps - made a 16 MB
// read take 37-47 us; the loop itself is a few microseconds: wave shuffles, then four values per quantity through LDS)
__global__ __launch_bounds__(256) void bbox_partial_kernel(const double* __restrict__ coords, long long n, int dim,
                                                           double* __restrict__ part /* (nblk, 6) */) {
    __shared__ double s_v[6][4];
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (dim == 2 && ((unsigned long long)coords & 15ULL) == 0ULL) {      // one 16-byte load per point
        const double2* c2 = reinterpret_cast<const double2*>(coords);
        const long long stride = (long long)gridDim.x * 256;
        long long i = blockIdx.x * 256LL + threadIdx.x;
        for (; i + 3 * stride < n; i += 4 * stride) {          // four loads in flight per thread
            const double2 a = c2[i], b = c2[i + stride], c = c2[i + 2 * stride], d = c2[i + 3 * stride];
            mn[0] = fmin(fmin(mn[0], a.x), fmin(fmin(b.x, c.x), d.x)); mx[0] = fmax(fmax(mx[0], a.x), fmax(fmax(b.x, c.x), d.x));
            mn[1] = fmin(fmin(mn[1], a.y), fmin(fmin(b.y, c.y), d.y)); mx[1] = fmax(fmax(mx[1], a.y), fmax(fmax(b.y, c.y), d.y));
        }
        for (; i < n; i += stride) {
            const double2 v = c2[i];
            mn[0] = fmin(mn[0], v.x); mx[0] = fmax(mx[0], v.x);
            mn[1] = fmin(mn[1], v.y); mx[1] = fmax(mx[1], v.y);
        }
    } else {
        for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
            for (int a = 0; a < dim; ++a) {
                const double v = coords[(size_t)i * dim + a];
                mn[a] = fmin(mn[a], v);
                mx[a] = fmax(mx[a], v);
            }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double lo = wave_min_f64(mn[a]), hi = wave_max_f64(mx[a]);
        if (lane == 0) { s_v[a][wv] = lo; s_v[3 + a][wv] = hi; }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int a = threadIdx.x;
        part[(size_t)blockIdx.x * 6 + a] = fmin(fmin(s_v[a][0], s_v[a][1]), fmin(s_v[a][2], s_v[a][3]));
        part[(size_t)blockIdx.x * 6 + 3 + a] = fmax(fmax(s_v[3 + a][0], s_v[3 + a][1]), fmax(s_v[3 + a][2], s_v[3 + a][3]));
    }
}

// the blocks' boxes folded into one, written where `out` points (the host's pinned block): no copy to wait for
__global__ __launch_bounds__(256) void bbox_final_kernel(const double* __restrict__ part, int nblk, double* __restrict__ out) {
    __shared__ double smn[3][256], smx[3][256];
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool bad = false;
    for (int b = threadIdx.x; b < nblk; b += 256)
        for (int a = 0; a < 3; ++a) {
            const double lo = part[(size_t)b * 6 + a], hi = part[(size_t)b * 6 + 3 + a];
            bad = bad || lo != lo || hi != hi;           // fmin / fmax drop a NaN: carry it by hand
            mn[a] = fmin(mn[a], lo);
            mx[a] = fmax(mx[a], hi);
        }
    for (int a = 0; a < 3; ++a) { smn[a][threadIdx.x] = bad ? NAN : mn[a]; smx[a][threadIdx.x] = mx[a]; }
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int a = 0; a < 3; ++a) {
                const double x = smn[a][threadIdx.x], y = smn[a][threadIdx.x + s];
                smn[a][threadIdx.x] = (x != x || y != y) ? NAN : fmin(x, y);
                smx[a][threadIdx.x] = fmax(smx[a][threadIdx.x], smx[a][threadIdx.x + s]);
            }
        __syncthreads();
    }
    if (threadIdx.x < 3) {
        out[threadIdx.x] = smn[threadIdx.x][0];
        out[3 + threadIdx.x] = smx[threadIdx.x][0];
    }
}

// ------------------------------------------------------------------------------------------------ binning

// Morton (Z-order) code of a cell: 256 consecutive points of the sorted order form a compact 2-D/3-D patch, which keeps
// the halo of a 256-spot workgroup tile of the BCD sweep small (perimeter instead of two full grid rows).
__host__ __device__ __forceinline__ unsigned long long spread_bits_2(unsigned long long v) {   // abcd -> 0a0b0c0d
    v &= 0xffffffffULL;
    v = (v | (v << 16)) & 0x0000ffff0000ffffULL;
    v = (v | (v << 8)) & 0x00ff00ff00ff00ffULL;
    v = (v | (v << 4)) & 0x0f0f0f0f0f0f0f0fULL;
    v = (v | (v << 2)) & 0x3333333333333333ULL;
    v = (v | (v << 1)) & 0x5555555555555555ULL;
    return v;
}
__host__ __device__ __forceinline__ unsigned long long spread_bits_3(unsigned long long v) {   // 21 bits -> every third bit
    v &= 0x1fffffULL;
    v = (v | (v << 32)) & 0x1f00000000ffffULL;
    v = (v | (v << 16)) & 0x1f0000ff0000ffULL;
    v = (v | (v << 8)) & 0x100f00f00f00f00fULL;
    v = (v | (v << 4)) & 0x10c30c30c30c30c3ULL;
    v = (v | (v << 2)) & 0x1249249249249249ULL;
    return v;
}
__device__ __forceinline__ unsigned long long morton_key(const int c[3], int dim) {
    if (dim == 1) return (unsigned long long)c[0];
    if (dim == 2) return spread_bits_2((unsigned)c[0]) | (spread_bits_2((unsigned)c[1]) << 1);
    return spread_bits_3((unsigned)c[0]) | (spread_bits_3((unsigned)c[1]) << 1) | (spread_bits_3((unsigned)c[2]) << 2);
}
__device__ __forceinline__ unsigned compact_bits_2(unsigned long long v) {                 // 0a0b0c0d -> abcd
    v &= 0x5555555555555555ULL;
    v = (v | (v >> 1)) & 0x3333333333333333ULL;
    v = (v | (v >> 2)) & 0x0f0f0f0f0f0f0f0fULL;
    v = (v | (v >> 4)) & 0x00ff00ff00ff00ffULL;
    v = (v | (v >> 8)) & 0x0000ffff0000ffffULL;
    v = (v | (v >> 16)) & 0x00000000ffffffffULL;
    return (unsigned)v;
}
__device__ __forceinline__ unsigned compact_bits_3(unsigned long long v) {                 // every third bit -> 21 bits
    v &= 0x1249249249249249ULL;
    v = (v | (v >> 2)) & 0x10c30c30c30c30c3ULL;
    v = (v | (v >> 4)) & 0x100f00f00f00f00fULL;
    v = (v | (v >> 8)) & 0x1f0000ff0000ffULL;
    v = (v | (v >> 16)) & 0x1f00000000ffffULL;
    v = (v | (v >> 32)) & 0x1fffffULL;
    return (unsigned)v;
}

__global__ __launch_bounds__(256) void cell_key_kernel(const double* __restrict__ coords, long long n, GridParams gp,
                                                       unsigned long long* __restrict__ keys, int* __restrict__ vals) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= n) return;
    int c[3] = {0, 0, 0};
    for (int a = 0; a < gp.dim; ++a) c[a] = cell_coord(coords[(size_t)i * gp.dim + a], gp.mn[a], gp.inv_h[a], gp.nc[a]);
    keys[i] = morton_key(c, gp.dim);
    vals[i] = (int)i;
}

// cell table (row-major cell id -> [start, end) in the sorted order); equal Morton key <=> same cell
__global__ __launch_bounds__(256) void cell_range_kernel(const unsigned long long* __restrict__ skeys,
                                                         const double* __restrict__ sc, long long n, GridParams gp,
                                                         int* __restrict__ cstart, int* __restrict__ cend) {
    const long long p = blockIdx.x * 256LL + threadIdx.x;
    if (p >= n) return;
    const unsigned long long k = skeys[p];
    const bool first = (p == 0 || skeys[p - 1] != k), last = (p == n - 1 || skeys[p + 1] != k);
    if (!first && !last) return;
    int id = 0;
    for (int a = 0; a < gp.dim; ++a) id += cell_coord(sc[(size_t)a * n + p], gp.mn[a], gp.inv_h[a], gp.nc[a]) * gp.stride[a];
    if (first) cstart[id] = (int)p;
    if (last) cend[id] = (int)p + 1;
}

// sorted coordinate planes sc[a*n + p] and rank[perm[p]] = p
__global__ __launch_bounds__(256) void gather_sorted_kernel(const double* __restrict__ coords, const int* __restrict__ perm,
                                                            long long n, int dim, double* __restrict__ sc,
                                                            int* __restrict__ rank, double2* __restrict__ sc2) {
    const long long p = blockIdx.x * 256LL + threadIdx.x;
    if (p >= n) return;
    const int o = perm[p];
    for (int a = 0; a < 3; ++a) sc[(size_t)a * n + p] = (a < dim) ? coords[(size_t)o * dim + a] : 0.0;
    if (sc2) sc2[p] = make_double2(coords[(size_t)o * dim], dim > 1 ? coords[(size_t)o * dim + 1] : 0.0);
    rank[o] = (int)p;
}

// ---- binning without a sort (Morton key space of at most a few million bins): count per key, scan, place.
// The order produced is the stable sort's: cells in Morton order, points of a cell by ascending index.
// pass 1: key of every point, and its arrival number among the points of the same key (any order)
__global__ __launch_bounds__(256) void cell_count_kernel(const double* __restrict__ coords, long long n, GridParams gp,
                                                         unsigned* __restrict__ key32, int* __restrict__ arrival,
                                                         int* __restrict__ count) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= n) return;
    int c[3] = {0, 0, 0};
    for (int a = 0; a < gp.dim; ++a) c[a] = cell_coord(coords[(size_t)i * gp.dim + a], gp.mn[a], gp.inv_h[a], gp.nc[a]);
    const unsigned k = (unsigned)morton_key(c, gp.dim);
    key32[i] = k;
    arrival[i] = atomicAdd(&count[k], 1);
}
// pass 2: the members of every key, contiguous, in arrival order
__global__ __launch_bounds__(256) void cell_place_kernel(const unsigned* __restrict__ key32, const int* __restrict__ arrival,
                                                         const int* __restrict__ start, long long n, int* __restrict__ members) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= n) return;
    members[start[key32[i]] + arrival[i]] = (int)i;
}
// pass 3: position of point i = start of its key + number of members with a smaller index (cells hold a handful of
// points); writes everything the sorted order defines: perm, rank, sorted coordinate planes
__global__ __launch_bounds__(256) void cell_rank_kernel(const double* __restrict__ coords, const unsigned* __restrict__ key32,
                                                        const int* __restrict__ start, const int* __restrict__ members,
                                                        long long n, int dim, int* __restrict__ perm, int* __restrict__ rank,
                                                        double* __restrict__ sc, double2* __restrict__ sc2,
                                                        const unsigned char* __restrict__ need) {
    // need != NULL (a spot shard's binning): only the cells the shard will look at are laid out - perm / rank / coordinates of
    // the others are never written, and never read (cell_need_kernel)
    // thread t takes the point that ARRIVED at slot t: its sorted position lies in the same cell's range as t, so the writes of
    // a wave (perm, the coordinate planes, the pairs) fall into one contiguous stretch - five scattered stores per point became
    // two gathers (key, coordinates) and one scattered store (rank)
    const long long t = blockIdx.x * 256LL + threadIdx.x;
    if (t >= n) return;
    const int i = members[t];
    const unsigned k = key32[i];
    if (need && !need[k]) return;
    const int s = start[k], e = start[k + 1];
    int below = 0;
    for (int q = s; q < e; ++q) below += (members[q] < i) ? 1 : 0;
    const int p = s + below;
    perm[p] = i;
    rank[i] = p;
    for (int a = 0; a < dim; ++a) sc[(size_t)a * n + p] = coords[(size_t)i * dim + a];   // planes past dim: zeroed by the caller (one contiguous fill)
    if (sc2) sc2[p] = make_double2(coords[(size_t)i * dim], dim > 1 ? coords[(size_t)i * dim + 1] : 0.0);   // (x, y) pairs: one 16-byte gather per k-NN candidate
}

// pass 4: the cell table (row-major cell id -> [start, end) of the sorted order) straight from the key starts: an occupied
// key IS a cell, its Morton code gives the cell coordinates back
__global__ __launch_bounds__(256) void cell_table_kernel(const int* __restrict__ start, long long bins, GridParams gp,
                                                         int* __restrict__ cstart, int* __restrict__ cend) {
    const long long k = blockIdx.x * 256LL + threadIdx.x;
    if (k >= bins) return;
    const int s0 = start[k], s1 = start[k + 1];
    if (s1 <= s0) return;
    int c[3] = {0, 0, 0};
    if (gp.dim == 1) c[0] = (int)k;
    else if (gp.dim == 2) { c[0] = (int)compact_bits_2((unsigned long long)k); c[1] = (int)compact_bits_2((unsigned long long)k >> 1); }
    else { c[0] = (int)compact_bits_3((unsigned long long)k); c[1] = (int)compact_bits_3((unsigned long long)k >> 1); c[2] = (int)compact_bits_3((unsigned long long)k >> 2); }
    const int id = c[0] * gp.stride[0] + c[1] * gp.stride[1] + c[2] * gp.stride[2];
    cstart[id] = s0;
    cend[id] = s1;
}

// A spot shard owns positions [lo, hi) of the sorted order.  Its build looks at: the own rows, the rows of cells within BAND_R cells
// of an own cell (the band, whose lists it finds itself), and - walking those lists - cells within BAND_R shells of a band cell.
// Only those cells need their points laid out (perm, rank, sorted coordinates): the ranking pass, the one pass of the binning
// that gathers coordinates and scatters, then costs the shard's share instead of all n points.  Two dilations by BAND_R of the
// set of own cells (keys whose range meets [lo, hi)); a walk that goes further reports itself (knn_kernel: far) and the build
// is redone by exchange with a full binning.
__device__ __forceinline__ void cell_of_key(long long k, int dim, int c[3]) {
    c[0] = c[1] = c[2] = 0;
    if (dim == 1) c[0] = (int)k;
    else if (dim == 2) { c[0] = (int)compact_bits_2((unsigned long long)k); c[1] = (int)compact_bits_2((unsigned long long)k >> 1); }
    else { c[0] = (int)compact_bits_3((unsigned long long)k); c[1] = (int)compact_bits_3((unsigned long long)k >> 1); c[2] = (int)compact_bits_3((unsigned long long)k >> 2); }
}
template <int PASS>
__global__ __launch_bounds__(256) void cell_need_kernel(const int* __restrict__ start, long long bins, GridParams gp, long long lo,
                                                        long long hi, int R, const unsigned char* __restrict__ in,
                                                        unsigned char* __restrict__ out) {
    const long long k = blockIdx.x * 256LL + threadIdx.x;
    if (k >= bins) return;
    const bool seed = PASS == 0 ? (start[k + 1] > start[k] && (long long)start[k] < hi && (long long)start[k + 1] > lo) : (in[k] != 0);
    if (!seed) return;
    int c[3];
    cell_of_key(k, gp.dim, c);
    const int r1 = gp.dim > 1 ? R : 0, r2 = gp.dim > 2 ? R : 0;
    for (int dz = -r2; dz <= r2; ++dz)
        for (int dy = -r1; dy <= r1; ++dy)
            for (int dx = -R; dx <= R; ++dx) {
                int cc[3] = {c[0] + dx, c[1] + dy, c[2] + dz};
                if (cc[0] < 0 || cc[0] >= gp.nc[0] || cc[1] < 0 || cc[1] >= gp.nc[1] || cc[2] < 0 || cc[2] >= gp.nc[2]) continue;
                const unsigned long long kk = morton_key(cc, gp.dim);
                if ((long long)kk < bins) out[kk] = 1;
            }
}

// ------------------------------------------------------------------------------------------------ host side
// The bounding box is the one thing the host must read before it can queue the rest of a build (grid parameters size every
// launch).  bbox_begin queues it - block partials, one workgroup folds them and writes the six numbers into a pinned block -
// and make_grid waits for its event.  (Queueing it ahead of the fit's other host work - a hint entry the fit called before it
// set up the leverage job - was tried: the box arrives earlier, the leverage scores later, the wall time is the same.)
struct BboxJob {
    const double* coords = nullptr;
    long long n = 0;
    int dim = 0, dev = 0;
    hipEvent_t ev = nullptr;
    double* host = nullptr;      // pinned_block_get(): mn[3], mx[3]
    DevBuf part;
    ~BboxJob() {
        if (ev) { (void)hipEventSynchronize(ev); (void)hipEventDestroy(ev); }
        if (host) pinned_block_put(host);
    }
};

static int bbox_begin(const double* d_coords, long long n, int dim, hipStream_t st, BboxJob* job) {
    job->coords = d_coords; job->n = n; job->dim = dim;
    FDX_HIP(hipGetDevice(&job->dev));
    // (256 to 16384 blocks, one to sixteen points per thread, four loads in flight or one: 33-60 us for the 16 MB of a million 2-D
    // points whatever the shape - the kernel's time is not its loop; 512 blocks measured best)
    const int nblk = (int)std::min<long long>(512, (n + 255) / 256);
    FDX_TRY(job->part.alloc((size_t)nblk * 6 * sizeof(double)));
    job->host = (double*)pinned_block_get();
    FDX_REQUIRE(job->host != nullptr, "graph: pinned host block");
    void* host_dev = nullptr;
    FDX_HIP(hipHostGetDevicePointer(&host_dev, job->host, 0));
    FDX_HIP(hipEventCreateWithFlags(&job->ev, hipEventDisableTiming));
    hipLaunchKernelGGL(bbox_partial_kernel, dim3(nblk), dim3(256), 0, st, d_coords, n, dim, job->part.as<double>());
    hipLaunchKernelGGL(bbox_final_kernel, dim3(1), dim3(256), 0, st, job->part.as<double>(), nblk, (double*)host_dev);
    FDX_CHECK_LAUNCH();
    FDX_HIP(hipEventRecord(job->ev, st));
    return 0;
}

// The cache lookup's compare kernels (graph_cache.cpp) write into a pinned block as the box kernels do, and nothing else of a
// lookup runs on the device: a hit is decided by the flags alone, so no box is computed for it (25 us of kernels on every hit);
// a miss computes its box in the build that follows, as a build without a candidate does.
int flag_words(hipStream_t st, const std::function<int(long long*)>& queue, long long words[4]) {
    BboxJob job;                                               // (its pinned block and event; no box kernels)
    job.host = (double*)pinned_block_get();
    FDX_REQUIRE(job.host != nullptr, "graph: pinned host block");
    void* host_dev = nullptr;
    FDX_HIP(hipHostGetDevicePointer(&host_dev, job.host, 0));
    FDX_HIP(hipEventCreateWithFlags(&job.ev, hipEventDisableTiming));
    for (int j = 0; j < 4; ++j) job.host[j] = 0.0;             // (all bits zero)
    FDX_TRY(queue(reinterpret_cast<long long*>(host_dev)));
    FDX_HIP(hipEventRecord(job.ev, st));
    FDX_HIP(hipEventSynchronize(job.ev));
    std::memcpy(words, job.host, 4 * sizeof(long long));
    return 0;
}

// under_wait: queued behind the bounding-box kernels and ahead of the host's wait for them - fills whose sizes depend on n alone
// run on the device while the host takes the six numbers over (they used to sit in the chain of dependent launches after it)
static int make_grid(const double* d_coords, long long n, int dim, double target_per_cell, double min_h,
                     GridParams* gp, hipStream_t st, const std::function<int()>* under_wait = nullptr) {
    auto job = std::make_unique<BboxJob>();
    FDX_TRY(bbox_begin(d_coords, n, dim, st, job.get()));
    if (under_wait && *under_wait) FDX_TRY((*under_wait)());
    FDX_HIP(hipEventSynchronize(job->ev));
    double mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
    for (int a = 0; a < dim; ++a) {
        mn[a] = job->host[a];
        mx[a] = job->host[3 + a];
        if (!(std::isfinite(mn[a]) && std::isfinite(mx[a])))
            return fail(FDX_ERR_INVALID, "graph: coordinates contain NaN or infinity");
    }
    job.reset();
    // cell edge from the occupied volume: ~target_per_cell points per cell over the axes with non-zero extent
    double vol = 1.0;
    int eff = 0;
    for (int a = 0; a < dim; ++a)
        if (mx[a] > mn[a]) { vol *= (mx[a] - mn[a]); ++eff; }
    double h = 1.0;
    if (eff > 0) h = std::pow(vol * target_per_cell / (double)std::max<long long>(n, 1), 1.0 / eff);
    if (min_h > 0.0) h = std::max(h, min_h);
    if (!(h > 0.0) || !std::isfinite(h)) h = 1.0;
    for (int attempt = 0; attempt < 64; ++attempt) {
        double cells = 1.0;
        for (int a = 0; a < 3; ++a) {
            gp->mn[a] = (a < dim) ? mn[a] : 0.0;
            gp->h[a] = h;
            gp->inv_h[a] = 1.0 / h;
            double nca = (a < dim && mx[a] > mn[a]) ? std::floor((mx[a] - mn[a]) / h) + 1.0 : 1.0;
            cells *= nca;
            gp->nc[a] = (int)std::min(nca, 2.0e9);
        }
        const int max_axis = std::max(gp->nc[0], std::max(gp->nc[1], gp->nc[2]));
        const bool morton_ok = (dim < 3) || max_axis < (1 << 21);   // 21 bits per axis in the 3-D Morton key
        if (cells <= std::max(4.0 * (double)n, 4096.0) && cells < 2.0e9 && morton_ok) break;
        h *= 1.5;   // very elongated / clustered inputs: coarsen until the table is O(N)
    }
    gp->dim = dim;
    // slowest-varying axis = most cells
    int order[3] = {0, 1, 2};
    std::sort(order, order + 3, [&](int a, int b) { return gp->nc[a] < gp->nc[b]; });
    int stride = 1;
    for (int t = 0; t < 3; ++t) { gp->stride[order[t]] = stride; stride *= gp->nc[order[t]]; }
    return 0;
}

// shard_lo < shard_hi: a spot shard's binning - the ranking pass lays out only the cells the shard's build looks at
// (cell_need_kernel; counting path only: the sorting path lays out everything)
int bin_points(const double* d_coords, long long n, int dim, double target_per_cell, double min_h,
                      BinnedPoints* b, hipStream_t st, long long shard_lo, long long shard_hi, int shard_R,
               const std::function<int()>* extra_under_wait) {
    b->n = n;
    FDX_TRY(b->sc.alloc((size_t)n * 3 * sizeof(double)));
    const std::function<int()> under_wait = [&]() -> int {
        // the coordinate planes past `dim` read as zero (8 MB at a million 2-D points: 16 us that used to sit between place and rank)
        if (dim < 3) FDX_HIP(hipMemsetAsync(b->sc.as<double>() + (size_t)dim * n, 0, (size_t)(3 - dim) * n * sizeof(double), st));
        if (extra_under_wait && *extra_under_wait) FDX_TRY((*extra_under_wait)());
        return 0;
    };
    FDX_TRY(make_grid(d_coords, n, dim, target_per_cell, min_h, &b->gp, st, &under_wait));
    trace_host("bin: make_grid (bbox kernel + read-back)");
    b->n_cells = b->gp.nc[0] * b->gp.nc[1] * b->gp.nc[2];
    DevBuf& keys = b->keys;
    DevBuf& vals = b->vals;
    DevBuf& skeys = b->skeys;
    DevBuf& tmp = b->sort_tmp;
    FDX_TRY(keys.alloc((size_t)n * 8));
    FDX_TRY(vals.alloc((size_t)n * 4));
    FDX_TRY(skeys.alloc((size_t)n * 8));
    FDX_TRY(b->perm.alloc((size_t)n * 4));
    FDX_TRY(b->rank.alloc((size_t)n * 4));
    if (dim <= 2) FDX_TRY(b->sc2.alloc((size_t)n * 2 * sizeof(double)));
    trace_host("bin: allocations");
    const int nb = ceil_div(n, 256);
    typedef unsigned long long u64;
    const int max_axis = std::max(b->gp.nc[0], std::max(b->gp.nc[1], b->gp.nc[2]));
    int axis_bits = 1;
    while ((1LL << axis_bits) < (long long)max_axis) ++axis_bits;
    const int bits = std::min(64, axis_bits * dim);      // significant bits of the Morton key
    const bool counting = bits <= 22 && (1LL << bits) <= 8 * n + 1024 && !fdx::env("FDX_GRAPH_SORT");
    const bool shard_need = counting && shard_hi > shard_lo && (shard_lo > 0 || shard_hi < n) && shard_R > 0;
    {
        // the cell table, the key counters and (spot shards) the need flags start as zero: one block, one fill
        auto up16 = [](size_t v) { return (v + 15) / 16 * 16; };
        const size_t cells_b = up16((size_t)b->n_cells * 4);
        const size_t count_b = counting ? up16((size_t)((1LL << bits) + 1) * 4) : 0;
        const size_t need_b = shard_need ? up16((size_t)(1LL << bits) * 2) : 0;
        FDX_TRY(b->cstart.alloc(2 * cells_b + count_b + need_b));
        FDX_HIP(hipMemsetAsync(b->cstart.p, 0, 2 * cells_b + count_b + need_b, st));
        b->cend_p = reinterpret_cast<int*>(static_cast<char*>(b->cstart.p) + cells_b);
        b->count_p = counting ? reinterpret_cast<int*>(static_cast<char*>(b->cstart.p) + 2 * cells_b) : nullptr;
        b->need_p = shard_need ? reinterpret_cast<unsigned char*>(static_cast<char*>(b->cstart.p) + 2 * cells_b + count_b) : nullptr;
    }
    trace_host("bin: 1 memset");
    // Up to 4M keys (and no more than 8 per point) the order comes from counting instead of sorting: 6 launches instead of
    // the ~30 of rocprim's sort at this size (1M points: 0.42 -> 0.1 ms); FDX_GRAPH_SORT=1 forces the sort.
    if (counting) {
        const long long bins = 1LL << bits;
        b->bins = bins;
        FDX_TRY(tmp.alloc((size_t)n * 4));                        // members in arrival order (keys: 32-bit keys, vals: arrival numbers)
        FDX_TRY(b->start.alloc((size_t)(bins + 1) * 4));
        trace_host("bin: start alloc");
        hipLaunchKernelGGL(cell_count_kernel, dim3(nb), dim3(256), 0, st, d_coords, n, b->gp, keys.as<unsigned>(), vals.as<int>(),
                           b->count_p);
        FDX_CHECK_LAUNCH();
        trace_host("bin: count kernel");
        FDX_TRY(exclusive_scan_int(b->count_p, b->start.as<int>(), bins + 1, st, b->scan_tmp));
        trace_host("bin: scan");
        hipLaunchKernelGGL(cell_place_kernel, dim3(nb), dim3(256), 0, st, keys.as<unsigned>(), vals.as<int>(), b->start.as<int>(), n,
                           tmp.as<int>());
        FDX_CHECK_LAUNCH();
        const unsigned char* need = nullptr;
        if (shard_need) {
            unsigned char* n1 = b->need_p;
            unsigned char* n2 = n1 + bins;
            hipLaunchKernelGGL(cell_need_kernel<0>, dim3(ceil_div(bins, 256)), dim3(256), 0, st, b->start.as<int>(), bins, b->gp, shard_lo,
                               shard_hi, shard_R, (const unsigned char*)nullptr, n1);
            hipLaunchKernelGGL(cell_need_kernel<1>, dim3(ceil_div(bins, 256)), dim3(256), 0, st, b->start.as<int>(), bins, b->gp, shard_lo,
                               shard_hi, shard_R, (const unsigned char*)n1, n2);
            FDX_CHECK_LAUNCH();
            need = n2;
        }
        hipLaunchKernelGGL(cell_rank_kernel, dim3(nb), dim3(256), 0, st, d_coords, keys.as<unsigned>(), b->start.as<int>(),
                           tmp.as<int>(), n, dim, b->perm.as<int>(), b->rank.as<int>(), b->sc.as<double>(), b->sc2.as<double2>(), need);
        FDX_CHECK_LAUNCH();
        hipLaunchKernelGGL(cell_table_kernel, dim3(ceil_div(bins, 256)), dim3(256), 0, st, b->start.as<int>(), bins, b->gp,
                           b->cstart.as<int>(), b->cend_p);
        FDX_CHECK_LAUNCH();
        trace_host("bin: place/rank/table kernels");
        return 0;                        // no sync: the temporaries live in *b, whose owners synchronise before dropping it
    } else {
        hipLaunchKernelGGL(cell_key_kernel, dim3(nb), dim3(256), 0, st, d_coords, n, b->gp, keys.as<u64>(), vals.as<int>());
        FDX_CHECK_LAUNCH();
        FDX_TRY(with_temp(tmp, [&](void* t, size_t& bytes) {
            return rocprim::radix_sort_pairs(t, bytes, keys.as<u64>(), skeys.as<u64>(), vals.as<int>(), b->perm.as<int>(), (size_t)n, 0,
                                             (unsigned)bits, st);
        }));
        hipLaunchKernelGGL(gather_sorted_kernel, dim3(nb), dim3(256), 0, st, d_coords, b->perm.as<int>(), n, dim, b->sc.as<double>(), b->rank.as<int>(), b->sc2.as<double2>());
        FDX_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(cell_range_kernel, dim3(nb), dim3(256), 0, st, skeys.as<u64>(), b->sc.as<double>(), n, b->gp,
                       b->cstart.as<int>(), b->cend_p);
    FDX_CHECK_LAUNCH();
    trace_host("bin: place/rank/range kernels");
    return 0;                            // no sync: the temporaries live in *b, whose owners synchronise before dropping it
}

}  // namespace fdx
