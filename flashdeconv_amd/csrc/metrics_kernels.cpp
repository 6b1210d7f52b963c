// Deconvolution accuracy metrics on the device (flashdeconv/utils/metrics.py:12-266): RMSE, MAE, Pearson, Spearman, per-spot
// Jensen-Shannon divergence and rare-cell detection counts of a (n, K) row-major pred / true pair, float32 or float64, with
// float64 arithmetic throughout.  Not on the fit path: the reference scores a fit on the host, where two scipy.stats.spearmanr
// paths over the n*K values cost seconds; here the proportions of fit(output="torch") never leave HBM.
//
// Moments.  mx_col_stats reads both matrices once (block = a contiguous chunk of rows; thread = one column of one row lane, so
// a block's lanes read lanes*K contiguous elements per step) and keeps per-column sums of squared / absolute errors, sums,
// min / max, NaN flags and the rare-cell counts in registers.  A second pass (mx_centred) subtracts the means the first pass's
// final kernel left in device memory and sums the centred products Pearson needs, per column and about the overall means.
// Every block writes its partials to a slab; one wave per (column, field) reduces the slab in a fixed order (no float atomics), so two calls
// on the same inputs give the same bits.
//
// Spearman.  Ranks come from sorts: a rocPRIM radix sort of the n*K values (payload: the flat row-major index) gives the overall
// order; a second, stable radix sort of that order by column index (ceil(log2 K) bits, one pass) gives every column's order
// without a type-major copy or a segmented sort (one workgroup per segment would sort each million-entry column alone).
// Average ranks of tie runs: an inclusive max-scan of "i if i starts a run" gives each position its run start; the last position
// of a run writes start + end + 2 (twice the 1-based average rank) at the run start, and every position reads it back from
// there.  Proportions are mostly exact zeros, so one run can hold most of the array: nothing walks a run element by element.
// Spearman is then Pearson of the twice-ranks through mx_centred with the exact mean (segment length + 1).
//
// Workspace comes from the library's caching pool (pool.cpp) and goes back to it when the call returns; fdx_trim() hands it to
// the driver.  At 1M x 30 float64 the Spearman path holds about 1.2 GB at its peak (plus rocPRIM's sort buffers).
#include "fdx_internal.h"
#include "fdx_kernels.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <cmath>
#include <limits>
#include <vector>

namespace fdx {

namespace {

constexpr int MX_THREADS = 256;
constexpr int MX_MAX_BLOCKS = 1024;           // row chunks per column group: the slab's depth
constexpr int F1 = FDX_MX_JSD_SUM + 1;         // first-pass fields per column (include/fdx.h; the JSD sum: overall row only)
constexpr int MX_JSD_TILE = 2048;      // elements per matrix of a staged JSD tile (2 x 16 KB of LDS)
constexpr int F2 = 6;                          // centred sums: 3 about the column means, 3 about the overall means

// Column geometry shared by both passes: CW columns per block (all of them up to 256), lanes = row lanes per block.
struct ColGeom {
    int cw, lanes, gy, nbx;
    long long chunk;
};

ColGeom col_geom(long long n, int K) {
    ColGeom g;
    g.cw = K < MX_THREADS ? K : MX_THREADS;
    g.lanes = MX_THREADS / g.cw;
    g.gy = ceil_div(K, g.cw);
    long long want = (n + (long long)g.lanes * 32 - 1) / ((long long)g.lanes * 32);   // >= 32 rows per lane
    g.nbx = (int)(want < 1 ? 1 : want > MX_MAX_BLOCKS ? MX_MAX_BLOCKS : want);
    g.chunk = (n + g.nbx - 1) / g.nbx;
    return g;
}

__device__ __forceinline__ double clip01(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }   // NaN stays

// Pass 1: per column sse, sae, sum p, sum t, min/max p, min/max t, NaN flags, rare-cell counts (metrics.py:36, 63, 221-235).
template <typename T>
__global__ __launch_bounds__(MX_THREADS) void mx_col_stats(const T* __restrict__ P, long long ldp, const T* __restrict__ Q,
                                                           long long ldq, long long n, int K, int cw, int lanes, long long chunk,
                                                           double thr, double* __restrict__ slab) {
    const int lane = threadIdx.x / cw, c = blockIdx.y * cw + threadIdx.x % cw;
    const bool active = lane < lanes && c < K;
    double sse = 0, sae = 0, sp = 0, st = 0, nanp = 0, nant = 0;
    double mnp = INFINITY, mxp = -INFINITY, mnt = INFINITY, mxt = -INFINITY;
    long long nrare = 0, tp = 0, fp = 0, fn = 0;
    const double half = thr * 0.5;
    if (active) {
        const long long r0 = (long long)blockIdx.x * chunk;
        const long long r1 = r0 + chunk < n ? r0 + chunk : n;
        for (long long r = r0 + lane; r < r1; r += lanes) {
            const double p = (double)P[r * ldp + c], t = (double)Q[r * ldq + c];
            const double d = p - t;
            sse += d * d;
            sae += fabs(d);
            sp += p;
            st += t;
            mnp = fmin(mnp, p); mxp = fmax(mxp, p);
            mnt = fmin(mnt, t); mxt = fmax(mxt, t);
            if (p != p) nanp = 1;
            if (t != t) nant = 1;
            const bool rare = t > 0.0 && t < thr, present = p > half;
            nrare += rare;
            tp += present && rare;
            fp += present && !rare && t == 0.0;
            fn += !present && rare;
        }
    }
    __shared__ double red[MX_THREADS];
    const double v[F1] = {sse, sae, sp, st, mnp, mxp, mnt, mxt, nanp, nant, (double)nrare, (double)tp, (double)fp, (double)fn, 0.0};
    double* out = slab + ((size_t)blockIdx.x * K + (size_t)(c < K ? c : 0)) * F1;
#pragma unroll
    for (int f = 0; f < F1; ++f) {
        red[threadIdx.x] = v[f];
        __syncthreads();
        if (active && lane == 0) {                 // lanes in a fixed order
            double a = red[threadIdx.x];
            for (int l = 1; l < lanes; ++l) {
                const double b = red[l * cw + threadIdx.x];
                a = (f == FDX_MX_MIN_P || f == FDX_MX_MIN_T) ? fmin(a, b)
                  : (f == FDX_MX_MAX_P || f == FDX_MX_MAX_T || f == FDX_MX_NAN_P || f == FDX_MX_NAN_T) ? fmax(a, b) : a + b;
            }
            out[f] = a;
        }
        __syncthreads();
    }
}

// Pass 2: centred sums about the column means and about the overall means, mu = [p means (K), p overall, t means (K), t overall].
template <typename T>
__global__ __launch_bounds__(MX_THREADS) void mx_centred(const T* __restrict__ P, long long ldp, const T* __restrict__ Q,
                                                         long long ldq, long long n, int K, int cw, int lanes, long long chunk,
                                                         const double* __restrict__ mu, double* __restrict__ slab) {
    const int lane = threadIdx.x / cw, c = blockIdx.y * cw + threadIdx.x % cw;
    const bool active = lane < lanes && c < K;
    double cpt = 0, cpp = 0, ctt = 0, apt = 0, app = 0, att = 0;
    if (active) {
        const double mp = mu[c], mt = mu[K + 1 + c], ap = mu[K], at = mu[2 * K + 1];
        const long long r0 = (long long)blockIdx.x * chunk;
        const long long r1 = r0 + chunk < n ? r0 + chunk : n;
        for (long long r = r0 + lane; r < r1; r += lanes) {
            const double p = (double)P[r * ldp + c], t = (double)Q[r * ldq + c];
            const double dp = p - mp, dt = t - mt, ep = p - ap, et = t - at;
            cpt += dp * dt; cpp += dp * dp; ctt += dt * dt;
            apt += ep * et; app += ep * ep; att += et * et;
        }
    }
    __shared__ double red[MX_THREADS];
    const double v[F2] = {cpt, cpp, ctt, apt, app, att};
    double* out = slab + ((size_t)blockIdx.x * K + (size_t)(c < K ? c : 0)) * F2;
#pragma unroll
    for (int f = 0; f < F2; ++f) {
        red[threadIdx.x] = v[f];
        __syncthreads();
        if (active && lane == 0) {
            double a = red[threadIdx.x];
            for (int l = 1; l < lanes; ++l) a += red[l * cw + threadIdx.x];
            out[f] = a;
        }
        __syncthreads();
    }
}

__device__ __forceinline__ double mx_jsd_row(const double* p, const double* q, int K, double lo, double hi) {
    double sp = 0.0, st = 0.0;
    for (int c = 0; c < K; ++c) {
        sp += clip01(p[c], lo, hi);
        st += clip01(q[c], lo, hi);
    }
    double klp = 0.0, klt = 0.0;
    for (int c = 0; c < K; ++c) {
        const double a = clip01(p[c], lo, hi) / sp, b = clip01(q[c], lo, hi) / st;
        const double m = 0.5 * (a + b);
        klp += a * log(a / m);
        klt += b * log(b / m);
    }
    return 0.5 * (klp + klt);
}

__device__ __forceinline__ void mx_block_sum_to(double acc, double* __restrict__ out) {
    __shared__ double red[MX_THREADS];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = MX_THREADS / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = red[0];
}

// Per-spot JSD (metrics.py:141-157), K <= MX_JSD_TILE: a tile of R rows of both matrices is staged in LDS as float64 with
// coalesced loads (the block reads R * K contiguous elements of each), then thread r < R computes spot r of the tile.  Tiles are
// grid-strided; the block's sum of its spots (a thread's spots in order, then a fixed tree) goes to jslab[block].
template <typename T>
__global__ __launch_bounds__(MX_THREADS) void mx_jsd_tiled(const T* __restrict__ P, long long ldp, const T* __restrict__ Q,
                                                           long long ldq, long long n, int K, int R, double eps,
                                                           double* __restrict__ jsd, double* __restrict__ jslab) {
    extern __shared__ double tile[];
    double* tp = tile;
    double* tq = tile + (size_t)R * K;
    double acc = 0.0;
    const long long ntiles = (n + R - 1) / R;
    for (long long b = blockIdx.x; b < ntiles; b += gridDim.x) {
        const long long r0 = b * R;
        const int rows = (int)(n - r0 < R ? n - r0 : R);
        const int cnt = rows * K;
        for (int e = threadIdx.x; e < cnt; e += MX_THREADS) {
            const int r = e / K, c = e - r * K;
            tp[e] = (double)P[(r0 + r) * ldp + c];
            tq[e] = (double)Q[(r0 + r) * ldq + c];
        }
        __syncthreads();
        if ((int)threadIdx.x < rows) {
            const double j = mx_jsd_row(tp + (size_t)threadIdx.x * K, tq + (size_t)threadIdx.x * K, K, eps, 1.0 - eps);
            jsd[r0 + threadIdx.x] = j;
            acc += j;
        }
        __syncthreads();
    }
    mx_block_sum_to(acc, jslab + blockIdx.x);
}

// The same for wide rows (K > MX_JSD_TILE): thread = spot, read from global memory.
template <typename T>
__global__ __launch_bounds__(MX_THREADS) void mx_jsd(const T* __restrict__ P, long long ldp, const T* __restrict__ Q, long long ldq,
                                                     long long n, int K, double eps, double* __restrict__ jsd,
                                                     double* __restrict__ jslab) {
    double acc = 0.0;
    for (long long r = (long long)blockIdx.x * MX_THREADS + threadIdx.x; r < n; r += (long long)gridDim.x * MX_THREADS) {
        const T* p = P + r * ldp;
        const T* q = Q + r * ldq;
        const double lo = eps, hi = 1.0 - eps;
        double sp = 0.0, st = 0.0;
        for (int c = 0; c < K; ++c) {
            sp += clip01((double)p[c], lo, hi);
            st += clip01((double)q[c], lo, hi);
        }
        double klp = 0.0, klt = 0.0;
        for (int c = 0; c < K; ++c) {
            const double a = clip01((double)p[c], lo, hi) / sp, b = clip01((double)q[c], lo, hi) / st;
            const double m = 0.5 * (a + b);
            klp += a * log(a / m);
            klt += b * log(b / m);
        }
        const double j = 0.5 * (klp + klt);
        jsd[r] = j;
        acc += j;
    }
    mx_block_sum_to(acc, jslab + blockIdx.x);
}

__device__ __forceinline__ bool mx_is_min(int f) { return f == FDX_MX_MIN_P || f == FDX_MX_MIN_T; }
__device__ __forceinline__ bool mx_is_max(int f) {
    return f == FDX_MX_MAX_P || f == FDX_MX_MAX_T || f == FDX_MX_NAN_P || f == FDX_MX_NAN_T;
}

// slab (nbx, K, F) -> out (K, F): one wave per (column, field); lane l combines blocks l, l + 64, ... in order, then a fixed
// tree over the lanes.  F == F1: the first pass's fields (min / max / flags / sums), else sums.
template <int F>
__global__ __launch_bounds__(64) void mx_slab_reduce(const double* __restrict__ slab, int nbx, int K, double* __restrict__ out) {
    const int it = blockIdx.x, c = it / F, f = it % F;
    const bool mn = F == F1 && mx_is_min(f), mx = F == F1 && mx_is_max(f);
    double a = mn ? INFINITY : mx ? -INFINITY : 0.0;
    for (int b = threadIdx.x; b < nbx; b += 64) {
        const double v = slab[((size_t)b * K + c) * F + f];
        a = mn ? fmin(a, v) : mx ? fmax(a, v) : a + v;
    }
    __shared__ double red[64];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int s = 32; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const double v = red[threadIdx.x + s];
            red[threadIdx.x] = mn ? fmin(red[threadIdx.x], v) : mx ? fmax(red[threadIdx.x], v) : red[threadIdx.x] + v;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[it] = red[0];
}

// One workgroup, after mx_slab_reduce<F1> filled stats rows 0..K-1: row K = the columns combined in order, the JSD sum (jslab,
// nbj entries) into row K's FDX_MX_JSD_SUM, and the means pass 2 reads (mu).
__global__ __launch_bounds__(MX_THREADS) void mx_stats_final(int K, long long n, const double* __restrict__ jslab, int nbj,
                                                             double* __restrict__ stats, double* __restrict__ mu) {
    if (threadIdx.x < F1) {
        const int f = threadIdx.x;
        double a = stats[f];
        for (int c = 1; c < K; ++c) {
            const double v = stats[(size_t)c * F1 + f];
            a = mx_is_min(f) ? fmin(a, v) : mx_is_max(f) ? fmax(a, v) : a + v;
        }
        if (f == FDX_MX_JSD_SUM) {
            a = 0.0;
            for (int b = 0; b < nbj; ++b) a += jslab[b];
        }
        stats[(size_t)K * F1 + f] = a;
    }
    __syncthreads();
    for (int c = threadIdx.x; c <= K; c += MX_THREADS) {
        const double cnt = c < K ? (double)n : (double)n * (double)K;
        mu[c] = stats[(size_t)c * F1 + FDX_MX_SUM_P] / cnt;
        mu[K + 1 + c] = stats[(size_t)c * F1 + FDX_MX_SUM_T] / cnt;
    }
}

// tmp (K, F2) from mx_slab_reduce<F2> -> out rows 0..K-1: the column-centred sums; row K: the overall-centred sums over all columns.
__global__ __launch_bounds__(MX_THREADS) void mx_centred_final(int K, const double* __restrict__ tmp, double* __restrict__ out) {
    for (int c = threadIdx.x; c < K; c += MX_THREADS)
        for (int f = 0; f < 3; ++f) out[(size_t)c * 3 + f] = tmp[(size_t)c * F2 + f];
    if (threadIdx.x < 3) {
        double a = 0.0;
        for (int c = 0; c < K; ++c) a += tmp[(size_t)c * F2 + 3 + threadIdx.x];
        out[(size_t)K * 3 + threadIdx.x] = a;
    }
}

// mu of the twice-ranks: every column (n + 1), overall (m + 1)
__global__ void mx_fill_mu(double* mu, int K, double col, double all) {
    for (int c = threadIdx.x; c <= K; c += blockDim.x) mu[c] = mu[K + 1 + c] = c < K ? col : all;
}

// ---- ranks ----------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void mx_compact(const T* __restrict__ X, long long ld, long long n, int K, T* __restrict__ out) {
    const long long j = (long long)blockIdx.x * MX_THREADS + threadIdx.x;
    if (j < n * K) out[j] = X[(j / K) * ld + j % K];
}

// i if position i starts a tie run (or a segment of `seg` positions), else 0: the max-scan input
template <typename T>
struct RunHead {
    const T* key;
    int seg;
    __device__ int operator()(int i) const { return (i % seg == 0 || !(key[i] == key[i - 1])) ? i : 0; }
};

// last position of a run: avg[start] = twice the 1-based average rank of the run inside its segment
template <typename T>
__global__ void mx_run_tail(const T* __restrict__ key, const int* __restrict__ start, int m, int seg, unsigned* __restrict__ avg) {
    const int i = blockIdx.x * MX_THREADS + threadIdx.x;
    if (i >= m) return;
    if ((i + 1) % seg == 0 || !(key[i + 1] == key[i])) {
        const int s0 = i - i % seg, s = start[i];
        avg[s] = (unsigned)(s - s0) + (unsigned)(i - s0) + 2u;
    }
}

__global__ void mx_rank_scatter(const int* __restrict__ idx, const int* __restrict__ start, const unsigned* __restrict__ avg, int m,
                                unsigned* __restrict__ rank) {
    const int i = blockIdx.x * MX_THREADS + threadIdx.x;
    if (i < m) rank[idx[i]] = avg[start[i]];
}

__global__ void mx_col_of(const int* __restrict__ idx, int m, int K, int* __restrict__ col) {
    const int i = blockIdx.x * MX_THREADS + threadIdx.x;
    if (i < m) col[i] = idx[i] % K;
}

template <typename T>
__global__ void mx_gather(const T* __restrict__ key, const int* __restrict__ idx, int m, T* __restrict__ out) {
    const int i = blockIdx.x * MX_THREADS + threadIdx.x;
    if (i < m) out[i] = key[idx[i]];
}

double corr_from_sums(double cpt, double cpp, double ctt, double N) {
    // np.corrcoef (cov with ddof 1, then divided by both standard deviations, clipped) of the centred sums
    const double den = N - 1.0;
    double r = (cpt / den) / std::sqrt(cpp / den) / std::sqrt(ctt / den);
    if (r > 1.0) r = 1.0;
    if (r < -1.0) r = -1.0;
    return r;
}

struct Work {
    const void* P; const void* Q;
    int dtype;
    long long ldp, ldq, n;
    int K;
    hipStream_t st;
};

// pass 1 + pass 2 (+ JSD when jsd_dev): stats (K+1, F1) and centred (K+1, 3) into res_dev
template <typename T>
int run_moments(const Work& w, double thr, double eps, double* jsd_dev, double* stats_dev, double* cent_dev) {
    const T* P = (const T*)w.P;
    const T* Q = (const T*)w.Q;
    const ColGeom g = col_geom(w.n, w.K);
    const bool tiled = w.K <= MX_JSD_TILE;
    const int R = tiled ? (MX_JSD_TILE / w.K < MX_THREADS ? MX_JSD_TILE / w.K : MX_THREADS) : MX_THREADS;   // spots per tile / block
    const long long units = (w.n + R - 1) / R;
    const int nbj = jsd_dev ? (int)(units < MX_MAX_BLOCKS ? units : MX_MAX_BLOCKS) : 0;
    DevBuf slab, jslab, mu, tmp;
    FDX_TRY(slab.alloc((size_t)g.nbx * w.K * F1 * sizeof(double)));
    FDX_TRY(jslab.alloc((size_t)(nbj > 0 ? nbj : 1) * sizeof(double)));
    FDX_TRY(mu.alloc((size_t)(2 * w.K + 2) * sizeof(double)));
    FDX_TRY(tmp.alloc((size_t)w.K * F2 * sizeof(double)));
    hipLaunchKernelGGL(mx_col_stats<T>, dim3(g.nbx, g.gy), dim3(MX_THREADS), 0, w.st, P, w.ldp, Q, w.ldq, w.n, w.K, g.cw, g.lanes,
                       g.chunk, thr, slab.as<double>());
    FDX_CHECK_LAUNCH();
    if (nbj > 0) {
        if (tiled)
            hipLaunchKernelGGL(mx_jsd_tiled<T>, dim3(nbj), dim3(MX_THREADS), (size_t)2 * R * w.K * sizeof(double), w.st, P, w.ldp, Q,
                               w.ldq, w.n, w.K, R, eps, jsd_dev, jslab.as<double>());
        else
            hipLaunchKernelGGL(mx_jsd<T>, dim3(nbj), dim3(MX_THREADS), 0, w.st, P, w.ldp, Q, w.ldq, w.n, w.K, eps, jsd_dev,
                               jslab.as<double>());
        FDX_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(mx_slab_reduce<F1>, dim3(w.K * F1), dim3(64), 0, w.st, slab.as<double>(), g.nbx, w.K, stats_dev);
    FDX_CHECK_LAUNCH();
    hipLaunchKernelGGL(mx_stats_final, dim3(1), dim3(MX_THREADS), 0, w.st, w.K, w.n, jslab.as<double>(), nbj, stats_dev,
                       mu.as<double>());
    FDX_CHECK_LAUNCH();
    DevBuf slab2;
    FDX_TRY(slab2.alloc((size_t)g.nbx * w.K * F2 * sizeof(double)));
    hipLaunchKernelGGL(mx_centred<T>, dim3(g.nbx, g.gy), dim3(MX_THREADS), 0, w.st, P, w.ldp, Q, w.ldq, w.n, w.K, g.cw, g.lanes,
                       g.chunk, mu.as<double>(), slab2.as<double>());
    FDX_CHECK_LAUNCH();
    hipLaunchKernelGGL(mx_slab_reduce<F2>, dim3(w.K * F2), dim3(64), 0, w.st, slab2.as<double>(), g.nbx, w.K, tmp.as<double>());
    FDX_CHECK_LAUNCH();
    hipLaunchKernelGGL(mx_centred_final, dim3(1), dim3(MX_THREADS), 0, w.st, w.K, tmp.as<double>(), cent_dev);
    FDX_CHECK_LAUNCH();
    return 0;
}

template <typename T>
int run_scan_ranks(const T* skey, const int* sidx, int m, int seg, DevBuf& start, DevBuf& avg, DevBuf& scan_tmp,
                   unsigned* rank, hipStream_t st) {
    auto heads = rocprim::make_transform_iterator(rocprim::make_counting_iterator(0), RunHead<T>{skey, seg});
    size_t bytes = 0;
    FDX_HIP(rocprim::inclusive_scan(nullptr, bytes, heads, start.as<int>(), (size_t)m, rocprim::maximum<int>(), st));
    if (scan_tmp.bytes < bytes) FDX_TRY(scan_tmp.alloc(bytes));
    FDX_HIP(rocprim::inclusive_scan(scan_tmp.p, bytes, heads, start.as<int>(), (size_t)m, rocprim::maximum<int>(), st));
    const int nb = ceil_div(m, MX_THREADS);
    hipLaunchKernelGGL(mx_run_tail<T>, dim3(nb), dim3(MX_THREADS), 0, st, skey, start.as<int>(), m, seg, avg.as<unsigned>());
    FDX_CHECK_LAUNCH();
    hipLaunchKernelGGL(mx_rank_scatter, dim3(nb), dim3(MX_THREADS), 0, st, sidx, start.as<int>(), avg.as<unsigned>(), m, rank);
    FDX_CHECK_LAUNCH();
    return 0;
}

// twice-ranks of one matrix: overall (rank_all, may be null) and per column (rank_col, may be null), both row-major (n, K)
template <typename T>
int rank_matrix(const T* X, long long ld, long long n, int K, unsigned* rank_all, unsigned* rank_col, hipStream_t st) {
    const int m = (int)(n * K);
    const int nb = ceil_div(m, MX_THREADS);
    DevBuf compact, skey, sidx, start, avg, tmp;
    const T* key = X;
    if (ld != K) {
        FDX_TRY(compact.alloc((size_t)m * sizeof(T)));
        hipLaunchKernelGGL(mx_compact<T>, dim3(nb), dim3(MX_THREADS), 0, st, X, (long long)ld, n, K, compact.as<T>());
        FDX_CHECK_LAUNCH();
        key = compact.as<T>();
    }
    FDX_TRY(skey.alloc((size_t)m * sizeof(T)));
    FDX_TRY(sidx.alloc((size_t)m * sizeof(int)));
    FDX_TRY(start.alloc((size_t)m * sizeof(int)));
    FDX_TRY(avg.alloc((size_t)m * sizeof(unsigned)));
    size_t bytes = 0;
    auto iota = rocprim::make_counting_iterator(0);
    FDX_HIP(rocprim::radix_sort_pairs(nullptr, bytes, key, skey.as<T>(), iota, sidx.as<int>(), (size_t)m, 0, 8 * sizeof(T), st));
    FDX_TRY(tmp.alloc(bytes));
    FDX_HIP(rocprim::radix_sort_pairs(tmp.p, bytes, key, skey.as<T>(), iota, sidx.as<int>(), (size_t)m, 0, 8 * sizeof(T), st));
    if (rank_all) FDX_TRY(run_scan_ranks<T>(skey.as<T>(), sidx.as<int>(), m, m, start, avg, tmp, rank_all, st));
    if (rank_col) {
        // a stable sort of the value order by column: each column's values in ascending order, columns one after the other
        int bits = 1;
        while ((1 << bits) < K) ++bits;
        DevBuf col, col2, sidx2;
        FDX_TRY(col.alloc((size_t)m * sizeof(int)));
        FDX_TRY(col2.alloc((size_t)m * sizeof(int)));
        FDX_TRY(sidx2.alloc((size_t)m * sizeof(int)));
        hipLaunchKernelGGL(mx_col_of, dim3(nb), dim3(MX_THREADS), 0, st, sidx.as<int>(), m, K, col.as<int>());
        FDX_CHECK_LAUNCH();
        size_t b2 = 0;
        FDX_HIP(rocprim::radix_sort_pairs(nullptr, b2, col.as<int>(), col2.as<int>(), sidx.as<int>(), sidx2.as<int>(), (size_t)m, 0,
                                          (unsigned)bits, st));
        if (tmp.bytes < b2) FDX_TRY(tmp.alloc(b2));
        FDX_HIP(rocprim::radix_sort_pairs(tmp.p, b2, col.as<int>(), col2.as<int>(), sidx.as<int>(), sidx2.as<int>(), (size_t)m, 0,
                                          (unsigned)bits, st));
        hipLaunchKernelGGL(mx_gather<T>, dim3(nb), dim3(MX_THREADS), 0, st, key, sidx2.as<int>(), m, skey.as<T>());
        FDX_CHECK_LAUNCH();
        FDX_TRY(run_scan_ranks<T>(skey.as<T>(), sidx2.as<int>(), m, (int)n, start, avg, tmp, rank_col, st));
    }
    return 0;
}

// Spearman sums: per-column rank sums into rows 0..K-1 of rsum_dev (when per_type), overall into row K (when overall)
template <typename T>
int run_spearman(const Work& w, int flags, double* rsum_dev) {
    const long long m = w.n * w.K;
    const bool all = flags & FDX_SPEARMAN_OVERALL, per = flags & FDX_SPEARMAN_PER_TYPE;
    DevBuf ra_p, ra_t, rc_p, rc_t, mu, slab, tmp, out;
    if (all) { FDX_TRY(ra_p.alloc((size_t)m * 4)); FDX_TRY(ra_t.alloc((size_t)m * 4)); }
    if (per) { FDX_TRY(rc_p.alloc((size_t)m * 4)); FDX_TRY(rc_t.alloc((size_t)m * 4)); }
    FDX_TRY(rank_matrix<T>((const T*)w.P, w.ldp, w.n, w.K, ra_p.as<unsigned>(), rc_p.as<unsigned>(), w.st));
    FDX_TRY(rank_matrix<T>((const T*)w.Q, w.ldq, w.n, w.K, ra_t.as<unsigned>(), rc_t.as<unsigned>(), w.st));
    const ColGeom g = col_geom(w.n, w.K);
    FDX_TRY(mu.alloc((size_t)(2 * w.K + 2) * sizeof(double)));
    FDX_TRY(slab.alloc((size_t)g.nbx * w.K * F2 * sizeof(double)));
    FDX_TRY(tmp.alloc((size_t)w.K * F2 * sizeof(double)));
    FDX_TRY(out.alloc((size_t)(w.K + 1) * 3 * sizeof(double)));
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 0 ? !per : !all) continue;
        const unsigned* a = (pass == 0 ? rc_p : ra_p).as<unsigned>();
        const unsigned* b = (pass == 0 ? rc_t : ra_t).as<unsigned>();
        hipLaunchKernelGGL(mx_fill_mu, dim3(1), dim3(MX_THREADS), 0, w.st, mu.as<double>(), w.K, (double)w.n + 1.0, (double)m + 1.0);
        FDX_CHECK_LAUNCH();
        hipLaunchKernelGGL(mx_centred<unsigned>, dim3(g.nbx, g.gy), dim3(MX_THREADS), 0, w.st, a, (long long)w.K, b, (long long)w.K,
                           w.n, w.K, g.cw, g.lanes, g.chunk, mu.as<double>(), slab.as<double>());
        FDX_CHECK_LAUNCH();
        hipLaunchKernelGGL(mx_slab_reduce<F2>, dim3(w.K * F2), dim3(64), 0, w.st, slab.as<double>(), g.nbx, w.K, tmp.as<double>());
        FDX_CHECK_LAUNCH();
        hipLaunchKernelGGL(mx_centred_final, dim3(1), dim3(MX_THREADS), 0, w.st, w.K, tmp.as<double>(), out.as<double>());
        FDX_CHECK_LAUNCH();
        if (pass == 0)
            FDX_HIP(hipMemcpyAsync(rsum_dev, out.p, (size_t)w.K * 3 * sizeof(double), hipMemcpyDeviceToDevice, w.st));
        else
            FDX_HIP(hipMemcpyAsync(rsum_dev + (size_t)w.K * 3, out.as<double>() + (size_t)w.K * 3, 3 * sizeof(double),
                                   hipMemcpyDeviceToDevice, w.st));
    }
    return 0;
}

int check_args(const char* who, const void* P, const void* Q, int32_t dtype, int64_t n, int32_t K, int64_t ldp, int64_t ldq) {
    const std::string w(who);
    FDX_REQUIRE(P && Q, w + ": null matrix");
    FDX_REQUIRE(dtype == FDX_F32 || dtype == FDX_F64, w + ": dtype must be FDX_F32 or FDX_F64");
    FDX_REQUIRE(n >= 1 && K >= 1 && ldp >= K && ldq >= K, w + ": bad shape");
    FDX_REQUIRE(n * (int64_t)K <= (int64_t)INT32_MAX, w + ": n * K must be at most 2^31 - 1");
    return 0;
}

// the one device sequence behind all three entries: a device result block, one copy back
int run_all(const char* who, const void* P, const void* Q, int32_t dtype, int64_t n, int32_t K, int64_t ldp, int64_t ldq,
            bool moments, double thr, double eps, double* jsd_dev, int flags, double* stats_host, int64_t* rare_host,
            double* rho_host, void* stream) {
    FDX_TRY(check_args(who, P, Q, dtype, n, K, ldp, ldq));
    FDX_REQUIRE(!(flags & ~(FDX_SPEARMAN_OVERALL | FDX_SPEARMAN_PER_TYPE)), std::string(who) + ": unknown Spearman flags");
    hipStream_t st = (hipStream_t)stream;
    PoolStream pool_stream(st);
    const Work w{P, Q, dtype, ldp, ldq, n, K, st};
    const size_t nstat = (size_t)(K + 1) * F1, ncent = (size_t)(K + 1) * 3;
    DevBuf res;
    FDX_TRY(res.alloc((nstat + 2 * ncent) * sizeof(double)));
    double* stats = res.as<double>();
    double* cent = stats + nstat;
    double* rsum = cent + ncent;
    if (moments)
        FDX_TRY(dtype == FDX_F32 ? run_moments<float>(w, thr, eps, jsd_dev, stats, cent)
                                 : run_moments<double>(w, thr, eps, jsd_dev, stats, cent));
    if (flags) FDX_TRY(dtype == FDX_F32 ? run_spearman<float>(w, flags, rsum) : run_spearman<double>(w, flags, rsum));
    std::vector<double> h(nstat + 2 * ncent);
    FDX_TRY(copy_d2h(h.data(), res.p, h.size() * sizeof(double), st));
    res.mark_idle();
    if (moments) {
        const double* s = h.data();
        const double* c = s + nstat;
        for (int r = 0; r <= K; ++r) {
            double* o = stats_host + (size_t)r * FDX_METRICS_FIELDS;
            for (int f = 0; f < F1; ++f) o[f] = s[(size_t)r * F1 + f];
            o[FDX_MX_C_PT] = c[(size_t)r * 3 + 0];
            o[FDX_MX_C_PP] = c[(size_t)r * 3 + 1];
            o[FDX_MX_C_TT] = c[(size_t)r * 3 + 2];
        }
        if (rare_host) {
            const double* o = s + (size_t)K * F1;
            rare_host[0] = (int64_t)o[FDX_MX_N_RARE];
            rare_host[1] = (int64_t)o[FDX_MX_TP];
            rare_host[2] = (int64_t)o[FDX_MX_FP];
            rare_host[3] = (int64_t)o[FDX_MX_FN];
        }
    }
    if (flags && rho_host) {
        const double* rs = h.data() + nstat + ncent;
        for (int r = 0; r <= K; ++r) {
            const bool want = r < K ? (flags & FDX_SPEARMAN_PER_TYPE) : (flags & FDX_SPEARMAN_OVERALL);
            rho_host[r] = want ? corr_from_sums(rs[r * 3], rs[r * 3 + 1], rs[r * 3 + 2], r < K ? (double)n : (double)n * K)
                               : std::numeric_limits<double>::quiet_NaN();
        }
    }
    return 0;
}

}  // namespace

}  // namespace fdx

using namespace fdx;

extern "C" {

int fdx_metrics_moments_dev(const void* pred_dev, const void* true_dev, int32_t dtype, int64_t n, int32_t K, int64_t ld_pred,
                            int64_t ld_true, double threshold, double epsilon, double* jsd_out_dev, double* stats_host,
                            int64_t* rare_host, void* stream) {
    FDX_REQUIRE(stats_host, "fdx_metrics_moments_dev: null stats_host");
    return run_all("fdx_metrics_moments_dev", pred_dev, true_dev, dtype, n, K, ld_pred, ld_true, true, threshold, epsilon,
                   jsd_out_dev, 0, stats_host, rare_host, nullptr, stream);
}

int fdx_metrics_spearman_dev(const void* pred_dev, const void* true_dev, int32_t dtype, int64_t n, int32_t K, int64_t ld_pred,
                             int64_t ld_true, int32_t flags, double* rho_host, void* stream) {
    FDX_REQUIRE(rho_host, "fdx_metrics_spearman_dev: null rho_host");
    FDX_REQUIRE(flags != 0, "fdx_metrics_spearman_dev: flags select nothing");
    return run_all("fdx_metrics_spearman_dev", pred_dev, true_dev, dtype, n, K, ld_pred, ld_true, false, 0.0, 0.0, nullptr, flags,
                   nullptr, nullptr, rho_host, stream);
}

int fdx_metrics_evaluate_dev(const void* pred_dev, const void* true_dev, int32_t dtype, int64_t n, int32_t K, int64_t ld_pred,
                             int64_t ld_true, double threshold, double epsilon, int32_t flags, double* jsd_out_dev,
                             double* stats_host, int64_t* rare_host, double* rho_host, void* stream) {
    FDX_REQUIRE(stats_host && (flags == 0 || rho_host), "fdx_metrics_evaluate_dev: null output");
    return run_all("fdx_metrics_evaluate_dev", pred_dev, true_dev, dtype, n, K, ld_pred, ld_true, true, threshold, epsilon,
                   jsd_out_dev, flags, stats_host, rare_host, rho_host, stream);
}

}  // extern "C"
