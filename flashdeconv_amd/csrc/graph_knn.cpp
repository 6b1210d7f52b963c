// Graph build, step 3 (graph_internal.h): exact k nearest neighbours on the binned points, the band of a spot shard, and the plan
// that carries a two-phase build from its lists to its rows.
#include "graph_internal.h"

namespace fdx {

// ------------------------------------------------------------------------------------------------ k-NN
// one slot of an ascending list: (slot, carried) <- (min, max).  Distances are never NaN, and the plain instructions spare
// the canonicalising v_max_f64 x, x that fmin / fmax put in front of every slot value coming out of a loop.
__device__ __forceinline__ void minmax_f64(double& slot, double& carried) {
    double lo, hi;
    asm("v_min_f64 %0, %2, %3\n\tv_max_f64 %1, %2, %3" : "=&v"(lo), "=&v"(hi) : "v"(slot), "v"(carried));
    slot = lo;
    carried = hi;
}

// kk = k+1 nearest INCLUDING self (cKDTree.query(coords, k+1), graph.py:63); nbr_out has stride kk, -1 padded, entries in
// no particular order (the symmetrisation sorts rows by original index).
//
// What the kernel waits for is its gathers (SQ counters: waves parked on s_waitcnt 68 % of their life, VALU issuing 15 %): a
// wave's 64 lanes look into ~16 different cell neighbourhoods, so every load instruction is ~20 cache lines for the texture
// path.  Hence: ONE gather per candidate (the (x, y) pair from sc2; the caller index perm[q] is not loaded at all), and a
// per-lane list of (squared distance, position) ordered by DISTANCE ONLY - among equal distances the first met stays ahead.
// That list holds the right neighbour SET unless the kk-th and (kk+1)-th distances are equal; waves where some lane has such
// a tie walk the candidates a second time and give the places at the threshold distance to the lowest caller indices (the
// rule of the (distance, index) order).  A list slot costs v_min_f64 + v_max_f64 + one compare + two selects.
template <int KMAX, int BATCH>
__global__ __launch_bounds__(128) void knn_kernel(const double* __restrict__ sc, const double2* __restrict__ sc2,
                                                  const int* __restrict__ perm, const int* __restrict__ rank,
                                                  const int* __restrict__ cstart, const int* __restrict__ cend,
                                                  long long n, GridParams gp, int kk, int* __restrict__ nbr_out,
                                                  int* __restrict__ nbr_cnt, double* __restrict__ nn_dist,
                                                  long long lo, long long hi, int* __restrict__ indeg,
                                                  int* __restrict__ arrival, int* __restrict__ tie_count,
                                                  const int* __restrict__ row_list, const int* __restrict__ row_count,
                                                  int* __restrict__ far_flag, int far_R, int far_drop, int n_direct, int list_cap) {
    // rows [lo, hi) of the sorted order, or (n_direct >= 0: a spot shard's own rows AND its band in one launch - each of the two
    // launches lasted one walk's latency, ~50 us, whatever its size) rows lo .. lo + n_direct - 1 followed by the first
    // min(*row_count, list_cap) rows of row_list; ties and far walks are counted for the own rows only
    long long p = lo + blockIdx.x * (long long)blockDim.x + threadIdx.x;
    bool listed = false, ghost = false;
    if (n_direct >= 0) {
        const long long i = p - lo;
        if (i >= n_direct) {
            const long long j = i - n_direct;
            if (j >= list_cap || j >= (long long)*row_count) return;
            p = row_list[j];
            listed = true;
        }
    } else if (p >= hi) {
        if (!indeg) return;
        ghost = true;                                     // whole-graph build: the block's in-degree counters meet at barriers below -
        p = hi - 1;                                       // a lane past the end walks as the last row and writes nothing
    }
    const double px = sc[p], py = sc[(size_t)n + p], pz = sc[2 * (size_t)n + p];
    const double pc[3] = {px, py, pz};
    int c[3];
    for (int a = 0; a < 3; ++a) c[a] = (a < gp.dim) ? cell_coord(pc[a], gp.mn[a], gp.inv_h[a], gp.nc[a]) : 0;
    double bd[KMAX];
    int bq[KMAX];
#pragma unroll
    for (int s = 0; s < KMAX; ++s) { bd[s] = INFINITY; bq[s] = -1; }
    const bool skip_self = nn_dist != nullptr;            // nearest OTHER point: self never enters the list

    // done when the kk-th best is provably inside the block of cells within R of c
    auto covered = [&](int R) -> bool {
        bool covers_all = true;
        double safe = INFINITY;
        for (int a = 0; a < gp.dim; ++a) {
            const double slack = 1e-12 * (fabs(pc[a]) + gp.h[a] * (double)gp.nc[a]);
            if (c[a] - R > 0) {
                covers_all = false;
                safe = fmin(safe, pc[a] - (gp.mn[a] + (double)(c[a] - R) * gp.h[a]) - slack);
            }
            if (c[a] + R < gp.nc[a] - 1) {
                covers_all = false;
                safe = fmin(safe, (gp.mn[a] + (double)(c[a] + R + 1) * gp.h[a]) - pc[a] - slack);
            }
        }
        if (covers_all) return true;
        double kth = INFINITY;                            // bd[kk-1] without dynamic register indexing
#pragma unroll
        for (int s = 0; s < KMAX; ++s) if (s == (skip_self ? 0 : kk - 1)) kth = bd[s];
        return safe > 0.0 && kth < safe * safe;
    };

    // Shells 0 and 1 together (one and two dimensions: the 3 x 3 block of cells, ~36 candidates at ~4 points per cell - with
    // k <= 8 that block always suffices), as a FLAT candidate list served in batches of BATCH gathers per round trip
    // (walking cell by cell and candidate by candidate is two dependent loads deep each time: ~45 round trips per point).
    // The nine cells' (first position, count) sit in LDS, one column per lane: the walk steps through them with a running
    // cell number, and a register array indexed by it is nine selects per candidate.  A lane only ever reads its own column -
    // no barrier anywhere.
    const bool use_block = KMAX <= 16 && gp.dim <= 2 && sc2 != nullptr;
    __shared__ int s_cs[9][128], s_cn[9][128];
    const int tid = threadIdx.x;
    int total = 0;
    if (use_block) {
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const int x = c[0] + (j % 3) - 1, y = c[1] + (j / 3) - 1;
            const bool ok = x >= 0 && x < gp.nc[0] && y >= 0 && y < gp.nc[1];
            const int cell = ok ? x * gp.stride[0] + y * gp.stride[1] : 0;
            const int a = ok ? cstart[cell] : 0, b = ok ? cend[cell] : 0;
            s_cs[j][tid] = a;
            s_cn[j][tid] = b - a;
            total += b - a;
        }
    }
    auto walk_block = [&](auto&& f) {
        int j = -1, rem = 0, q = 0;
        for (int base = 0; base < total; base += BATCH) {
            int qv[BATCH];
            double2 xy[BATCH];
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                qv[u] = -1;
                if (base + u < total) {
                    while (rem == 0) { ++j; q = s_cs[j][tid]; rem = s_cn[j][tid]; }   // base + u < total: a non-empty cell is ahead
                    qv[u] = q++;
                    --rem;
                    xy[u] = sc2[qv[u]];
                }
            }
#pragma unroll
            for (int u = 0; u < BATCH; ++u)
                if (qv[u] >= 0) f(qv[u], dist2_exact(xy[u].x - px, xy[u].y - py, 0.0));   // planes past dim are zero
        }
    };
    // the shell max_a |dc_a| == R of the cell block around c
    auto walk_shell = [&](int R, auto&& f) {
        const int lo0 = max(0, c[0] - R), hi0 = min(gp.nc[0] - 1, c[0] + R);
        const int lo1 = max(0, c[1] - R), hi1 = min(gp.nc[1] - 1, c[1] + R);
        const int lo2 = max(0, c[2] - R), hi2 = min(gp.nc[2] - 1, c[2] + R);
        for (int z = lo2; z <= hi2; ++z)
            for (int y = lo1; y <= hi1; ++y) {
                const bool edge_zy = (abs(z - c[2]) == R) || (abs(y - c[1]) == R);
                for (int x = lo0; x <= hi0; ++x) {
                    if (!edge_zy && abs(x - c[0]) != R) {      // interior of the shell: jump to the far face
                        if (x < c[0] + R) { x = c[0] + R - 1; }
                        continue;
                    }
                    const int cell = x * gp.stride[0] + y * gp.stride[1] + z * gp.stride[2];
                    const int s0 = cstart[cell], s1 = cend[cell];
                    for (int q = s0; q < s1; ++q)
                        f(q, dist2_exact(sc[q] - px, sc[(size_t)n + q] - py, sc[2 * (size_t)n + q] - pz));
                }
            }
    };

    // ---- the walk: the KMAX nearest by distance
    auto keep = [&](int q, double d2) {
        if (skip_self && q == (int)p) return;
#pragma unroll
        for (int s = 0; s < KMAX; ++s) {
            const bool ahead = d2 < bd[s];                // equal: the slot's occupant stays
            minmax_f64(bd[s], d2);
            const int t = ahead ? q : bq[s];
            q = ahead ? bq[s] : q;
            bq[s] = t;
        }
    };
    const int maxR = max(gp.nc[0], max(gp.nc[1], gp.nc[2]));
    int R_first = 0, R_end = 0;                           // shells [R_first, R_end) were walked one by one
    bool done = false;
    if (use_block) {
        walk_block(keep);
        done = covered(1);
        R_first = 2;
    }
    R_end = R_first;
    for (int R = R_first; R <= maxR && !done; ++R) {
        walk_shell(R, keep);
        done = covered(R);
        R_end = R + 1;
    }
    if (nn_dist) {
        nn_dist[perm[p]] = sqrt(bd[0]);
        return;
    }
    // a walk that went past shell far_R of its cell: a spot shard's band (the rows of the cells within far_R cells of an own one)
    // then does not hold every row that can point at an own row - the sharded build falls back to exchanging the lists
    const bool went_far = R_end > far_R + 1;
    {
        const unsigned long long mf = __ballot(went_far && !listed);
        if (far_flag && mf != 0ULL && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)mf) - 1)) atomicOr(far_flag, 1);
    }
    // a spot shard with band recompute lays out only the cells within reach of such walks (bin_points): what a longer walk
    // met there is not data.  Its row gets an empty list - the build is redone by exchange anyway (far_flag; for a band row
    // the rank that owns it raises it).
    if (far_drop && went_far) {
        for (int s = 0; s < kk; ++s) nbr_out[(size_t)p * kk + s] = -1;
        nbr_cnt[p] = 0;
        return;
    }

    // ---- the threshold: the kk-th smallest distance, how many list entries lie below it, and whether the (kk+1)-th equals it
    double thr = INFINITY, next = INFINITY;
#pragma unroll
    for (int s = 0; s < KMAX; ++s) {
        if (s == kk - 1) thr = bd[s];
        if (s == kk) next = bd[s];
    }
    // Spots whose kk-th and (kk+1)-th nearest are at EXACTLY the same distance: their neighbour set is not unique (cKDTree
    // keeps whichever its traversal meets first, graph.py:60-63; here the lower spot index wins).  The (kk+1)-th best of the
    // walked block is the true one whenever it ties with the kk-th: a point at that distance lies inside the radius the
    // walk was proven to cover.  Needs a spare slot (KMAX > kk: the launch takes care of it); without one every lane takes
    // the index-ordered route.
    const bool tie = (KMAX > kk) ? (next == thr && thr < INFINITY) : true;
    if (tie_count) {
        const unsigned long long m = __ballot(tie && !listed && !ghost);
        if (m != 0ULL && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1)) atomicAdd(tie_count, (int)__popcll(m));
    }
    if (__ballot(tie) != 0ULL) {
        // second walk (every lane of the wave; a lane without a tie finds its own list again): entries below the threshold stay,
        // the places at the threshold go to the lowest caller indices among ALL candidates at that distance
        int below = 0;
#pragma unroll
        for (int s = 0; s < KMAX; ++s) below += (s < kk && bd[s] < thr) ? 1 : 0;
        const int at_thr = kk - below;
        int tl[KMAX];
#pragma unroll
        for (int s = 0; s < KMAX; ++s) tl[s] = 0x7fffffff;
        auto ties = [&](int q, double d2) {
            int v = 0x7fffffff;
            if (d2 == thr) v = perm[q];
#pragma unroll
            for (int s = 0; s < KMAX; ++s) {
                const int t = min(tl[s], v);
                v = max(tl[s], v);
                tl[s] = t;
            }
        };
        if (use_block) walk_block(ties);
        for (int R = R_first; R < R_end; ++R) walk_shell(R, ties);
#pragma unroll
        for (int s = 0; s < KMAX; ++s)
            if (s >= below && s < kk) {                   // slot s takes the (s - below)-th lowest index at the threshold
                int o = 0x7fffffff;
#pragma unroll
                for (int t = 0; t < KMAX; ++t) if (t == s - below) o = tl[t];
                bq[s] = (s - below < at_thr && o != 0x7fffffff) ? rank[o] : -1;
            }
    }

    // ---- the neighbours.  Self is dropped (graph.py:70-74); if self is not among the kk nearest (coincident points) all kk
    // stay, as in the reference.  indeg != NULL (whole graph in one piece): the symmetrisation's first pass rides along -
    // every list entry counts itself into its target's in-degree, and the number it draws is its place in the target's
    // reverse list (all counters asked at once: one round trip)
    // Most targets are rows of the same block (128 consecutive rows of the Morton order: an ~11 x 11 patch): those count in LDS
    // and the block adds each row's sum to the global counter once - 6 returning atomics per row on L2 became ~2.5.
    int arr[KMAX];
    if (indeg) {
        __shared__ int s_loc[128], s_base[128];
        const long long blk0 = lo + blockIdx.x * (long long)blockDim.x;
        s_loc[tid] = 0;
        __syncthreads();
        constexpr int LOCAL = 0x40000000;
#pragma unroll
        for (int s = 0; s < KMAX; ++s) {
            arr[s] = 0;
            if (s < kk && bq[s] >= 0 && bq[s] != (int)p && !ghost) {
                const long long t = (long long)bq[s] - blk0;
                arr[s] = (t >= 0 && t < 128) ? (atomicAdd(&s_loc[t], 1) | LOCAL) : atomicAdd(&indeg[bq[s]], 1);
            }
        }
        __syncthreads();
        {
            const int c = s_loc[tid];
            s_base[tid] = c > 0 ? atomicAdd(&indeg[blk0 + tid], c) : 0;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < KMAX; ++s)
            if (arr[s] & LOCAL) arr[s] = s_base[bq[s] - blk0] + (arr[s] & ~LOCAL);
        if (ghost) return;
    }
    int cnt = 0;
#pragma unroll
    for (int s = 0; s < KMAX; ++s)
        if (s < kk && bq[s] >= 0 && bq[s] != (int)p) {
            if (indeg) arrival[(size_t)p * kk + cnt] = arr[s];
            nbr_out[(size_t)p * kk + cnt++] = bq[s];
        }
    for (int s = cnt; s < kk; ++s) nbr_out[(size_t)p * kk + s] = -1;
    nbr_cnt[p] = cnt;
}

// ------------------------------------------------------------------------------------------------ more than three dimensions
// utils/graph.py:16-22 takes coordinates of any dimension (cKDTree does).  The grid of this file bins three axes; points with 4 to
// FDX_KNN_MAX_DIM coordinates are put in solver order by their FIRST THREE coordinates (locality of the sweep's tiles only - any
// order gives the same graph) and searched exhaustively: lane = row, candidates in ascending CALLER index staged through LDS 256 at
// a time, squared distances summed coordinate by coordinate without contraction, a candidate enters the list on strictly smaller
// distance - i.e. the (distance, index) rule of knn_kernel.  O(n^2 dim): for the tens of thousands of spots such data has.
__global__ __launch_bounds__(256) void take3_kernel(const double* __restrict__ coords, long long n, int dim, double* __restrict__ out) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= n) return;
    for (int a = 0; a < 3; ++a) out[(size_t)i * 3 + a] = coords[(size_t)i * dim + a];
}

template <int KMAX>
__global__ __launch_bounds__(256) void knn_brute_kernel(const double* __restrict__ coords, const int* __restrict__ perm,
                                                        const int* __restrict__ rank, long long n, int dim, int kk,
                                                        int* __restrict__ nbr_out, int* __restrict__ nbr_cnt, long long lo, long long hi,
                                                        int* __restrict__ tie_count) {
#pragma clang fp contract(off)
    __shared__ double tile[256 * FDX_KNN_MAX_DIM];
    const long long p = lo + blockIdx.x * 256LL + threadIdx.x;
    const bool live = p < hi;
    const int op = live ? perm[p] : 0;
    double x[FDX_KNN_MAX_DIM];
    for (int a = 0; a < FDX_KNN_MAX_DIM; ++a) x[a] = (a < dim) ? coords[(size_t)op * dim + a] : 0.0;
    double bd[KMAX];
    int bq[KMAX];
#pragma unroll
    for (int s = 0; s < KMAX; ++s) { bd[s] = INFINITY; bq[s] = -1; }
    for (long long o0 = 0; o0 < n; o0 += 256) {
        const int cnt = (int)min(256LL, n - o0);
        __syncthreads();
        for (int t = threadIdx.x; t < cnt * dim; t += 256) tile[t] = coords[(size_t)o0 * dim + t];
        __syncthreads();
        if (!live) continue;
        for (int c = 0; c < cnt; ++c) {
            double d2 = 0.0;
            for (int a = 0; a < dim; ++a) { const double dx = tile[c * dim + a] - x[a]; d2 = d2 + dx * dx; }
            int q = (int)(o0 + c);                       // caller index; turned into a position when the list is written
#pragma unroll
            for (int s = 0; s < KMAX; ++s) {
                const bool ahead = d2 < bd[s];            // equal: the occupant (lower caller index) stays
                const double td = ahead ? bd[s] : d2;
                const int tq = ahead ? bq[s] : q;
                bd[s] = ahead ? d2 : bd[s];
                bq[s] = ahead ? q : bq[s];
                d2 = td;
                q = tq;
            }
        }
    }
    if (!live) return;
    double thr = INFINITY, next = INFINITY;
#pragma unroll
    for (int s = 0; s < KMAX; ++s) {
        if (s == kk - 1) thr = bd[s];
        if (s == kk) next = bd[s];
    }
    if (tie_count && KMAX > kk && next == thr && thr < INFINITY) atomicAdd(tie_count, 1);
    int cnt = 0;
#pragma unroll
    for (int s = 0; s < KMAX; ++s)
        if (s < kk && bq[s] >= 0 && bq[s] != op) nbr_out[(size_t)p * kk + cnt++] = rank[bq[s]];
    for (int s = cnt; s < kk; ++s) nbr_out[(size_t)p * kk + s] = -1;
    nbr_cnt[p] = cnt;
}

// ------------------------------------------------------------------------------------------------ band of a spot shard
// A shard owns rows [lo, hi) of the sorted order.  Row p of the symmetrised k-NN graph is out(p) U in(p): in(p) needs the list of
// every row q that points at p.  When q's walk stayed within BAND_R shells of its own cell (knn_kernel reports the rows for which
// it did not), q can only point at rows of cells at most BAND_R cells away - so the rows that can point at an OWN row all live in
// cells within BAND_R cells of a cell that holds an own row: the BAND.  The shard finds the lists of its band itself ("recompute,
// don't communicate") instead of receiving the lists of all n rows.  BAND_R = 2: at ~4 points per cell the 3 x 3 block serves the
// k <= 8 nearest of MOST points (the flat walk of knn_kernel), but on uniform random points 1-3 % of the walks need shell 2 (the
// 7-th nearest lies beyond the distance to the block's edge); shell 3 would need fewer than 7 points in a disc of 12 cells.
// counters: [0] cells listed, [1] band rows listed, [2] a walk left the block (knn_kernel), [3] the band list overflowed
__global__ __launch_bounds__(256) void band_cells_kernel(const double* __restrict__ sc, long long n, GridParams gp, long long lo,
                                                         long long hi, int* __restrict__ cell_flag, int* __restrict__ cell_list,
                                                         int* __restrict__ counters) {
    const long long p = lo + blockIdx.x * 256LL + threadIdx.x;
    if (p >= hi) return;
    int c[3];
    for (int a = 0; a < 3; ++a) c[a] = (a < gp.dim) ? cell_coord(sc[(size_t)a * n + p], gp.mn[a], gp.inv_h[a], gp.nc[a]) : 0;
    const int r1 = gp.dim > 1 ? BAND_R : 0, r2 = gp.dim > 2 ? BAND_R : 0;
    for (int dz = -r2; dz <= r2; ++dz)
        for (int dy = -r1; dy <= r1; ++dy)
            for (int dx = -BAND_R; dx <= BAND_R; ++dx) {
                const int x = c[0] + dx, y = c[1] + dy, z = c[2] + dz;
                if (x < 0 || x >= gp.nc[0] || y < 0 || y >= gp.nc[1] || z < 0 || z >= gp.nc[2]) continue;
                const int cell = x * gp.stride[0] + y * gp.stride[1] + z * gp.stride[2];
                if (cell_flag[cell] == 0 && atomicExch(&cell_flag[cell], 1) == 0) cell_list[atomicAdd(&counters[0], 1)] = cell;
            }
}

__global__ __launch_bounds__(256) void band_rows_kernel(const int* __restrict__ cell_list, const int* __restrict__ cstart,
                                                        const int* __restrict__ cend, long long lo, long long hi, int cap,
                                                        int* __restrict__ band, int* __restrict__ counters) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= counters[0]) return;
    const int cell = cell_list[i];
    for (int q = cstart[cell]; q < cend[cell]; ++q) {
        if (q >= lo && q < hi) continue;
        const int at = atomicAdd(&counters[1], 1);
        if (at < cap) band[at] = q;
        else counters[3] = 1;
    }
}

// The same band from the need flags of the shard's binning (cell_need_kernel<0>: the keys within BAND_R cells of a key that holds
// an own row - exactly the band's cells): one thread per key, the rows of a flagged key outside [lo, hi) appended with one atomic
// per wave.  (band_cells_kernel + band_rows_kernel: 25 flag reads per OWN ROW and an atomic per band row - 55 + 17 us for a
// 125k-row shard whose whole k-NN search is 60.)
__global__ __launch_bounds__(256) void band_rows_need_kernel(const int* __restrict__ start, long long bins,
                                                             const unsigned char* __restrict__ need1, long long lo, long long hi,
                                                             int cap, int* __restrict__ band, int* __restrict__ counters) {
    const long long k = blockIdx.x * 256LL + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int s0 = 0, s1 = 0;
    if (k < bins && need1[k]) { s0 = start[k]; s1 = start[k + 1]; }
    // rows of the key are positions [s0, s1); those inside [lo, hi) are own rows
    const int a0 = (int)min((long long)s1, max((long long)s0, lo)), a1 = (int)max((long long)a0, min((long long)s1, hi));   // own part [a0, a1)
    const int cnt = (s1 - s0) - (a1 - a0);
    int incl = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(incl, off, 64);
        if (lane >= off) incl += v;
    }
    const int total = __shfl(incl, 63, 64);
    if (total == 0) return;
    int base = 0;
    if (lane == 63) base = atomicAdd(&counters[1], total);
    base = __shfl(base, 63, 64);
    int at = base + incl - cnt;
    for (int q = s0; q < s1; ++q) {
        if (q >= a0 && q < a1) continue;
        if (at < cap) band[at] = q;
        else counters[3] = 1;
        ++at;
    }
}

// ------------------------------------------------------------------------------------------------ host side
template <int KMAX>
static void launch_knn_range(const BinnedPoints& b, const int* perm, int kk, int* nbr, int* cnt, double* nn_dist, long long lo,
                             long long hi, hipStream_t st, int* indeg = nullptr, int* arrival = nullptr, int* ties = nullptr,
                             const int* row_list = nullptr, const int* row_count = nullptr, int* far_flag = nullptr, int far_drop = 0,
                             int n_direct = -1, int list_cap = 0) {
    const int far_R = BAND_R;
    if (hi <= lo) return;
    const long long n_threads = n_direct >= 0 ? (long long)n_direct + list_cap : hi - lo;
    // candidates per round trip: 4 leaves the kernel 77 registers (6 waves per SIMD), 6: 87 (5 waves), 8: 97 (4 waves);
    // 1M spots, wall per fit: 4.69 / 4.84 / 4.88 ms
    // a launch of a few hundred thousand rows does not fill the chip anyway (a spot shard's own rows + band): what it takes is one
    // walk's chain of round trips, and 8 candidates per round trip halve that chain (97 registers, 4 waves per SIMD - no loss here)
    const int batch = (KMAX <= 16 && n_threads > 300000) ? 4 : 8;
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(ceil_div(n_threads, 128)), dim3(128), 0, st, b.sc.as<double>(), b.sc2.as<double2>(), perm,
                           b.rank.as<int>(), b.cstart.as<int>(), b.cend_p, b.n, b.gp, kk, nbr, cnt, nn_dist, lo, hi, indeg, arrival,
                           KMAX > kk ? ties : nullptr, row_list, row_count, far_flag, far_R, far_drop,
                           n_direct, list_cap);
    };
    if constexpr (KMAX <= 16) {
        if (batch == 4) go(knn_kernel<KMAX, 4>);
        else go(knn_kernel<KMAX, 8>);
    } else {
        go(knn_kernel<KMAX, 8>);
    }
}

template <int KMAX>
static void launch_knn(const BinnedPoints& b, const int* perm, int kk, int* nbr, int* cnt, double* nn_dist, hipStream_t st) {
    launch_knn_range<KMAX>(b, perm, kk, nbr, cnt, nn_dist, 0, b.n, st);
}

int graph_nearest_distance(const double* d_coords, long long n, int dim, double* d_out, hipStream_t st) {
    FDX_REQUIRE(dim >= 1 && dim <= 3, "graph: coordinate dimension must be 1, 2 or 3");
    FDX_REQUIRE(n >= 2 && n < 0x7fffff00LL, "graph: nearest distance needs at least two points");
    BinnedPoints b;
    FDX_TRY(bin_points(d_coords, n, dim, 2.0, 0.0, &b, st));
    launch_knn<8>(b, b.perm.as<int>(), 2, nullptr, nullptr, d_out, st);
    FDX_CHECK_LAUNCH();
    FDX_HIP(hipStreamSynchronize(st));
    return 0;
}

// ---- k-NN graph in two phases, so that a spot shard can build only its own rows ------------------------------------
// Phase 1 (knn_lists): bin ALL points (replicated; the Morton order defines the solver positions on every rank) and find
// the k nearest neighbours of the rows [lo, hi) only.  Phase 2 (from_knn_lists): row p of the symmetrised graph is
// out(p) U in(p); in(p) needs the lists of every row that points at p, so between the phases the ranks all-gather
// their list rows (the one exchange step of the build).  Phase 2 then touches own rows only: rows outside [lo, hi) keep
// degree 0 (their slices have width 0), which is all graph_localize reads of a full graph anyway (symmetry).
// Single GPU: [lo, hi) = [0, n), no exchange - the same code.

int graph_knn_lists(const double* d_coords, long long n, int dim, int k, long long lo, long long hi, int* nbr, int* cnt,
                    fdx_graph_plan** out, hipStream_t st, bool band, const GraphBuildHooks* hooks) {
    FDX_REQUIRE(dim >= 1 && dim <= FDX_KNN_MAX_DIM, "graph: k-NN graphs take coordinates of 1 to 8 dimensions");
    FDX_REQUIRE(dim <= 3 || n <= (1 << 18), "graph: coordinates of more than 3 dimensions are searched exhaustively: at most 262144 spots");
    FDX_REQUIRE(n >= 2 && n < 0x7fffff00LL, "graph: n out of range");
    FDX_REQUIRE(k >= 1, "graph: k must be positive");
    FDX_REQUIRE(0 <= lo && lo <= hi && hi <= n, "graph: bad row range");
    const int k_act = (int)std::min<long long>(k, n - 1);           // graph.py:51
    const int kk = k_act + 1;
    FDX_REQUIRE(kk <= 64, "graph: k_neighbors above 63 is not supported");
    FDX_REQUIRE((long long)n * kk < 0x7fffff00LL, "graph: n*k too large");
    auto* plan = new fdx_graph_plan();
    plan->n = n;
    plan->kk = kk;
    plan->st = st;
    // ~4 points per grid cell: the 3 x 3 block of cells then always holds the k <= 8 nearest (no second shell, no divergence),
    // and the 256-spot Morton tiles come out more compact (1M jittered-lattice spots: graph 1.11 -> 0.95 ms, sweep 0.192 -> 0.186 ms;
    // uniform random spots: unchanged)
    const double tpc = 4.0;
    int rc = 0;
    if (dim > 3) {
        // solver order from the first three coordinates, exhaustive search in all of them
        DevBuf c3;
        rc = c3.alloc((size_t)n * 3 * sizeof(double));
        if (!rc) rc = graph_hook_under_wait(hooks);
        if (!rc) {
            hipLaunchKernelGGL(take3_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, d_coords, n, dim, c3.as<double>());
            rc = bin_points(c3.as<double>(), n, 3, tpc, 0.0, &plan->b, st);
        }
        if (!rc) rc = plan->ties.alloc(8);
        if (!rc && hipMemsetAsync(plan->ties.p, 0, 8, st) != hipSuccess) rc = fail(FDX_ERR_HIP, "graph: memset failed");
        if (rc) { delete plan; return rc; }
        const BinnedPoints& bb = plan->b;
        int* ties_hd = plan->ties.as<int>();
        if (band && (lo > 0 || hi < n)) {               // no band in this search: report it, the caller exchanges the lists
            const int one = 1;
            if (hipMemcpyAsync(ties_hd + 1, &one, 4, hipMemcpyHostToDevice, st) != hipSuccess) { delete plan; return fail(FDX_ERR_HIP, "graph: copy failed"); }
            if (hipMemsetAsync(cnt, 0, (size_t)n * 4, st) != hipSuccess) { delete plan; return fail(FDX_ERR_HIP, "graph: memset failed"); }
        }
        if (hi > lo) {
            const dim3 grid(ceil_div(hi - lo, 256)), blk(256);
            if (kk < 8) hipLaunchKernelGGL(knn_brute_kernel<8>, grid, blk, 0, st, d_coords, bb.perm.as<int>(), bb.rank.as<int>(), n, dim, kk, nbr, cnt, lo, hi, ties_hd);
            else if (kk < 16) hipLaunchKernelGGL(knn_brute_kernel<16>, grid, blk, 0, st, d_coords, bb.perm.as<int>(), bb.rank.as<int>(), n, dim, kk, nbr, cnt, lo, hi, ties_hd);
            else if (kk < 32) hipLaunchKernelGGL(knn_brute_kernel<32>, grid, blk, 0, st, d_coords, bb.perm.as<int>(), bb.rank.as<int>(), n, dim, kk, nbr, cnt, lo, hi, ties_hd);
            else hipLaunchKernelGGL(knn_brute_kernel<64>, grid, blk, 0, st, d_coords, bb.perm.as<int>(), bb.rank.as<int>(), n, dim, kk, nbr, cnt, lo, hi, ties_hd);
        }
        if (hipGetLastError() != hipSuccess) { delete plan; return fail(FDX_ERR_HIP, "graph: k-NN kernel launch failed"); }
        if (hipStreamSynchronize(st) != hipSuccess) { delete plan; return fail(FDX_ERR_HIP, "graph: sync failed"); }   // c3 and `one` die here
        *out = plan;
        return 0;
    }
    const bool shard_band = band && (lo > 0 || hi < n) && hi > lo;
    // the in-degree counters (whole graph) and the tie / far words start as zero: filled while the host waits for the bounding box
    const bool whole = lo == 0 && hi == n;
    const std::function<int()> fills = [&]() -> int {
        if (whole) {
            FDX_TRY(plan->indeg.alloc((size_t)(n + 1) * 4));
            FDX_TRY(plan->arrival.alloc((size_t)n * kk * 4));
            FDX_HIP(hipMemsetAsync(plan->indeg.p, 0, plan->indeg.bytes, st));
        }
        FDX_TRY(plan->ties.alloc(8));
        FDX_HIP(hipMemsetAsync(plan->ties.p, 0, 8, st));
        FDX_TRY(graph_hook_under_wait(hooks));
        return 0;
    };
    rc = shard_band ? bin_points(d_coords, n, dim, tpc, 0.0, &plan->b, st, lo, hi, BAND_R, &fills)
                    : bin_points(d_coords, n, dim, tpc, 0.0, &plan->b, st, 0, 0, 0, &fills);
    if (rc) { delete plan; return rc; }
    const BinnedPoints& b = plan->b;
    const int* perm = b.perm.as<int>();
    int* indeg = whole ? plan->indeg.as<int>() : nullptr;
    int* arrival = whole ? plan->arrival.as<int>() : nullptr;
    int* ties = plan->ties.as<int>();
    band = band && (lo > 0 || hi < n);
    if (band) {
        // every row without a list must read as empty: one fill of 4 bytes per row (the only pass over all n rows left in a shard's
        // symmetrisation; the lists themselves are written for the own rows and the band only)
        if (hipMemsetAsync(cnt, 0, (size_t)n * 4, st) != hipSuccess) { delete plan; return fail(FDX_ERR_HIP, "graph: memset failed"); }
    }
    // one slot more than the list length, for the tie test (kk = 64 has none: no tie count there).
    // Where the kernel's time goes at 1M spots (300 us): ~110 us are the 7M in-degree counters (returning atomics; measured
    // with the counters taken out), the rest the walk - waves parked on its gathers two thirds of their life.
    const long long rows = hi - lo;
    // a shard's own rows and its band share ONE launch; the kernel's int row counts hold both (n * kk < 2^31 and kk >= 2 above:
    // rows <= n < 2^30)
    const bool merged = band && rows > 0;
    if (band && rows > 0) {
        // the band: cells next to a cell with an own row -> their rows outside [lo, hi) -> the lists of those rows.  Room for as
        // many band rows as own rows (a band is a surface: thousands of rows beside a million); an overflow is reported and the
        // caller falls back to exchanging the lists.  The band is listed FIRST (it needs the binning only): own rows and band then
        // share one k-NN launch.
        const int n_cells = b.n_cells;
        DevBuf cell_flag, cell_list;
        plan->band_cap = (int)std::min<long long>(n - rows, std::max<long long>(rows, 4096));
        rc = cell_flag.alloc((size_t)std::max(n_cells, 1) * 4);
        if (!rc) rc = cell_list.alloc((size_t)std::max(n_cells, 1) * 4);
        if (!rc) rc = plan->band_rows.alloc((size_t)std::max(plan->band_cap, 1) * 4);
        if (!rc) rc = plan->band_counters.alloc(16);
        if (rc) { delete plan; return rc; }
        const bool from_need = b.need_p && b.bins > 0;
        if ((!from_need && hipMemsetAsync(cell_flag.p, 0, cell_flag.bytes, st) != hipSuccess) ||
            hipMemsetAsync(plan->band_counters.p, 0, 16, st) != hipSuccess) {
            delete plan;
            return fail(FDX_ERR_HIP, "graph: memset failed");
        }
        int* ctr = plan->band_counters.as<int>();
        if (from_need) {
            // the shard's binning has flagged the band's keys already (first dilation of cell_need_kernel)
            hipLaunchKernelGGL(band_rows_need_kernel, dim3(ceil_div(b.bins, 256)), dim3(256), 0, st, b.start.as<int>(), b.bins,
                               b.need_p, lo, hi, plan->band_cap, plan->band_rows.as<int>(), ctr);
        } else {
            hipLaunchKernelGGL(band_cells_kernel, dim3(ceil_div(rows, 256)), dim3(256), 0, st, b.sc.as<double>(), n, b.gp, lo, hi,
                               cell_flag.as<int>(), cell_list.as<int>(), ctr);
            // at most (2 BAND_R + 1)^dim cells per own row, and never more than there are cells
            const long long side = 2 * BAND_R + 1;
            const long long max_cells = std::min<long long>(n_cells, rows * (dim == 1 ? side : dim == 2 ? side * side : side * side * side));
            hipLaunchKernelGGL(band_rows_kernel, dim3(ceil_div(max_cells, 256)), dim3(256), 0, st, cell_list.as<int>(), b.cstart.as<int>(),
                               b.cend_p, lo, hi, plan->band_cap, plan->band_rows.as<int>(), ctr);
        }
        // cell_flag / cell_list go back to the pool here: the pool orders their next use on this stream behind these kernels
    }
    const int* bl = plan->band_rows.as<int>();
    const int* bctr = plan->band_counters.p ? plan->band_counters.as<int>() + 1 : nullptr;
    const int nd = merged ? (int)rows : -1, lc = merged ? plan->band_cap : 0;
    const int fd = shard_band ? 1 : 0;
    const int* rl = merged ? bl : nullptr;
    const int* rcnt = merged ? bctr : nullptr;
    if (kk < 8) launch_knn_range<8>(b, perm, kk, nbr, cnt, nullptr, lo, hi, st, indeg, arrival, ties, rl, rcnt, ties + 1, fd, nd, lc);
    else if (kk < 16) launch_knn_range<16>(b, perm, kk, nbr, cnt, nullptr, lo, hi, st, indeg, arrival, ties, rl, rcnt, ties + 1, fd, nd, lc);
    else if (kk < 32) launch_knn_range<32>(b, perm, kk, nbr, cnt, nullptr, lo, hi, st, indeg, arrival, ties, rl, rcnt, ties + 1, fd, nd, lc);
    else launch_knn_range<64>(b, perm, kk, nbr, cnt, nullptr, lo, hi, st, indeg, arrival, ties, rl, rcnt, ties + 1, fd, nd, lc);
    trace_host("knn: kernel launched");
    if (hipGetLastError() != hipSuccess) { delete plan; return fail(FDX_ERR_HIP, "graph: k-NN kernel launch failed"); }
    *out = plan;
    return 0;
}

void graph_plan_destroy(fdx_graph_plan* plan) { delete plan; }
int graph_plan_kk(const fdx_graph_plan* plan) { return plan->kk; }
// the caller has written other lists into nbr / cnt than the ones the k-NN kernel produced: the in-degrees and reverse-list places
// that kernel drew for ITS lists (whole-graph builds) no longer apply - the symmetrisation counts again
int graph_plan_lists_replaced(fdx_graph_plan* plan) {
    if (plan->indeg.p || plan->arrival.p) {
        FDX_HIP(hipStreamSynchronize(plan->st));        // the k-NN kernel may still be writing them
        plan->indeg.release();
        plan->arrival.release();
    }
    return 0;
}
// ids (n_rows, kk): caller ids as a k-nearest query returns them (the point itself usually among them, -1 padded); row r answers for
// caller id rows[r] (rows NULL: r itself).  Written where the symmetrisation expects a row's list: at the row's solver position,
// as solver positions, the point itself dropped (utils/graph.py:70-74), compacted, -1 padded.
__global__ __launch_bounds__(256) void lists_from_ids_kernel(const long long* __restrict__ ids, const long long* __restrict__ rows,
                                                            long long n_rows, int kk, const int* __restrict__ rank,
                                                            int* __restrict__ nbr, int* __restrict__ cnt) {
    const long long r = blockIdx.x * 256LL + threadIdx.x;
    if (r >= n_rows) return;
    const long long self = rows ? rows[r] : r;
    const int p = rank[self];
    int c = 0;
    for (int j = 0; j < kk; ++j) {
        const long long id = ids[(size_t)r * kk + j];
        if (id >= 0 && id != self) nbr[(size_t)p * kk + c++] = rank[id];
    }
    cnt[p] = c;
    for (; c < kk; ++c) nbr[(size_t)p * kk + c] = -1;
}

int graph_plan_set_lists(fdx_graph_plan* plan, const long long* ids_host, const long long* rows_host, long long n_rows, int* nbr,
                         int* cnt, hipStream_t st) {
    FDX_REQUIRE(n_rows >= 0 && n_rows <= plan->n, "graph: more list rows than spots");
    if (n_rows == 0) return graph_plan_lists_replaced(plan);
    DevBuf d_ids, d_rows;
    FDX_TRY(d_ids.alloc((size_t)n_rows * plan->kk * 8));
    FDX_TRY(copy_h2d(d_ids.p, ids_host, (size_t)n_rows * plan->kk * 8, st));
    if (rows_host) {
        for (long long r = 0; r < n_rows; ++r) FDX_REQUIRE(rows_host[r] >= 0 && rows_host[r] < plan->n, "graph: list row out of range");
        FDX_TRY(d_rows.alloc((size_t)n_rows * 8));
        FDX_TRY(copy_h2d(d_rows.p, rows_host, (size_t)n_rows * 8, st));
    }
    hipLaunchKernelGGL(lists_from_ids_kernel, dim3(ceil_div(n_rows, 256)), dim3(256), 0, st, d_ids.as<long long>(),
                       rows_host ? d_rows.as<long long>() : (const long long*)nullptr, n_rows, plan->kk, plan->b.rank.as<int>(), nbr, cnt);
    FDX_CHECK_LAUNCH();
    FDX_HIP(hipStreamSynchronize(st));            // the host arrays are the caller's
    return graph_plan_lists_replaced(plan);
}

// the same with the query answers already on the device (ids_dev: n_rows x kk int64; rows_host NULL: row r answers for caller id r)
int graph_plan_set_lists_device(fdx_graph_plan* plan, const long long* ids_dev, const long long* rows_host, long long n_rows, int* nbr,
                                int* cnt, hipStream_t st) {
    FDX_REQUIRE(n_rows >= 0 && n_rows <= plan->n, "graph: more list rows than spots");
    if (n_rows == 0) return graph_plan_lists_replaced(plan);
    DevBuf d_rows;
    if (rows_host) {
        for (long long r = 0; r < n_rows; ++r) FDX_REQUIRE(rows_host[r] >= 0 && rows_host[r] < plan->n, "graph: list row out of range");
        FDX_TRY(d_rows.alloc((size_t)n_rows * 8));
        FDX_TRY(copy_h2d(d_rows.p, rows_host, (size_t)n_rows * 8, st));
    }
    hipLaunchKernelGGL(lists_from_ids_kernel, dim3(ceil_div(n_rows, 256)), dim3(256), 0, st, ids_dev,
                       rows_host ? d_rows.as<long long>() : (const long long*)nullptr, n_rows, plan->kk, plan->b.rank.as<int>(), nbr, cnt);
    FDX_CHECK_LAUNCH();
    FDX_HIP(hipStreamSynchronize(st));            // rows_host is the caller's
    return graph_plan_lists_replaced(plan);
}

int graph_plan_order(const fdx_graph_plan* plan, int* d_perm_out, int* d_rank_out, hipStream_t st) {
    if (d_perm_out) FDX_HIP(hipMemcpyAsync(d_perm_out, plan->b.perm.p, (size_t)plan->n * 4, hipMemcpyDeviceToDevice, st));
    if (d_rank_out) FDX_HIP(hipMemcpyAsync(d_rank_out, plan->b.rank.p, (size_t)plan->n * 4, hipMemcpyDeviceToDevice, st));
    return 0;
}

}  // namespace fdx
