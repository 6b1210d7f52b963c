// The QUERIES of the restated cKDTree on the device.  The tree is built on the device (kdtree_build_dev.cpp) or on the host
// (kdtree_host.cpp: introselect's permutation replayed step by step) and uploaded - 24 bytes per node, 4 per point; one lane
// answers one query with exactly the host's sequence of node visits,
// heap operations and comparisons (kd_query_one of kdtree_host.cpp): best-first over the nodes with scipy's binary heap, the far node's record
// (node, distance, per-axis side distances) held IN the heap entry - the host keeps it in a pool and the index in the heap: the
// same priorities, the same sift sequences -, a leaf's points tested in index-array order against the strict bound.  Sums and
// products are rounded one by one (no contraction), as the host compiles them.  The two heaps of a lane live in a global work
// area laid out lane-interleaved (entry j of lane l at [j][l]): a wave's accesses to "its" entry j coalesce.  Entry counts are
// bounded (far-node heap: KD_QCAP; a deeper heap than that - never seen, the heap holds about one entry per tree level - raises
// a flag and the caller repeats the queries on the host).  1M lattice points, k = 6: 11-15 ms on the host's threads -> see DESIGN.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "kdtree_dev.h"

namespace fdx {
namespace {
constexpr int KD_QCAP = 48;
struct KdBounds { double mins[3], maxes[3]; };

// NBL: the k-nearest heap of a lane (kk <= 16 entries, by far the busiest of the two: a pop and a push per accepted candidate)
// lives in LDS, lane-interleaved like its global form - 12 bytes x kk x 256 lanes
template <int M, bool NBL>
__global__ __launch_bounds__(256) void kd_query_kernel(const double* __restrict__ coords, const int4* __restrict__ meta,
                                                       const double* __restrict__ split, const int* __restrict__ indices,
                                                       const KdBounds bnd, int kk, const long long* __restrict__ rows, long long n_rows,
                                                       long long* __restrict__ ids_out, double* __restrict__ q_pri, int* __restrict__ q_node,
                                                       double* __restrict__ q_side, double* __restrict__ nb_pri, int* __restrict__ nb_idx,
                                                       long long L, int* __restrict__ overflow) {
#pragma clang fp contract(off)
    const long long gid = blockIdx.x * 256LL + threadIdx.x;
    auto QP = [&](int j) -> double& { return q_pri[(size_t)j * L + gid]; };
    auto QN = [&](int j) -> int& { return q_node[(size_t)j * L + gid]; };
    auto QS = [&](int j, int a) -> double& { return q_side[((size_t)j * M + a) * L + gid]; };
    extern __shared__ __attribute__((aligned(16))) unsigned char kd_smem[];
    double* const l_pri = reinterpret_cast<double*>(kd_smem);
    int* const l_idx = reinterpret_cast<int*>(kd_smem + (size_t)kk * 256 * sizeof(double));
    auto NP = [&](int j) -> double& { return NBL ? l_pri[j * 256 + (int)threadIdx.x] : nb_pri[(size_t)j * L + gid]; };
    auto NI = [&](int j) -> int& { return NBL ? l_idx[j * 256 + (int)threadIdx.x] : nb_idx[(size_t)j * L + gid]; };
    for (long long r = gid; r < n_rows; r += L) {
        const long long self = rows ? rows[r] : r;
        double x[M];
#pragma unroll
        for (int a = 0; a < M; ++a) x[a] = coords[(size_t)self * M + a];
        int qn = 0, nn = 0;
        double upper = HUGE_VAL;
        bool over = false;
        // current node record
        int c_node = 0;
        double c_md = 0.0, c_side[M];
#pragma unroll
        for (int a = 0; a < M; ++a) {
            double sd = fmax(0.0, fmax(bnd.mins[a] - x[a], x[a] - bnd.maxes[a]));
            sd = sd * sd;
            c_md += sd - 0.0;
            c_side[a] = sd;
        }
        for (;;) {
            const int4 nd = meta[c_node];                          // x: split dim (-1 leaf), y / z: start / end or less / greater
            if (nd.x < 0) {
                for (int i = nd.y; i < nd.z; ++i) {
                    const int id = indices[i];
                    double d = 0.0;
#pragma unroll
                    for (int a = 0; a < M; ++a) {
                        const double diff = coords[(size_t)id * M + a] - x[a];
                        d += diff * diff;
                    }
                    if (d < upper) {
                        if (nn == kk) {                            // remove the root: the last entry sifts down from the top
                            const double mp = NP(nn - 1);
                            const int mi = NI(nn - 1);
                            --nn;
                            int h = 0;
                            for (;;) {
                                const int j = 2 * h + 1, k2 = 2 * h + 2;
                                const double pj = j < nn ? NP(j) : 0.0, pk = k2 < nn ? NP(k2) : 0.0;
                                if (!((j < nn && mp > pj) || (k2 < nn && mp > pk))) break;
                                const int l = (k2 < nn && pj > pk) ? k2 : j;
                                NP(h) = l == j ? pj : pk;
                                NI(h) = NI(l);
                                h = l;
                            }
                            if (nn > 0) { NP(h) = mp; NI(h) = mi; }
                        }
                        {                                          // push (-d, id): sift up from the end
                            const double np = -d;
                            int h = nn++;
                            while (h > 0) {
                                const int par = (h - 1) / 2;
                                const double pp = NP(par);
                                if (!(np < pp)) break;
                                NP(h) = pp;
                                NI(h) = NI(par);
                                h = par;
                            }
                            NP(h) = np;
                            NI(h) = id;
                        }
                        if (nn == kk) upper = -NP(0);
                    }
                }
                if (qn == 0) break;
                // pop the nearest pending node
                c_md = QP(0);
                c_node = QN(0);
#pragma unroll
                for (int a = 0; a < M; ++a) c_side[a] = QS(0, a);
                {
                    --qn;
                    const double mp = QP(qn);
                    const int mnode = QN(qn);
                    double ms[M];
#pragma unroll
                    for (int a = 0; a < M; ++a) ms[a] = QS(qn, a);
                    int h = 0;
                    for (;;) {
                        const int j = 2 * h + 1, k2 = 2 * h + 2;
                        const double pj = j < qn ? QP(j) : 0.0, pk = k2 < qn ? QP(k2) : 0.0;
                        if (!((j < qn && mp > pj) || (k2 < qn && mp > pk))) break;
                        const int l = (k2 < qn && pj > pk) ? k2 : j;
                        QP(h) = l == j ? pj : pk;
                        QN(h) = QN(l);
#pragma unroll
                        for (int a = 0; a < M; ++a) QS(h, a) = QS(l, a);
                        h = l;
                    }
                    if (qn > 0) {
                        QP(h) = mp;
                        QN(h) = mnode;
#pragma unroll
                        for (int a = 0; a < M; ++a) QS(h, a) = ms[a];
                    }
                }
            } else {
                if (c_md > upper) break;                           // the nearest remaining cell is too far: done
                const double sp = split[c_node];
                double xs = x[0];
#pragma unroll
                for (int a = 1; a < M; ++a) xs = nd.x == a ? x[a] : xs;
                int f_node;
                double side_distance;
                if (xs < sp) { c_node = nd.y; f_node = nd.z; side_distance = sp - xs; }
                else { c_node = nd.z; f_node = nd.y; side_distance = xs - sp; }
                side_distance = side_distance * side_distance;
                double f_side[M], f_md = c_md;
                double old = c_side[0];
#pragma unroll
                for (int a = 0; a < M; ++a) { f_side[a] = c_side[a]; old = nd.x == a ? c_side[a] : old; }
                f_md += side_distance - old;
#pragma unroll
                for (int a = 0; a < M; ++a) f_side[a] = nd.x == a ? side_distance : f_side[a];
                if (c_md > f_md) {                                 // the closer one is followed
                    const double t = c_md; c_md = f_md; f_md = t;
                    const int tn = c_node; c_node = f_node; f_node = tn;
#pragma unroll
                    for (int a = 0; a < M; ++a) { const double ts = c_side[a]; c_side[a] = f_side[a]; f_side[a] = ts; }
                }
                if (f_md <= upper) {
                    if (qn >= KD_QCAP) { over = true; break; }
                    int h = qn++;
                    while (h > 0) {
                        const int par = (h - 1) / 2;
                        const double pp = QP(par);
                        if (!(f_md < pp)) break;
                        QP(h) = pp;
                        QN(h) = QN(par);
#pragma unroll
                        for (int a = 0; a < M; ++a) QS(h, a) = QS(par, a);
                        h = par;
                    }
                    QP(h) = f_md;
                    QN(h) = f_node;
#pragma unroll
                    for (int a = 0; a < M; ++a) QS(h, a) = f_side[a];
                }
            }
        }
        if (over) {
            atomicOr(overflow, 1);
            for (int i = 0; i < kk; ++i) ids_out[(size_t)r * kk + i] = -1;
            continue;
        }
        // nearest first: the heap gives them farthest first
        const int found = nn;
        for (int i = found; i < kk; ++i) ids_out[(size_t)r * kk + i] = -1;
        for (int i = found - 1; i >= 0; --i) {
            ids_out[(size_t)r * kk + i] = (long long)NI(0);
            const double mp = NP(nn - 1);
            const int mi = NI(nn - 1);
            --nn;
            int h = 0;
            for (;;) {
                const int j = 2 * h + 1, k2 = 2 * h + 2;
                const double pj = j < nn ? NP(j) : 0.0, pk = k2 < nn ? NP(k2) : 0.0;
                if (!((j < nn && mp > pj) || (k2 < nn && mp > pk))) break;
                const int l = (k2 < nn && pj > pk) ? k2 : j;
                NP(h) = l == j ? pj : pk;
                NI(h) = NI(l);
                h = l;
            }
            if (nn > 0) { NP(h) = mp; NI(h) = mi; }
        }
    }
}
}  // namespace

int kd_queries_device(const double* coords_dev, int dim, int kk, const KdDeviceTree& tree, const long long* rows_host, long long nq,
                      long long* ids_dev, int* over, hipStream_t st) {
    const int4* meta_d = tree.meta.as<int4>();
    const double* split_d = tree.split.as<double>();
    const int* idx_d = tree.idx.as<int>();
    const long long L = std::min<long long>((nq + 255) / 256, 1024) * 256;   // (twice the lanes in flight - the kernel has the registers for it - measured no faster: 1.85 ms either way)
    DevBuf d_rows, d_over, qp, qnode, qs, np, ni;
    PinnedScope stage;
    FDX_TRY(d_over.alloc(4));
    FDX_TRY(qp.alloc((size_t)KD_QCAP * L * 8));
    FDX_TRY(qnode.alloc((size_t)KD_QCAP * L * 4));
    FDX_TRY(qs.alloc((size_t)KD_QCAP * dim * L * 8));
    FDX_TRY(np.alloc((size_t)kk * L * 8));
    FDX_TRY(ni.alloc((size_t)kk * L * 4));
    FDX_HIP(hipMemsetAsync(d_over.p, 0, 4, st));
    if (rows_host) {
        FDX_TRY(stage.get((size_t)nq * 8));
        std::memcpy(stage.p, rows_host, (size_t)nq * 8);
        FDX_TRY(d_rows.alloc((size_t)nq * 8));
        FDX_HIP(hipMemcpyAsync(d_rows.p, stage.p, (size_t)nq * 8, hipMemcpyHostToDevice, st));
    }
    KdBounds bnd{};
    for (int a = 0; a < dim; ++a) { bnd.mins[a] = tree.mins[a]; bnd.maxes[a] = tree.maxes[a]; }
    const dim3 grid((unsigned)(L / 256)), blk(256);
    const long long* rows_d = rows_host ? d_rows.as<long long>() : nullptr;
    const bool nbl = kk <= 16;
    const size_t nb_lds = nbl ? (size_t)kk * 256 * 12 : 0;
#define FDX_KD_LAUNCH(MM)                                                                                                              \
    do {                                                                                                                               \
        if (nbl)                                                                                                                       \
            hipLaunchKernelGGL((kd_query_kernel<MM, true>), grid, blk, nb_lds, st, coords_dev, meta_d, split_d, idx_d, bnd, kk, rows_d, nq,   \
                               ids_dev, qp.as<double>(), qnode.as<int>(), qs.as<double>(), np.as<double>(), ni.as<int>(), L, d_over.as<int>()); \
        else                                                                                                                           \
            hipLaunchKernelGGL((kd_query_kernel<MM, false>), grid, blk, 0, st, coords_dev, meta_d, split_d, idx_d, bnd, kk, rows_d, nq,       \
                               ids_dev, qp.as<double>(), qnode.as<int>(), qs.as<double>(), np.as<double>(), ni.as<int>(), L, d_over.as<int>()); \
    } while (0)
    if (dim == 1) FDX_KD_LAUNCH(1);
    else if (dim == 2) FDX_KD_LAUNCH(2);
    else FDX_KD_LAUNCH(3);
#undef FDX_KD_LAUNCH
    FDX_CHECK_LAUNCH();
    *over = 0;
    FDX_HIP(hipMemcpyAsync(over, d_over.p, 4, hipMemcpyDeviceToHost, st));
    FDX_HIP(hipStreamSynchronize(st));                     // the staging and the work areas are this function's; the flag decides the route
    return 0;
}

}  // namespace fdx
