// Gene-pair spatial co-expression (additive, not in the reference): per pair (a, b) of columns of a spot-by-gene matrix Y (n, G) the
// seventeen sums from which the bivariate Moran's R, Pearson's r and the exact permutation variances of R are assembled on the host
// (flashdeconv_amd/utils/gene_pairs.py), and the local score per spot and pair, over the model's graph - A its symmetric binary
// adjacency, deg_i = sum_j A_ij, lag_g,i = sum_{j in N(i)} y_jg in the graph's stored neighbour order.  Planes of the (17, P)
// result, everything float64 on the value converted from storage:
//   0 ua = sum y_a    1 ub = sum y_b    2 qa = sum y_a^2    3 qb = sum y_b^2    4 Da = sum deg y_a    5 Db = sum deg y_b
//   6 S = sum y_a y_b     7 Xab = sum y_a lag_b     8 Xba = sum y_b lag_a
//   9 La = sum lag_a^2    10 Lb = sum lag_b^2       11 DLa = sum deg lag_a     12 DLb = sum deg lag_b
//   13 amin   14 amax   15 bmin   16 bmax
// include/fdx.h has the definitions.
//
// Order of the sums: that of the gene spatial sums (gene_spatial_kernels.cpp) - segments of FDX_GENE_SPATIAL_SEGMENT_POSITIONS
// positions of the graph's order, a segment summed position after position into zeroed accumulators, the segment sums folded in
// ascending order (planes 13-16: the smaller / larger kept); gene_pass.h has the rule for what changes no bit of it.  A thread owns
// ONE pair - a workgroup 256 pairs - and reads the columns a and b of the row and of its neighbours through the walk of
// gene_walk.h; nothing is shared between pairs and there are no floating-point atomics, so A PAIR'S RESULT DEPENDS ONLY ON THE
// GRAPH AND ITS TWO COLUMNS, never on which other pairs share the call, on their order or on how a CSR call was cut into chunks.
// That is also why the host may hand the sums kernel the pairs sorted by column (neighbouring threads then read neighbouring
// columns of a row) and have every pair's sums written where the caller listed it.
//
// The local kernel takes the same walk and the same sorted pairs and writes, instead of accumulating, the pair's score of the row
// to out[row * ldo + p], p the pair's place in the caller's list.
//
// CSR: the distinct genes of a chunk of pairs are gathered into a dense (n, S) matrix of the storage type - one pass over the stored
// entries with a G-sized column-to-slot map; an entry that is not stored is the value 0 - and the dense kernels run on it with
// remapped indices.  The chunks are cut on the host so that the gathered matrix stays within max_gather_bytes.
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

constexpr int GP_PAIRS = 256;                                // pairs of a workgroup, one per thread
constexpr int GP_PLANES = 17, GP_SUM_PLANES = 13;            // planes 13 .. 16: amin, amax, bmin, bmax

// part[s][plane][p] for the segments seg0 + s, s < n_seg, of this launch; workgroup x takes segments [x * stripe, (x + 1) * stripe),
// workgroup row y the pairs [256 y, 256 y + 256) of `pairs`, which the host sorted by column (a wave's reads of a row then share
// cache lines); pair p of that order is the call's pair where[p], and that is where its sums go.  deg_part: null, or the segments'
// {sum deg, sum deg^2} (written by row 0).
template <typename T>
__global__ __launch_bounds__(256) void gp_dense_kernel(const T* __restrict__ Y, long long ldy, GraphTables g, int seg0, int n_seg,
                                                       int stripe, const int2* __restrict__ pairs, const int* __restrict__ where, int P,
                                                       double* __restrict__ part, long long* __restrict__ deg_part) {
    __shared__ GsSegmentTables sh;
    __shared__ long long red[2][4];
    const int p = blockIdx.y * GP_PAIRS + threadIdx.x;
    const bool ok = p < P;
    const int2 ab = ok ? pairs[p] : make_int2(0, 0);
    const int dst = ok ? where[p] : 0;
    const T* yap = Y + ab.x;
    const T* ybp = Y + ab.y;
    const bool owner = blockIdx.y == 0 && deg_part != nullptr;
    const int s0 = blockIdx.x * stripe, s1 = min(n_seg, s0 + stripe);
    for (int s = s0; s < s1; ++s) {
        const int p0 = (seg0 + s) * GS_SEG;
        const int cnt = min(GS_SEG, g.n - p0);
        gs_stage_segment(g, p0, p0 + cnt, sh, red, owner, nullptr, owner ? deg_part + 2 * (size_t)(seg0 + s) : nullptr);
        double ua = 0.0, ub = 0.0, qa = 0.0, qb = 0.0, Da = 0.0, Db = 0.0, S = 0.0, Xab = 0.0, Xba = 0.0;
        double La = 0.0, Lb = 0.0, DLa = 0.0, DLb = 0.0;
        double amin = INFINITY, amax = -INFINITY, bmin = INFINITY, bmax = -INFINITY;
        gs_walk_segment(yap, ybp, ldy, g, p0, cnt, sh, [&](int, int dg, double ya, double yb, double laga, double lagb) {
            const double d = (double)dg;
            ua += ya;                 ub += yb;
            qa += ya * ya;            qb += yb * yb;
            Da += d * ya;             Db += d * yb;
            S += ya * yb;
            Xab += ya * lagb;         Xba += yb * laga;
            La += laga * laga;        Lb += lagb * lagb;
            DLa += d * laga;          DLb += d * lagb;
            amin = fmin(amin, ya);    bmin = fmin(bmin, yb);
            amax = fmax(amax, ya);    bmax = fmax(bmax, yb);
        });
        if (ok) {
            double* out = part + (size_t)s * GP_PLANES * P + dst;
            const double v[GP_PLANES] = {ua, ub, qa, qb, Da, Db, S, Xab, Xba, La, Lb, DLa, DLb, amin, amax, bmin, bmax};
#pragma unroll
            for (int k = 0; k < GP_PLANES; ++k) out[(size_t)k * P] = v[k];
        }
    }
}

// out[row * ldo + q] = coef_q [(y_a - mean_a_q)(lag_b - mean_b_q deg) + (y_b - mean_b_q)(lag_a - mean_a_q deg)] for every row (the
// caller's order) and pair, q = where[p] the place of the sorted pair p in the caller's list; the grid of gp_dense_kernel over all
// segments.
template <typename T>
__global__ __launch_bounds__(256) void gp_local_kernel(const T* __restrict__ Y, long long ldy, GraphTables g, int n_seg, int stripe,
                                                       const int2* __restrict__ pairs, const int* __restrict__ where, int P,
                                                       const double* __restrict__ mean_a, const double* __restrict__ mean_b,
                                                       const double* __restrict__ coef,
                                                       double* __restrict__ out, long long ldo) {
    __shared__ GsSegmentTables sh;
    __shared__ long long red[2][4];
    const int p = blockIdx.y * GP_PAIRS + threadIdx.x;
    const bool ok = p < P;
    const int2 ab = ok ? pairs[p] : make_int2(0, 0);
    const T* yap = Y + ab.x;
    const T* ybp = Y + ab.y;
    const int dst = ok ? where[p] : 0;
    const double ma = ok ? mean_a[dst] : 0.0, mb = ok ? mean_b[dst] : 0.0, cf = ok ? coef[dst] : 0.0;
    const int s0 = blockIdx.x * stripe, s1 = min(n_seg, s0 + stripe);
    for (int s = s0; s < s1; ++s) {
        const int p0 = s * GS_SEG;
        const int cnt = min(GS_SEG, g.n - p0);
        gs_stage_segment(g, p0, p0 + cnt, sh, red, false, nullptr, nullptr);
        gs_walk_segment(yap, ybp, ldy, g, p0, cnt, sh, [&](int r, int dg, double ya, double yb, double laga, double lagb) {
            const double d = (double)dg;
            if (ok) out[(long long)sh.row[r] * ldo + dst] = cf * ((ya - ma) * (lagb - mb * d) + (yb - mb) * (laga - ma * d));
        });
    }
}

// dense (n, S) = the columns of the CSR matrix that slot_of (G ints, -1: not wanted) sends to a slot; dense was zeroed.  A wave per
// row, a lane per stored entry: the entries of a row have distinct columns, so every element has one writer.
template <typename T>
__global__ __launch_bounds__(256) void gp_gather_kernel(const long long* __restrict__ indptr, const int* __restrict__ indices,
                                                        const T* __restrict__ values, long long n, int G, const int* __restrict__ slot_of,
                                                        int S, T* __restrict__ dense) {
    const int lane = threadIdx.x & 63;
    for (long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); row < n; row += (long long)gridDim.x * 4) {
        const long long e1 = indptr[row + 1];
        for (long long e = indptr[row] + lane; e < e1; e += 64) {
            const int c = indices[e];
            const int slot = (unsigned)c < (unsigned)G ? slot_of[c] : -1;
            if (slot >= 0) dense[row * S + slot] = values[e];
        }
    }
}

// What a call leaves behind: the sums (local == false) or the local scores.
struct PairOutput {
    bool local = false;
    double* sums = nullptr;                                  // (17, P) device
    int64_t* counts_out = nullptr;                           // host
    const double *mean_a = nullptr, *mean_b = nullptr, *coef = nullptr;   // P each, device
    double* out = nullptr;                                   // (n, ldo) device
    long long ldo = 0;
};

// The pairs [q0, q0 + Pc) of the call over the dense matrix Yd (`pairs`: the HOST array of the call's P pairs, indices into Yd's
// columns), queued on st.  Sums: folded into columns q0 .. of o.sums; deg_part (null: not wanted) receives the segments' degree sums.
template <typename T>
int run_dense_pairs(const GraphTables& t, const T* Yd, long long ldy, const int32_t* pairs, int q0, int Pc, int P, const PairOutput& o,
                    long long* deg_part, hipStream_t st) {
    const int n_seg = ceil_div(t.n, GS_SEG), stripe = stripe_segments();
    const unsigned rows = (unsigned)ceil_div(Pc, GP_PAIRS);
    const int32_t* mine = pairs + 2 * (size_t)q0;
    DevBuf pairs_buf;
    FDX_TRY(pairs_buf.alloc(3 * (size_t)Pc * sizeof(int)));
    // sorted by (a, b): changes no bit - a pair's numbers are its own - and took the 1,000-pair sums from 56 to 47 ms
    std::vector<int> host(3 * (size_t)Pc);
    int* where = host.data() + 2 * (size_t)Pc;
    for (int p = 0; p < Pc; ++p) where[p] = p;
    std::sort(where, where + Pc, [&](int x, int y) {
        const int ax = mine[2 * (size_t)x], ay = mine[2 * (size_t)y];
        return ax != ay ? ax < ay : mine[2 * (size_t)x + 1] != mine[2 * (size_t)y + 1] ? mine[2 * (size_t)x + 1] < mine[2 * (size_t)y + 1] : x < y;
    });
    for (int p = 0; p < Pc; ++p) {
        host[2 * (size_t)p] = mine[2 * (size_t)where[p]];
        host[2 * (size_t)p + 1] = mine[2 * (size_t)where[p] + 1];
    }
    FDX_TRY(copy_h2d(pairs_buf.p, host.data(), host.size() * sizeof(int), st));
    if (o.local) {
        hipLaunchKernelGGL(gp_local_kernel, dim3((unsigned)ceil_div(n_seg, stripe), rows), dim3(256), 0, st, Yd, ldy, t, n_seg, stripe,
                           pairs_buf.as<int2>(), pairs_buf.as<int>() + 2 * (size_t)Pc, Pc, o.mean_a + q0, o.mean_b + q0, o.coef + q0,
                           o.out + q0, o.ldo);
        FDX_CHECK_LAUNCH();
        return 0;
    }
    return for_segment_batches(n_seg, (size_t)GP_PLANES * Pc * sizeof(double), [&](int sb0, int nb, double* part) {
        hipLaunchKernelGGL(gp_dense_kernel, dim3((unsigned)ceil_div(nb, stripe), rows), dim3(256), 0, st, Yd, ldy, t, sb0, nb, stripe,
                           pairs_buf.as<int2>(), pairs_buf.as<int>() + 2 * (size_t)Pc, Pc, part, deg_part);
        FDX_CHECK_LAUNCH();
        // the fold takes one min and one max plane a call: planes 0 .. 14 (13 amin, 14 amax), then 15 bmin and 16 bmax
        const SegmentBlocks b{part, (long long)GP_PLANES * Pc, (long long)Pc, 1LL, sb0, nb};
        FDX_TRY(launch_gene_fold(b, 0, GP_SUM_PLANES + 2, Pc, nullptr, 1, o.sums + q0, 0, (long long)P, GP_SUM_PLANES, GP_SUM_PLANES + 1, st));
        return launch_gene_fold(b, GP_SUM_PLANES + 2, 2, Pc, nullptr, 1, o.sums + (size_t)(GP_SUM_PLANES + 2) * P + q0, 0, (long long)P, 0, 1,
                                st);
    });
}

// The CSR route: chunks of consecutive pairs whose distinct genes fit the gather budget, each gathered and run densely.
template <typename T>
int run_csr_pairs(const GraphTables& t, const fdx_csr_view* Y, const T* values, const int32_t* pairs, int P, size_t max_gather_bytes,
                  const PairOutput& o, long long* deg_part, hipStream_t st) {
    const size_t budget = max_gather_bytes ? max_gather_bytes : SCRATCH_BUDGET_BYTES;
    const size_t row_bytes = (size_t)t.n * sizeof(T);
    const int cap = (int)std::min<size_t>((size_t)std::min<long long>(2LL * P, Y->G), std::max<size_t>(2, budget / row_bytes));
    // the chunks and, per pair, its two slots in its chunk's gathered matrix
    struct Chunk { int q0; std::vector<int> genes; };            // pairs [q0, the next chunk's q0) and their genes in slot order
    std::vector<Chunk> chunks(1, Chunk{0, {}});
    std::vector<int> slot_of((size_t)Y->G, -1), local(2 * (size_t)P);
    for (int p = 0; p < P; ++p) {
        const int a = pairs[2 * (size_t)p], b = pairs[2 * (size_t)p + 1];
        const int need = (slot_of[a] < 0) + (b != a && slot_of[b] < 0);
        if ((int)chunks.back().genes.size() + need > cap && p > chunks.back().q0) {     // (a chunk holds one pair at the least)
            for (int c : chunks.back().genes) slot_of[c] = -1;
            chunks.push_back(Chunk{p, {}});
        }
        for (int c : {a, b})
            if (slot_of[c] < 0) {
                slot_of[c] = (int)chunks.back().genes.size();
                chunks.back().genes.push_back(c);
            }
        local[2 * (size_t)p] = slot_of[a];
        local[2 * (size_t)p + 1] = slot_of[b];
    }
    DevBuf map_buf, dense;
    FDX_TRY(map_buf.alloc((size_t)Y->G * sizeof(int)));
    FDX_TRY(dense.alloc((size_t)cap * row_bytes));
    for (size_t c = 0; c < chunks.size(); ++c) {
        const int S = (int)chunks[c].genes.size();
        std::fill(slot_of.begin(), slot_of.end(), -1);
        for (int s = 0; s < S; ++s) slot_of[chunks[c].genes[s]] = s;
        FDX_TRY(copy_h2d(map_buf.p, slot_of.data(), slot_of.size() * sizeof(int), st));
        FDX_HIP(hipMemsetAsync(dense.p, 0, (size_t)S * row_bytes, st));
        hipLaunchKernelGGL(gp_gather_kernel, dim3((unsigned)std::min<long long>(ceil_div(t.n, 4), 1 << 16)), dim3(256), 0, st,
                           (const long long*)Y->indptr, Y->indices, values, (long long)t.n, Y->G, map_buf.as<int>(), S, dense.as<T>());
        FDX_CHECK_LAUNCH();
        const int q0 = chunks[c].q0, Pc = (c + 1 < chunks.size() ? chunks[c + 1].q0 : P) - q0;
        FDX_TRY(run_dense_pairs(t, dense.as<T>(), (long long)S, local.data(), q0, Pc, P, o, c == 0 ? deg_part : nullptr, st));
    }
    return 0;
}

int gene_pair_entry(const char* who, const fdx_graph* g, const GeneMatrix& y, const int32_t* pairs, int32_t P, size_t max_gather_bytes,
                    const PairOutput& o, void* stream) {
    const std::string w(who);
    hipStream_t st = (hipStream_t)stream;
    const bool outputs = o.local ? (o.mean_a && o.mean_b && o.coef && o.out) : (o.sums && o.counts_out);
    FDX_TRY(check_gene_matrix(who, y, g && pairs && outputs, false, "ldy < G"));
    FDX_REQUIRE(y.G >= 1, w + ": G must be at least 1");
    FDX_REQUIRE(P >= 1, w + ": P must be at least 1");
    FDX_REQUIRE(P <= GP_PAIRS * 65535, w + ": too many pairs for one call");
    for (long long i = 0; i < 2LL * P; ++i) FDX_REQUIRE(pairs[i] >= 0 && pairs[i] < y.G, w + ": pair index out of range");
    FDX_REQUIRE(!o.local || o.ldo >= P, w + ": ldo < P");
    FDX_REQUIRE(y.n >= 0 && y.n < (1LL << 31) - 128, w + ": n must be between 0 and 2^31 - 129");
    GraphTables t;
    FDX_TRY(whole_graph_tables(g, who, &t));
    FDX_REQUIRE(y.n == t.n, w + ": Y has " + std::to_string(y.n) + " rows but the graph has " + std::to_string(t.n) + " spots");
    PoolStream pool_stream(st);
    if (!o.local) {
        o.counts_out[0] = t.n;
        o.counts_out[1] = o.counts_out[2] = 0;
    }
    if (t.n == 0) {                                 // empty sums; no value to be the smallest or the largest; no row to score
        if (o.local) return 0;
        std::vector<double> h((size_t)GP_PLANES * P, 0.0);
        std::fill(h.begin() + (size_t)GP_SUM_PLANES * P, h.end(), std::numeric_limits<double>::quiet_NaN());
        FDX_TRY(copy_h2d(o.sums, h.data(), h.size() * sizeof(double), st));
        FDX_HIP(hipStreamSynchronize(st));
        return 0;
    }
    const int n_seg = ceil_div(t.n, GS_SEG);
    DevBuf deg_buf, counts;
    long long* deg_part = nullptr;
    if (!o.local) {
        FDX_TRY(deg_buf.alloc((size_t)n_seg * 2 * sizeof(long long)));
        FDX_TRY(counts.alloc(2 * sizeof(long long)));
        deg_part = deg_buf.as<long long>();
    }
    FDX_TRY(dispatch_gene_matrix(
        y,
        [&](auto* Yd) { return run_dense_pairs(t, Yd, y.ldy, pairs, 0, P, P, o, deg_part, st); },
        [&](auto* values) { return run_csr_pairs(t, y.csr, values, pairs, P, max_gather_bytes, o, deg_part, st); }));
    if (o.local) return 0;
    FDX_TRY(launch_segment_degree_counts(deg_part, n_seg, counts.as<long long>(), st));
    long long host[2];
    FDX_TRY(copy_d2h(host, counts.p, sizeof(host), st));         // the call's one host synchronisation
    o.counts_out[1] = host[0];
    o.counts_out[2] = host[1];
    return 0;
}

PairOutput sums_output(double* sums_dev, int64_t* counts_out) {
    PairOutput o;
    o.sums = sums_dev;
    o.counts_out = counts_out;
    return o;
}

PairOutput local_output(const double* mean_a, const double* mean_b, const double* coef, double* out_dev, int64_t ldo) {
    PairOutput o;
    o.local = true;
    o.mean_a = mean_a;
    o.mean_b = mean_b;
    o.coef = coef;
    o.out = out_dev;
    o.ldo = ldo;
    return o;
}

}  // namespace
}  // namespace fdx

using namespace fdx;

extern "C" {

int fdx_gene_pair_sums_dev(const fdx_graph* g, const void* Y_dev, int32_t dtype, int64_t n, int32_t G, int64_t ldy, const int32_t* pairs,
                           int32_t P, double* sums_dev, int64_t* counts_out, void* stream) {
    return gene_pair_entry("fdx_gene_pair_sums_dev", g, GeneMatrix(Y_dev, dtype, n, G, ldy), pairs, P, 0, sums_output(sums_dev, counts_out),
                           stream);
}

int fdx_gene_pair_sums_csr_dev(const fdx_graph* g, const fdx_csr_view* Y, const int32_t* pairs, int32_t P, int64_t max_gather_bytes,
                               double* sums_dev, int64_t* counts_out, void* stream) {
    return gene_pair_entry("fdx_gene_pair_sums_csr_dev", g, GeneMatrix(Y), pairs, P, max_gather_bytes > 0 ? (size_t)max_gather_bytes : 0,
                           sums_output(sums_dev, counts_out), stream);
}

int fdx_gene_pair_local_dev(const fdx_graph* g, const void* Y_dev, int32_t dtype, int64_t n, int32_t G, int64_t ldy, const int32_t* pairs,
                            int32_t P, const double* mean_a_dev, const double* mean_b_dev, const double* coef_dev, double* out_dev,
                            int64_t ldo, void* stream) {
    return gene_pair_entry("fdx_gene_pair_local_dev", g, GeneMatrix(Y_dev, dtype, n, G, ldy), pairs, P, 0,
                           local_output(mean_a_dev, mean_b_dev, coef_dev, out_dev, ldo), stream);
}

int fdx_gene_pair_local_csr_dev(const fdx_graph* g, const fdx_csr_view* Y, const int32_t* pairs, int32_t P, int64_t max_gather_bytes,
                                const double* mean_a_dev, const double* mean_b_dev, const double* coef_dev, double* out_dev, int64_t ldo,
                                void* stream) {
    return gene_pair_entry("fdx_gene_pair_local_csr_dev", g, GeneMatrix(Y), pairs, P, max_gather_bytes > 0 ? (size_t)max_gather_bytes : 0,
                           local_output(mean_a_dev, mean_b_dev, coef_dev, out_dev, ldo), stream);
}

}  // extern "C"
