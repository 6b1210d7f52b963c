// Per-label gene sums under permuted labels: the device half of the ligand-receptor test between spot groups (additive, not in the
// reference; flashdeconv_amd/utils/ligrec.py has the definitions, include/fdx.h the contract).  With l_i in {-1, 0 .. C - 1} the label
// of spot i, `genes` the S distinct columns the pairs name and l^r_i = l[pi_r(i)] (pi_r: the keyed bijection of perm_device.h):
//   u^r[c, s] = sum_{i : l^r_i = c} y[i, genes[s]]        float64 on the value converted from storage; the observed u: the identity
//   T^r[p, a, b] = (u^r[a, lig_p] / n_a + u^r[b, rec_p] / n_b) * 0.5
// and per (p, a, b), over the call's permutations in order, #{T^r >= T}, #{T^r <= T}, sum d, sum d^2 with d = T^r - T.  No graph.
//
//   prepare    label_stage.h: labels -> one byte per spot (LP_NONE for -1), the range check, n_c
//   stage      label_stage.h: the bytes of a group of B = 16 permutations interleaved per spot, in the caller's spot order
//   gather     gene_gather.h: the S columns in the storage type, spot-major in tiles of TS = 16 genes (one spot's tile: 64 bytes of
//              float32); CSR through the scatter route; a copy above max_gather_bytes (default SCRATCH_BUDGET_BYTES) goes in stripes
//   null       a workgroup of 256 threads owns a tile of TS genes, a group of B permutations and a SEGMENT of LG_SEG = 2048 spots.
//              Thread (j, s) alone owns the LDS cells acc[c][j][s], c < C: for every spot of the segment in ascending order it adds
//              y[i, s] into acc[byte of (i, j)][j][s] - a plain read-add-write of a cell no other thread touches.  No floating-point
//              atomics, no barrier, a fixed order.  An exact zero is skipped (y == 0, so -0.0 as well): adding +-0.0 to a sum that
//              began as +0.0 changes no bit of it, whatever the sign of the other values, so the skip is not visible in the result;
//              negative values are added like any other.  (A column of nothing but -0.0 sums to +0.0.)  The cells go to
//              part[segment][r][c][s]; the fold of gene_pass.h adds the segments in ascending order into u^r.
//   nnz        #{i in c : y != 0} of the observed labels: 32-bit integer atomics in LDS, 64-bit to global (integers: order-free)
//   accumulate one thread per (p, a, b) in permutation order: two IEEE divisions, one addition, one multiplication by 0.5 for T^r, the
//              subtraction, then sum_d += d and sumsq_d += d * d with the square rounded on its own (__dmul_rn, then __dadd_rn: NOT
//              contracted into an fma, as NumPy adds the rounded squares).  Where n_a < 1 or n_b < 1 nothing is counted or added.
//
// LDS: C * B * TS * 8 = 2 KiB per label (C = 10: 20 KiB, eight workgroups - the CU's 32 waves; C = 16: 32 KiB, five; C = 32: 64 KiB,
// two; C = 64: 128 KiB, one workgroup of four waves).  One shape for every C: the cells a CU holds, 160 KiB / (8 C), bound the threads
// that can work whatever the workgroup, so a second shape for large C would buy nothing.  Banks: lane = 16 j + s, so a half-wave
// of a ds_read_b64 is the pair of permutations (2k, 2k + 1), each reading 16 consecutive doubles at dword offset
// 512 c + 32 j + 2 s: mod 64 the even j covers banks 0 .. 31 and the odd j banks 32 .. 63 whatever their labels c are, and a 16-lane
// group of a ds_write_b64 is one j with 32 consecutive dwords.  The rows therefore need no padding: the plain layout is conflict-free.
//
// Order: every u^r[c, s] is the segments' sums added in ascending order, a segment's sum its spots added in ascending order.  The
// segment length is a constant, so u^r DEPENDS ONLY ON THE LABELS, THE COLUMN AND THE PERMUTATION - not on the tile, the batch,
// max_batch, the stripe, the other genes, the other pairs or how a range of permutations is split into calls.
#include <algorithm>
#include <vector>

#include "fdx_internal.h"
#include "gene_gather.h"
#include "gene_pass.h"
#include "label_gene_plan.h"
#include "label_stage.h"
#include "perm_device.h"

namespace fdx {
namespace {

// (label_gene_plan.h: the constants of the shape - LG_B, LG_TS, LG_SEG ... - and the plan of a call, plain host code)

// part[(seg * rows + r) * C + c][tile * TS + s] for the tiles of a stripe (width W genes), r < nb the permutation of the batch
template <typename T>
__global__ __launch_bounds__(LG_THREADS) void lg_null_kernel(const T* __restrict__ Yt, const unsigned char* __restrict__ Lr, int n, int C,
                                                             int nb, int rows, int W, double* __restrict__ part) {
    extern __shared__ double lg_acc[];                          // [c][j][s]: thread t = 16 j + s owns lg_acc[c * 256 + t]
    const int t = threadIdx.x, j = t >> 4, s = t & (LG_TS - 1);
    const int r = blockIdx.x * LG_B + j;
    if (r >= nb) return;                                        // past the batch (no barrier below: a thread shares nothing)
    for (int c = 0; c < C; ++c) lg_acc[c * LG_THREADS + t] = 0.0;
    const int i0 = blockIdx.z * LG_SEG, i1 = min(n, i0 + LG_SEG);
    const T* col = Yt + ((size_t)blockIdx.y * n + i0) * LG_TS + s;
    const unsigned char* lab = Lr + ((size_t)blockIdx.x * n + i0) * LG_B + j;
    const int len = i1 - i0;
    int k = 0;
    for (; k + 8 <= len; k += 8) {                              // eight loads of each kind in flight, added one after the other
        T y[8];
        unsigned l[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            y[e] = col[(size_t)(k + e) * LG_TS];
            l[e] = lab[(size_t)(k + e) * LG_B];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (y[e] != (T)0 && l[e] != LP_NONE) lg_acc[l[e] * LG_THREADS + t] += (double)y[e];
    }
    for (; k < len; ++k) {
        const T y = col[(size_t)k * LG_TS];
        const unsigned l = lab[(size_t)k * LG_B];
        if (y != (T)0 && l != LP_NONE) lg_acc[l * LG_THREADS + t] += (double)y;
    }
    double* out = part + (((size_t)blockIdx.z * rows + r) * C) * W + (size_t)blockIdx.y * LG_TS + s;
    for (int c = 0; c < C; ++c) out[(size_t)c * W] = lg_acc[c * LG_THREADS + t];
}

// nnz[c * S + s0 + w] += #{i of the segment with byte c : Yt[tile][i][w] != 0}; grid (tiles, segments)
template <typename T>
__global__ __launch_bounds__(LG_THREADS) void lg_nnz_kernel(const T* __restrict__ Yt, const unsigned char* __restrict__ codes, int n, int C,
                                                            int s0, int S, unsigned long long* __restrict__ nnz) {
    __shared__ unsigned hist[LP_MAX_LABELS * LG_TS];
    for (int i = threadIdx.x; i < C * LG_TS; i += LG_THREADS) hist[i] = 0u;
    __syncthreads();
    const int s = threadIdx.x & (LG_TS - 1);
    const int i0 = blockIdx.y * LG_SEG, i1 = min(n, i0 + LG_SEG);
    const T* col = Yt + (size_t)blockIdx.x * n * LG_TS + s;
    for (int i = i0 + (int)(threadIdx.x >> 4); i < i1; i += LG_THREADS / LG_TS) {
        const unsigned l = codes[i];
        if (l != LP_NONE && col[(size_t)i * LG_TS] != (T)0) atomicAdd(&hist[l * LG_TS + s], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C * LG_TS; i += LG_THREADS) {
        const int gene = s0 + (int)blockIdx.x * LG_TS + (i & (LG_TS - 1));
        if (hist[i] && gene < S) atomicAdd(&nnz[(size_t)(i / LG_TS) * S + gene], (unsigned long long)hist[i]);
    }
}

// T[p, a, b] of the sums u (C, S): one IEEE division per mean, one addition, one multiplication by 0.5
__device__ __forceinline__ double lg_statistic(const double* __restrict__ u, int S, int a, int b, int lig, int rec, double na, double nb) {
    return __dmul_rn(__dadd_rn(__ddiv_rn(u[(size_t)a * S + lig], na), __ddiv_rn(u[(size_t)b * S + rec], nb)), 0.5);
}

// the batch's T^r against the observed T, one thread per (p, a, b), in permutation order; U (batch, C, S)
__global__ __launch_bounds__(256) void lg_accum_kernel(const double* __restrict__ U, int batch, const double* __restrict__ u_obs,
                                                       const long long* __restrict__ label_counts, const int* __restrict__ slots, int C, int S,
                                                       long long X, long long* __restrict__ count_ge, long long* __restrict__ count_le,
                                                       double* __restrict__ sum_d, double* __restrict__ sumsq_d) {
    const long long x = (long long)blockIdx.x * 256 + threadIdx.x;
    if (x >= X) return;
    const int b = (int)(x % C), a = (int)((x / C) % C);
    const long long p = x / ((long long)C * C);
    const long long ca = label_counts[a], cb = label_counts[b];
    if (ca < 1 || cb < 1) return;                               // an empty group: nothing counted, nothing added
    const double na = (double)ca, nb = (double)cb;
    const int lig = slots[2 * p], rec = slots[2 * p + 1];
    const double t0 = lg_statistic(u_obs, S, a, b, lig, rec, na, nb);
    long long ge = count_ge[x], le = count_le[x];
    double sd = sum_d[x], sq = sumsq_d[x];
    for (int r = 0; r < batch; ++r) {
        const double tr = lg_statistic(U + (size_t)r * C * S, S, a, b, lig, rec, na, nb);
        const double d = __dsub_rn(tr, t0);
        ge += tr >= t0 ? 1 : 0;
        le += tr <= t0 ? 1 : 0;
        sd = __dadd_rn(sd, d);
        sq = __dadd_rn(sq, __dmul_rn(d, d));                    // the sum of the rounded squares: no fma
    }
    count_ge[x] = ge;
    count_le[x] = le;
    sum_d[x] = sd;
    sumsq_d[x] = sq;
}

struct LgRequest {
    const int32_t *labels, *genes, *pairs;
    int C, S, P;
    unsigned long long seed;
    long long first_perm, n_perm;
    double* null_dev;
};

// the sums of nb permutations of the staged groups over the stripe's tiles, folded into U (rows of C * S, the stripe at column s0)
template <typename T>
int lg_sums(const LgPlan& plan, const T* Yt, const unsigned char* Lr, int n, int C, int S, int s0, int tiles, int nb, double* part, double* U,
            hipStream_t st) {
    auto* kernel = lg_null_kernel<T>;
    if (plan.lds > 64 * 1024) FDX_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));
    hipLaunchKernelGGL(kernel, dim3((unsigned)ceil_div(nb, LG_B), (unsigned)tiles, (unsigned)plan.nseg), dim3(LG_THREADS), plan.lds, st, Yt, Lr,
                       n, C, nb, plan.batch, plan.W, part);
    FDX_CHECK_LAUNCH();
    const SegmentBlocks blocks{part, (long long)plan.batch * C * plan.W, (long long)plan.W, 1, 0, plan.nseg};
    return launch_gene_fold(blocks, 0, nb * C, std::min(tiles * LG_TS, S - s0), nullptr, 1, U + s0, 0, S, -1, -1, st);
}

// Everything of a call, queued on st; out: plan.words words
template <typename T>
int lg_run(const LgPlan& plan, const GeneMatrix& y, const T* data, const LgRequest& q, long long* out, hipStream_t st) {
    const int n = (int)y.n, C = q.C, S = q.S;
    DevBuf yt_buf, list_buf, slot_buf, codes_buf, lr_buf, part_buf, u_buf;
    FDX_TRY(yt_buf.alloc(plan.tile_copy_bytes(n, sizeof(T))));
    FDX_TRY(codes_buf.alloc((size_t)n));
    FDX_TRY(lr_buf.alloc(plan.stage_bytes(n)));
    FDX_TRY(part_buf.alloc(plan.part_bytes(C)));
    if (!q.null_dev && q.n_perm > 0) FDX_TRY(u_buf.alloc(plan.u_bytes(C, S)));
    std::vector<int> list;                                      // dense: the genes; CSR: the column-to-slot map
    if (y.sparse) {
        list.assign((size_t)y.G, -1);
        for (int s = 0; s < S; ++s) list[q.genes[s]] = s;
    } else {
        list.assign(q.genes, q.genes + S);
    }
    FDX_TRY(list_buf.alloc(list.size() * sizeof(int)));
    FDX_TRY(copy_h2d(list_buf.p, list.data(), list.size() * sizeof(int), st));
    std::vector<int> slots((size_t)2 * q.P);                    // the pairs as places in `genes` (the entry has checked them)
    for (size_t k = 0; k < slots.size(); ++k) slots[k] = (int)(std::lower_bound(q.genes, q.genes + S, q.pairs[k]) - q.genes);
    FDX_TRY(slot_buf.alloc(slots.size() * sizeof(int)));
    FDX_TRY(copy_h2d(slot_buf.p, slots.data(), slots.size() * sizeof(int), st));

    T* Yt = yt_buf.as<T>();
    unsigned char *codes = codes_buf.as<unsigned char>(), *Lr = lr_buf.as<unsigned char>();
    double* part = part_buf.as<double>();
    double* u_obs = reinterpret_cast<double*>(out);
    long long* label_counts = out + plan.o_counts;
    FDX_HIP(hipMemsetAsync(out, 0, plan.words * sizeof(long long), st));
    hipLaunchKernelGGL(lp_prepare_kernel<false>, dim3(std::min(1024, ceil_div(n, 256))), dim3(256), 0, st, q.labels, (const int*)nullptr, n,
                       C, codes, reinterpret_cast<unsigned long long*>(label_counts), (unsigned long long*)nullptr,
                       reinterpret_cast<int*>(out + plan.o_flag));
    FDX_CHECK_LAUNCH();
    const int *genes_dev = y.sparse ? nullptr : list_buf.as<int>(), *slot_dev = y.sparse ? list_buf.as<int>() : nullptr;
    auto gather = [&](int t0, int tiles) {
        return gather_gene_tiles<T, LG_TS>(nullptr, n, y, data, genes_dev, slot_dev, S, t0 * LG_TS, tiles, Yt, st);
    };
    // the observed sums: the identity as permutation 0 of one group through the null kernel, so they share its summation order
    LpPermArgs pa{};
    hipLaunchKernelGGL((lp_stage_kernel<LG_B, true>), dim3((unsigned)ceil_div(n, 256), 1), dim3(256), 0, st, codes, (const int*)nullptr, n,
                       (long long)n, Lr, pa);
    FDX_CHECK_LAUNCH();
    for (int t0 = 0; t0 < plan.tiles_all; t0 += plan.stripe_tiles) {
        const int tiles = std::min(plan.stripe_tiles, plan.tiles_all - t0);
        FDX_TRY(gather(t0, tiles));
        FDX_TRY(lg_sums(plan, Yt, Lr, n, C, S, t0 * LG_TS, tiles, 1, part, u_obs, st));
        hipLaunchKernelGGL(lg_nnz_kernel<T>, dim3((unsigned)tiles, (unsigned)plan.nseg), dim3(LG_THREADS), 0, st, Yt, codes, n, C, t0 * LG_TS, S,
                           reinterpret_cast<unsigned long long*>(out + plan.o_nnz));
        FDX_CHECK_LAUNCH();
    }
    pa.keys = perm_keys(q.seed, q.first_perm, n);
    for (long long done = 0; done < q.n_perm; done += plan.batch) {
        const int nb = (int)std::min<long long>(plan.batch, q.n_perm - done);      // the last batch may be ragged
        pa.keys.first = q.first_perm + done;
        pa.batch = nb;
        hipLaunchKernelGGL((lp_stage_kernel<LG_B, false>), dim3((unsigned)ceil_div(n, 256), (unsigned)ceil_div(nb, LG_B)), dim3(256), 0, st,
                           codes, (const int*)nullptr, n, (long long)n, Lr, pa);
        FDX_CHECK_LAUNCH();
        double* U = q.null_dev ? q.null_dev + (size_t)done * C * S : u_buf.as<double>();
        for (int t0 = 0; t0 < plan.tiles_all; t0 += plan.stripe_tiles) {
            const int tiles = std::min(plan.stripe_tiles, plan.tiles_all - t0);
            if (plan.stripes > 1) FDX_TRY(gather(t0, tiles));   // (one stripe: the observed pass has left it in Yt)
            FDX_TRY(lg_sums(plan, Yt, Lr, n, C, S, t0 * LG_TS, tiles, nb, part, U, st));
        }
        hipLaunchKernelGGL(lg_accum_kernel, dim3((unsigned)ceil_div((long long)plan.X, 256)), dim3(256), 0, st, U, nb, u_obs, label_counts,
                           slot_buf.as<int>(), C, S, (long long)plan.X, out + plan.null.count_ge, out + plan.null.count_le,
                           reinterpret_cast<double*>(out + plan.null.sum_d), reinterpret_cast<double*>(out + plan.null.sumsq_d));
        FDX_CHECK_LAUNCH();
    }
    return 0;
}

int label_gene_entry(const char* who, const GeneMatrix& y, const int32_t* labels_dev, int32_t C, const int32_t* genes, int32_t S,
                     const int32_t* pairs, int32_t P, uint64_t seed, int64_t first_perm, int64_t n_perm, int32_t max_batch,
                     int64_t max_gather_bytes, double* null_dev, double* u_out, int64_t* nnz_out, int64_t* label_counts_out,
                     int64_t* count_ge_out, int64_t* count_le_out, double* sum_d_out, double* sumsq_d_out, int32_t* batch_out, void* stream) {
    const std::string w(who);
    hipStream_t st = (hipStream_t)stream;
    const bool rest = labels_dev && genes && pairs && u_out && nnz_out && label_counts_out && count_ge_out && count_le_out && sum_d_out &&
                      sumsq_d_out;
    FDX_TRY(check_gene_matrix(who, y, rest, false, "ldy < G"));
    FDX_REQUIRE(y.G >= 1, w + ": G must be at least 1");
    FDX_REQUIRE(y.n >= 1 && y.n <= LG_MAX_SPOTS, w + ": n must be between 1 and 2^24");
    FDX_REQUIRE(C >= 1 && C <= LP_MAX_LABELS, w + ": the number of labels must be between 1 and 64");
    FDX_REQUIRE(S >= 1 && S <= LG_MAX_GENES, w + ": S must be between 1 and 4096");
    for (int s = 0; s < S; ++s) {
        FDX_REQUIRE(genes[s] >= 0 && genes[s] < y.G, w + ": gene index out of range");
        FDX_REQUIRE(s == 0 || genes[s - 1] < genes[s], w + ": genes must be sorted and distinct");
    }
    FDX_REQUIRE(P >= 1 && (long long)P * C * C <= LG_MAX_STATS, w + ": P must be at least 1 and P * C^2 at most 2^22");
    for (long long k = 0; k < 2LL * P; ++k)
        FDX_REQUIRE(std::binary_search(genes, genes + S, pairs[k]), w + ": a pair names a column that genes does not list");
    FDX_REQUIRE(first_perm >= 0 && n_perm >= 0 && max_batch >= 0 && max_gather_bytes >= 0,
                w + ": first_perm, n_perm, max_batch and max_gather_bytes must not be negative");
    FDX_REQUIRE(first_perm <= (1LL << 62) && n_perm <= (1LL << 40), w + ": too many permutations");
    PoolStream pool_stream(st);
    const size_t elem = y.dtype == FDX_F32 ? sizeof(float) : sizeof(double);
    const LgPlan plan = lg_plan(y.n, elem, C, S, P, n_perm, max_batch,
                                max_gather_bytes > 0 ? (size_t)max_gather_bytes : SCRATCH_BUDGET_BYTES, !null_dev, SCRATCH_BUDGET_BYTES);
    if (batch_out) *batch_out = n_perm > 0 ? plan.batch : 0;
    const LgRequest q{labels_dev, genes, pairs, C, S, P, (unsigned long long)seed, first_perm, n_perm, null_dev};
    DevBuf out;
    FDX_TRY(out.alloc(plan.words * sizeof(long long)));
    FDX_TRY(dispatch_gene_matrix(
        y, [&](auto* Yd) { return lg_run(plan, y, Yd, q, out.as<long long>(), st); },
        [&](auto* values) { return lg_run(plan, y, values, q, out.as<long long>(), st); }));
    std::vector<long long> host(plan.words);
    FDX_TRY(copy_d2h(host.data(), out.p, host.size() * sizeof(long long), st));   // the call's one host synchronisation
    FDX_REQUIRE(host[plan.o_flag] == 0, w + ": a label lies outside [-1, C)");
    std::memcpy(u_out, host.data(), (size_t)C * S * sizeof(double));
    std::copy(host.begin() + plan.o_nnz, host.begin() + plan.o_nnz + (size_t)C * S, nnz_out);
    std::copy(host.begin() + plan.o_counts, host.begin() + plan.o_counts + C, label_counts_out);
    plan.null.unpack(host.data(), count_ge_out, count_le_out, sum_d_out, sumsq_d_out);
    return 0;
}

}  // namespace
}  // namespace fdx

using namespace fdx;

extern "C" {

int fdx_label_gene_sums_dev(const void* Y_dev, int32_t dtype, int64_t n, int32_t G, int64_t ldy, const int32_t* labels_dev, int32_t C,
                            const int32_t* genes, int32_t S, const int32_t* pairs, int32_t P, uint64_t seed, int64_t first_perm,
                            int64_t n_perm, int32_t max_batch, int64_t max_gather_bytes, double* null_dev, double* u_out, int64_t* nnz_out,
                            int64_t* label_counts_out, int64_t* count_ge_out, int64_t* count_le_out, double* sum_d_out, double* sumsq_d_out,
                            int32_t* batch_out, void* stream) {
    return label_gene_entry("fdx_label_gene_sums_dev", GeneMatrix(Y_dev, dtype, n, G, ldy), labels_dev, C, genes, S, pairs, P, seed, first_perm,
                            n_perm, max_batch, max_gather_bytes, null_dev, u_out, nnz_out, label_counts_out, count_ge_out, count_le_out,
                            sum_d_out, sumsq_d_out, batch_out, stream);
}

int fdx_label_gene_sums_csr_dev(const fdx_csr_view* Y, const int32_t* labels_dev, int32_t C, const int32_t* genes, int32_t S,
                                const int32_t* pairs, int32_t P, uint64_t seed, int64_t first_perm, int64_t n_perm, int32_t max_batch,
                                int64_t max_gather_bytes, double* null_dev, double* u_out, int64_t* nnz_out, int64_t* label_counts_out,
                                int64_t* count_ge_out, int64_t* count_le_out, double* sum_d_out, double* sumsq_d_out, int32_t* batch_out,
                                void* stream) {
    return label_gene_entry("fdx_label_gene_sums_csr_dev", GeneMatrix(Y), labels_dev, C, genes, S, pairs, P, seed, first_perm, n_perm, max_batch,
                            max_gather_bytes, null_dev, u_out, nnz_out, label_counts_out, count_ge_out, count_le_out, sum_d_out, sumsq_d_out,
                            batch_out, stream);
}

}  // extern "C"
