// Neighbourhood enrichment of spot labels (join counts; not in the reference): with A the symmetric binary adjacency held as the
// sliced ELL and l_i in {-1, 0 .. C - 1} the label of spot i in the caller's order, the kernels count
//   N_ab = #{(i, j) : A_ij = 1, l_i = a, l_j = b}     over ordered pairs, a, b in [0, C)
// for the observed labels and for the labels l^r_i = l[pi_r(i)] of permutations r = first_perm .. first_perm + n_perm - 1 (pi_r: the
// keyed bijection of perm_device.h), and rank the observed matrix against that null.  Everything is an integer: every count is
// exact, nothing depends on the order of a sum, two calls return the same bits.  The statistics (the analytic moments, z scores,
// p values) are assembled on the host (flashdeconv_amd/utils/neighborhoods.py).
//
//   prepare    labels -> one byte per spot (the label, or LP_NONE for -1), the range check (a flag, reported as an error after the
//              call's one copy), n_a, sum deg and sum deg^2
//   stage      Lr[g][q][j] = byte of l[pi_r(perm[q])], r = first + g * B + j, for the B permutations of group g interleaved per
//              graph position q: one 8- or 16-byte load returns a position's label under every permutation of its group.  LP_NONE
//              for -1, for positions n .. ld - 1 (the ELL pad index n among them: padding needs no mask) and for permutations past
//              the batch.  pi_r is evaluated once per spot and permutation, never per edge.  The observed pass stages the identity
//              as permutation 0 of one group.
//   count      one lane per position, one wave per 64-position slice (the walk of ss_lag_kernel): the lane keeps its own B bytes in
//              registers, reads each ELL index once, gathers the neighbour's B bytes in one load and adds 1 to hist[j][a][b] in
//              LDS (32-bit integer atomics) wherever neither byte is LP_NONE.  The workgroup then adds its non-zero bins to the
//              batch's (batch, C, C) int64 matrix with 64-bit integer atomics.
//   accumulate one thread per pair (a, b), in permutation order: N^r to the null, count_ge, count_le, sum d, sum d^2 against the
//              observed matrix, and the batch's matrix back to zero
//
// B and the workgroup follow from C so that B * C^2 * 4 bytes of histogram fit the CU's 160 KiB of LDS:
//   C <= 16        B = 16, 256 threads    <= 16 KiB: eight workgroups, the CU's 32 waves
//   17 <= C <= 32  B = 16, 1024 threads   18 - 64 KiB: two workgroups, 32 waves
//   33 <= C <= 64  B = 8,  1024 threads   34 - 128 KiB: two workgroups up to C = 50, one (16 waves, four per SIMD) above
// A workgroup's bins are 32-bit: the launcher keeps a workgroup's edge visits below 2^32 (more workgroups where 64 * ell_rows, the
// bound of the whole grid, is not).
#include "fdx_graph.h"
#include "fdx_internal.h"
#include "gene_pass.h"
#include "label_stage.h"
#include "perm_device.h"

#include <algorithm>
#include <vector>

namespace fdx {

constexpr int LP_MAX_GROUPS = 64;        // groups of B permutations per launch chain (a grid dimension)
constexpr int LP_TARGET_WAVES = 8192;    // waves of a count launch over all its groups: the chip's 256 CUs x 32

// (label_stage.h: lp_prepare_kernel - here with deg_sums = {sum deg, sum deg^2} - and lp_stage_kernel, shared with the label gene sums)

template <int B>
__device__ __forceinline__ void lp_load(const unsigned char* __restrict__ Lr, long long q, unsigned (&w)[B / 4]) {
    if constexpr (B == 8) {
        const uint2 v = *reinterpret_cast<const uint2*>(Lr + (size_t)q * 8);
        w[0] = v.x; w[1] = v.y;
    } else {
        const uint4 v = *reinterpret_cast<const uint4*>(Lr + (size_t)q * 16);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
}

// acc[blockIdx.y][j][a][b] += the workgroup's count of ordered neighbour pairs (p, entry) with bytes (a, b) under permutation j of
// group blockIdx.y.  blockDim.x / 64 waves, a slice each at a time; hist is B * C * C words of dynamic LDS.
template <int B>
__global__ void lp_count_kernel(const unsigned char* __restrict__ Lr_all, long long ld, const int* __restrict__ ell_base,
                                const int* __restrict__ slice_off, int n, int n_slices, int C,
                                unsigned long long* __restrict__ acc_all) {
    extern __shared__ unsigned lp_hist[];
    const int bins = B * C * C;
    for (int i = threadIdx.x; i < bins; i += blockDim.x) lp_hist[i] = 0u;
    __syncthreads();
    const unsigned char* Lr = Lr_all + (size_t)blockIdx.y * ld * B;
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wpb = blockDim.x >> 6;
    const int CC = C * C;
    for (int slice = blockIdx.x * wpb + wib; slice < n_slices; slice += gridDim.x * wpb) {
        const long long p = (long long)slice * 64 + lane;
        const bool active = p < n;
        const int w0 = slice_off[slice];
        const int w = slice_off[slice + 1] - w0;
        const int* ell = ell_base + (size_t)w0 * 64 + lane;
        unsigned mine[B / 4];
        lp_load<B>(Lr, p, mine);                                   // p < ld; positions from n on hold LP_NONE
        int row[B];                                                // (j * C + a) * C of the lane's own byte
#pragma unroll
        for (int j = 0; j < B; ++j) row[j] = j * CC + (int)((mine[j / 4] >> (8 * (j % 4))) & 0xffu) * C;
        int q_next = (w > 0 && active) ? ell[0] : n;
        for (int m = 0; m < w; ++m) {
            const int q = q_next;
            if (m + 1 < w) q_next = active ? ell[(size_t)(m + 1) * 64] : n;
            unsigned nb[B / 4];
            lp_load<B>(Lr, q, nb);
#pragma unroll
            for (int j = 0; j < B; ++j) {
                const unsigned both = (mine[j / 4] | nb[j / 4]) >> (8 * (j % 4));
                if (!(both & 0x80u)) atomicAdd(&lp_hist[row[j] + (int)((nb[j / 4] >> (8 * (j % 4))) & 0xffu)], 1u);
            }
        }
    }
    __syncthreads();
    unsigned long long* acc = acc_all + (size_t)blockIdx.y * bins;
    for (int i = threadIdx.x; i < bins; i += blockDim.x) {
        const unsigned v = lp_hist[i];
        if (v) atomicAdd(&acc[i], (unsigned long long)v);
    }
}

// obs[i] = acc[i] (the identity's matrix: permutation 0 of the one group), acc[i] = 0
__global__ __launch_bounds__(256) void lp_observed_kernel(long long* __restrict__ acc, long long CC, long long* __restrict__ obs) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= CC) return;
    obs[i] = acc[i];
    acc[i] = 0;
}

// the batch's N^r against the observed matrix, one thread per pair, in permutation order: d = N^r - N; null (may be null) gets
// every N^r; acc goes back to zero
__global__ __launch_bounds__(256) void lp_accum_kernel(long long* __restrict__ acc, int batch, long long CC,
                                                       const long long* __restrict__ obs, long long* __restrict__ null_out,
                                                       long long* __restrict__ count_ge, long long* __restrict__ count_le,
                                                       double* __restrict__ sum_d, double* __restrict__ sumsq_d) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= CC) return;
    const long long c0 = obs[i];
    long long ge = count_ge[i], le = count_le[i];
    double s = sum_d[i], q = sumsq_d[i];
    for (int j = 0; j < batch; ++j) {
        const long long c = acc[(size_t)j * CC + i];
        acc[(size_t)j * CC + i] = 0;
        if (null_out) null_out[(size_t)j * CC + i] = c;
        const double d = (double)(c - c0);
        ge += c >= c0 ? 1 : 0;
        le += c <= c0 ? 1 : 0;
        s = __dadd_rn(s, d);
        q = __dadd_rn(q, __dmul_rn(d, d));                         // the sum of the rounded squares, as NumPy adds them: no fma
    }
    count_ge[i] = ge;
    count_le[i] = le;
    sum_d[i] = s;
    sumsq_d[i] = q;
}

// What a call runs with: B and the workgroup from C (header), the groups per launch chain from the scratch budget, max_batch and
// n_perm, the grid of a count launch, and the packed device result (64-bit words).
struct LabelPairPlan {
    int B, threads, groups, batch;       // batch: permutations per launch chain, at most groups * B
    long long ld;
    int n_slices, blocks;                // blocks: grid.x of a count launch with `groups` groups
    size_t lds_bytes;
    size_t CC;
    // result words: [obs CC | label counts C | W, sum deg^2 | flag | null: count_ge CC | count_le CC | sum_d CC | sumsq_d CC]
    size_t o_counts, o_deg, o_flag, words;
    NullSumsLayout null;
};

static int count_blocks(const LabelPairPlan& p, int groups, long long ell_rows, int max_width) {
    const int wpb = p.threads / 64;
    const int need = ceil_div(p.n_slices, wpb);
    int blocks = std::max(1, std::min(need, LP_TARGET_WAVES / (wpb * groups)));
    if (64 * ell_rows >= (1LL << 32)) {
        // a workgroup visits at most (slices per wave) * wpb * 64 * (widest slice) edges: below 2^32 with enough workgroups
        const long long per_slice = 64LL * std::max(1, max_width);
        const long long slices_per_block = std::max<long long>(wpb, ((1LL << 32) - 1) / per_slice / wpb * wpb);
        blocks = std::max(blocks, ceil_div(p.n_slices, slices_per_block));
    }
    return std::min(blocks, need);
}

static LabelPairPlan label_pair_plan(long long n, int C, long long n_perm, int max_batch) {
    LabelPairPlan p;
    p.B = C <= 32 ? 16 : 8;
    p.threads = C <= 16 ? 256 : 1024;
    p.CC = (size_t)C * C;
    p.lds_bytes = (size_t)p.B * p.CC * sizeof(unsigned);
    p.ld = round_up(n + 1, 64);
    p.n_slices = ceil_div(n, 64);
    const size_t per_group = (size_t)p.ld * p.B + (size_t)p.B * p.CC * sizeof(long long);
    const long long fit_groups = (long long)std::max<size_t>(1, SCRATCH_BUDGET_BYTES / per_group);   // a whole group at the least
    const long long batch = perm_batch(fit_groups * p.B, (long long)LP_MAX_GROUPS * p.B, max_batch, n_perm);
    p.batch = (int)batch;
    p.groups = ceil_div(batch, p.B);
    p.o_counts = p.CC;
    p.o_deg = p.o_counts + C;
    p.o_flag = p.o_deg + 2;
    p.null = NullSumsLayout(p.CC, p.o_flag + 1);
    p.words = p.null.end;
    return p;
}

template <int B>
static int launch_count(const LabelPairPlan& p, int groups, int blocks, const unsigned char* Lr, const GraphTables& g, int C,
                        long long* acc, hipStream_t st) {
    if (p.lds_bytes > 64 * 1024)
        FDX_HIP(hipFuncSetAttribute((const void*)lp_count_kernel<B>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes));
    hipLaunchKernelGGL(lp_count_kernel<B>, dim3(blocks, groups), dim3(p.threads), p.lds_bytes, st, Lr, p.ld, g.ell, g.slice_off, g.n,
                       p.n_slices, C, reinterpret_cast<unsigned long long*>(acc));
    FDX_CHECK_LAUNCH();
    return 0;
}

// scratch: [codes n | Lr groups * ld * B | acc groups * B * CC words], each 16-byte aligned; out: p.words words, zeroed here
template <int B>
static int launch_label_pairs(const LabelPairPlan& p, const fdx_graph* graph, const GraphTables& g, const int* labels, int C,
                              unsigned long long seed, long long first_perm, long long n_perm, long long* null_dev,
                              unsigned char* codes, unsigned char* Lr, long long* acc, long long* out, hipStream_t st) {
    const int n = g.n;
    FDX_HIP(hipMemsetAsync(out, 0, p.words * sizeof(long long), st));
    FDX_HIP(hipMemsetAsync(acc, 0, (size_t)p.groups * B * p.CC * sizeof(long long), st));
    long long* obs = out;
    hipLaunchKernelGGL(lp_prepare_kernel<true>, dim3(std::min(1024, ceil_div(n, 256))), dim3(256), 0, st, labels, g.deg, n, C, codes,
                       reinterpret_cast<unsigned long long*>(out + p.o_counts), reinterpret_cast<unsigned long long*>(out + p.o_deg),
                       reinterpret_cast<int*>(out + p.o_flag));
    FDX_CHECK_LAUNCH();
    LpPermArgs pa{};
    hipLaunchKernelGGL((lp_stage_kernel<B, true>), dim3(ceil_div(p.ld, 256), 1), dim3(256), 0, st, codes, g.perm, n, p.ld, Lr, pa);
    FDX_CHECK_LAUNCH();
    FDX_TRY(launch_count<B>(p, 1, count_blocks(p, 1, graph->ell_rows, graph->max_deg), Lr, g, C, acc, st));
    hipLaunchKernelGGL(lp_observed_kernel, dim3(ceil_div((long long)p.CC, 256)), dim3(256), 0, st, acc, (long long)p.CC, obs);
    FDX_CHECK_LAUNCH();
    if (n_perm <= 0) return 0;

    pa.keys = perm_keys(seed, first_perm, n);
    for (long long done = 0; done < n_perm; done += p.batch) {
        const int b = (int)std::min<long long>(p.batch, n_perm - done);     // the last batch may be ragged
        const int groups = ceil_div(b, B);
        pa.keys.first = first_perm + done;
        pa.batch = b;
        hipLaunchKernelGGL((lp_stage_kernel<B, false>), dim3(ceil_div(p.ld, 256), groups), dim3(256), 0, st, codes, g.perm, n, p.ld,
                           Lr, pa);
        FDX_CHECK_LAUNCH();
        FDX_TRY(launch_count<B>(p, groups, count_blocks(p, groups, graph->ell_rows, graph->max_deg), Lr, g, C, acc, st));
        hipLaunchKernelGGL(lp_accum_kernel, dim3(ceil_div((long long)p.CC, 256)), dim3(256), 0, st, acc, b, (long long)p.CC, obs,
                           null_dev ? null_dev + (size_t)done * p.CC : nullptr, out + p.null.count_ge, out + p.null.count_le,
                           reinterpret_cast<double*>(out + p.null.sum_d), reinterpret_cast<double*>(out + p.null.sumsq_d));
        FDX_CHECK_LAUNCH();
    }
    return 0;
}

}  // namespace fdx

using namespace fdx;

extern "C" {

int fdx_label_pair_counts_dev(const fdx_graph* g, const int32_t* labels_dev, int32_t C, uint64_t seed, int64_t first_perm,
                              int64_t n_perm, int32_t max_batch, int64_t* null_dev, int64_t* label_counts_out, int64_t* pair_out,
                              int64_t* counts_out, int64_t* count_ge_out, int64_t* count_le_out, double* sum_d_out,
                              double* sumsq_d_out, int32_t* batch_out, void* stream) {
    FDX_REQUIRE(g && label_counts_out && pair_out && counts_out && count_ge_out && count_le_out && sum_d_out && sumsq_d_out,
                "fdx_label_pair_counts_dev: null argument");
    FDX_REQUIRE(C >= 1 && C <= LP_MAX_LABELS, "fdx_label_pair_counts_dev: the number of labels must be between 1 and 64");
    FDX_REQUIRE(first_perm >= 0 && n_perm >= 0 && max_batch >= 0,
                "fdx_label_pair_counts_dev: first_perm, n_perm and max_batch must not be negative");
    GraphTables t;
    FDX_TRY(whole_graph_tables(g, "fdx_label_pair_counts_dev", &t));
    FDX_REQUIRE(t.n == 0 || labels_dev, "fdx_label_pair_counts_dev: null argument");
    hipStream_t st = (hipStream_t)stream;
    PoolStream pool_stream(st);
    const size_t CC = (size_t)C * C;
    counts_out[0] = t.n;
    counts_out[1] = counts_out[2] = 0;
    if (batch_out) *batch_out = 0;
    if (t.n == 0) {                                     // nothing to count: every N^r equals N = 0
        std::fill(label_counts_out, label_counts_out + C, (int64_t)0);
        std::fill(pair_out, pair_out + CC, (int64_t)0);
        NullSumsLayout(CC, 0).fill_empty(n_perm, count_ge_out, count_le_out, sum_d_out, sumsq_d_out);
        return 0;
    }
    const LabelPairPlan plan = label_pair_plan(t.n, C, n_perm, max_batch);
    FDX_REQUIRE(g->ell_rows * 64 < (1LL << 32) || (long long)(plan.threads / 64) * 64 * std::max(1, g->max_deg) < (1LL << 32),
                "fdx_label_pair_counts_dev: a slice of the graph is too wide for the 32-bit bins of a workgroup");
    if (batch_out) *batch_out = n_perm > 0 ? plan.batch : 0;
    const size_t codes_bytes = (size_t)round_up(t.n, 16);
    const size_t lr_bytes = (size_t)plan.groups * plan.ld * plan.B;
    const size_t acc_bytes = (size_t)plan.groups * plan.B * CC * sizeof(long long);
    DevBuf scratch, out;
    FDX_TRY(scratch.alloc(codes_bytes + lr_bytes + acc_bytes));
    FDX_TRY(out.alloc(plan.words * sizeof(long long)));
    unsigned char* codes = scratch.as<unsigned char>();
    unsigned char* Lr = codes + codes_bytes;
    long long* acc = reinterpret_cast<long long*>(Lr + lr_bytes);
    long long* nd = reinterpret_cast<long long*>(null_dev);
    if (plan.B == 16)
        FDX_TRY(launch_label_pairs<16>(plan, g, t, labels_dev, C, seed, first_perm, n_perm, nd, codes, Lr, acc, out.as<long long>(), st));
    else
        FDX_TRY(launch_label_pairs<8>(plan, g, t, labels_dev, C, seed, first_perm, n_perm, nd, codes, Lr, acc, out.as<long long>(), st));
    std::vector<long long> host(plan.words);
    FDX_TRY(copy_d2h(host.data(), out.p, host.size() * sizeof(long long), st));   // the call's one host synchronisation
    FDX_REQUIRE(host[plan.o_flag] == 0, "fdx_label_pair_counts_dev: a label lies outside [-1, C)");
    std::copy(host.begin(), host.begin() + CC, pair_out);
    std::copy(host.begin() + plan.o_counts, host.begin() + plan.o_counts + C, label_counts_out);
    counts_out[1] = host[plan.o_deg];
    counts_out[2] = host[plan.o_deg + 1];
    plan.null.unpack(host.data(), count_ge_out, count_le_out, sum_d_out, sumsq_d_out);
    return 0;
}

}  // extern "C"
