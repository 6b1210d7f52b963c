// The shared half of the per-gene passes: stripe, batches, fold and the description of Y (gene_pass.h states the rule).
#include "gene_pass.h"

#include <climits>
#include <cmath>
#include <cstdlib>

#include "fdx_env.h"

namespace fdx {

int stripe_segments() {
    const char* v = env("FDX_EXPR_STRIPE_SEGMENTS");
    const int s = v ? atoi(v) : 1;
    return s >= 1 ? s : 1;
}

namespace {
// acc folded with in[s * stride], s0 <= s < s1, in ascending order: added (OP 0), or the smaller (1) / larger (2) kept
template <int OP>
__device__ __forceinline__ double fold_values(const double* in, size_t stride, int s0, int s1, double acc) {
    auto take = [&](double v) { acc = OP == 1 ? fmin(acc, v) : OP == 2 ? fmax(acc, v) : acc + v; };
    int s = s0;
    for (; s + 8 <= s1; s += 8) {                   // eight loads in flight, folded one after the other
        double v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = in[(size_t)(s + i) * stride];
#pragma unroll
        for (int i = 0; i < 8; ++i) take(v[i]);
    }
    for (; s < s1; ++s) take(in[(size_t)s * stride]);
    return acc;
}

// grid (gene tiles of 256, planes, groups); gene_pass.h: launch_gene_fold
__global__ __launch_bounds__(256) void gene_fold_kernel(SegmentBlocks b, int plane0, int G, const int* __restrict__ group_seg,
                                                        double* out, long long group_stride, long long out_ld, int min_plane,
                                                        int max_plane) {
    const int j = blockIdx.x * 256 + threadIdx.x, plane = blockIdx.y, c = blockIdx.z;
    if (j >= G) return;
    const int g_lo = group_seg ? group_seg[c] : 0, g_hi = group_seg ? group_seg[c + 1] : INT_MAX;
    const int s0 = max(g_lo, b.sb0) - b.sb0, s1 = min(g_hi, b.sb0 + b.nb) - b.sb0;
    const bool fresh = b.sb0 <= g_lo;               // the group begins in this batch (or after it)
    const double* in = b.part + (size_t)(plane0 + plane) * b.plane_stride + (size_t)j * b.gene_stride;
    double* o = out + (size_t)c * group_stride + (size_t)plane * out_ld + j;
    if (plane == min_plane) *o = fold_values<1>(in, b.seg_stride, s0, s1, fresh ? INFINITY : *o);
    else if (plane == max_plane) *o = fold_values<2>(in, b.seg_stride, s0, s1, fresh ? -INFINITY : *o);
    else *o = fold_values<0>(in, b.seg_stride, s0, s1, fresh ? 0.0 : *o);
}
}  // namespace

int launch_gene_fold(const SegmentBlocks& b, int plane0, int planes, int G, const int* group_seg, int groups, double* out,
                     long long group_stride, long long out_ld, int min_plane, int max_plane, hipStream_t st) {
    hipLaunchKernelGGL(gene_fold_kernel, dim3((unsigned)ceil_div(G, 256), (unsigned)planes, (unsigned)groups), dim3(256), 0, st, b,
                       plane0, G, group_seg, out, group_stride, out_ld, min_plane, max_plane);
    FDX_CHECK_LAUNCH();
    return 0;
}

int check_gene_matrix(const char* who, const GeneMatrix& y, bool rest_present, bool weighted_sums, const char* dense_shape) {
    const std::string w(who);
    const bool may_be_null = weighted_sums && y.n == 0;
    const void* rows = y.sparse ? (y.csr ? y.csr->indptr : nullptr) : y.dense;
    FDX_REQUIRE(rest_present && (!y.sparse || y.csr) && (rows || may_be_null), w + ": null argument");
    const bool G_ok = !weighted_sums || y.G >= 1;
    if (y.sparse) FDX_REQUIRE(G_ok && (y.csr->nnz == 0 || (y.csr->indices && y.csr->data)), w + ": bad view");
    else FDX_REQUIRE(G_ok && y.ldy >= y.G, w + ": " + dense_shape);
    FDX_REQUIRE(y.dtype == FDX_F32 || y.dtype == FDX_F64, w + ": dtype must be FDX_F32 or FDX_F64");
    return 0;
}

}  // namespace fdx
