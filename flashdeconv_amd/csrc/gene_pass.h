// What the per-gene passes over a spot-by-gene matrix Y share (expression_kernels.cpp: the weighted gene sums; gene_spatial_kernels.cpp:
// the gene spatial sums).  A pass cuts its rows into SEGMENTS by a rule of its own, sums a segment in a fixed order into a block of
// scratch, and a fold adds the blocks of a group of segments in ascending order.  Three things change no bit of the result:
//   the stripe   a workgroup of a segment kernel takes stripe_segments() consecutive segments (FDX_EXPR_STRIPE_SEGMENTS, default 1);
//   the batch    at most SCRATCH_BUDGET_BYTES of blocks are in flight; more segments go in batches (for_segment_batches), and
//                every batch's fold continues from what the batch before left in the result;
//   the thread   that owns a gene.  No floating-point atomics anywhere.
#pragma once
#include <algorithm>

#include "fdx_internal.h"

namespace fdx {

// The one scratch budget of the library's batched passes: segment blocks here, permutation / band planes in the spatial statistics.
constexpr size_t SCRATCH_BUDGET_BYTES = (size_t)1 << 30;

int stripe_segments();
// Segments whose blocks (seg_bytes each) are in flight at once: what the budget holds, one at the least.
inline int segment_batch(int n_seg, size_t seg_bytes) {
    return (int)std::max<size_t>(1, std::min<size_t>((size_t)n_seg, SCRATCH_BUDGET_BYTES / seg_bytes));
}
// Allocates segment_batch blocks from the pool once and calls int body(int sb0, int nb, double* part) for the batches [sb0, sb0 + nb)
// in ascending order; body queues the batch's segment kernel(s) into `part` and their fold(s).  Stops at the first non-zero return.
template <class Body>
int for_segment_batches(int n_seg, size_t seg_bytes, Body&& body) {
    const int batch = segment_batch(n_seg, seg_bytes);
    DevBuf part;
    FDX_TRY(part.alloc((size_t)batch * seg_bytes));
    for (int sb0 = 0; sb0 < n_seg; sb0 += batch) FDX_TRY(body(sb0, std::min(batch, n_seg - sb0), part.as<double>()));
    return 0;
}

// One batch as the fold reads it: element (s, plane, j) lies at part[(s - sb0) * seg_stride + plane * plane_stride + j * gene_stride].
struct SegmentBlocks { const double* part; long long seg_stride, plane_stride, gene_stride; int sb0, nb; };
// out[c * group_stride + p * out_ld + j], p < planes, c < groups, j < G = plane plane0 + p folded over the segments of group c,
// [group_seg[c], group_seg[c + 1]) (device; null: one group of every segment), that lie in the batch, in ascending order: added, or
// for p = min_plane / max_plane (-1: none) the smaller / larger kept.  A group that begins in this batch starts from the identity
// (0, +inf, -inf), one that began earlier from out; every batch writes every group (one behind it its value again, one ahead of it
// the identity, which its own batch overwrites).
int launch_gene_fold(const SegmentBlocks& b, int plane0, int planes, int G, const int* group_seg, int groups, double* out,
                     long long group_stride, long long out_ld, int min_plane, int max_plane, hipStream_t st);

// Y (n, G) as an entry was handed it: dense (FDX_F32 / FDX_F64, row stride ldy) or, `sparse`, a CSR view (null: refused below).
struct GeneMatrix {
    const void* dense = nullptr;
    const fdx_csr_view* csr = nullptr;
    bool sparse = false;
    long long ldy = 0, n = 0;
    int dtype = 0, G = 0;
    GeneMatrix(const void* Y, int dtype_, long long n_, int G_, long long ldy_) : dense(Y), ldy(ldy_), n(n_), dtype(dtype_), G(G_) {}
    explicit GeneMatrix(const fdx_csr_view* v) : csr(v), sparse(true), n(v ? v->n : 0), dtype(v ? v->dtype : 0), G(v ? v->G : 0) {}
};
// "<who>: null argument" (unless rest_present - the entry's other pointers - and Y are there), "<who>: <dense_shape>" (ldy < G) or
// "<who>: bad view" (indices and data wherever nnz > 0), "<who>: dtype must be FDX_F32 or FDX_F64", in this order.  weighted_sums:
// n = 0 excuses a null dense pointer / indptr, and G < 1 is a bad shape / view (the gene spatial entries refuse it later, themselves).
int check_gene_matrix(const char* who, const GeneMatrix& y, bool rest_present, bool weighted_sums, const char* dense_shape);

// The one place where (dense | CSR) x (float32 | float64) becomes a template instantiation: dense(const T* Y) or csr(const T* values).
template <class Dense, class Csr>
int dispatch_gene_matrix(const GeneMatrix& y, Dense&& dense, Csr&& csr) {
    if (y.sparse) return y.dtype == FDX_F32 ? csr((const float*)y.csr->data) : csr((const double*)y.csr->data);
    return y.dtype == FDX_F32 ? dense((const float*)y.dense) : dense((const double*)y.dense);
}

// The weighted gene sums (expression_kernels.cpp; fdx.h: fdx_weighted_gene_sums_dev, whose arguments these are, already checked).
int launch_weighted_gene_sums(const GeneMatrix& y, const double* W, long long ldw, int K, const int* rows, const int* group_off, int C,
                              double* A, double* B, double* q, double* u, hipStream_t st);

}  // namespace fdx
