// Marker genes of spot groups (additive, not in the reference): per (group c, gene g) of a spot-by-gene matrix Y the sums a Welch test
// and a Wilcoxon rank-sum test of "group c against the rest" are assembled from - u = sum y, q = sum y^2, nnz = #{y != 0} and
// R2 = sum of the twice-midranks of the group's values among the N used values of the gene - and per gene T = sum over tie runs of
// (t^3 - t).  include/fdx.h has the definitions; the statistics are assembled on the host (flashdeconv_amd/utils/group_genes.py).
//
// u and q ARE the weighted gene sums with W = 1 (expression_kernels.cpp: launch_weighted_gene_sums on the rows sorted by label):
// there is one summation order in the tree.  Everything else is an integer and therefore exact in any order: integer atomics in
// global memory and LDS carry nnz, R2 and T; there is no floating-point atomic.
//
// The ranking never touches a zero.  Expression matrices are mostly exact zeros, all tied: with neg_g negatives and z_g = N - nz_g
// zeros of gene g, the zero run holds the 1-based ranks neg_g + 1 .. neg_g + z_g, twice their mean is 2 neg_g + z_g + 1, and a nonzero
// at place k of the gene's nz_g sorted nonzeros has as many values before it as k, plus z_g when it is positive.  So
//   1. gg_count_*     counts nnz[c][g] and neg_g (dense: a wave per (segment quarter, 64 genes); CSR: a wave per row);
//      gg_init_kernel leaves nz_g and starts R2[c][g] = (2 neg_g + z_g + 1) (n_c - nnz[c][g]) and T_g = z_g^3 - z_g;
//   2. the genes are cut into STRIPES of consecutive genes from the COUNTS (one read-back of nz_g), so that a stripe's keys, payloads
//      and sort workspace fit max_sort_bytes - counted first, not sized for the worst case: the worst case of a 90 % zero matrix is
//      ten times what it needs.  A gene is never cut: one gene a stripe at the least (at most 2 000 000 entries, 64 MB);
//   3. gg_compact_*   writes the stripe's entries with y != 0 (-0.0 and a stored CSR zero are zeros) as (order-preserving key of the
//      value - all 32 / 64 bits of the storage type, float32 -> float64 is monotone and one-to-one -, gene-in-stripe << 8 | label)
//      behind one cursor: a wave counts its entries (dense: a quarter segment of 64 genes; CSR: a row), reserves them with ONE integer
//      atomic and walks its rows a second time to write them;
//   4. rocPRIM radix sort by value over the whole stripe, a max-scan of "i if the value differs from its predecessor's" names every
//      distinct value by the place of its first entry (32 bits, whatever the key's width), then a STABLE rocPRIM radix sort by gene
//      (bits 8 .. of the payload; the label rides in the key, the value's name is the sorted value) - the two sorts of the Spearman
//      ranks in metrics_kernels.cpp.  Each gene's nonzeros are now contiguous in ascending value, gene after gene, and gene g's
//      begin at the prefix sum of the counts;
//   5. a second max-scan of run heads (gene or value name changes) gives every entry its run's start; the LAST entry of a run [s, e)
//      writes the run's twice-midrank s' + e' + 1 (+ 2 z_g behind the negatives; s', e' relative to the gene's start) at the run's
//      start and adds t^3 - t to T_g; every entry then reads it through its start and adds it to R2[label][g], through sums per (gene,
//      label) in LDS.  Nothing walks a run.
// A stripe changes which sort an entry takes part in, never a rank: ranks are per gene.  Flat positions are ints: a stripe holds at
// most 2^30 entries.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "fdx_internal.h"
#include "gene_pass.h"

namespace fdx {
namespace {

using u32 = unsigned int;
using u64 = unsigned long long;

constexpr int SEG = FDX_EXPRESSION_SEGMENT_ROWS;
constexpr int GG_LABEL_BITS = 8;                     // a payload is gene-in-stripe << 8 | label: C <= 256 ...
constexpr int GG_STRIPE_GENES_MAX = 1 << 24;         // ... and at most 2^24 genes a stripe
constexpr long long GG_STRIPE_ENTRIES_MAX = 1LL << 30;
constexpr int GG_ROWS_AHEAD = 8;                     // rows a lane of the dense kernels has in flight

// order-preserving unsigned keys of IEEE values: negatives reversed below the positives
__device__ __forceinline__ u32 order_key(float v) {
    const u32 b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ u64 order_key(double v) {
    const u64 b = (u64)__double_as_longlong(v);
    return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
}
template <typename T> struct KeyOf { using type = u32; };
template <> struct KeyOf<double> { using type = u64; };

// key[i] = label, C for a row left out (and for a label outside [-1, C), counted in counts[C + 1] and refused by the host);
// counts[0 .. C - 1] the group sizes, counts[C] the rows left out
__global__ __launch_bounds__(256) void gg_label_kernel(const int* __restrict__ labels, int n, int C, u32* __restrict__ key,
                                                       u64* __restrict__ counts) {
    __shared__ u32 h[(1 << GG_LABEL_BITS) + 2];
    for (int k = threadIdx.x; k < C + 2; k += 256) h[k] = 0;
    __syncthreads();
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int l = labels[i];
        const int k = (l >= 0 && l < C) ? l : (l == -1 ? C : C + 1);
        atomicAdd(&h[k], 1u);
        key[i] = (u32)min(k, C);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < C + 2; k += 256)
        if (h[k]) atomicAdd(&counts[k], (u64)h[k]);
}

__global__ __launch_bounds__(256) void gg_fill_kernel(double* __restrict__ w, long long n, double v) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) w[i] = v;
}

// seg: {first, end, group} per segment of the sorted row list.  grid (tiles of 64 genes, segments); wave w takes the w-th quarter
// of the segment's positions, lane l gene 64 * blockIdx.x + l: a row is read 64 consecutive values at a time.
template <typename T>
__global__ __launch_bounds__(256) void gg_count_dense_kernel(const T* __restrict__ Y, long long ldy, const int* __restrict__ rows,
                                                             const int* __restrict__ seg, int G, u64* __restrict__ nnz,
                                                             u64* __restrict__ neg) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane;
    if (j >= G) return;
    const int s = blockIdx.y, s0 = seg[3 * s], s1 = seg[3 * s + 1], c = seg[3 * s + 2];
    const int quarter = (s1 - s0 + 3) / 4;
    const int p0 = s0 + w * quarter, p1 = min(s1, p0 + quarter);
    u32 nz = 0, ng = 0;
    for (int pb = p0; pb < p1; pb += GG_ROWS_AHEAD) {
        T v[GG_ROWS_AHEAD];
#pragma unroll
        for (int i = 0; i < GG_ROWS_AHEAD; ++i) v[i] = pb + i < p1 ? Y[(long long)rows[pb + i] * ldy + j] : (T)0;
#pragma unroll
        for (int i = 0; i < GG_ROWS_AHEAD; ++i) {
            nz += v[i] != (T)0;
            ng += v[i] < (T)0;
        }
    }
    if (nz) atomicAdd(&nnz[(size_t)c * G + j], (u64)nz);
    if (ng) atomicAdd(&neg[j], (u64)ng);
}

// a wave per position of the sorted row list: the stored entries of its row, 64 at a time
template <typename T>
__global__ __launch_bounds__(256) void gg_count_csr_kernel(const long long* __restrict__ indptr, const int* __restrict__ indices,
                                                           const T* __restrict__ values, const int* __restrict__ rows,
                                                           const u32* __restrict__ lab, int N, int G, u64* __restrict__ nnz,
                                                           u64* __restrict__ neg) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= N) return;
    const long long r = rows[p];
    const size_t c = lab[p];
    const long long e1 = indptr[r + 1];
    for (long long e = indptr[r] + lane; e < e1; e += 64) {
        const T v = values[e];
        const int col = indices[e];
        if (v != (T)0 && (u32)col < (u32)G) {
            atomicAdd(&nnz[c * G + col], 1ull);
            if (v < (T)0) atomicAdd(&neg[col], 1ull);
        }
    }
}

// nz_g = sum_c nnz[c][g]; with z = N - nz_g:  T_g = z^3 - z,  R2[c][g] = (2 neg_g + z + 1) (n_c - nnz[c][g]) - the zero run's share
__global__ __launch_bounds__(256) void gg_init_kernel(const u64* __restrict__ nnz, const u64* __restrict__ neg,
                                                      const u64* __restrict__ counts, int C, int G, u64 N, u64* __restrict__ nzg,
                                                      u64* __restrict__ R2, u64* __restrict__ T) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    u64 nz = 0;
    for (int c = 0; c < C; ++c) nz += nnz[(size_t)c * G + g];
    const u64 z = N - nz, mid2 = 2 * neg[g] + z + 1;
    nzg[g] = nz;
    T[g] = z * z * z - z;
    for (int c = 0; c < C; ++c) R2[(size_t)c * G + g] = mid2 * (counts[c] - nnz[(size_t)c * G + g]);
}

// The entries with y != 0 of the genes [g0, g0 + Gs) behind *cursor (cap slots: what the counts said; nothing is written past it).
// Grid and the walk of gg_count_dense_kernel.  A wave walks its rows twice: once to count its entries per lane - ONE integer atomic
// then reserves the wave's slots (an atomic per eight rows had 400 000 of them queue on one address: 4.6 of the call's 11.6 ms at
// 100 000 x 2 000) - and once more, from L2, to write them, every lane behind its own offset.
template <typename T>
__global__ __launch_bounds__(256) void gg_compact_dense_kernel(const T* __restrict__ Y, long long ldy, const int* __restrict__ rows,
                                                               const int* __restrict__ seg, int g0, int Gs, int cap,
                                                               int* __restrict__ cursor, typename KeyOf<T>::type* __restrict__ key,
                                                               u32* __restrict__ pay) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane;
    const bool ok = j < Gs;
    const int s = blockIdx.y, s0 = seg[3 * s], s1 = seg[3 * s + 1], c = seg[3 * s + 2];
    const int quarter = (s1 - s0 + 3) / 4;
    const int p0 = s0 + w * quarter, p1 = min(s1, p0 + quarter);   // the wave's: every lane makes every step
    const T* col = Y + g0 + (ok ? j : 0);
    const u32 payload = ((u32)j << GG_LABEL_BITS) | (u32)c;
    int cnt = 0;
    for (int pb = p0; pb < p1; pb += GG_ROWS_AHEAD) {
        T v[GG_ROWS_AHEAD];
#pragma unroll
        for (int i = 0; i < GG_ROWS_AHEAD; ++i) v[i] = (ok && pb + i < p1) ? col[(long long)rows[pb + i] * ldy] : (T)0;
#pragma unroll
        for (int i = 0; i < GG_ROWS_AHEAD; ++i) cnt += v[i] != (T)0;
    }
    int incl = cnt;                                     // inclusive scan over the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
    }
    const int total = __shfl(incl, 63, 64);
    if (total == 0) return;                             // the whole wave
    int base = 0;
    if (lane == 63) base = atomicAdd(cursor, total);
    base = __shfl(base, 63, 64);
    int pos = base + incl - cnt;
    for (int pb = p0; pb < p1; pb += GG_ROWS_AHEAD) {
        T v[GG_ROWS_AHEAD];
#pragma unroll
        for (int i = 0; i < GG_ROWS_AHEAD; ++i) v[i] = (ok && pb + i < p1) ? col[(long long)rows[pb + i] * ldy] : (T)0;
#pragma unroll
        for (int i = 0; i < GG_ROWS_AHEAD; ++i) {
            if (v[i] != (T)0) {
                if (pos >= 0 && pos < cap) {
                    key[pos] = order_key(v[i]);
                    pay[pos] = payload;
                }
                ++pos;
            }
        }
    }
}

// a wave per position, as gg_count_csr_kernel: the stored entries with y != 0 and a column in [g0, g1) - counted, reserved with one
// atomic a row, written on a second walk
template <typename T>
__global__ __launch_bounds__(256) void gg_compact_csr_kernel(const long long* __restrict__ indptr, const int* __restrict__ indices,
                                                             const T* __restrict__ values, const int* __restrict__ rows,
                                                             const u32* __restrict__ lab, int N, int g0, int g1, int cap,
                                                             int* __restrict__ cursor, typename KeyOf<T>::type* __restrict__ key,
                                                             u32* __restrict__ pay) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= N) return;                                 // a whole wave leaves
    const long long r = rows[p];
    const u32 c = lab[p];
    const long long e0 = indptr[r], e1 = indptr[r + 1];
    int total = 0;
    for (long long eb = e0; eb < e1; eb += 64) {
        const long long e = eb + lane;
        const bool in = e < e1;
        const T v = in ? values[e] : (T)0;
        const int col = in ? indices[e] : -1;
        total += (int)__popcll(__ballot(v != (T)0 && col >= g0 && col < g1));
    }
    if (total == 0) return;
    int base = 0;
    if (lane == 0) base = atomicAdd(cursor, total);
    base = __shfl(base, 0, 64);
    for (long long eb = e0; eb < e1; eb += 64) {
        const long long e = eb + lane;
        const bool in = e < e1;
        const T v = in ? values[e] : (T)0;
        const int col = in ? indices[e] : -1;
        const bool keep = v != (T)0 && col >= g0 && col < g1;
        const u64 mask = __ballot(keep);
        const int pos = base + (int)__popcll(mask & ((1ull << lane) - 1ull));
        if (keep && pos >= 0 && pos < cap) {
            key[pos] = order_key(v);
            pay[pos] = ((u32)(col - g0) << GG_LABEL_BITS) | c;
        }
        base += (int)__popcll(mask);
    }
}

// the max-scan inputs: i where entry i starts a run, else 0
template <typename K>
struct ValueHead {                                      // ... of equal values, in the order of the value sort
    const K* key;
    __device__ int operator()(int i) const { return (i == 0 || key[i] != key[i - 1]) ? i : 0; }
};
struct RunHead {                                        // ... of one gene's equal values, in the order of the gene sort
    const u32* pay;
    const int* vid;
    __device__ int operator()(int i) const {
        return (i == 0 || (pay[i] >> GG_LABEL_BITS) != (pay[i - 1] >> GG_LABEL_BITS) || vid[i] != vid[i - 1]) ? i : 0;
    }
};

// the last entry of a run [s, i + 1) of gene g, whose entries begin at off[g] - off[g0]: the run's twice-midrank to mid2[s], its
// t^3 - t to T[g]
__global__ __launch_bounds__(256) void gg_run_tail_kernel(const u32* __restrict__ pay, const int* __restrict__ vid,
                                                          const int* __restrict__ start, int M, int g0, const long long* __restrict__ off,
                                                          const u64* __restrict__ neg, const u64* __restrict__ nzg, u64 N,
                                                          u32* __restrict__ mid2, u64* __restrict__ T) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const u32 gi = pay[i] >> GG_LABEL_BITS;
    if (i + 1 < M && (pay[i + 1] >> GG_LABEL_BITS) == gi && vid[i + 1] == vid[i]) return;
    const int g = g0 + (int)gi, s = start[i];
    const long long o = off[g] - off[g0];
    const u64 ks = (u64)(s - o), ke = (u64)(i + 1 - o), z = N - nzg[g];
    mid2[s] = (u32)(ks + ke + 1 + (ks >= neg[g] ? 2 * z : 0));
    const u64 t = ke - ks;
    if (t > 1) atomicAdd(&T[g], t * t * t - t);
}

// R2[label][gene] += the twice-midrank of every entry.  The entries lie gene after gene, so a workgroup's GG_ADD_ENTRIES consecutive
// entries belong to few genes: their sums per (gene, label) are formed in LDS (64-bit integer atomics), for the first
// GG_ADD_SLOTS / C genes of the chunk, and each goes to global memory once; entries of further genes - a chunk of many sparse genes
// and many groups - add to global memory themselves (19 M of those took 3.4 ms at 100 000 x 2 000).
constexpr int GG_ADD_ENTRIES = 4096, GG_ADD_SLOTS = 4096;
__global__ __launch_bounds__(256) void gg_rank_add_kernel(const u32* __restrict__ pay, const int* __restrict__ start,
                                                          const u32* __restrict__ mid2, int M, int g0, int G, int C,
                                                          u64* __restrict__ R2) {
    __shared__ u64 acc[GG_ADD_SLOTS];
    const int i0 = blockIdx.x * GG_ADD_ENTRIES, i1 = min(M, i0 + GG_ADD_ENTRIES);
    const u32 first = pay[i0] >> GG_LABEL_BITS, last = pay[i1 - 1] >> GG_LABEL_BITS;
    const u32 span = (u32)(GG_ADD_SLOTS / C);
    const int used = (int)min(span, last - first + 1) * C;
    for (int k = threadIdx.x; k < used; k += 256) acc[k] = 0;
    __syncthreads();
    for (int i = i0 + threadIdx.x; i < i1; i += 256) {
        const u32 p = pay[i], gi = p >> GG_LABEL_BITS, c = p & ((1u << GG_LABEL_BITS) - 1);
        const u64 v = mid2[start[i]];
        const u32 d = gi - first;
        if (d < span) atomicAdd(&acc[d * C + c], v);
        else atomicAdd(&R2[(size_t)c * G + g0 + (int)gi], v);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < used; k += 256)
        if (acc[k]) atomicAdd(&R2[(size_t)(k % C) * G + g0 + (int)first + k / C], acc[k]);
}

struct GroupRows {                                      // the used rows sorted by label, and their segments
    const int* rows;
    const u32* lab;
    const int* seg;
    int N, n_seg;
};
struct GroupOut { u64 *nnz, *R2, *T; };

// workspace of the two sorts and the scans of a stripe of M entries
template <typename K>
int sort_workspace(size_t M, size_t* bytes) {
    rocprim::double_buffer<K> kb(nullptr, nullptr);
    rocprim::double_buffer<u32> pb(nullptr, nullptr);
    rocprim::double_buffer<int> vb(nullptr, nullptr);
    size_t a = 0, b = 0, c = 0;
    FDX_HIP(rocprim::radix_sort_pairs(nullptr, a, kb, pb, M, 0, 8 * sizeof(K), (hipStream_t)0));
    FDX_HIP(rocprim::radix_sort_pairs(nullptr, b, pb, vb, M, GG_LABEL_BITS, 32, (hipStream_t)0));
    auto heads = rocprim::make_transform_iterator(rocprim::make_counting_iterator(0), RunHead{nullptr, nullptr});
    FDX_HIP(rocprim::inclusive_scan(nullptr, c, heads, (int*)nullptr, M, rocprim::maximum<int>(), (hipStream_t)0));
    *bytes = std::max(a, std::max(b, c));
    return 0;
}

// Steps 2 - 5 of the file comment.  nz_dev: nz_g per gene (gg_init_kernel); info: {stripes, entries of the largest, workspace bytes}
template <typename T>
int rank_stripes(const GeneMatrix& y, const T* data, const GroupRows& gr, int C, const u64* neg, const u64* nz_dev, size_t budget,
                 const GroupOut& o, long long* info, hipStream_t st) {
    using K = typename KeyOf<T>::type;
    const int G = y.G;
    std::vector<long long> off((size_t)G + 1, 0);
    FDX_TRY(copy_d2h(off.data() + 1, nz_dev, (size_t)G * sizeof(long long), st));
    for (int g = 0; g < G; ++g) off[g + 1] += off[g];
    // entries a stripe may hold: two key buffers, two payload buffers, the value names twice, and the workspace
    const size_t per_entry = 2 * sizeof(K) + 4 * sizeof(u32);
    long long m_cap = (long long)std::min<size_t>(budget / per_entry, (size_t)GG_STRIPE_ENTRIES_MAX);
    size_t ws = 0;
    FDX_TRY(sort_workspace<K>((size_t)std::max<long long>(m_cap, 1), &ws));
    if ((size_t)m_cap * per_entry + ws > budget) m_cap = budget > ws ? (long long)((budget - ws) / per_entry) : 0;
    std::vector<int> cut{0};                             // stripe s: genes [cut[s], cut[s + 1])
    long long m_max = 0;
    for (int g = 0; g < G;) {
        int g1 = g + 1;
        while (g1 < G && g1 - g < GG_STRIPE_GENES_MAX && off[g1 + 1] - off[g] <= m_cap) ++g1;
        m_max = std::max(m_max, off[g1] - off[g]);
        cut.push_back(g1);
        g = g1;
    }
    const int n_stripes = (int)cut.size() - 1;
    if (m_max > GG_STRIPE_ENTRIES_MAX) return fail(FDX_ERR_UNSUPPORTED, "gene group sums: a gene has more entries than a stripe holds");
    FDX_TRY(sort_workspace<K>((size_t)std::max<long long>(m_max, 1), &ws));
    if (info) {
        info[0] = n_stripes;
        info[1] = m_max;
        info[2] = (long long)((size_t)m_max * per_entry + ws);
    }
    if (m_max == 0) return 0;                           // no nonzero anywhere: the zero runs were everything
    DevBuf off_dev, cursor, keyA, keyB, payA, payB, vidA, vidB, tmp;
    FDX_TRY(off_dev.alloc(off.size() * sizeof(long long)));
    FDX_TRY(copy_h2d(off_dev.p, off.data(), off.size() * sizeof(long long), st));
    FDX_TRY(cursor.alloc((size_t)n_stripes * sizeof(int)));
    FDX_HIP(hipMemsetAsync(cursor.p, 0, (size_t)n_stripes * sizeof(int), st));
    FDX_TRY(keyA.alloc((size_t)m_max * sizeof(K)));
    FDX_TRY(keyB.alloc((size_t)m_max * sizeof(K)));
    FDX_TRY(payA.alloc((size_t)m_max * sizeof(u32)));
    FDX_TRY(payB.alloc((size_t)m_max * sizeof(u32)));
    FDX_TRY(vidA.alloc((size_t)m_max * sizeof(int)));
    FDX_TRY(vidB.alloc((size_t)m_max * sizeof(int)));
    FDX_TRY(tmp.alloc(ws));
    for (int s = 0; s < n_stripes; ++s) {
        const int g0 = cut[s], g1 = cut[s + 1], Gs = g1 - g0;
        const int M = (int)(off[g1] - off[g0]);
        if (M == 0) continue;
        if (y.sparse)
            hipLaunchKernelGGL(gg_compact_csr_kernel<T>, dim3((unsigned)ceil_div(gr.N, 4)), dim3(256), 0, st,
                               (const long long*)y.csr->indptr, y.csr->indices, data, gr.rows, gr.lab, gr.N, g0, g1, M,
                               cursor.as<int>() + s, keyA.as<K>(), payA.as<u32>());
        else
            hipLaunchKernelGGL(gg_compact_dense_kernel<T>, dim3((unsigned)ceil_div(Gs, 64), (unsigned)gr.n_seg), dim3(256), 0, st, data,
                               y.ldy, gr.rows, gr.seg, g0, Gs, M, cursor.as<int>() + s, keyA.as<K>(), payA.as<u32>());
        FDX_CHECK_LAUNCH();
        // by value over the stripe, then the names of the distinct values
        rocprim::double_buffer<K> kb(keyA.as<K>(), keyB.as<K>());
        rocprim::double_buffer<u32> pb(payA.as<u32>(), payB.as<u32>());
        // rocPRIM is asked before every call what it wants for THIS size (its choice of algorithm moves with the size)
        size_t bytes = 0;
        auto workspace = [&]() {
            if (bytes > tmp.bytes) FDX_TRY(tmp.alloc(bytes));
            return 0;
        };
        FDX_HIP(rocprim::radix_sort_pairs(nullptr, bytes, kb, pb, (size_t)M, 0, 8 * sizeof(K), st));
        FDX_TRY(workspace());
        FDX_HIP(rocprim::radix_sort_pairs(tmp.p, bytes, kb, pb, (size_t)M, 0, 8 * sizeof(K), st));
        auto vheads = rocprim::make_transform_iterator(rocprim::make_counting_iterator(0), ValueHead<K>{kb.current()});
        FDX_HIP(rocprim::inclusive_scan(nullptr, bytes, vheads, vidA.as<int>(), (size_t)M, rocprim::maximum<int>(), st));
        FDX_TRY(workspace());
        FDX_HIP(rocprim::inclusive_scan(tmp.p, bytes, vheads, vidA.as<int>(), (size_t)M, rocprim::maximum<int>(), st));
        // stable, by gene: bits 8 .. of the payload
        int bits = 1;
        while ((1u << bits) < (u32)Gs) ++bits;
        rocprim::double_buffer<int> vb(vidA.as<int>(), vidB.as<int>());
        FDX_HIP(rocprim::radix_sort_pairs(nullptr, bytes, pb, vb, (size_t)M, GG_LABEL_BITS, (unsigned)(GG_LABEL_BITS + bits), st));
        FDX_TRY(workspace());
        FDX_HIP(rocprim::radix_sort_pairs(tmp.p, bytes, pb, vb, (size_t)M, GG_LABEL_BITS, (unsigned)(GG_LABEL_BITS + bits), st));
        const u32* pay = pb.current();
        const int* vid = vb.current();
        // the key buffers are free now: run starts in one, the runs' twice-midranks in the other
        int* start = keyA.as<int>();
        u32* mid2 = keyB.as<u32>();
        auto rheads = rocprim::make_transform_iterator(rocprim::make_counting_iterator(0), RunHead{pay, vid});
        FDX_HIP(rocprim::inclusive_scan(nullptr, bytes, rheads, start, (size_t)M, rocprim::maximum<int>(), st));
        FDX_TRY(workspace());
        FDX_HIP(rocprim::inclusive_scan(tmp.p, bytes, rheads, start, (size_t)M, rocprim::maximum<int>(), st));
        const dim3 grid((unsigned)ceil_div(M, 256));
        hipLaunchKernelGGL(gg_run_tail_kernel, grid, dim3(256), 0, st, pay, vid, start, M, g0, off_dev.as<long long>(), neg, nz_dev,
                           (u64)gr.N, mid2, o.T);
        FDX_CHECK_LAUNCH();
        hipLaunchKernelGGL(gg_rank_add_kernel, dim3((unsigned)ceil_div(M, GG_ADD_ENTRIES)), dim3(256), 0, st, pay, start, mid2, M, g0, G,
                           C, o.R2);
        FDX_CHECK_LAUNCH();
    }
    if (info) info[2] = (long long)((size_t)m_max * per_entry + std::max(ws, tmp.bytes));    // what rocPRIM asked for on the way
    return 0;
}

int gene_group_entry(const char* who, const GeneMatrix& y, const int32_t* labels_dev, int32_t C, int64_t max_sort_bytes, double* u_dev,
                     double* q_dev, int64_t* nnz_dev, int64_t* R2_dev, int64_t* T_dev, int64_t* n_c_out, int64_t* N_out,
                     int64_t* info_out, void* stream) {
    const std::string w(who);
    FDX_TRY(check_gene_matrix(who, y, u_dev && q_dev && nnz_dev && R2_dev && T_dev && n_c_out && N_out && (y.n == 0 || labels_dev), true,
                              "bad shape"));
    FDX_REQUIRE(C >= 1 && C <= (1 << GG_LABEL_BITS), w + ": C must be 1 .. 256");
    FDX_REQUIRE(y.n >= 0 && y.n <= FDX_GENE_GROUP_MAX_ROWS, w + ": at most 2000000 rows (the tie sums are 64-bit integers)");
    FDX_REQUIRE(max_sort_bytes >= 0, w + ": max_sort_bytes < 0");
    hipStream_t st = (hipStream_t)stream;
    PoolStream pool_stream(st);
    const int n = (int)y.n, G = y.G;
    const size_t CG = (size_t)C * G;
    // the rows sorted by label (stable: ascending inside a group), the rows left out last
    DevBuf counts, lab_in, lab, rows, tmp;
    FDX_TRY(counts.alloc((size_t)(C + 2) * sizeof(u64)));
    FDX_HIP(hipMemsetAsync(counts.p, 0, (size_t)(C + 2) * sizeof(u64), st));
    FDX_TRY(lab_in.alloc((size_t)n * sizeof(u32)));
    FDX_TRY(lab.alloc((size_t)n * sizeof(u32)));
    FDX_TRY(rows.alloc((size_t)n * sizeof(int)));
    if (n > 0) {
        hipLaunchKernelGGL(gg_label_kernel, dim3((unsigned)std::min(ceil_div(n, 256), 1024)), dim3(256), 0, st, labels_dev, n, C,
                           lab_in.as<u32>(), counts.as<u64>());
        FDX_CHECK_LAUNCH();
        int bits = 1;
        while ((1 << bits) < C + 1) ++bits;
        auto iota = rocprim::make_counting_iterator(0);
        size_t bytes = 0;
        FDX_HIP(rocprim::radix_sort_pairs(nullptr, bytes, lab_in.as<u32>(), lab.as<u32>(), iota, rows.as<int>(), (size_t)n, 0, (unsigned)bits,
                                          st));
        FDX_TRY(tmp.alloc(bytes));
        FDX_HIP(rocprim::radix_sort_pairs(tmp.p, bytes, lab_in.as<u32>(), lab.as<u32>(), iota, rows.as<int>(), (size_t)n, 0, (unsigned)bits,
                                          st));
    }
    std::vector<u64> cnt((size_t)C + 2);
    FDX_TRY(copy_d2h(cnt.data(), counts.p, cnt.size() * sizeof(u64), st));
    FDX_REQUIRE(cnt[(size_t)C + 1] == 0, w + ": a label lies outside [-1, C)");
    std::vector<int> group_off((size_t)C + 1, 0), seg;
    for (int c = 0; c < C; ++c) {
        n_c_out[c] = (int64_t)cnt[c];
        group_off[c + 1] = group_off[c] + (int)cnt[c];
        for (int p = group_off[c]; p < group_off[c + 1]; p += SEG) {
            seg.push_back(p);
            seg.push_back(std::min(group_off[c + 1], p + SEG));
            seg.push_back(c);
        }
    }
    const int N = group_off[C], n_seg = (int)(seg.size() / 3);
    *N_out = N;
    if (info_out) info_out[0] = info_out[1] = info_out[2] = 0;
    // u and q: the weighted gene sums with W = 1 on these rows (B = W'Y is u once more and is dropped)
    {
        DevBuf ones, A, B;
        FDX_TRY(ones.alloc((size_t)n * sizeof(double)));
        FDX_TRY(A.alloc((size_t)C * sizeof(double)));
        FDX_TRY(B.alloc(CG * sizeof(double)));
        if (n > 0) {
            hipLaunchKernelGGL(gg_fill_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, ones.as<double>(), (long long)n, 1.0);
            FDX_CHECK_LAUNCH();
        }
        FDX_TRY(launch_weighted_gene_sums(y, ones.as<double>(), 1, 1, rows.as<int>(), group_off.data(), C, A.as<double>(), B.as<double>(),
                                          q_dev, u_dev, st));
    }
    const GroupOut out{(u64*)nnz_dev, (u64*)R2_dev, (u64*)T_dev};
    FDX_HIP(hipMemsetAsync(nnz_dev, 0, CG * sizeof(u64), st));
    if (N == 0) {
        FDX_HIP(hipMemsetAsync(R2_dev, 0, CG * sizeof(u64), st));
        FDX_HIP(hipMemsetAsync(T_dev, 0, (size_t)G * sizeof(u64), st));
        return 0;
    }
    DevBuf seg_dev, neg, nzg;
    FDX_TRY(seg_dev.alloc(seg.size() * sizeof(int)));
    FDX_TRY(copy_h2d(seg_dev.p, seg.data(), seg.size() * sizeof(int), st));
    FDX_TRY(neg.alloc((size_t)G * sizeof(u64)));
    FDX_TRY(nzg.alloc((size_t)G * sizeof(u64)));
    FDX_HIP(hipMemsetAsync(neg.p, 0, (size_t)G * sizeof(u64), st));
    const GroupRows gr{rows.as<int>(), lab.as<u32>(), seg_dev.as<int>(), N, n_seg};
    FDX_TRY(dispatch_gene_matrix(
        y,
        [&](auto* Yd) {
            using T = std::remove_cv_t<std::remove_pointer_t<decltype(Yd)>>;
            hipLaunchKernelGGL(gg_count_dense_kernel<T>, dim3((unsigned)ceil_div(G, 64), (unsigned)n_seg), dim3(256), 0, st, Yd, y.ldy,
                               gr.rows, gr.seg, G, out.nnz, neg.as<u64>());
            FDX_CHECK_LAUNCH();
            return 0;
        },
        [&](auto* values) {
            using T = std::remove_cv_t<std::remove_pointer_t<decltype(values)>>;
            hipLaunchKernelGGL(gg_count_csr_kernel<T>, dim3((unsigned)ceil_div(N, 4)), dim3(256), 0, st, (const long long*)y.csr->indptr,
                               y.csr->indices, values, gr.rows, gr.lab, N, G, out.nnz, neg.as<u64>());
            FDX_CHECK_LAUNCH();
            return 0;
        }));
    hipLaunchKernelGGL(gg_init_kernel, dim3((unsigned)ceil_div(G, 256)), dim3(256), 0, st, out.nnz, neg.as<u64>(), counts.as<u64>(), C, G,
                       (u64)N, nzg.as<u64>(), out.R2, out.T);
    FDX_CHECK_LAUNCH();
    const size_t budget = max_sort_bytes > 0 ? (size_t)max_sort_bytes : SCRATCH_BUDGET_BYTES;
    auto ranks = [&](auto* data) { return rank_stripes(y, data, gr, C, neg.as<u64>(), nzg.as<u64>(), budget, out, (long long*)info_out, st); };
    return dispatch_gene_matrix(y, ranks, ranks);
}

}  // namespace
}  // namespace fdx

using namespace fdx;

extern "C" {

int fdx_gene_group_sums_dev(const void* Y_dev, int32_t dtype, int64_t n, int32_t G, int64_t ldy, const int32_t* labels_dev, int32_t C,
                            int64_t max_sort_bytes, double* u_dev, double* q_dev, int64_t* nnz_dev, int64_t* R2_dev, int64_t* T_dev,
                            int64_t* n_c_out, int64_t* N_out, int64_t* info_out, void* stream) {
    return gene_group_entry("fdx_gene_group_sums_dev", GeneMatrix(Y_dev, dtype, n, G, ldy), labels_dev, C, max_sort_bytes, u_dev, q_dev,
                            nnz_dev, R2_dev, T_dev, n_c_out, N_out, info_out, stream);
}

int fdx_gene_group_sums_csr_dev(const fdx_csr_view* Y, const int32_t* labels_dev, int32_t C, int64_t max_sort_bytes, double* u_dev,
                                double* q_dev, int64_t* nnz_dev, int64_t* R2_dev, int64_t* T_dev, int64_t* n_c_out, int64_t* N_out,
                                int64_t* info_out, void* stream) {
    return gene_group_entry("fdx_gene_group_sums_csr_dev", GeneMatrix(Y), labels_dev, C, max_sort_bytes, u_dev, q_dev, nnz_dev, R2_dev,
                            T_dev, n_c_out, N_out, info_out, stream);
}

}  // extern "C"
