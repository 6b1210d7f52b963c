// Cell-type expression in tissue (additive, not in the reference): the sufficient statistics of the per-gene regressions
// Y[:, g] ~ W s_g, s_g >= 0 over groups of rows - A = W'W, B = W'Y, q = sum y^2, u = sum y - from one pass over Y as it lies in HBM
// (float32 / float64 dense with any row stride, or CSR), and the G x C small non-negative solves (include/fdx.h has the definitions).
//
// Order of the sums.  The rows of a group, in the order of the sorted row list, are cut into SEGMENTS of FDX_EXPRESSION_SEGMENT_ROWS
// rows; a segment is summed row after row into zeroed accumulators (fma), its sums go to a scratch block, and the fold adds the
// segment sums of a group in ascending order.  That order is a function of the row list alone; gene_pass.h has the rule for what
// changes no bit of it (stripe, batches of segments, the thread of a gene) and the fold.
//
// Dense: a thread per two gene columns (coalesced rows), a chunk of 32 (last chunk: 16) accumulators per gene in registers, the
// weights of a row wave-uniform from a padded copy of W in segment order (Wp), staged in LDS 64 rows at a time and read by
// broadcast; more than 32 types re-read Y per chunk.  A = W'W is the
// same kernel with Y := Wp.  CSR: a workgroup per (stripe, 8 types) walks its rows in order, a barrier after each; a thread owns
// (entry slot, type) and adds into the segment's block [gene][type] in global memory - the entries of a row have distinct columns,
// so no two threads meet between barriers; rows need not be sorted.
#include <algorithm>
#include <vector>

#include "fdx_internal.h"
#include "fdx_kernels.h"
#include "gene_pass.h"

namespace fdx {
namespace {

constexpr int SEG = FDX_EXPRESSION_SEGMENT_ROWS;
constexpr int EXPR_KC = 32, EXPR_KC_TAIL = 16;   // accumulators a thread of the dense kernel keeps: full chunks, and a last chunk of <= 16
constexpr int EXPR_CSR_KC = 8;                   // types a workgroup of the CSR kernel adds per pass over its rows
constexpr int EXPR_NNLS_LDS_MAX_K = 88;          // the solve keeps A_c in LDS up to here (88 * 88 doubles < 64 KB), reads it through L2 above

// Wp (n_sel, Kpad): row p = W[rows[p]] (rows null: W[p]), zeros in columns K .. Kpad - 1
__global__ __launch_bounds__(256) void expr_gather_w_kernel(const double* __restrict__ W, long long ldw, const int* __restrict__ rows,
                                                            long long n_sel, int K, int Kpad, double* __restrict__ Wp) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_sel * Kpad) return;
    const long long p = idx / Kpad;
    const int k = (int)(idx - p * Kpad);
    const long long r = rows ? (long long)rows[p] : p;
    Wp[idx] = k < K ? W[r * ldw + k] : 0.0;
}

// part[s][k0 + k][j] = sum over the rows of segment s of Wp[p][k0 + k] * Y[row(p)][j]; with qu also planes Kpad (sum y^2) and
// Kpad + 1 (sum y).  seg: {first, end} positions per segment; workgroup x takes segments [x * stripe, (x + 1) * stripe).
// A workgroup owns 512 genes, two per thread (j and j + 256: each weight read feeds two fma), and walks its segment in blocks of
// EXPR_RB rows: the block's weights (and row numbers) are staged in LDS - the next block while this one is summed, one barrier per
// block - and read back by broadcast; Y is read eight rows ahead into registers.  Positions past the segment's end hold weight 0
// and value 0: fma(0, 0, acc) leaves acc as it is.
constexpr int EXPR_RB = 64, EXPR_GENES = 512, EXPR_CSR_UNROLL = 8;

template <typename T, int KC>
__global__ __launch_bounds__(256) void expr_dense_kernel(const T* __restrict__ Y, long long ldy, const int* __restrict__ yrows,
                                                         const double* __restrict__ Wp, int Kpad, int k0, const int* __restrict__ seg,
                                                         int n_seg, int stripe, int G, int qu, double* __restrict__ part, int planes) {
    __shared__ double wsh[2][EXPR_RB * KC];
    __shared__ int rsh[2][EXPR_RB];
    const int tid = threadIdx.x;
    const int j0 = blockIdx.y * EXPR_GENES + tid, j1 = j0 + 256;
    const bool ok0 = j0 < G, ok1 = j1 < G;
    const T* y0p = Y + (ok0 ? j0 : 0);
    const T* y1p = Y + (ok1 ? j1 : 0);
    const int s0 = blockIdx.x * stripe, s1 = min(n_seg, s0 + stripe);
    for (int s = s0; s < s1; ++s) {
        const int p0 = seg[2 * s], p1 = seg[2 * s + 1];
        auto stage = [&](int buf, int pb) {
#pragma unroll
            for (int t = 0; t < EXPR_RB * KC / 256; ++t) {
                const int e = tid + 256 * t, r = e / KC, k = e % KC;
                const int p = pb + r;
                wsh[buf][e] = p < p1 ? Wp[(size_t)p * Kpad + k0 + k] : 0.0;
            }
            if (tid < EXPR_RB) {
                const int p = pb + tid;
                rsh[buf][tid] = p < p1 ? (yrows ? yrows[p] : p) : -1;
            }
        };
        double acc0[KC], acc1[KC];
#pragma unroll
        for (int k = 0; k < KC; ++k) acc0[k] = acc1[k] = 0.0;
        double q0 = 0.0, u0 = 0.0, q1 = 0.0, u1 = 0.0;
        __syncthreads();                            // the previous segment's last block has been read
        stage(0, p0);
        __syncthreads();
        int buf = 0;
        for (int pb = p0; pb < p1; pb += EXPR_RB, buf ^= 1) {
            if (pb + EXPR_RB < p1) stage(buf ^ 1, pb + EXPR_RB);
            T c0[8], c1[8], n0[8], n1[8];
            auto load8 = [&](int r8, T (&v0)[8], T (&v1)[8]) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int row = rsh[buf][r8 + i];
                    v0[i] = row >= 0 ? y0p[(long long)row * ldy] : (T)0;
                    v1[i] = row >= 0 ? y1p[(long long)row * ldy] : (T)0;
                }
            };
            load8(0, c0, c1);
            for (int r8 = 0; r8 < EXPR_RB; r8 += 8) {
                if (r8 + 8 < EXPR_RB) load8(r8 + 8, n0, n1);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const double ya = (double)c0[i], yb = (double)c1[i];
                    const double* w = &wsh[buf][(r8 + i) * KC];
#pragma unroll
                    for (int k = 0; k < KC; ++k) {
                        const double wk = w[k];
                        acc0[k] = fma(wk, ya, acc0[k]);
                        acc1[k] = fma(wk, yb, acc1[k]);
                    }
                    q0 = fma(ya, ya, q0);
                    u0 += ya;
                    q1 = fma(yb, yb, q1);
                    u1 += yb;
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    c0[i] = n0[i];
                    c1[i] = n1[i];
                }
            }
            __syncthreads();                        // the next block is staged, this one has been read
        }
        double* out = part + (size_t)s * planes * G;
        if (ok0) {
#pragma unroll
            for (int k = 0; k < KC; ++k) out[(size_t)(k0 + k) * G + j0] = acc0[k];
            if (qu) {
                out[(size_t)Kpad * G + j0] = q0;
                out[(size_t)(Kpad + 1) * G + j0] = u0;
            }
        }
        if (ok1) {
#pragma unroll
            for (int k = 0; k < KC; ++k) out[(size_t)(k0 + k) * G + j1] = acc1[k];
            if (qu) {
                out[(size_t)Kpad * G + j1] = q1;
                out[(size_t)(Kpad + 1) * G + j1] = u1;
            }
        }
    }
}

// part[s][g][k] (k < Kpad) and qu_part[s][{q, u}][g] for the segments of this launch; grid (stripes, Kpad / 8); thread = (entry slot
// tid >> 3 of 32, type 8 * blockIdx.y + (tid & 7)).  A row's entries have distinct columns: between two barriers every element of the
// block has one owner.
template <typename T>
__global__ __launch_bounds__(256) void expr_csr_kernel(const long long* __restrict__ indptr, const int* __restrict__ indices,
                                                       const T* __restrict__ values, const int* __restrict__ yrows,
                                                       const double* __restrict__ Wp, int Kpad, const int* __restrict__ seg, int n_seg,
                                                       int stripe, int G, double* part, double* qu_part) {
    const int slot = threadIdx.x >> 3, k = blockIdx.y * EXPR_CSR_KC + (threadIdx.x & 7);
    const bool qu = blockIdx.y == 0 && (threadIdx.x & 7) == 0;
    const int s0 = blockIdx.x * stripe, s1 = min(n_seg, s0 + stripe);
    for (int s = s0; s < s1; ++s) {
        double* P = part + (size_t)s * G * Kpad + k;
        double* Q = qu_part + (size_t)s * 2 * G;
        for (int g = slot; g < G; g += 32) P[(size_t)g * Kpad] = 0.0;
        if (blockIdx.y == 0)
            for (int g = threadIdx.x; g < 2 * G; g += 256) Q[g] = 0.0;
        __syncthreads();
        const int p0 = seg[2 * s], p1 = seg[2 * s + 1];
        for (int p = p0; p < p1; ++p) {
            const long long r = yrows ? (long long)yrows[p] : (long long)p;
            const long long e0 = indptr[r], e1 = indptr[r + 1];
            const double w = Wp[(size_t)p * Kpad + k];
            // eight entries of the row per thread and step: their columns differ, so the eight read-add-writes are independent
            // and their loads go out together (one after the other, each waits a memory round trip for the one before)
            for (long long e = e0 + slot; e < e1; e += 32 * EXPR_CSR_UNROLL) {
                int c[EXPR_CSR_UNROLL];
                double y[EXPR_CSR_UNROLL], v[EXPR_CSR_UNROLL], vq[EXPR_CSR_UNROLL], vu[EXPR_CSR_UNROLL];
#pragma unroll
                for (int i = 0; i < EXPR_CSR_UNROLL; ++i) {
                    const long long ei = e + 32 * i;
                    const bool in = ei < e1;
                    c[i] = in ? indices[ei] : -1;
                    y[i] = in ? (double)values[ei] : 0.0;
                }
#pragma unroll
                for (int i = 0; i < EXPR_CSR_UNROLL; ++i) {
                    v[i] = c[i] >= 0 ? P[(size_t)c[i] * Kpad] : 0.0;
                    vq[i] = qu && c[i] >= 0 ? Q[c[i]] : 0.0;
                    vu[i] = qu && c[i] >= 0 ? Q[G + c[i]] : 0.0;
                }
#pragma unroll
                for (int i = 0; i < EXPR_CSR_UNROLL; ++i) {
                    if (c[i] >= 0) {
                        P[(size_t)c[i] * Kpad] = fma(w, y[i], v[i]);
                        if (qu) {
                            Q[c[i]] = fma(y[i], y[i], vq[i]);
                            Q[G + c[i]] = vu[i] + y[i];
                        }
                    }
                }
            }
            __syncthreads();                        // the next row adds after this one: fixed order per (gene, type)
        }
    }
}

__device__ __forceinline__ double readlane_f64(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// One wave per (group blockIdx.y, gene): lane l holds s_k and t_k = (A s - b)_k for k = l + 64 u, u < T.  A_c in LDS (LDS_A: K <=
// EXPR_NNLS_LDS_MAX_K, staged once per workgroup of 4 genes) or read through L2; row k serves as column k (A_c is symmetric).
template <int T, bool LDS_A>
__global__ __launch_bounds__(256) void nnls_gram_kernel(const double* __restrict__ A, const double* __restrict__ B,
                                                        const double* __restrict__ q, int K, int G, double ridge, int max_iter,
                                                        double tol, double* __restrict__ S, int* __restrict__ n_iter,
                                                        int* __restrict__ converged, double* __restrict__ rss) {
    extern __shared__ double a_sh[];
    const int c = blockIdx.y;
    const double* Ac = A + (size_t)c * K * K;
    if (LDS_A) {
        for (int i = threadIdx.x; i < K * K; i += 256) a_sh[i] = Ac[i];
        __syncthreads();
    }
    const double* Am = LDS_A ? a_sh : Ac;
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (g >= G) return;
    double dsum = 0.0;
    for (int k = 0; k < K; ++k) dsum += Am[(size_t)k * K + k];
    const double rd = ridge * (dsum / (double)K);
    const double* b = B + (size_t)c * K * G + g;
    double s[T], t[T];
#pragma unroll
    for (int u = 0; u < T; ++u) {
        const int k = lane + 64 * u;
        s[u] = 0.0;
        t[u] = k < K ? -b[(size_t)k * G] : 0.0;
    }
    int it = 1, cv = 0;
    for (; it <= max_iter; ++it) {
        double dmax = 0.0, smax = 0.0;
#pragma unroll
        for (int v = 0; v < T; ++v) {
            const int kend = min(64, K - 64 * v);
            for (int kl = 0; kl < kend; ++kl) {
                const int k = 64 * v + kl;
                const double sk = readlane_f64(s[v], kl), tk = readlane_f64(t[v], kl);
                const double akk = Am[(size_t)k * K + k];
                const double D = akk + rd;
                double nw = 0.0;
                if (D > 0.0) nw = fmax(0.0, fma(akk, sk, -tk) / D);
                const double delta = nw - sk;
                dmax = fmax(dmax, fabs(delta));
                smax = fmax(smax, nw);
                if (delta != 0.0) {
                    if (lane == kl) s[v] = nw;
#pragma unroll
                    for (int u = 0; u < T; ++u) {
                        const int j = lane + 64 * u;
                        if (j < K) t[u] = fma(Am[(size_t)k * K + j], delta, t[u]);
                    }
                }
            }
        }
        if (dmax <= tol * smax) {
            cv = 1;
            break;
        }
    }
#pragma unroll
    for (int u = 0; u < T; ++u) {
        const int k = lane + 64 * u;
        if (k < K) S[((size_t)c * K + k) * G + g] = s[u];
    }
    if (lane == 0) {
        n_iter[(size_t)c * G + g] = cv ? it : max_iter;
        converged[(size_t)c * G + g] = cv;
    }
    if (rss) {                                      // s' A s with A s formed afresh, s.b: fixed butterfly over the lanes
        double as[T];
#pragma unroll
        for (int u = 0; u < T; ++u) as[u] = 0.0;
#pragma unroll
        for (int v = 0; v < T; ++v) {
            const int kend = min(64, K - 64 * v);
            for (int kl = 0; kl < kend; ++kl) {
                const int k = 64 * v + kl;
                const double sk = readlane_f64(s[v], kl);
                if (sk != 0.0) {
#pragma unroll
                    for (int u = 0; u < T; ++u) {
                        const int j = lane + 64 * u;
                        if (j < K) as[u] = fma(Am[(size_t)k * K + j], sk, as[u]);
                    }
                }
            }
        }
        double sb = 0.0, sas = 0.0;
#pragma unroll
        for (int u = 0; u < T; ++u) {
            const int k = lane + 64 * u;
            if (k < K) {
                sb = fma(s[u], b[(size_t)k * G], sb);
                sas = fma(s[u], as[u], sas);
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            sb += __shfl_xor(sb, off, 64);
            sas += __shfl_xor(sas, off, 64);
        }
        if (lane == 0) rss[(size_t)c * G + g] = fmax(0.0, q[(size_t)c * G + g] - 2.0 * sb + sas);
    }
}

// The segments of the weighted sums on the device: {first, end} positions per segment, the C + 1 segment offsets of the groups
struct ExprSegments { const int *seg, *group_seg; int n_seg, C; };
// out (C, planes, G) = the planes plane0 .. of the batch b folded per group: sums only
int fold_groups(const SegmentBlocks& b, int plane0, int planes, int G, const ExprSegments& sg, double* out, hipStream_t st) {
    return launch_gene_fold(b, plane0, planes, G, sg.group_seg, sg.C, out, (long long)planes * G, (long long)G, -1, -1, st);
}

// One dense pass over `Yd` (n_sel positions through yrows) for all chunks of Wp, in batches of segments, folded into `out`
// (planes 0 .. K - 1 -> out[c][k][g]) and, with q_out / u_out, the two moment planes.
template <typename T>
int dense_passes(const T* Yd, long long ldy, const int* yrows, const double* Wp, int K, int Kpad, const ExprSegments& sg, int G,
                 double* out, double* q_out, double* u_out, hipStream_t st) {
    const bool qu = q_out != nullptr;
    const int planes = Kpad + (qu ? 2 : 0);
    const int stripe = stripe_segments();
    return for_segment_batches(sg.n_seg, (size_t)planes * G * sizeof(double), [&](int sb0, int nb, double* part) {
        const dim3 grid((unsigned)ceil_div(nb, stripe), (unsigned)ceil_div(G, EXPR_GENES));
        for (int k0 = 0; k0 < Kpad;) {
            const bool full = Kpad - k0 >= EXPR_KC;
            auto* kernel = full ? expr_dense_kernel<T, EXPR_KC> : expr_dense_kernel<T, EXPR_KC_TAIL>;
            hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, Yd, ldy, yrows, Wp, Kpad, k0, sg.seg + 2 * (size_t)sb0, nb, stripe, G,
                               qu && k0 == 0, part, planes);      // the moment planes ride with the first chunk
            FDX_CHECK_LAUNCH();
            k0 += full ? EXPR_KC : EXPR_KC_TAIL;
        }
        const SegmentBlocks b{part, (long long)planes * G, (long long)G, 1LL, sb0, nb};
        FDX_TRY(fold_groups(b, 0, K, G, sg, out, st));
        if (!qu) return 0;
        FDX_TRY(fold_groups(b, Kpad, 1, G, sg, q_out, st));
        return fold_groups(b, Kpad + 1, 1, G, sg, u_out, st);
    });
}

// The CSR pass: a batch's scratch is [segment][gene][type] for the batch's segments, then [segment][{q, u}][gene]
template <typename T>
int csr_passes(const fdx_csr_view* Y, const T* values, const int* yrows, const double* Wp, int K, int Kpad, const ExprSegments& sg, double* B,
               double* q_out, double* u_out, hipStream_t st) {
    const int G = Y->G;
    const int stripe = stripe_segments();
    const size_t seg_bytes = (size_t)(Kpad + 2) * G * sizeof(double);
    const size_t qu_offset = (size_t)segment_batch(sg.n_seg, seg_bytes) * G * Kpad;
    return for_segment_batches(sg.n_seg, seg_bytes, [&](int sb0, int nb, double* part) {
        double* qu_part = part + qu_offset;
        hipLaunchKernelGGL(expr_csr_kernel<T>, dim3((unsigned)ceil_div(nb, stripe), (unsigned)(Kpad / EXPR_CSR_KC)), dim3(256), 0, st,
                           (const long long*)Y->indptr, Y->indices, values, yrows, Wp, Kpad, sg.seg + 2 * (size_t)sb0, nb,
                           stripe, G, part, qu_part);
        FDX_CHECK_LAUNCH();
        const SegmentBlocks b{part, (long long)G * Kpad, 1LL, (long long)Kpad, sb0, nb}, m{qu_part, 2LL * G, (long long)G, 1LL, sb0, nb};
        FDX_TRY(fold_groups(b, 0, K, G, sg, B, st));
        FDX_TRY(fold_groups(m, 0, 1, G, sg, q_out, st));
        return fold_groups(m, 1, 1, G, sg, u_out, st);
    });
}

}  // namespace

// group_off on the HOST (fdx.h).  Everything queued on st; scratch from the pool.  Declared in gene_pass.h: the marker-gene sums
// (gene_group_kernels.cpp) take their u and q from here.
int launch_weighted_gene_sums(const GeneMatrix& y, const double* W, long long ldw, int K, const int* rows, const int* group_off, int C,
                              double* A, double* B, double* q, double* u, hipStream_t st) {
    // the segments of every group, as positions of the sorted row list
    std::vector<int> tab;                          // {first, end} per segment, then the C + 1 segment offsets of the groups
    std::vector<int> gseg((size_t)C + 1);
    for (int c = 0; c < C; ++c) {
        const long long lo = rows ? group_off[c] : 0, hi = rows ? group_off[c + 1] : y.n;
        gseg[c] = (int)(tab.size() / 2);
        for (long long p = lo; p < hi; p += SEG) {
            tab.push_back((int)p);
            tab.push_back((int)std::min<long long>(hi, p + SEG));
        }
    }
    const int n_seg = (int)(tab.size() / 2);
    gseg[C] = n_seg;
    const long long n_sel = rows ? group_off[C] : y.n;
    if (n_seg == 0) {                              // nothing listed: every sum is empty
        FDX_HIP(hipMemsetAsync(A, 0, (size_t)C * K * K * sizeof(double), st));
        FDX_HIP(hipMemsetAsync(B, 0, (size_t)C * K * y.G * sizeof(double), st));
        FDX_HIP(hipMemsetAsync(q, 0, (size_t)C * y.G * sizeof(double), st));
        FDX_HIP(hipMemsetAsync(u, 0, (size_t)C * y.G * sizeof(double), st));
        return 0;
    }
    tab.insert(tab.end(), gseg.begin(), gseg.end());
    const int Kpad = (int)round_up(K, EXPR_KC_TAIL);
    if ((n_sel * Kpad + 255) / 256 > 0x7fffffffLL) return fail(FDX_ERR_UNSUPPORTED, "weighted gene sums: too many rows for one call");
    DevBuf tab_dev, wp;
    FDX_TRY(tab_dev.alloc(tab.size() * sizeof(int)));
    FDX_TRY(wp.alloc((size_t)n_sel * Kpad * sizeof(double)));
    FDX_TRY(copy_h2d(tab_dev.p, tab.data(), tab.size() * sizeof(int), st));
    const ExprSegments sg{tab_dev.as<int>(), tab_dev.as<int>() + 2 * (size_t)n_seg, n_seg, C};
    double* Wp = wp.as<double>();
    hipLaunchKernelGGL(expr_gather_w_kernel, dim3((unsigned)ceil_div(n_sel * Kpad, 256)), dim3(256), 0, st, W, ldw, rows, n_sel, K, Kpad,
                       Wp);
    FDX_CHECK_LAUNCH();
    // A = W'W: the dense pass with Y := Wp (already in segment order)
    FDX_TRY(dense_passes(Wp, (long long)Kpad, nullptr, Wp, K, Kpad, sg, K, A, nullptr, nullptr, st));
    return dispatch_gene_matrix(
        y, [&](auto* Yd) { return dense_passes(Yd, y.ldy, rows, Wp, K, Kpad, sg, y.G, B, q, u, st); },
        [&](auto* values) { return csr_passes(y.csr, values, rows, Wp, K, Kpad, sg, B, q, u, st); });
}

namespace {

int launch_nnls_gram(const double* A, const double* B, const double* q, int C, int K, int G, double ridge, int max_iter, double tol,
                     double* S, int* n_iter, int* converged, double* rss, hipStream_t st) {
    const dim3 grid((unsigned)ceil_div(G, 4), (unsigned)C);
    const int T = ceil_div(K, 64);
#define FDX_NNLS(T_, LDS_, BYTES_)                                                                                                   \
    hipLaunchKernelGGL((nnls_gram_kernel<T_, LDS_>), grid, dim3(256), BYTES_, st, A, B, q, K, G, ridge, max_iter, tol, S, n_iter, \
                       converged, rss)
    const size_t lds = (size_t)K * K * sizeof(double);
    if (K <= EXPR_NNLS_LDS_MAX_K) {
        if (T == 1) FDX_NNLS(1, true, lds);
        else FDX_NNLS(2, true, lds);
    } else if (T == 2) FDX_NNLS(2, false, 0);
    else if (T == 3) FDX_NNLS(3, false, 0);
    else if (T == 4) FDX_NNLS(4, false, 0);
    else FDX_NNLS(5, false, 0);
#undef FDX_NNLS
    FDX_CHECK_LAUNCH();
    return 0;
}

int check_groups(const char* who, int64_t n, int32_t K, int64_t ldw, const int32_t* rows_dev, const int32_t* group_off, int32_t C) {
    const std::string w(who);
    FDX_REQUIRE(K >= 1 && K <= FDX_EXPRESSION_MAX_K, w + ": K must be 1 .. 272");
    FDX_REQUIRE(ldw >= K, w + ": ldw < K");
    FDX_REQUIRE(n >= 0 && n < 0x7fffff00LL, w + ": n out of range");
    FDX_REQUIRE(C >= 1 && C <= 65535, w + ": C must be 1 .. 65535");
    if (!rows_dev) {
        FDX_REQUIRE(C == 1, w + ": rows_dev == NULL means one group of all rows (C = 1)");
        return 0;
    }
    FDX_REQUIRE(group_off && group_off[0] == 0, w + ": group_off must start at 0");
    for (int c = 0; c < C; ++c) FDX_REQUIRE(group_off[c] <= group_off[c + 1], w + ": group_off must ascend");
    FDX_REQUIRE(group_off[C] <= n, w + ": more rows listed than Y has");
    return 0;
}

int weighted_gene_sums_entry(const char* who, const GeneMatrix& y, const double* W_dev, int64_t ldw, int32_t K, const int32_t* rows_dev,
                             const int32_t* group_off, int32_t C, double* A_dev, double* B_dev, double* q_dev, double* u_dev,
                             void* stream) {
    FDX_TRY(check_gene_matrix(who, y, A_dev && B_dev && q_dev && u_dev && (y.n == 0 || W_dev), true, "bad shape"));
    FDX_TRY(check_groups(who, y.n, K, ldw, rows_dev, group_off, C));
    PoolStream pool_stream((hipStream_t)stream);
    return launch_weighted_gene_sums(y, W_dev, ldw, K, rows_dev, group_off, C, A_dev, B_dev, q_dev, u_dev, (hipStream_t)stream);
}

}  // namespace
}  // namespace fdx

using namespace fdx;

extern "C" {

int fdx_weighted_gene_sums_dev(const void* Y_dev, int32_t dtype, int64_t n, int32_t G, int64_t ldy, const double* W_dev, int64_t ldw,
                               int32_t K, const int32_t* rows_dev, const int32_t* group_off, int32_t C, double* A_dev, double* B_dev,
                               double* q_dev, double* u_dev, void* stream) {
    return weighted_gene_sums_entry("fdx_weighted_gene_sums_dev", GeneMatrix(Y_dev, dtype, n, G, ldy), W_dev, ldw, K, rows_dev, group_off, C,
                                    A_dev, B_dev, q_dev, u_dev, stream);
}

int fdx_weighted_gene_sums_csr_dev(const fdx_csr_view* Y, const double* W_dev, int64_t ldw, int32_t K, const int32_t* rows_dev,
                                   const int32_t* group_off, int32_t C, double* A_dev, double* B_dev, double* q_dev, double* u_dev,
                                   void* stream) {
    return weighted_gene_sums_entry("fdx_weighted_gene_sums_csr_dev", GeneMatrix(Y), W_dev, ldw, K, rows_dev, group_off, C, A_dev, B_dev,
                                    q_dev, u_dev, stream);
}

int fdx_nnls_gram_dev(const double* A_dev, const double* B_dev, const double* q_dev, int32_t C, int32_t K, int32_t G, double ridge,
                      int32_t max_iter, double tol, double* S_dev, int32_t* n_iter_dev, int32_t* converged_dev, double* rss_dev,
                      void* stream) {
    FDX_REQUIRE(A_dev && B_dev && S_dev && n_iter_dev && converged_dev, "fdx_nnls_gram_dev: null argument");
    FDX_REQUIRE((q_dev != nullptr) == (rss_dev != nullptr), "fdx_nnls_gram_dev: q_dev and rss_dev go together");
    FDX_REQUIRE(K >= 1 && K <= FDX_EXPRESSION_MAX_K, "fdx_nnls_gram_dev: K must be 1 .. 272");
    FDX_REQUIRE(G >= 1 && C >= 1 && C <= 65535, "fdx_nnls_gram_dev: bad shape");
    FDX_REQUIRE(ridge >= 0.0 && max_iter >= 1 && tol > 0.0, "fdx_nnls_gram_dev: ridge >= 0, max_iter >= 1 and tol > 0 are required");
    hipStream_t st = (hipStream_t)stream;
    PoolStream pool_stream(st);
    return launch_nnls_gram(A_dev, B_dev, q_dev, C, K, G, ridge, max_iter, tol, S_dev, n_iter_dev, converged_dev, rss_dev, st);
}

}  // extern "C"
