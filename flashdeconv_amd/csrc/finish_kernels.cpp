// End-of-solve kernels.
//   objective_partials  <- flashdeconv/core/solver.py:226-284 (compute_objective) with L = D - A
//                          (flashdeconv/core/spatial.py:70-73); includes the Laplacian SpMV.
//   normalize_export    <- flashdeconv/core/solver.py:431-452 (normalize_proportions) fused with the layout change
//                          from the solver's type-major / Morton-ordered beta to the reference's (n_spots, n_types)
//                          row-major arrays in the caller's spot order.
//   spot_diagnostics    <- the per-spot terms of that objective, kept instead of summed (not in the reference): the squared
//                          sketch residual, the squared norm of the sketched row, the neighbour disagreement.
// All map one lane to one spot (coalesced reads of the type planes) and stage the wave's 64 x K tile in LDS.
#include "fdx_internal.h"
#include "fdx_kernels.h"

namespace fdx {

// obj = 0.5*(YtY - 2*cross + quad) + 0.5*lambda*spat + rho*l1 ; this kernel emits per-block (cross, quad, spat, l1).
__global__ __launch_bounds__(256) void objective_partials_kernel(
    const double* __restrict__ beta, long long ld, const double* __restrict__ H, long long ldh,
    const double* __restrict__ XtX, const int* __restrict__ ell_base, const int* __restrict__ slice_off,
    const int* __restrict__ deg, int n, int n_slices, int K, int use_lds, int skip_quad, double* __restrict__ partials) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    __shared__ double red[4][4];
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int slice = blockIdx.x * 4 + wib;
    double cross = 0.0, quad = 0.0, spat = 0.0, l1 = 0.0;
    if (slice < n_slices) {
        const int i = slice * 64 + lane;
        const bool active = i < n;
        const int ii = active ? i : n - 1;
        double* tile = smem + (size_t)wib * K * 64;  // [k][lane]
        if (use_lds)
            for (int k = 0; k < K; ++k) tile[k * 64 + lane] = beta[(size_t)k * ld + ii];
        const int w0 = slice_off[slice];
        const int w = slice_off[slice + 1] - w0;
        const int* ell = ell_base + (size_t)w0 * 64 + lane;
        const double dg = (double)deg[ii];
        for (int k = 0; k < K; ++k) {
            const double bk = use_lds ? tile[k * 64 + lane] : beta[(size_t)k * ld + ii];
            double nb = 0.0;
            for (int m = 0; m < w; ++m) nb += beta[(size_t)k * ld + ell[(size_t)m * 64]];
            double gb = 0.0;
            const double* g = XtX + (size_t)k * K;
            if (!skip_quad)                                   // otherwise launch_beta_quad supplies the quadratic term
                for (int l = 0; l < K; ++l) gb = fma(g[l], use_lds ? tile[l * 64 + lane] : beta[(size_t)l * ld + ii], gb);
            cross = fma(bk, H[(size_t)k * ldh + ii], cross);
            quad = fma(bk, gb, quad);
            spat = fma(bk, dg * bk - nb, spat);
            l1 += fabs(bk);
        }
        if (!active) { cross = quad = spat = l1 = 0.0; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        cross += __shfl_xor(cross, off, 64);
        quad += __shfl_xor(quad, off, 64);
        spat += __shfl_xor(spat, off, 64);
        l1 += __shfl_xor(l1, off, 64);
    }
    if (lane == 0) { red[wib][0] = cross; red[wib][1] = quad; red[wib][2] = spat; red[wib][3] = l1; }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int o = threadIdx.x;
        partials[(size_t)blockIdx.x * 4 + o] = ((red[0][o] + red[1][o]) + red[2][o]) + red[3][o];
    }
}

// beta (K, ld) type-major in solver order -> beta_out / prop_out (n, K) row-major at row perm[i] (perm may be null).
__global__ __launch_bounds__(256) void normalize_export_kernel(const double* __restrict__ beta, long long ld,
                                                               const int* __restrict__ perm, int n, int n_slices, int K,
                                                               int use_lds, double* __restrict__ beta_out,
                                                               double* __restrict__ prop_out) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    __shared__ double inv_s[4][64];
    __shared__ int row_s[4][64];
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int slice = blockIdx.x * 4 + wib;
    if (slice >= n_slices) return;
    const int i = slice * 64 + lane;
    const bool active = i < n;
    const int ii = active ? i : n - 1;
    const int Ks = K | 1;                        // odd row stride: the 64 lanes of a column write hit 64 different banks
    double* tile = smem + (size_t)wib * Ks * 64; // [spot][k], row stride Ks
    double s = 0.0;
    for (int k = 0; k < K; ++k) {
        const double v = beta[(size_t)k * ld + ii];
        s += v;
        if (use_lds) tile[lane * Ks + k] = v;
    }
    // normalize_proportions: all-zero rows -> 1/K, otherwise beta / max(rowsum, 1e-10)   (solver.py:445-451).  np.maximum hands a
    // NaN sum on (fmax would answer 1e-10): a row that holds a NaN comes out all NaN, and a NaN sum is neither 0 nor negative below
    const double den = (s < 1e-10) ? 1e-10 : s;
    const int orow = perm ? perm[ii] : ii;
    if (!use_lds) {
        if (active)
            for (int k = 0; k < K; ++k) {
                const double v = beta[(size_t)k * ld + ii];
                if (beta_out) beta_out[(size_t)orow * K + k] = v;
                if (prop_out) prop_out[(size_t)orow * K + k] = (s == 0.0) ? 1.0 / (double)K : v / den;
            }
        return;
    }
    inv_s[wib][lane] = (s == 0.0) ? -1.0 : den;
    row_s[wib][lane] = active ? orow : -1;
    // same-wave LDS hand-off: the wave's own ds_writes are ordered before its later ds_reads
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
    // element f = lane + 64 j of the wave's 64 x K block: (spot, type) advance by (64 / K, 64 % K) with a carry - one integer
    // division per lane instead of one per element; the results are written once and never read here: non-temporal stores
    const int total = 64 * K;
    const int ds = 64 / K, dk = 64 - ds * K;
    int sp = lane / K, k = lane - sp * K;
    const double inv_K = 1.0 / (double)K;
    for (int f = lane; f < total; f += 64) {
        const int row = row_s[wib][sp];
        if (row >= 0) {
            const double v = tile[sp * Ks + k];
            const double dd = inv_s[wib][sp];
            if (beta_out) __builtin_nontemporal_store(v, beta_out + (size_t)row * K + k);
            if (prop_out) __builtin_nontemporal_store((dd < 0.0) ? inv_K : v / dd, prop_out + (size_t)row * K + k);
        }
        sp += ds;
        k += dk;
        if (k >= K) { k -= K; ++sp; }
    }
}

// Per-spot goodness of fit: out = [residual_sq | sketch_sq | neighbor_sq], three planes of n doubles, written at row perm[i] (the
// caller's spot order; perm may be null).  residual_sq = ||s_i - beta_i Xs||^2 in its expanded form row_sq_i - 2 beta_i.h_i +
// beta_i' XtX beta_i, clamped at 0; neighbor_sq = 0.5 * sum_{j in N(i)} ||beta_i - beta_j||^2 in the difference form (>= 0 per
// spot; over a symmetric graph the plane sums to tr(beta' L beta)).  XtX has row stride ldg (the bordered matrix of a padded solve:
// only the K real types enter).  A lane reads its own column of the [k][lane] tile only (64 consecutive doubles per LDS read: no
// bank conflict, no hand-off between lanes); ELL pad entries (m >= deg) point at the all-zero row and are masked out - in the
// difference form they would add ||beta_i||^2.  Each lane owns its spot: no atomics, no cross-lane reduction.  LDS_TILE is a
// template parameter: chosen at run time inside the loops, the two sources of an own abundance became one generic (flat) load
// behind a branch per gather.
template <bool LDS_TILE>
__global__ __launch_bounds__(256) void spot_diagnostics_kernel(
    const double* __restrict__ beta, long long ld, const double* __restrict__ H, long long ldh,
    const double* __restrict__ XtX, int ldg, const double* __restrict__ row_sq, const int* __restrict__ ell_base,
    const int* __restrict__ slice_off, const int* __restrict__ deg, const int* __restrict__ perm, int n, int n_slices, int K,
    double* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int slice = blockIdx.x * 4 + wib;
    if (slice >= n_slices) return;               // (no block-wide barrier below)
    const int i = slice * 64 + lane;
    const bool active = i < n;
    const int ii = active ? i : n - 1;
    double* tile = smem + (size_t)wib * K * 64;  // [k][lane]
    if (LDS_TILE)
        for (int k = 0; k < K; ++k) tile[k * 64 + lane] = beta[(size_t)k * ld + ii];
    const int w0 = slice_off[slice];
    const int w = slice_off[slice + 1] - w0;
    const int* ell = ell_base + (size_t)w0 * 64 + lane;
    const int dg = deg[ii];
    auto own = [&](int k) { return LDS_TILE ? tile[k * 64 + lane] : beta[(size_t)k * ld + ii]; };
    // neighbours, entry by entry: ONE index per list entry, then its K abundances as K independent gathers (type by type with the
    // index inside, as the objective kernel walks the list, every gather waits for an index load of its own: 1.68 ms at 1M x 30,
    // bound by that chain of latencies at two workgroups per CU); the next entry's index is fetched a step ahead
    double nbr = 0.0;
    int j_next = w > 0 ? ell[0] : 0;
    for (int m = 0; m < w; ++m) {
        const int j = j_next;
        if (m + 1 < w) j_next = ell[(size_t)(m + 1) * 64];
        double a0 = 0.0, a1 = 0.0;
        int k = 0;
#pragma unroll 4
        for (; k + 1 < K; k += 2) {
            const double d0 = own(k) - beta[(size_t)k * ld + j];
            const double d1 = own(k + 1) - beta[(size_t)(k + 1) * ld + j];
            a0 = fma(d0, d0, a0);
            a1 = fma(d1, d1, a1);
        }
        if (k < K) {
            const double d0 = own(k) - beta[(size_t)k * ld + j];
            a0 = fma(d0, d0, a0);
        }
        if (m < dg) nbr += a0 + a1;
    }
    double cross = 0.0, quad = 0.0;
    for (int k = 0; k < K; ++k) {
        const double bk = own(k);
        double gb = 0.0;
        const double* g = XtX + (size_t)k * ldg;
        for (int l = 0; l < K; ++l) gb = fma(g[l], own(l), gb);
        cross = fma(bk, H[(size_t)k * ldh + ii], cross);
        quad = fma(bk, gb, quad);
    }
    if (!active) return;                         // tail lanes of the last slice computed on a copy of spot n - 1: nothing to write
    const double rs = row_sq[i];
    const size_t o = perm ? (size_t)perm[i] : (size_t)i;
    // 24 bytes per spot at three scattered rows of 8: plain stores (non-temporal ones measured the same time: DESIGN.md section 3)
    out[o] = fmax(fma(-2.0, cross, rs) + quad, 0.0);
    out[(size_t)n + o] = rs;
    out[2 * (size_t)n + o] = 0.5 * nbr;
}

static inline size_t tile_lds_bytes(int K) { return (size_t)(K | 1) * 256 * sizeof(double); }
static inline bool tile_fits(int K) { return tile_lds_bytes(K) <= 128 * 1024; }

int objective_partials_count(int n_slices) { return ceil_div(n_slices, 4); }

int launch_objective_partials(const double* beta, long long ld, const double* H, long long ldh, const double* XtX,
                              const int* ell, const int* slice_off, const int* deg, int n, int n_slices, int K,
                              double* partials, hipStream_t st, int skip_quad) {
    if (n <= 0) return 0;
    const int use_lds = tile_fits(K) ? 1 : 0;
    const size_t lds = use_lds ? tile_lds_bytes(K) : 0;
    if (lds > 64 * 1024)
        FDX_HIP(hipFuncSetAttribute((const void*)objective_partials_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(objective_partials_kernel, dim3(ceil_div(n_slices, 4)), dim3(256), lds, st, beta, ld, H, ldh, XtX,
                       ell, slice_off, deg, n, n_slices, K, use_lds, skip_quad, partials);
    FDX_CHECK_LAUNCH();
    return 0;
}

int launch_normalize_export(const double* beta, long long ld, const int* perm, int n, int n_slices, int K,
                            double* beta_out, double* prop_out, hipStream_t st) {
    if (n <= 0) return 0;
    const int use_lds = tile_fits(K) ? 1 : 0;
    const size_t lds = use_lds ? tile_lds_bytes(K) : 0;
    if (lds > 64 * 1024)
        FDX_HIP(hipFuncSetAttribute((const void*)normalize_export_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(normalize_export_kernel, dim3(ceil_div(n_slices, 4)), dim3(256), lds, st, beta, ld, perm, n,
                       n_slices, K, use_lds, beta_out, prop_out);
    FDX_CHECK_LAUNCH();
    return 0;
}

int launch_spot_diagnostics(const double* beta, long long ld, const double* H, long long ldh, const double* XtX, int ldg,
                            const double* row_sq, const int* ell, const int* slice_off, const int* deg, const int* perm, int n,
                            int n_slices, int K, double* out, hipStream_t st) {
    if (n <= 0) return 0;
    const dim3 grid(ceil_div(n_slices, 4));
    if (tile_fits(K)) {
        const size_t lds = (size_t)K * 256 * sizeof(double);
        if (lds > 64 * 1024)
            FDX_HIP(hipFuncSetAttribute((const void*)spot_diagnostics_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(spot_diagnostics_kernel<true>, grid, dim3(256), lds, st, beta, ld, H, ldh, XtX, ldg, row_sq, ell,
                           slice_off, deg, perm, n, n_slices, K, out);
    } else {
        hipLaunchKernelGGL(spot_diagnostics_kernel<false>, grid, dim3(256), 0, st, beta, ld, H, ldh, XtX, ldg, row_sq, ell,
                           slice_off, deg, perm, n, n_slices, K, out);
    }
    FDX_CHECK_LAUNCH();
    return 0;
}

}  // namespace fdx
