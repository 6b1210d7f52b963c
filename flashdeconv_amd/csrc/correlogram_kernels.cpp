// Spatial correlogram (not in the reference): the sums of spatial_stats_kernels.cpp per distance band, with no graph built.
// For radii r_1 < ... < r_B ordered pairs i != j go into band 1 where d_ij <= r_1 and into band b where r_{b-1} < d_ij <= r_b,
// d_ij = sqrt(dist2_exact(...)) as radius_kernel (graph_ell.cpp) decides membership; per band
//   deg_{b,i},   W_b = sum_i deg_{b,i},   sum_i deg_{b,i}^2,   lag_b = A_b Z,   C_b = Z' lag_b.
//
// Pipeline (fdx_spatial_correlogram_dev): bin_points with a cell edge just above r_B (one shell of cells holds every pair) ->
// the candidate count from the cell table, read back and held against max_candidates before any pair is walked ->
// launch_spatial_moments with the binning's perm (mean, Z planes in the binned order, m2, m4) -> per chunk of bands: the band-lag
// kernel below, the fixed-order reduction of its degree partials, launch_spatial_cross_batch with the band as the batch.
//
// Band-lag kernel: one wave per 64 consecutive binned positions, lane = point.  The wave takes the cells its points fall in one
// after the other (a cell's points are consecutive: at most a handful of segments per slice, often one); for a segment the
// candidate list - the cells of the 3^dim block - is wave-uniform, so candidates are staged 64 at a time in LDS
// (coordinates and KC columns of Z, loaded by all 64 lanes whether their point is in the segment or not) and read back as
// broadcasts.  A lane finds its pair's band by comparing d against the chunk's radii, held in scalars, and adds the KC values
// into S[band][column][lane] in LDS: lane-contiguous, one owner per slot, plain read-add-write.  The band is a run-time value
// per pair: accumulators in registers would be an array indexed at run time, i.e. scratch memory.  More than KC columns walk the
// candidates again - in a wave of their own (blockIdx.y), so that a small slide still fills the device.  No atomics; every sum
// is formed in candidate order (cells of the block in z, y, x order, positions ascending), which depends on neither the grid,
// nor KC, nor the chunk of bands.
#include "band_walk.h"
#include "gene_pass.h"

#include <vector>

namespace fdx {

constexpr int CG_MAX_KC = 16;                       // columns per walk at the most (the staging tile is sized by it)
// LDS for the band accumulators of a wave.  The kernel waits on LDS round trips, so resident waves count for more than columns
// per walk: 1M spots x 30 columns x 6 bands took 54.7 ms with 32 KB (3 waves per CU, 2 walks), 43.3 with 16 KB (7 waves, 4 walks),
// 40.8 with 8 KB (8 walks) - but 8 KB leaves one column per walk at ten bands.
constexpr size_t CG_ACC_BYTES = 16 * 1024;
constexpr int CG_WALK_CAP_BLOCKS = 4096;            // waves of the band-lag kernel at the most
// (band_walk.h: the cell edge, CgRadii and the wave hand-off, shared with the label walk of label_band_kernels.cpp)

// acc[c * 64] += z[c * 64] for N columns: every read issued before the first add (the two LDS regions never overlap, which the
// compiler cannot know; one column at a time is a chain of N read - read - add - write round trips)
template <int N>
__device__ __forceinline__ void cg_add_columns(double* __restrict__ acc, const double* __restrict__ z) {
    double a[N], v[N];
#pragma unroll
    for (int c = 0; c < N; ++c) { a[c] = acc[c * 64]; v[c] = z[c * 64]; }
#pragma unroll
    for (int c = 0; c < N; ++c) acc[c * 64] = a[c] + v[c];
}

// partials[2 * block] = the block's share of sum over occupied cells of count(cell) * count(the 3^dim block of cells around it),
// partials[2 * block + 1] = the largest block count among its occupied cells
__global__ __launch_bounds__(256) void cg_candidates_kernel(const int* __restrict__ cstart, const int* __restrict__ cend, GridParams gp,
                                                            long long* __restrict__ partials) {
    __shared__ long long red[256], red_max[256];
    const long long n_cells = (long long)gp.nc[0] * gp.nc[1] * gp.nc[2];
    long long s = 0, widest = 0;
    for (long long id = blockIdx.x * 256LL + threadIdx.x; id < n_cells; id += (long long)gridDim.x * 256) {
        const long long own = cend[id] - cstart[id];
        if (own <= 0) continue;
        // the cell's coordinates from its mixed-radix id (an axis of one cell shares its stride with the next: always 0)
        int c[3];
        for (int a = 0; a < 3; ++a) c[a] = (int)((id / gp.stride[a]) % gp.nc[a]);
        long long around = 0;
        for (int z = max(0, c[2] - CG_SHELLS); z <= min(gp.nc[2] - 1, c[2] + CG_SHELLS); ++z)
            for (int y = max(0, c[1] - CG_SHELLS); y <= min(gp.nc[1] - 1, c[1] + CG_SHELLS); ++y)
                for (int x = max(0, c[0] - CG_SHELLS); x <= min(gp.nc[0] - 1, c[0] + CG_SHELLS); ++x) {
                    const int cell = x * gp.stride[0] + y * gp.stride[1] + z * gp.stride[2];
                    around += cend[cell] - cstart[cell];
                }
        s += own * around;
        widest = max(widest, around);
    }
    red[threadIdx.x] = s;
    red_max[threadIdx.x] = widest;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            red[threadIdx.x] += red[threadIdx.x + off];
            red_max[threadIdx.x] = max(red_max[threadIdx.x], red_max[threadIdx.x + off]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        partials[2 * blockIdx.x] = red[0];
        partials[2 * blockIdx.x + 1] = red_max[0];
    }
}

int cg_guard(const char* who, const BinnedPoints& bins, long long max_candidates, long long* candidates, long long* max_around,
             hipStream_t st) {
    const long long n_cells = (long long)bins.gp.nc[0] * bins.gp.nc[1] * bins.gp.nc[2];
    const int blocks = (int)std::max<long long>(1, std::min<long long>(CG_COUNT_BLOCKS, ceil_div(n_cells, 256)));
    DevBuf part;
    FDX_TRY(part.alloc((size_t)blocks * 2 * sizeof(long long)));
    hipLaunchKernelGGL(cg_candidates_kernel, dim3(blocks), dim3(256), 0, st, bins.cstart.as<int>(), bins.cend_p, bins.gp,
                       part.as<long long>());
    FDX_CHECK_LAUNCH();
    std::vector<long long> host((size_t)blocks * 2);
    FDX_TRY(copy_d2h(host.data(), part.p, host.size() * sizeof(long long), st));
    long long total = 0, widest = 0;
    for (int b = 0; b < blocks; ++b) {
        total += host[2 * (size_t)b];
        widest = std::max(widest, host[2 * (size_t)b + 1]);
    }
    *candidates = total;
    if (max_around) *max_around = widest;
    if (total > max_candidates)
        return fail(FDX_ERR_INVALID, std::string(who) + ": the largest radius makes the walk examine " + std::to_string(total) +
                                         " candidate pairs, more than max_candidates = " + std::to_string(max_candidates) +
                                         " (smaller radii, or raise max_candidates)");
    return 0;
}

// lag[(b * K + k) * ld + p] = sum over the candidates q of position p with band(p, q) = b of Z[k][q], for the rc.nb bands of the
// chunk; positions n .. 64 n_slices - 1 get 0.  degree (may be null): degree[perm[p] * deg_ld + deg_col0 + b] = deg_{b,p}.
// Block (x, y) walks for columns [y KC, (y + 1) KC) over slices x, x + gridDim.x, ...; deg_partials[x][b] = {sum deg_b,
// sum deg_b^2} over those slices, from the blocks with y = 0.
// Dynamic LDS: S[nb][KC][64] doubles | zt[KC][64] | xt, yt, wt [64] | tot[nb][2] int64 | D[nb][64] int32.
__global__ __launch_bounds__(64) void cg_band_lag_kernel(const double* __restrict__ sc, const int* __restrict__ cstart,
                                                         const int* __restrict__ cend, GridParams gp, int n, int n_slices,
                                                         const double* __restrict__ Z, long long ld, int K, int KC, CgRadii rc,
                                                         double* __restrict__ lag, const int* __restrict__ perm,
                                                         int* __restrict__ degree, int deg_ld, int deg_col0,
                                                         long long* __restrict__ deg_partials) {
    extern __shared__ __attribute__((aligned(16))) double cg_smem[];
    const int lane = threadIdx.x;
    const int nb = rc.nb;
    double* S = cg_smem;
    double* zt = S + (size_t)nb * KC * 64;
    double* xt = zt + (size_t)KC * 64;
    double* yt = xt + 64;
    double* wt = yt + 64;
    long long* tot = reinterpret_cast<long long*>(wt + 64);
    int* D = reinterpret_cast<int*>(tot + 2 * nb);
    if (lane < 2 * nb) tot[lane] = 0;
    const double r_last = rc.r[nb - 1];
    const int k0 = blockIdx.y * KC;                                   // this wave's columns: one walk of the candidates
    const int kcn = K - k0 < KC ? K - k0 : KC;
    const bool count = k0 == 0;                                       // the first walk also counts the degrees

    for (int slice = blockIdx.x; slice < n_slices; slice += gridDim.x) {
        const long long p = (long long)slice * 64 + lane;
        const bool active = p < n;
        const double px = active ? sc[p] : 0.0, py = active ? sc[(size_t)n + p] : 0.0, pz = active ? sc[2 * (size_t)n + p] : 0.0;
        int c0 = 0, c1 = 0, c2 = 0;
        if (gp.dim > 0) c0 = cell_coord(px, gp.mn[0], gp.inv_h[0], gp.nc[0]);
        if (gp.dim > 1) c1 = cell_coord(py, gp.mn[1], gp.inv_h[1], gp.nc[1]);
        if (gp.dim > 2) c2 = cell_coord(pz, gp.mn[2], gp.inv_h[2], gp.nc[2]);
        const int my_cell = active ? c0 * gp.stride[0] + c1 * gp.stride[1] + c2 * gp.stride[2] : -1;
        const unsigned long long all_active = __ballot(active);

        cg_handoff();
        for (int i = 0; i < nb * kcn; ++i) S[(size_t)i * 64 + lane] = 0.0;
        if (count)
            for (int b = 0; b < nb; ++b) D[b * 64 + lane] = 0;

        unsigned long long todo = all_active;
        while (todo) {                                                // one cell's segment of the slice at a time
            const int leader = __builtin_ctzll(todo);
            const int cell = __builtin_amdgcn_readfirstlane(__shfl(my_cell, leader, 64));
            const int u0 = __builtin_amdgcn_readfirstlane(__shfl(c0, leader, 64));
            const int u1 = __builtin_amdgcn_readfirstlane(__shfl(c1, leader, 64));
            const int u2 = __builtin_amdgcn_readfirstlane(__shfl(c2, leader, 64));
            const bool mine = active && my_cell == cell;
            todo &= ~__ballot(mine);
            for (int z = max(0, u2 - CG_SHELLS); z <= min(gp.nc[2] - 1, u2 + CG_SHELLS); ++z)
                for (int y = max(0, u1 - CG_SHELLS); y <= min(gp.nc[1] - 1, u1 + CG_SHELLS); ++y)
                    for (int x = max(0, u0 - CG_SHELLS); x <= min(gp.nc[0] - 1, u0 + CG_SHELLS); ++x) {
                        const int cc = x * gp.stride[0] + y * gp.stride[1] + z * gp.stride[2];
                        const int qs = cstart[cc], qe = cend[cc];
                        for (int q0 = qs; q0 < qe; q0 += 64) {
                            const int cnt = qe - q0 < 64 ? qe - q0 : 64;
                            cg_handoff();                                      // the previous tile's readers are done
                            if (lane < cnt) {
                                const size_t q = (size_t)q0 + lane;
                                xt[lane] = sc[q];
                                yt[lane] = sc[(size_t)n + q];
                                wt[lane] = sc[2 * (size_t)n + q];
                                for (int kc = 0; kc < kcn; ++kc) zt[kc * 64 + lane] = Z[(size_t)(k0 + kc) * ld + q];
                            }
                            cg_handoff();
                            if (!mine) continue;
                            // four candidates' distances at a time: twelve LDS reads in flight, not three (slots past cnt hold
                            // an earlier tile's values, or none: they are computed and not looked at)
                            for (int t0 = 0; t0 < cnt; t0 += 4) {
                                double d2[4];
#pragma unroll
                                for (int u = 0; u < 4; ++u) d2[u] = dist2_exact(xt[t0 + u] - px, yt[t0 + u] - py, wt[t0 + u] - pz);
#pragma unroll
                                for (int u = 0; u < 4; ++u) {
                                    const int t = t0 + u;
                                    if (t >= cnt || q0 + t == (int)p || d2[u] > rc.d2_hi || d2[u] < rc.d2_lo) continue;
                                    const double d = sqrt(d2[u]);
                                    if (!(d <= r_last) || !(d > rc.lo)) continue;
                                    int b = 0;
                                    for (int i = 0; i + 1 < nb; ++i) b += d > rc.r[i] ? 1 : 0;   // = searchsorted(radii, d, "left")
                                    double* Sb = S + (size_t)b * kcn * 64 + lane;
                                    const double* zq = zt + t;
                                    int kc = 0;
                                    for (; kc + 8 <= kcn; kc += 8) cg_add_columns<8>(Sb + kc * 64, zq + kc * 64);
                                    if (kc + 4 <= kcn) { cg_add_columns<4>(Sb + kc * 64, zq + kc * 64); kc += 4; }
                                    for (; kc < kcn; ++kc) cg_add_columns<1>(Sb + kc * 64, zq + kc * 64);
                                    if (count) D[b * 64 + lane] += 1;
                                }
                            }
                        }
                    }
        }
        cg_handoff();
        for (int b = 0; b < nb; ++b)
            for (int kc = 0; kc < kcn; ++kc)
                lag[((size_t)b * K + k0 + kc) * ld + p] = active ? S[((size_t)b * kcn + kc) * 64 + lane] : 0.0;
        if (count) {
            const size_t orow = active ? (size_t)perm[p] : 0;
            for (int b = 0; b < nb; ++b) {
                const int dg = active ? D[b * 64 + lane] : 0;
                if (degree && active) degree[orow * deg_ld + deg_col0 + b] = dg;
                long long sd = dg, sd2 = (long long)dg * dg;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    sd += __shfl_xor(sd, off, 64);
                    sd2 += __shfl_xor(sd2, off, 64);
                }
                if (lane == 0) { tot[2 * b] += sd; tot[2 * b + 1] += sd2; }
            }
        }
    }
    cg_handoff();
    if (count && lane < 2 * nb) deg_partials[(size_t)blockIdx.x * 2 * nb + lane] = tot[lane];
}

static size_t cg_lds_bytes(int nb, int kc) {
    return ((size_t)nb * kc * 64 + (size_t)kc * 64 + 3 * 64) * sizeof(double) + (size_t)nb * 2 * sizeof(long long) +
           (size_t)nb * 64 * sizeof(int);
}

CorrelogramPlan correlogram_plan(long long n, int K, int B, int max_bands_per_pass) {
    CorrelogramPlan p;
    p.s = spatial_stats_plan(n, K);
    const size_t KK = (size_t)K * K;
    // per band in flight: its lag planes and its cross partials
    const size_t per_band = ((size_t)K * p.s.ld + (size_t)p.s.cross_blocks * KK) * sizeof(double);
    long long bc = (long long)std::max<size_t>(1, SCRATCH_BUDGET_BYTES / per_band);
    bc = std::min<long long>(bc, B);
    if (max_bands_per_pass > 0) bc = std::min<long long>(bc, max_bands_per_pass);
    p.bands_per_pass = (int)std::max<long long>(1, bc);
    p.kc = (int)std::max<size_t>(1, std::min<size_t>(std::min(K, CG_MAX_KC),
                                                     CG_ACC_BYTES / ((size_t)p.bands_per_pass * 64 * sizeof(double))));
    p.walk_blocks = std::max(1, std::min(CG_WALK_CAP_BLOCKS, p.s.n_slices));
    p.lds_bytes = cg_lds_bytes(p.bands_per_pass, p.kc);
    p.part_doubles = std::max({p.s.partials_doubles, (size_t)p.bands_per_pass * p.s.cross_blocks * KK,
                               (size_t)p.walk_blocks * 2 * p.bands_per_pass, (size_t)CG_COUNT_BLOCKS});
    p.scratch_doubles = (size_t)K * p.s.ld + (size_t)p.bands_per_pass * K * p.s.ld + p.part_doubles;
    return p;
}

}  // namespace fdx

using namespace fdx;

extern "C" int fdx_spatial_correlogram_dev(const double* coords_dev, int64_t n, int32_t dim, const double* V_dev, int64_t ldv, int32_t K,
                                           const double* radii, int32_t B, int32_t max_bands_per_pass, int64_t max_candidates,
                                           double* mean, double* m2, double* m4, double* C, int64_t* W, int64_t* sum_deg_sq,
                                           int32_t* degree_dev, int32_t* bands_per_pass_out, int64_t* candidates_out, void* stream) {
    FDX_REQUIRE(radii && mean && m2 && C && W && sum_deg_sq, "fdx_spatial_correlogram_dev: null argument");
    FDX_REQUIRE(n >= 0 && n < (1LL << 31) - 128, "fdx_spatial_correlogram_dev: n must be between 0 and 2^31 - 129");
    FDX_REQUIRE(n == 0 || (coords_dev && V_dev), "fdx_spatial_correlogram_dev: null argument");
    FDX_REQUIRE(dim >= 1 && dim <= 3, "fdx_spatial_correlogram_dev: coordinate dimension must be 1, 2 or 3");
    FDX_REQUIRE(K >= 1 && ldv >= K, "fdx_spatial_correlogram_dev: K must be positive and ldv at least K");
    FDX_REQUIRE(B >= 1 && B <= CG_MAX_BANDS, "fdx_spatial_correlogram_dev: between 1 and 32 radii");
    FDX_REQUIRE(max_bands_per_pass >= 0 && max_candidates >= 0,
                "fdx_spatial_correlogram_dev: max_bands_per_pass and max_candidates must not be negative");
    for (int b = 0; b < B; ++b)
        FDX_REQUIRE(std::isfinite(radii[b]) && radii[b] > (b ? radii[b - 1] : 0.0),
                    "fdx_spatial_correlogram_dev: radii must be positive, finite and strictly ascending");
    hipStream_t st = (hipStream_t)stream;
    PoolStream pool_stream(st);
    const size_t KK = (size_t)K * K;
    std::fill(W, W + B, (int64_t)0);
    std::fill(sum_deg_sq, sum_deg_sq + B, (int64_t)0);
    if (bands_per_pass_out) *bands_per_pass_out = 0;
    if (candidates_out) *candidates_out = 0;
    if (n == 0) {                                       // no spots: no mean
        SpatialSumsLayout(K).fill_empty(mean, m2, nullptr, m4);
        std::fill(C, C + (size_t)B * KK, 0.0);
        return 0;
    }

    BinnedPoints bins;
    struct Drain {                                      // the binning's temporaries: nothing may still read them when they go back
        hipStream_t st;
        ~Drain() { (void)hipStreamSynchronize(st); }
    } drain{st};
    const double r_max = radii[B - 1];
    FDX_TRY(bin_points(coords_dev, n, dim, 1.0, r_max * CG_CELL_MARGIN, &bins, st));
    FDX_REQUIRE(bins.gp.h[0] >= r_max * CG_CELL_MARGIN, "fdx_spatial_correlogram_dev: the grid's cells are smaller than the largest radius");

    const CorrelogramPlan plan = correlogram_plan(n, K, B, max_bands_per_pass);
    if (bands_per_pass_out) *bands_per_pass_out = plan.bands_per_pass;
    // the default limit: the walk's cost is candidates x walks (column groups x chunks of bands), held to about ten seconds
    if (max_candidates == 0)
        max_candidates = FDX_CORRELOGRAM_MAX_CANDIDATE_WALKS / ((long long)ceil_div(K, plan.kc) * ceil_div(B, plan.bands_per_pass));
    DevBuf scratch, out;
    FDX_TRY(scratch.alloc(plan.scratch_doubles * sizeof(double)));
    const size_t out_doubles = 3 * (size_t)K + (size_t)B * KK + 2 * (size_t)B;
    FDX_TRY(out.alloc(out_doubles * sizeof(double)));
    const long long plane = (long long)K * plan.s.ld;
    double* Zp = scratch.as<double>();
    double* lag = Zp + plane;
    double* part = lag + (size_t)plan.bands_per_pass * plane;
    double* d_mean = out.as<double>();
    double* d_m2 = d_mean + K;
    double* d_m4 = d_m2 + K;
    double* d_C = d_m4 + K;
    long long* d_counts = reinterpret_cast<long long*>(d_C + (size_t)B * KK);   // (B, 2)

    // the guard: what the walk would examine, known before it starts
    long long candidates = 0;
    const int guarded = cg_guard("fdx_spatial_correlogram_dev", bins, max_candidates, &candidates, nullptr, st);
    if (candidates_out) *candidates_out = candidates;
    FDX_TRY(guarded);

    FDX_TRY(launch_spatial_moments(plan.s, V_dev, ldv, (int)n, K, bins.perm.as<int>(), Zp, part, d_mean, d_m2, d_m4, st));
    for (int b0 = 0; b0 < B; b0 += plan.bands_per_pass) {
        const CgRadii rc = cg_chunk_radii(radii, b0, std::min(plan.bands_per_pass, B - b0));
        hipLaunchKernelGGL(cg_band_lag_kernel, dim3(plan.walk_blocks, ceil_div(K, plan.kc)), dim3(64), plan.lds_bytes, st, bins.sc.as<double>(),
                           bins.cstart.as<int>(), bins.cend_p, bins.gp, (int)n, plan.s.n_slices, Zp, plan.s.ld, K, plan.kc, rc, lag,
                           bins.perm.as<int>(), degree_dev, (int)B, b0, reinterpret_cast<long long*>(part));
        FDX_CHECK_LAUNCH();
        FDX_TRY(launch_reduce_i64(reinterpret_cast<long long*>(part), plan.walk_blocks, 2LL * rc.nb, d_counts + 2 * (size_t)b0, st));
        FDX_TRY(launch_spatial_cross_batch(plan.s, Zp, lag, plane, rc.nb, K, part, d_C + (size_t)b0 * KK, st));
    }
    std::vector<double> host(out_doubles);
    FDX_TRY(copy_d2h(host.data(), out.p, out_doubles * sizeof(double), st));
    const double* h = host.data();
    std::copy(h, h + K, mean);
    std::copy(h + K, h + 2 * (size_t)K, m2);
    if (m4) std::copy(h + 2 * (size_t)K, h + 3 * (size_t)K, m4);
    std::copy(h + 3 * (size_t)K, h + 3 * (size_t)K + (size_t)B * KK, C);
    const double* hc = h + 3 * (size_t)K + (size_t)B * KK;
    for (int b = 0; b < B; ++b) {
        std::memcpy(&W[b], hc + 2 * (size_t)b, sizeof(int64_t));
        std::memcpy(&sum_deg_sq[b], hc + 2 * (size_t)b + 1, sizeof(int64_t));
    }
    return 0;
}
