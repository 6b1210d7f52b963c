// Label co-occurrence by distance band (not in the reference): the join counts of label_pair_kernels.cpp per distance band of the
// correlogram, with no graph built.  For radii r_1 < ... < r_B ordered pairs i != j go into band 1 where d_ij <= r_1 (d = 0 among
// them) and into band b where r_{b-1} < d_ij <= r_b, d_ij = sqrt(dist2_exact(...)) as cg_band_lag_kernel decides it; with labels
// l_i in {-1, 0 .. C - 1} in the caller's order
//   N_b[a][c] = #{(i, j) in band b : l_i = a, l_j = c}      deg_{b,i}      W_b = sum_i deg_{b,i}      sum_i deg_{b,i}^2
//   and sum_i (sum_{b' <= b} deg_{b',i})^2, which no per-band sum gives
// for the observed labels and for l^r_i = l[pi_r(i)], r = first_perm .. first_perm + n_perm - 1 (pi_r: perm_device.h, the relabelling
// of fdx_label_pair_counts_dev); each N^r_b and each running sum over bands Ncum^r_b is ranked against its observed value.
//
// Pipeline (fdx_label_cooccurrence_dev): bin_points with the cell edge of the correlogram -> cg_guard (band_walk.h: the candidate
// pairs and the most candidates of one point, read back; too many: refused, nothing walked) -> lp_prepare_kernel (label_stage.h:
// bytes, n_a, the range flag) -> the observed pass: lp_stage_kernel with the identity and the binning's perm, the walk per chunk of
// bands, which also writes every position's band degrees to an (n, B) plane in the caller's order; lb_degree_sums_kernel and
// launch_reduce_i64 turn the plane into the three degree sums (integers from the whole plane: no chunk of bands is seen in them)
// -> per launch chain of permutations: lp_stage_kernel (groups of P interleaved per binned position), the walk per chunk of bands
// with the groups in gridDim.y, lb_accum_kernel.
//
// The walk (lb_walk_kernel): a workgroup of several waves; a wave takes 64 consecutive binned positions, lane = point, and walks
// the cell segments of its slice and the 3^dim block of each as cg_band_lag_kernel does.  Per tile of 64 candidates the wave
// stages the coordinates and the P label bytes of every candidate (ONE 8- or 16-byte load each) in a tile of its own in LDS and
// reads them back as broadcasts.  A pair's band does not depend on the permutation: it is found once, and then for every j < P
// where neither byte has bit 7 set the lane adds 1 to hist[band][j][a_j][c_j] - 32-bit bins in LDS shared by the workgroup's
// waves, LDS integer atomics.  The workgroup adds its non-zero bins to the launch's int64 totals with 64-bit integer atomics, as
// lp_count_kernel does.  Everything is an integer, there are no floating-point atomics, two calls return the same bits.
//
// A workgroup's 32-bit bins cannot overflow: a bin takes at most one increment per ordered pair (p, q) of a position p the
// workgroup walks, a position has at most M candidates q - M the largest count of a 3^dim block of cells around an occupied cell,
// which cg_guard reads back with the candidate count - and the launcher (lb_grid) gives a workgroup at most
// floor((2^32 - 1) / (64 M)) slices: more workgroups, or fewer walking waves in each, where the plan's grid would exceed that; a
// call with M >= 2^26, where one slice alone could overflow, is refused.  This holds whatever max_candidates the caller allows.
#include "band_walk.h"
#include "fdx_internal.h"
#include "gene_pass.h"
#include "label_band_plan.h"
#include "label_stage.h"
#include "perm_device.h"

#include <algorithm>
#include <vector>

namespace fdx {

static_assert(LB_SCRATCH_BUDGET == SCRATCH_BUDGET_BYTES, "label_band_plan.h restates the library's scratch budget");
static_assert(LB_MAX_AROUND * 64 <= (1LL << 32), "a slice's pair visits must fit a 32-bit bin");

template <int P>
__device__ __forceinline__ void lb_load(const unsigned char* __restrict__ src, unsigned (&w)[P / 4]) {
    if constexpr (P == 8) {
        const uint2 v = *reinterpret_cast<const uint2*>(src);
        w[0] = v.x; w[1] = v.y;
    } else {
        const uint4 v = *reinterpret_cast<const uint4*>(src);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
}

// acc[blockIdx.y][b0 + b][j][a][c] (B_all bands a group) += the workgroup's count of ordered pairs (p, q), q != p, in band b of the
// chunk rc with bytes (a, c) under permutation j of group blockIdx.y.  blockDim.x / 64 waves, of which the first `walking` take a
// slice each at a time: wave w of block x walks slices x * walking + w, + gridDim.x * walking, ...  OBSERVED (the identity staged as
// permutation 0 of one group): only j = 0 is counted, and degree[perm[p] * B_all + b0 + b] = deg_{b,p}.
// Dynamic LDS: hist[nb][P][C][C] u32 | per wave: xt, yt, wt [64] doubles, lt [64][P] bytes, OBSERVED: D[nb][64] int32.
template <int P, bool OBSERVED>
__global__ __launch_bounds__(1024) void lb_walk_kernel(const double* __restrict__ sc, const int* __restrict__ cstart,
                                                       const int* __restrict__ cend, GridParams gp, int n, int n_slices,
                                                       const unsigned char* __restrict__ Lr_all, long long ld, int C, CgRadii rc,
                                                       int b0, int B_all, int walking, unsigned long long* __restrict__ acc_all,
                                                       const int* __restrict__ perm, int* __restrict__ degree) {
    extern __shared__ __attribute__((aligned(16))) unsigned lb_smem[];
    const int nb = rc.nb;
    const int CC = C * C;
    const int bins = nb * P * CC;
    unsigned* hist = lb_smem;
    for (int i = threadIdx.x; i < bins; i += blockDim.x) hist[i] = 0u;
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t wave_bytes = lb_wave_bytes(P, nb, OBSERVED);
    unsigned char* tile = reinterpret_cast<unsigned char*>(hist + bins) + (size_t)wib * wave_bytes;
    double* xt = reinterpret_cast<double*>(tile);
    double* yt = xt + 64;
    double* wt = yt + 64;
    unsigned char* lt = reinterpret_cast<unsigned char*>(wt + 64);
    int* D = reinterpret_cast<int*>(lt + 64 * P);
    const unsigned char* Lr = Lr_all + (size_t)blockIdx.y * ld * P;
    const double r_last = rc.r[nb - 1];
    constexpr int PJ = OBSERVED ? 1 : P;                              // permutations counted

    if (wib < walking) {
        for (long long slice = (long long)blockIdx.x * walking + wib; slice < n_slices; slice += (long long)gridDim.x * walking) {
            const long long p = slice * 64 + lane;
            const bool active = p < n;
            const double px = active ? sc[p] : 0.0, py = active ? sc[(size_t)n + p] : 0.0, pz = active ? sc[2 * (size_t)n + p] : 0.0;
            int c0 = 0, c1 = 0, c2 = 0;
            if (gp.dim > 0) c0 = cell_coord(px, gp.mn[0], gp.inv_h[0], gp.nc[0]);
            if (gp.dim > 1) c1 = cell_coord(py, gp.mn[1], gp.inv_h[1], gp.nc[1]);
            if (gp.dim > 2) c2 = cell_coord(pz, gp.mn[2], gp.inv_h[2], gp.nc[2]);
            const int my_cell = active ? c0 * gp.stride[0] + c1 * gp.stride[1] + c2 * gp.stride[2] : -1;
            unsigned mine_b[P / 4];
            lb_load<P>(Lr + (size_t)p * P, mine_b);                   // p < ld; positions from n on hold LP_NONE
            int row[PJ];                                              // (j * C + a) * C of the lane's own byte
#pragma unroll
            for (int j = 0; j < PJ; ++j) row[j] = j * CC + (int)((mine_b[j / 4] >> (8 * (j % 4))) & 0xffu) * C;
            if constexpr (OBSERVED) {
                cg_handoff();
                for (int b = 0; b < nb; ++b) D[b * 64 + lane] = 0;
            }

            unsigned long long todo = __ballot(active);
            while (todo) {                                            // one cell's segment of the slice at a time
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
                                cg_handoff();                                  // the previous tile's readers are done
                                if (lane < cnt) {
                                    const size_t q = (size_t)q0 + lane;
                                    xt[lane] = sc[q];
                                    yt[lane] = sc[(size_t)n + q];
                                    wt[lane] = sc[2 * (size_t)n + q];
                                    unsigned theirs[P / 4];
                                    lb_load<P>(Lr + q * P, theirs);
                                    unsigned* dst = reinterpret_cast<unsigned*>(lt + lane * P);
#pragma unroll
                                    for (int k = 0; k < P / 4; ++k) dst[k] = theirs[k];
                                }
                                cg_handoff();
                                if (!mine) continue;
                                // four candidates' distances at a time, as cg_band_lag_kernel (slots past cnt hold an earlier
                                // tile's values, or none: they are computed and not looked at)
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
                                        if constexpr (OBSERVED) D[b * 64 + lane] += 1;
                                        unsigned theirs[P / 4];
                                        lb_load<P>(lt + t * P, theirs);                                // a broadcast
                                        unsigned* hb = hist + (size_t)b * P * CC;
#pragma unroll
                                        for (int j = 0; j < PJ; ++j) {
                                            const unsigned both = (mine_b[j / 4] | theirs[j / 4]) >> (8 * (j % 4));
                                            if (!(both & 0x80u))
                                                atomicAdd(&hb[row[j] + (int)((theirs[j / 4] >> (8 * (j % 4))) & 0xffu)], 1u);
                                        }
                                    }
                                }
                            }
                        }
            }
            if constexpr (OBSERVED) {
                cg_handoff();
                if (active) {
                    int* out = degree + (size_t)perm[p] * B_all + b0;
                    for (int b = 0; b < nb; ++b) out[b] = D[b * 64 + lane];
                }
            }
        }
    }
    __syncthreads();
    unsigned long long* acc = acc_all + ((size_t)blockIdx.y * B_all + b0) * P * CC;
    for (int i = threadIdx.x; i < bins; i += blockDim.x) {
        const unsigned v = hist[i];
        if (v) atomicAdd(&acc[i], (unsigned long long)v);
    }
}

// partials[block][3 B] = the block's share of {sum_i deg_{b,i} | sum_i deg_{b,i}^2 | sum_i (sum_{b' <= b} deg_{b',i})^2} over the
// rows of the (n, B) degree plane; 256 threads, a row each at a time
__global__ __launch_bounds__(256) void lb_degree_sums_kernel(const int* __restrict__ degree, int n, int B, long long* __restrict__ partials) {
    __shared__ long long tot[4][3 * CG_MAX_BANDS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int i = lane; i < 3 * B; i += 64) tot[w][i] = 0;
    for (long long i0 = (long long)blockIdx.x * 256; i0 < n; i0 += (long long)gridDim.x * 256) {
        const long long i = i0 + threadIdx.x;
        const int* row = degree + (size_t)(i < n ? i : 0) * B;
        long long run = 0;
        for (int b = 0; b < B; ++b) {
            const long long dg = i < n ? row[b] : 0;
            run += dg;
            long long s = dg, s2 = dg * dg, c2 = run * run;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                s += __shfl_xor(s, off, 64);
                s2 += __shfl_xor(s2, off, 64);
                c2 += __shfl_xor(c2, off, 64);
            }
            if (lane == 0) { tot[w][b] += s; tot[w][B + b] += s2; tot[w][2 * B + b] += c2; }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * B; i += 256) partials[(size_t)blockIdx.x * 3 * B + i] = tot[0][i] + tot[1][i] + tot[2][i] + tot[3][i];
}

// obs[b][i] = acc[b][0][i] (the identity's counts: permutation 0 of the one group), for i < CC
__global__ __launch_bounds__(256) void lb_observed_kernel(const long long* __restrict__ acc, int B, int P, long long CC,
                                                          long long* __restrict__ obs) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= CC) return;
    obs[(size_t)blockIdx.y * CC + i] = acc[(size_t)blockIdx.y * P * CC + i];
}

// The batch's N^r_b and Ncum^r_b = sum_{b' <= b} N^r_{b'} against the observed ones, one thread per band b = blockIdx.y and pair
// i = (a, c), in permutation order: d = N^r - N; null (may be null) gets every N^r_b.  stats: [band | cumulative] x NullSumsLayout
// of B * CC statistics each.  acc is only read (a thread reads the bands below its own): the launcher zeroes it.
__global__ __launch_bounds__(256) void lb_accum_kernel(const long long* __restrict__ acc, int batch, int B, int P, long long CC,
                                                       const long long* __restrict__ obs, long long* __restrict__ null_out,
                                                       long long* __restrict__ stats, NullSumsLayout band, NullSumsLayout cum) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= CC) return;
    const int b = blockIdx.y;
    const size_t x = (size_t)b * CC + i;
    const long long n0 = obs[x];
    long long c0 = 0;
    for (int bb = 0; bb <= b; ++bb) c0 += obs[(size_t)bb * CC + i];
    double* fstats = reinterpret_cast<double*>(stats);
    long long ge = stats[band.count_ge + x], le = stats[band.count_le + x];
    long long cge = stats[cum.count_ge + x], cle = stats[cum.count_le + x];
    double s = fstats[band.sum_d + x], q = fstats[band.sumsq_d + x];
    double cs = fstats[cum.sum_d + x], cq = fstats[cum.sumsq_d + x];
    for (int r = 0; r < batch; ++r) {
        const long long* a = acc + (((size_t)(r / P) * B) * P + (r % P)) * CC + i;      // [group][band][j][CC]
        long long run = 0;
        for (int bb = 0; bb < b; ++bb) run += a[(size_t)bb * P * CC];
        const long long c = a[(size_t)b * P * CC];
        run += c;
        if (null_out) null_out[((size_t)r * B + b) * CC + i] = c;
        const double d = (double)(c - n0), dc = (double)(run - c0);
        ge += c >= n0 ? 1 : 0;
        le += c <= n0 ? 1 : 0;
        cge += run >= c0 ? 1 : 0;
        cle += run <= c0 ? 1 : 0;
        s = __dadd_rn(s, d);
        q = __dadd_rn(q, __dmul_rn(d, d));                            // the sum of the rounded squares, as NumPy adds them: no fma
        cs = __dadd_rn(cs, dc);
        cq = __dadd_rn(cq, __dmul_rn(dc, dc));
    }
    stats[band.count_ge + x] = ge;
    stats[band.count_le + x] = le;
    stats[cum.count_ge + x] = cge;
    stats[cum.count_le + x] = cle;
    fstats[band.sum_d + x] = s;
    fstats[band.sumsq_d + x] = q;
    fstats[cum.sum_d + x] = cs;
    fstats[cum.sumsq_d + x] = cq;
}

struct LbDevice {                      // what a walk launch reads, beside the plan
    const BinnedPoints* bins;
    const double* radii;
    int n, C, B;
    long long max_around;
    int max_blocks;
};

template <int P, bool OBSERVED>
static int launch_walk(const LabelBandPlan& p, const LbDevice& d, int groups, const unsigned char* Lr, long long* acc, int* degree,
                       hipStream_t st) {
    const size_t lds = lb_lds_bytes(p, OBSERVED);
    if (lds > 64 * 1024)
        FDX_HIP(hipFuncSetAttribute((const void*)lb_walk_kernel<P, OBSERVED>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const LbGrid g = lb_grid(p, groups, d.max_around, d.max_blocks);
    for (int b0 = 0; b0 < d.B; b0 += p.bands_per_pass) {
        const CgRadii rc = cg_chunk_radii(d.radii, b0, std::min(p.bands_per_pass, d.B - b0));
        hipLaunchKernelGGL((lb_walk_kernel<P, OBSERVED>), dim3(g.blocks, groups), dim3(p.waves * 64), lds, st, d.bins->sc.as<double>(),
                           d.bins->cstart.as<int>(), d.bins->cend_p, d.bins->gp, d.n, p.n_slices, Lr, p.ld, d.C, rc, b0, d.B, g.walking,
                           reinterpret_cast<unsigned long long*>(acc), d.bins->perm.as<int>(), degree);
        FDX_CHECK_LAUNCH();
    }
    return 0;
}

// scratch: codes, Lr (groups * ld * P), acc (groups * B * P * CC words); out: p.words words, zeroed here
template <int P>
static int launch_label_bands(const LabelBandPlan& p, const LbDevice& d, unsigned long long seed, long long first_perm, long long n_perm,
                              long long* null_dev, int* degree, const unsigned char* codes, unsigned char* Lr, long long* acc,
                              long long* partials, long long* out, hipStream_t st) {
    const size_t acc_bytes = (size_t)p.groups * d.B * P * p.CC * sizeof(long long);
    FDX_HIP(hipMemsetAsync(acc, 0, (size_t)d.B * P * p.CC * sizeof(long long), st));
    LpPermArgs pa{};
    hipLaunchKernelGGL((lp_stage_kernel<P, true>), dim3(ceil_div(p.ld, 256), 1), dim3(256), 0, st, codes, d.bins->perm.as<int>(), d.n, p.ld,
                       Lr, pa);
    FDX_CHECK_LAUNCH();
    FDX_TRY((launch_walk<P, true>(p, d, 1, Lr, acc, degree, st)));
    hipLaunchKernelGGL(lb_observed_kernel, dim3(ceil_div((long long)p.CC, 256), d.B), dim3(256), 0, st, acc, d.B, P, (long long)p.CC,
                       out + p.o_obs);
    FDX_CHECK_LAUNCH();
    hipLaunchKernelGGL(lb_degree_sums_kernel, dim3(p.deg_blocks), dim3(256), 0, st, degree, d.n, d.B, partials);
    FDX_CHECK_LAUNCH();
    FDX_TRY(launch_reduce_i64(partials, p.deg_blocks, 3LL * d.B, out + p.o_deg, st));
    if (n_perm <= 0) return 0;

    pa.keys = perm_keys(seed, first_perm, d.n);
    for (long long done = 0; done < n_perm; done += p.batch) {
        const int b = (int)std::min<long long>(p.batch, n_perm - done);     // the last batch may be ragged
        const int groups = ceil_div(b, P);
        pa.keys.first = first_perm + done;
        pa.batch = b;
        FDX_HIP(hipMemsetAsync(acc, 0, acc_bytes, st));
        hipLaunchKernelGGL((lp_stage_kernel<P, false>), dim3(ceil_div(p.ld, 256), groups), dim3(256), 0, st, codes, d.bins->perm.as<int>(),
                           d.n, p.ld, Lr, pa);
        FDX_CHECK_LAUNCH();
        FDX_TRY((launch_walk<P, false>(p, d, groups, Lr, acc, nullptr, st)));
        hipLaunchKernelGGL(lb_accum_kernel, dim3(ceil_div((long long)p.CC, 256), d.B), dim3(256), 0, st, acc, b, d.B, P, (long long)p.CC,
                           out + p.o_obs, null_dev ? null_dev + (size_t)done * d.B * p.CC : nullptr, out, p.band, p.cum);
        FDX_CHECK_LAUNCH();
    }
    return 0;
}

}  // namespace fdx

using namespace fdx;

extern "C" int fdx_label_cooccurrence_dev(const double* coords_dev, int64_t n, int32_t dim, const int32_t* labels_dev, int32_t C,
                                          const double* radii, int32_t B, uint64_t seed, int64_t first_perm, int64_t n_perm,
                                          int32_t max_batch, int32_t max_bands_per_pass, int32_t max_blocks, int64_t max_candidates,
                                          int32_t* degree_dev, int64_t* null_dev, int64_t* label_counts_out, int64_t* pair_out,
                                          int64_t* deg_sums_out, int64_t* count_ge_out, int64_t* count_le_out, double* sum_d_out,
                                          double* sumsq_d_out, int32_t* batch_out, int32_t* bands_per_pass_out, int64_t* candidates_out,
                                          void* stream) {
    const char* who = "fdx_label_cooccurrence_dev";
    FDX_REQUIRE(radii && label_counts_out && pair_out && deg_sums_out && count_ge_out && count_le_out && sum_d_out && sumsq_d_out,
                "fdx_label_cooccurrence_dev: null argument");
    FDX_REQUIRE(n >= 0 && n < (1LL << 31) - 128, "fdx_label_cooccurrence_dev: n must be between 0 and 2^31 - 129");
    FDX_REQUIRE(n == 0 || (coords_dev && labels_dev), "fdx_label_cooccurrence_dev: null argument");
    FDX_REQUIRE(dim >= 1 && dim <= 3, "fdx_label_cooccurrence_dev: coordinate dimension must be 1, 2 or 3");
    FDX_REQUIRE(C >= 1 && C <= LP_MAX_LABELS, "fdx_label_cooccurrence_dev: the number of labels must be between 1 and 64");
    FDX_REQUIRE(B >= 1 && B <= CG_MAX_BANDS, "fdx_label_cooccurrence_dev: between 1 and 32 radii");
    FDX_REQUIRE(first_perm >= 0 && n_perm >= 0 && max_batch >= 0 && max_bands_per_pass >= 0 && max_blocks >= 0 && max_candidates >= 0,
                "fdx_label_cooccurrence_dev: first_perm, n_perm, max_batch, max_bands_per_pass, max_blocks and max_candidates must not "
                "be negative");
    for (int b = 0; b < B; ++b)
        FDX_REQUIRE(std::isfinite(radii[b]) && radii[b] > (b ? radii[b - 1] : 0.0),
                    "fdx_label_cooccurrence_dev: radii must be positive, finite and strictly ascending");
    hipStream_t st = (hipStream_t)stream;
    PoolStream pool_stream(st);
    const LabelBandPlan plan = label_band_plan(n, C, B, n_perm, max_batch, max_bands_per_pass);
    const size_t X = (size_t)B * plan.CC;
    if (batch_out) *batch_out = n_perm > 0 && n > 1 ? plan.batch : 0;
    if (bands_per_pass_out) *bands_per_pass_out = n > 1 ? plan.bands_per_pass : 0;
    if (candidates_out) *candidates_out = n;                           // n <= 1: the one cell's count squared
    std::fill(label_counts_out, label_counts_out + C, (int64_t)0);
    std::fill(pair_out, pair_out + X, (int64_t)0);
    std::fill(deg_sums_out, deg_sums_out + 3 * (size_t)B, (int64_t)0);
    for (int half = 0; half < 2; ++half)                              // without pairs every N^r equals N = 0
        NullSumsLayout(X, 0).fill_empty(n_perm, count_ge_out + half * X, count_le_out + half * X, sum_d_out + half * X,
                                        sumsq_d_out + half * X);
    if (n == 0) return 0;

    DevBuf scratch, out;
    const size_t codes_bytes = (size_t)round_up(n, 16);
    const size_t lr_bytes = n > 1 ? (size_t)plan.groups * plan.ld * plan.P : 0;
    const size_t acc_bytes = n > 1 ? (size_t)plan.groups * X * plan.P * sizeof(long long) : 0;
    const size_t part_bytes = n > 1 ? (size_t)plan.deg_blocks * 3 * B * sizeof(long long) : 0;
    const size_t deg_bytes = n > 1 && !degree_dev ? (size_t)round_up((long long)n * B * sizeof(int), 16) : 0;
    FDX_TRY(scratch.alloc(codes_bytes + lr_bytes + acc_bytes + part_bytes + deg_bytes));
    FDX_TRY(out.alloc(plan.words * sizeof(long long)));
    unsigned char* codes = scratch.as<unsigned char>();
    unsigned char* Lr = codes + codes_bytes;
    long long* acc = reinterpret_cast<long long*>(Lr + lr_bytes);
    long long* partials = acc + acc_bytes / sizeof(long long);
    int* degree = degree_dev ? degree_dev : reinterpret_cast<int*>(reinterpret_cast<unsigned char*>(partials) + part_bytes);
    long long* o = out.as<long long>();
    FDX_HIP(hipMemsetAsync(o, 0, plan.words * sizeof(long long), st));
    hipLaunchKernelGGL(lp_prepare_kernel<false>, dim3(std::min(1024, ceil_div(n, 256))), dim3(256), 0, st, labels_dev, nullptr, (int)n, C,
                       codes, reinterpret_cast<unsigned long long*>(o + plan.o_counts), nullptr, reinterpret_cast<int*>(o + plan.o_flag));
    FDX_CHECK_LAUNCH();

    if (n > 1) {
        BinnedPoints bins;
        struct Drain {                                  // the binning's temporaries: nothing may still read them when they go back
            hipStream_t st;
            ~Drain() { (void)hipStreamSynchronize(st); }
        } drain{st};
        const double r_max = radii[B - 1];
        FDX_TRY(bin_points(coords_dev, n, dim, 1.0, r_max * CG_CELL_MARGIN, &bins, st));
        FDX_REQUIRE(bins.gp.h[0] >= r_max * CG_CELL_MARGIN, "fdx_label_cooccurrence_dev: the grid's cells are smaller than the largest radius");
        // the default limit: the walk's cost is candidates x walks - the observed one and one per launch chain of permutations,
        // each per chunk of bands - held to the correlogram's ten seconds
        if (max_candidates == 0) max_candidates = FDX_CORRELOGRAM_MAX_CANDIDATE_WALKS / lb_walks(plan, B, n_perm);
        long long candidates = 0, max_around = 0;
        const int guarded = cg_guard(who, bins, max_candidates, &candidates, &max_around, st);
        if (candidates_out) *candidates_out = candidates;
        FDX_TRY(guarded);
        FDX_REQUIRE(max_around < LB_MAX_AROUND,
                    "fdx_label_cooccurrence_dev: a spot has 2^26 candidates or more - one slice could overflow the 32-bit bins of a workgroup");
        const LbDevice d{&bins, radii, (int)n, C, B, max_around, max_blocks};
        if (plan.P == 16)
            FDX_TRY(launch_label_bands<16>(plan, d, seed, first_perm, n_perm, (long long*)null_dev, degree, codes, Lr, acc, partials, o, st));
        else
            FDX_TRY(launch_label_bands<8>(plan, d, seed, first_perm, n_perm, (long long*)null_dev, degree, codes, Lr, acc, partials, o, st));
        std::vector<long long> host(plan.words);
        FDX_TRY(copy_d2h(host.data(), out.p, host.size() * sizeof(long long), st));
        FDX_REQUIRE(host[plan.o_flag] == 0, "fdx_label_cooccurrence_dev: a label lies outside [-1, C)");
        std::copy(host.begin() + plan.o_counts, host.begin() + plan.o_counts + C, label_counts_out);
        std::copy(host.begin() + plan.o_obs, host.begin() + plan.o_obs + X, pair_out);
        std::copy(host.begin() + plan.o_deg, host.begin() + plan.o_deg + 3 * (size_t)B, deg_sums_out);
        if (n_perm > 0) {
            plan.band.unpack(host.data(), count_ge_out, count_le_out, sum_d_out, sumsq_d_out);
            plan.cum.unpack(host.data(), count_ge_out + X, count_le_out + X, sum_d_out + X, sumsq_d_out + X);
        }
        return 0;
    }
    // one spot: its label is counted and checked, there is no pair and nothing to walk
    if (degree_dev) FDX_HIP(hipMemsetAsync(degree_dev, 0, (size_t)B * sizeof(int), st));
    if (null_dev && n_perm > 0) FDX_HIP(hipMemsetAsync(null_dev, 0, (size_t)n_perm * X * sizeof(long long), st));
    std::vector<long long> host(plan.words);
    FDX_TRY(copy_d2h(host.data(), out.p, host.size() * sizeof(long long), st));
    FDX_REQUIRE(host[plan.o_flag] == 0, "fdx_label_cooccurrence_dev: a label lies outside [-1, C)");
    std::copy(host.begin() + plan.o_counts, host.begin() + plan.o_counts + C, label_counts_out);
    return 0;
}
