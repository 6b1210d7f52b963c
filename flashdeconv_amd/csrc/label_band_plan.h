// The host arithmetic of the label co-occurrence (label_band_kernels.cpp): the shape of the walk's workgroup, the bands of a pass,
// the permutations of a launch chain, the grid that keeps a workgroup's 32-bit bins from overflowing, and the layout of the packed
// device result.  Plain host code (no HIP; lb_wave_bytes is also what the kernel lays its LDS out by): tested by
// hosttest/label_band_plan_asan.cpp.
//
// The table the plan follows (C labels, B bands; hist = nb * P * C^2 * 4 bytes of 32-bit bins in LDS, shared by the workgroup):
//   P      permutations of a group = bytes of a staged position: 16 for C <= 32, 8 above (lp_stage_kernel's two widths)
//   nb     bands per pass: as many as LB_HIST_BYTES = 128 KiB of bins hold, B and max_bands_per_pass at the most, one at the least
//            C <= 8: all 32 bands (at most 4 KiB a band)    C = 10: 20    C = 16: 8    C = 32: 2    33 <= C <= 36: 3
//            37 <= C <= 45: 2    46 <= C <= 64: 1 (C = 64: 8 * 4096 * 4 = 128 KiB, the whole budget for one band)
//   waves  per workgroup: the largest of 16, 8, 4, 2, 1 whose staging tiles - 64 candidates x (3 doubles + P bytes), and in the
//          observed pass nb x 64 int32 of band degrees - fit beside the bins in the CU's 160 KiB: 16 at C = 10 with ten bands
//          (62.5 KiB + 16 x 5 KiB), 8 at C = 32 (128 KiB + 8 x 3 KiB) and at C = 64 (128 KiB + 8 x 2.25 KiB)
//   batch  permutations per launch chain: what SCRATCH_BUDGET_BYTES holds of (ld label bytes + B C^2 int64 totals) a permutation,
//          whole groups, LB_MAX_GROUPS groups (a grid dimension) and max_batch at the most
//   grid   blocks.x: LB_TARGET_WAVES waves over all groups of a launch, no more than the slices need, max_blocks at the most - and
//          as many as the 32-bit bins need (lb_grid), which goes before max_blocks
// All of these sizes are arithmetic: 160 KiB is the CU's LDS, nothing here has been tuned by measurement.  Measured: DESIGN.md.
#pragma once
#include <algorithm>
#include <cstddef>

#include "perm_plan.h"

#ifdef __HIPCC__
#define LB_HOST_DEVICE __host__ __device__
#else
#define LB_HOST_DEVICE
#endif

namespace fdx {

constexpr size_t LB_LDS_BYTES = 160 * 1024;          // a CU's LDS: what one workgroup may take
constexpr size_t LB_HIST_BYTES = 128 * 1024;         // of it, the bins at the most
constexpr int LB_MAX_WAVES = 16;
constexpr int LB_MAX_GROUPS = 64;                    // groups of P permutations per launch chain (a grid dimension)
constexpr int LB_TARGET_WAVES = 8192;                // waves of a walk launch over all its groups: the chip's 256 CUs x 32
constexpr int LB_DEG_BLOCKS = 1024;                  // blocks of the degree sums at the most
constexpr long long LB_MAX_AROUND = 1LL << 26;       // candidates of one point: 64 of them a slice stay below 2^32
constexpr size_t LB_SCRATCH_BUDGET = (size_t)1 << 30;   // = SCRATCH_BUDGET_BYTES (gene_pass.h; static_assert in label_band_kernels.cpp)

// LDS of one wave's staging: xt, yt, wt [64] doubles | the candidates' P bytes | observed pass: D[nb][64] int32
LB_HOST_DEVICE inline size_t lb_wave_bytes(int P, int nb, bool observed) {
    return 3 * 64 * sizeof(double) + (size_t)64 * P + (observed ? (size_t)nb * 64 * sizeof(int) : 0);
}

// What a call runs with, and the packed device result (64-bit words):
// [band null: count_ge X | count_le X | sum_d X | sumsq_d X | cumulative null: the same | obs X | label counts C | flag |
//  W B | sum deg^2 B | sum cumulative deg^2 B], X = B * C^2.
struct LabelBandPlan {
    int P, bands_per_pass, chunks, waves;
    int groups, batch;                   // batch: permutations per launch chain, at most groups * P
    long long ld;
    int n_slices, deg_blocks;
    size_t CC;
    NullSumsLayout band, cum;
    size_t o_obs, o_counts, o_flag, o_deg, words;
};

inline size_t lb_lds_bytes(const LabelBandPlan& p, bool observed) {
    return (size_t)p.bands_per_pass * p.P * p.CC * sizeof(unsigned) + (size_t)p.waves * lb_wave_bytes(p.P, p.bands_per_pass, observed);
}

inline LabelBandPlan label_band_plan(long long n, int C, int B, long long n_perm, long long max_batch, int max_bands_per_pass) {
    LabelBandPlan p;
    p.P = C <= 32 ? 16 : 8;
    p.CC = (size_t)C * C;
    const size_t band_bytes = (size_t)p.P * p.CC * sizeof(unsigned);
    long long nb = std::min<long long>(B, (long long)(LB_HIST_BYTES / band_bytes));
    if (max_bands_per_pass > 0) nb = std::min<long long>(nb, max_bands_per_pass);
    p.bands_per_pass = (int)std::max<long long>(1, nb);
    p.chunks = (B + p.bands_per_pass - 1) / p.bands_per_pass;
    p.waves = LB_MAX_WAVES;
    while (p.waves > 1 && lb_lds_bytes(p, true) > LB_LDS_BYTES) p.waves /= 2;
    p.ld = (n + 1 + 63) / 64 * 64;
    p.n_slices = (int)((n + 63) / 64);
    p.deg_blocks = (int)std::max<long long>(1, std::min<long long>(LB_DEG_BLOCKS, (n + 255) / 256));
    const size_t per_group = (size_t)p.ld * p.P + (size_t)p.P * B * p.CC * sizeof(long long);
    const long long fit_groups = (long long)std::max<size_t>(1, LB_SCRATCH_BUDGET / per_group);   // a whole group at the least
    p.batch = (int)perm_batch(fit_groups * p.P, (long long)LB_MAX_GROUPS * p.P, max_batch, n_perm);
    p.groups = (p.batch + p.P - 1) / p.P;
    const size_t X = (size_t)B * p.CC;
    p.band = NullSumsLayout(X, 0);
    p.cum = NullSumsLayout(X, p.band.end);
    p.o_obs = p.cum.end;
    p.o_counts = p.o_obs + X;
    p.o_flag = p.o_counts + C;
    p.o_deg = p.o_flag + 1;
    p.words = p.o_deg + 3 * (size_t)B;
    return p;
}

// walks of the candidates a call makes: per chunk of bands the observed one and one per launch chain of permutations
inline long long lb_walks(const LabelBandPlan& p, int B, long long n_perm) {
    const long long chains = n_perm > 0 ? (n_perm + p.batch - 1) / p.batch : 0;
    return (long long)p.chunks * (1 + chains);
}

// The grid of a walk launch with `groups` groups: blocks.x and the waves of a workgroup that walk.  A bin takes at most one
// increment per ordered pair of a position the workgroup walks, a position has at most max_around candidates, so a workgroup may
// walk floor((2^32 - 1) / (64 max_around)) slices (max_around < LB_MAX_AROUND: at least one): where that is below the workgroup's
// waves only that many waves walk, one slice each.
struct LbGrid { int blocks, walking; };
inline LbGrid lb_grid(const LabelBandPlan& p, int groups, long long max_around, int max_blocks) {
    LbGrid g;
    const long long may = ((1LL << 32) - 1) / (64 * std::max<long long>(1, max_around));     // slices a workgroup may walk
    g.walking = (int)std::max<long long>(1, std::min<long long>(p.waves, may));
    const long long need = ((long long)p.n_slices + g.walking - 1) / g.walking;              // one slice a walking wave
    long long blocks = std::max<long long>(1, std::min<long long>(need, LB_TARGET_WAVES / ((long long)p.waves * groups)));
    if (max_blocks > 0) blocks = std::min<long long>(blocks, max_blocks);
    const long long rounds = std::max<long long>(1, may / g.walking);                        // slices a walking wave may take
    const long long least = ((long long)p.n_slices + g.walking * rounds - 1) / (g.walking * rounds);
    g.blocks = (int)std::max<long long>(1, std::min(need, std::max(blocks, least)));
    return g;
}

}  // namespace fdx
