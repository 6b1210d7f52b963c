// The host arithmetic of the label gene sums (label_gene_kernels.cpp): the constants of the kernel's shape, the segments, the stripes
// of the gathered copy, the permutations of a launch chain and the layout of the packed device result.  Plain host code (no HIP):
// tested by hosttest/label_gene_plan_asan.cpp.
#pragma once
#include <algorithm>
#include <cstddef>

#include "perm_plan.h"

namespace fdx {

constexpr int LG_B = 16;                 // permutations of a group (the staging's 16-byte word)
constexpr int LG_TS = 16;                // genes of a tile
constexpr int LG_THREADS = LG_B * LG_TS;
constexpr int LG_SEG = 2048;             // spots of a segment: a constant of the order, never a function of the launch
constexpr int LG_MAX_GROUPS = 64;        // groups per launch chain (a grid dimension)
constexpr int LG_MAX_GENES = 4096;
constexpr long long LG_MAX_SPOTS = 1LL << 24;     // 8192 segments: a grid dimension, and the smallest scratch block stays at 1 GiB
constexpr long long LG_MAX_STATS = 1LL << 22;     // P * C^2
constexpr int LG_MAX_GRID_YZ = 65535;    // what a grid's second and third dimension may be

// What a call runs with, and the packed device result (64-bit words):
// [u C S | nnz C S | label counts C | flag | null: count_ge X | count_le X | sum_d X | sumsq_d X].
struct LgPlan {
    int nseg, tiles_all, stripe_tiles, stripes, W;              // W: genes of a full stripe
    int groups, batch;                                          // batch: permutations per launch chain, at most groups * LG_B
    size_t lds, X, o_nnz, o_counts, o_flag, words;
    NullSumsLayout null;
    // bytes of the scratch blocks the plan stands for
    size_t tile_copy_bytes(long long n, size_t elem) const { return (size_t)stripe_tiles * n * LG_TS * elem; }
    size_t stage_bytes(long long n) const { return (size_t)groups * n * LG_B; }
    size_t part_bytes(int C) const { return (size_t)nseg * batch * C * W * sizeof(double); }
    size_t u_bytes(int C, int S) const { return (size_t)batch * C * S * sizeof(double); }
};

// n spots of `elem` bytes a value, C labels, S genes, P pairs; gather_bytes: what the gathered copy of a stripe may take; budget: the
// scratch budget of the permutations in flight; own_u: the caller keeps no null, so a batch's u^r rows are scratch too.
inline LgPlan lg_plan(long long n, size_t elem, int C, int S, long long P, long long n_perm, long long max_batch, size_t gather_bytes,
                      bool own_u, size_t budget) {
    LgPlan p;
    p.nseg = (int)((n + LG_SEG - 1) / LG_SEG);
    p.tiles_all = (S + LG_TS - 1) / LG_TS;
    const size_t tile_bytes = (size_t)n * LG_TS * elem;
    const size_t group_tile_part = (size_t)p.nseg * LG_B * C * LG_TS * sizeof(double);      // a group's segment blocks of one tile
    p.stripe_tiles = (int)std::max<size_t>(1, std::min<size_t>({(size_t)p.tiles_all, (size_t)LG_MAX_GRID_YZ, gather_bytes / tile_bytes,
                                                               budget / 2 / group_tile_part}));
    p.stripes = (p.tiles_all + p.stripe_tiles - 1) / p.stripe_tiles;
    p.W = p.stripe_tiles * LG_TS;
    // per permutation in flight: its label bytes, its segment blocks of a stripe, and its row of u^r where the caller keeps no null
    const size_t per_perm = (size_t)n + (size_t)p.nseg * C * p.W * sizeof(double) + (own_u ? (size_t)C * S * sizeof(double) : 0);
    const long long fit_groups = (long long)std::max<size_t>(1, budget / (per_perm * LG_B));
    const long long cap_groups = std::min<long long>(LG_MAX_GROUPS, LG_MAX_GRID_YZ / (LG_B * C));   // the fold's planes are a grid dimension
    p.batch = (int)perm_batch(fit_groups * LG_B, cap_groups * LG_B, max_batch, n_perm);
    p.groups = (p.batch + LG_B - 1) / LG_B;
    p.lds = (size_t)C * LG_THREADS * sizeof(double);
    p.X = (size_t)P * C * C;
    p.o_nnz = (size_t)C * S;
    p.o_counts = 2 * (size_t)C * S;
    p.o_flag = p.o_counts + C;
    p.null = NullSumsLayout(p.X, p.o_flag + 1);
    p.words = p.null.end;
    return p;
}

}  // namespace fdx
