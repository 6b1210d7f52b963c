// Host-only exerciser of the label gene sums' plan (label_gene_plan.h) for a sanitizer build: g++ -fsanitize=address,undefined, no
// HIP, no GPU (tests/test_ligrec_plan_host.py compiles and runs it).  Over a range of shapes it holds the plan to what the launcher
// relies on - whole tiles in stripes that cover every gene, a batch within its caps, grid dimensions within 65,535, scratch within
// the budget wherever more than the smallest block is asked for - and replays the kernels' index arithmetic on buffers of exactly
// the planned sizes, so an index past a block ends in a redzone.
#include <cstdio>
#include <cstdint>
#include <vector>

#include "../label_gene_plan.h"

using namespace fdx;

static int check_plan(long long n, size_t elem, int C, int S, long long P, long long n_perm, long long max_batch, size_t gather, bool own_u,
                      size_t budget, bool replay) {
    const LgPlan p = lg_plan(n, elem, C, S, P, n_perm, max_batch, gather, own_u, budget);
    if (p.nseg < 1 || (long long)p.nseg * LG_SEG < n || (long long)(p.nseg - 1) * LG_SEG >= n) return 1;
    if (p.tiles_all * LG_TS < S || (p.tiles_all - 1) * LG_TS >= S) return 2;
    if (p.stripe_tiles < 1 || p.stripe_tiles > p.tiles_all || p.stripe_tiles > LG_MAX_GRID_YZ) return 3;
    if ((long long)p.stripes * p.stripe_tiles < p.tiles_all || (long long)(p.stripes - 1) * p.stripe_tiles >= p.tiles_all) return 4;
    if (p.W != p.stripe_tiles * LG_TS) return 5;
    if (p.batch < 1 || (max_batch > 0 && p.batch > max_batch) || (n_perm > 0 && p.batch > n_perm)) return 6;
    if (p.groups < 1 || p.groups > LG_MAX_GROUPS || (long long)p.groups * LG_B < p.batch || (long long)(p.groups - 1) * LG_B >= p.batch) return 7;
    if ((long long)p.batch * C > LG_MAX_GRID_YZ || p.nseg > LG_MAX_GRID_YZ) return 8;            // the fold's planes, the null kernel's segments
    if (p.lds != (size_t)C * 2048 || p.lds > 160 * 1024) return 9;
    // more than one tile a stripe / one group a chain only where the budget holds it
    if (p.stripe_tiles > 1 && (p.tile_copy_bytes(n, elem) > gather || (size_t)p.nseg * LG_B * C * p.W * sizeof(double) > budget / 2)) return 10;
    if (p.groups > 1 && p.stage_bytes(n) + (size_t)p.groups * LG_B * ((size_t)p.nseg * C * p.W * sizeof(double) + (own_u ? (size_t)C * S * 8 : 0)) > budget)
        return 11;
    // the packed result: [u | nnz | counts | flag | four null arrays] without gap or overlap
    const size_t cs = (size_t)C * S, X = (size_t)P * C * C;
    if (p.X != X || p.o_nnz != cs || p.o_counts != 2 * cs || p.o_flag != 2 * cs + C || p.null.count_ge != p.o_flag + 1 ||
        p.null.count_le != p.null.count_ge + X || p.null.sum_d != p.null.count_le + X || p.null.sumsq_d != p.null.sum_d + X ||
        p.null.end != p.null.sumsq_d + X || p.words != p.null.end)
        return 12;
    if (!replay) return 0;
    // the kernels' extreme indices on buffers of the planned sizes
    std::vector<unsigned char> yt(p.tile_copy_bytes(n, elem)), lr(p.stage_bytes(n));
    std::vector<double> part(p.part_bytes(C) / sizeof(double)), u(p.u_bytes(C, S) / sizeof(double));
    std::vector<int64_t> out(p.words), ge(X), le(X);
    std::vector<double> sd(X), sq(X);
    for (int t0 = 0; t0 < p.tiles_all; t0 += p.stripe_tiles) {
        const int tiles = std::min(p.stripe_tiles, p.tiles_all - t0), s0 = t0 * LG_TS;
        const int nb = p.batch;
        for (int g = 0; g < (nb + LG_B - 1) / LG_B; ++g)
            for (int tile = 0; tile < tiles; ++tile)
                for (int seg = 0; seg < p.nseg; ++seg)
                    for (int t : {0, LG_THREADS - 1}) {
                        const int j = t >> 4, s = t & (LG_TS - 1), r = g * LG_B + j;
                        const long long i0 = (long long)seg * LG_SEG, i1 = std::min<long long>(n, i0 + LG_SEG);
                        yt[(((size_t)tile * n + (i1 - 1)) * LG_TS + s) * elem + (elem - 1)] = 1;
                        lr[((size_t)g * n + (i1 - 1)) * LG_B + j] = 1;
                        if (r < nb) part[(((size_t)seg * p.batch + r) * C + (C - 1)) * p.W + (size_t)tile * LG_TS + s] = 1.0;
                    }
        // the fold: plane (r, c), gene j of the stripe's valid width, into the batch's rows of u at column s0
        const int width = std::min(tiles * LG_TS, S - s0);
        for (int plane : {0, nb * C - 1})
            for (int j : {0, width - 1}) {
                const double v = part[(size_t)(p.nseg - 1) * p.batch * C * p.W + (size_t)plane * p.W + j];
                if (own_u) u[(size_t)plane * S + s0 + j] = v;
            }
    }
    p.null.unpack(out.data(), ge.data(), le.data(), sd.data(), sq.data());
    return 0;
}

int main() {
    const size_t GiB = (size_t)1 << 30;
    int cases = 0;
    for (long long n : {1LL, 2LL, 2047LL, 2048LL, 2049LL, 4500LL, 100000LL})
        for (int C : {1, 2, 16, 17, 33, 64})
            for (int S : {1, 15, 16, 17, 40, 4096})
                for (long long R : {0LL, 1LL, 15LL, 16LL, 17LL, 1023LL, 1024LL, 1025LL, 100000LL})
                    for (long long mb : {0LL, 1LL, 24LL})
                        for (size_t gather : {(size_t)1, (size_t)n * 64, GiB})
                            for (size_t budget : {(size_t)1 << 16, (size_t)1 << 24, GiB}) {
                                const bool replay = n <= 4500 && C <= 17 && S <= 40 && R <= 17 && budget == ((size_t)1 << 16);
                                for (bool own : {false, true}) {
                                    const int rc = check_plan(n, (cases & 1) ? 8 : 4, C, S, S <= 40 ? 24 : 1024, R, mb, gather, own, budget, replay);
                                    if (rc) {
                                        std::printf("label gene plan: case n=%lld C=%d S=%d R=%lld max_batch=%lld gather=%zu budget=%zu own=%d: %d\n", n,
                                                    C, S, R, mb, gather, budget, (int)own, rc);
                                        return 1;
                                    }
                                    ++cases;
                                }
                            }
    // the largest request the entry accepts
    if (check_plan(LG_MAX_SPOTS, 8, 64, LG_MAX_GENES, 1024, 1 << 20, 0, GiB, true, GiB, false)) return 1;
    std::printf("label gene plan: %d cases ok under the sanitizers\n", cases + 1);
    return 0;
}
