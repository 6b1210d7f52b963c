// Host-only exerciser of the label co-occurrence's plan (label_band_plan.h) for a sanitizer build: g++ -fsanitize=address,undefined,
// no HIP, no GPU (tests/test_cooccurrence_plan_host.py compiles and runs it).  Over a range of shapes it holds the plan to what the
// launcher and the walk kernel rely on - the bins and the waves' tiles inside the CU's 160 KiB with at least one band a pass at
// C = 64, chunks that cover every band, a batch within its caps and the scratch budget, a packed result without gap or overlap, and a
// grid that covers every slice while no workgroup's pair visits reach 2^32 - and replays the kernels' extreme indices on buffers of
// exactly the planned sizes, so an index past a block ends in a redzone.
#include <cstdio>
#include <cstdint>
#include <vector>

#include "../label_band_plan.h"

using namespace fdx;

static int check_plan(long long n, int C, int B, long long n_perm, long long max_batch, int max_bpp, bool replay) {
    const LabelBandPlan p = label_band_plan(n, C, B, n_perm, max_batch, max_bpp);
    const size_t CC = (size_t)C * C, X = (size_t)B * CC;
    if (p.P != (C <= 32 ? 16 : 8) || p.CC != CC) return 1;
    if (p.bands_per_pass < 1 || p.bands_per_pass > B || (max_bpp > 0 && p.bands_per_pass > max_bpp)) return 2;
    if (p.chunks * p.bands_per_pass < B || (p.chunks - 1) * p.bands_per_pass >= B) return 3;
    if (p.waves < 1 || p.waves > LB_MAX_WAVES || (p.waves & (p.waves - 1))) return 4;
    if (lb_lds_bytes(p, true) > LB_LDS_BYTES || lb_lds_bytes(p, false) > lb_lds_bytes(p, true)) return 5;
    if ((size_t)p.bands_per_pass * p.P * CC * 4 > LB_HIST_BYTES) return 6;
    if (lb_wave_bytes(p.P, p.bands_per_pass, true) % 16 || lb_wave_bytes(p.P, p.bands_per_pass, false) % 16) return 7;
    if (p.ld % 64 || p.ld <= n || p.ld < 64LL * p.n_slices || 64LL * p.n_slices < n || 64LL * (p.n_slices - 1) >= n) return 8;
    if (p.batch < 1 || (max_batch > 0 && p.batch > max_batch) || (n_perm > 0 && p.batch > n_perm)) return 9;
    if (p.groups < 1 || p.groups > LB_MAX_GROUPS || (long long)p.groups * p.P < p.batch || (long long)(p.groups - 1) * p.P >= p.batch) return 10;
    if (p.groups > 1 && (size_t)p.groups * ((size_t)p.ld * p.P + (size_t)p.P * X * 8) > LB_SCRATCH_BUDGET) return 11;
    if (p.band.count_ge != 0 || p.band.end != 4 * X || p.cum.count_ge != 4 * X || p.cum.end != 8 * X || p.o_obs != 8 * X ||
        p.o_counts != 9 * X || p.o_flag != 9 * X + C || p.o_deg != p.o_flag + 1 || p.words != p.o_deg + 3 * (size_t)B)
        return 12;
    if (lb_walks(p, B, n_perm) != (long long)p.chunks * (1 + (n_perm > 0 ? (n_perm + p.batch - 1) / p.batch : 0))) return 13;
    // the grid: every slice walked, and no workgroup walks more pair visits than a 32-bit bin holds
    for (long long M : {1LL, 9LL, 729LL, 1LL << 20, (1LL << 22) + 1, (1LL << 24) - 1, LB_MAX_AROUND - 1})
        for (int groups : {1, p.groups})
            for (int max_blocks : {0, 1, 7}) {
                const LbGrid g = lb_grid(p, groups, M, max_blocks);
                if (g.walking < 1 || g.walking > p.waves || g.blocks < 1) return 14;
                const long long rounds = (p.n_slices + (long long)g.blocks * g.walking - 1) / ((long long)g.blocks * g.walking);
                if (rounds < 1) return 15;
                // a workgroup's slices x 64 positions x M candidates
                const unsigned __int128 visits = (unsigned __int128)rounds * g.walking * 64 * M;
                if (visits > 0xffffffffULL) return 16;
                if (max_blocks > 0 && g.blocks > max_blocks && (unsigned __int128)((p.n_slices + (long long)max_blocks * g.walking - 1) /
                                                                                   ((long long)max_blocks * g.walking)) * g.walking * 64 * M <= 0xffffffffULL)
                    return 17;                                          // max_blocks is exceeded only where the bins need it
            }
    if (!replay) return 0;
    // the kernels' extreme indices on buffers of the planned sizes
    std::vector<unsigned char> lds(lb_lds_bytes(p, true)), lr((size_t)p.groups * p.ld * p.P);
    std::vector<int64_t> acc((size_t)p.groups * X * p.P), out(p.words), null_out((size_t)p.batch * X);
    const size_t bins = (size_t)p.bands_per_pass * p.P * CC;
    const size_t tile = bins * 4 + (size_t)(p.waves - 1) * lb_wave_bytes(p.P, p.bands_per_pass, true);
    lds[tile + 3 * 64 * 8 + 63 * p.P + p.P - 1] = 1;                                                  // the last candidate's last byte
    lds[tile + 3 * 64 * 8 + 64 * p.P + ((size_t)(p.bands_per_pass - 1) * 64 + 63) * 4 + 3] = 1;      // D[nb - 1][63]
    lds[(((size_t)(p.bands_per_pass - 1) * p.P + p.P - 1) * CC + CC - 1) * 4 + 3] = 1;                // the last bin
    lr[((size_t)(p.groups - 1) * p.ld + 64 * (size_t)p.n_slices - 1) * p.P + p.P - 1] = 1;
    for (int b0 = 0; b0 < B; b0 += p.bands_per_pass) {
        const int nb = std::min(p.bands_per_pass, B - b0);
        acc[((size_t)(p.groups - 1) * B + b0) * p.P * CC + (size_t)nb * p.P * CC - 1] = 1;            // the flush's last bin
    }
    const int r = p.batch - 1;
    (void)acc[(((size_t)(r / p.P) * B + (B - 1)) * p.P + (r % p.P)) * CC + CC - 1];                   // the accumulate kernel's last read
    null_out[((size_t)r * B + B - 1) * CC + CC - 1] = 1;
    out[p.cum.sumsq_d + X - 1] = 1;
    out[p.o_deg + 3 * (size_t)B - 1] = 1;
    std::vector<int64_t> ge(X), le(X);
    std::vector<double> sd(X), sq(X);
    p.band.unpack(out.data(), ge.data(), le.data(), sd.data(), sq.data());
    p.cum.unpack(out.data(), ge.data(), le.data(), sd.data(), sq.data());
    return 0;
}

int main() {
    int cases = 0;
    for (long long n : {2LL, 63LL, 64LL, 65LL, 5000LL, 1000000LL, (1LL << 31) - 129})
        for (int C : {1, 2, 8, 9, 10, 16, 17, 32, 33, 36, 37, 45, 46, 64})
            for (int B : {1, 2, 10, 32})
                for (long long R : {0LL, 1LL, 7LL, 8LL, 9LL, 16LL, 17LL, 999LL, 100000LL})
                    for (long long mb : {0LL, 1LL, 24LL})
                        for (int bpp : {0, 1, 3}) {
                            const bool replay = n <= 5000 && R <= 17 && (C <= 17 || B <= 2);
                            const int rc = check_plan(n, C, B, R, mb, bpp, replay);
                            if (rc) {
                                std::printf("label band plan: case n=%lld C=%d B=%d R=%lld max_batch=%lld max_bands_per_pass=%d: %d\n", n, C, B, R,
                                            mb, bpp, rc);
                                return 1;
                            }
                            ++cases;
                        }
    // C = 64 works with one band a pass, and the table's examples
    if (label_band_plan(5000, 64, 32, 0, 0, 0).bands_per_pass != 1 || label_band_plan(5000, 64, 32, 0, 0, 0).waves != 8) return 1;
    if (label_band_plan(5000, 10, 10, 999, 0, 0).bands_per_pass != 10 || label_band_plan(5000, 10, 10, 999, 0, 0).waves != 16) return 1;
    if (label_band_plan(5000, 10, 32, 0, 0, 0).bands_per_pass != 20 || label_band_plan(5000, 16, 32, 0, 0, 0).bands_per_pass != 8) return 1;
    if (label_band_plan(5000, 32, 32, 0, 0, 0).bands_per_pass != 2 || label_band_plan(5000, 32, 32, 0, 0, 0).waves != 8) return 1;
    if (label_band_plan(5000, 36, 32, 0, 0, 0).bands_per_pass != 3 || label_band_plan(5000, 45, 32, 0, 0, 0).bands_per_pass != 2 ||
        label_band_plan(5000, 46, 32, 0, 0, 0).bands_per_pass != 1)
        return 1;
    std::printf("label band plan: %d cases ok under the sanitizers\n", cases);
    return 0;
}
