// Host-only exerciser of the schedule builders (tile_plan.cpp), of the packed spatial-sums layout (spatial_sums.h) and of the
// permutation entries' host arithmetic (perm_plan.h) for the sanitizer build: `make -C flashdeconv_amd/csrc asan-host`
// compiles this file and tile_plan.cpp with g++ -fsanitize=address,undefined and runs it.  No HIP, no GPU.
// (GPU AddressSanitizer is not available on the build pool; the pure-host parts of the library are what can be sanitised.)
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../perm_plan.h"
#include "../spatial_sums.h"
#include "../tile_plan.h"

using namespace fdx;

static int check_tile(int G, int d, int NW, int JW, int GB, unsigned seed) {
    std::mt19937 rng(seed);
    std::vector<int> bucket((size_t)G);
    std::vector<double> w((size_t)G);
    for (int g = 0; g < G; ++g) {
        bucket[(size_t)g] = (rng() % 41 == 0) ? -1 : (int)(rng() % (unsigned)d);
        w[(size_t)g] = (rng() & 1) ? 1.0 + (rng() % 100) * 0.01 : -1.0 - (rng() % 100) * 0.01;
    }
    TilePlanHost p;
    if (!build_tile_plan(bucket.data(), w.data(), G, d, NW, JW, GB, &p)) return d > 4 * NW * JW ? 0 : 1;
    // replay: every gene of Omega visited exactly once, in its bucket, inside its block
    std::vector<int> seen((size_t)G, 0);
    for (int wv = 0; wv < NW; ++wv)
        for (int c = 0; c < p.NBLK; ++c) {
            int e = p.ent_base[(size_t)wv * (p.NBLK + 1) + c];
            for (int j = 0; j < JW; ++j)
                for (int t = 0; t < p.len[((size_t)wv * p.NBLK + c) * JW + j]; ++t)
                    for (int q = 0; q < 4; ++q, ++e) {
                        const int g = p.gene[(size_t)e];
                        if (g < 0) continue;
                        if (g / GB != c || bucket[(size_t)g] != p.slot_bucket[((size_t)wv * JW + j) * 4 + q] || p.w[(size_t)e] != w[(size_t)g] ||
                            p.off[(size_t)e] != g - c * GB)
                            return 2;
                        ++seen[(size_t)g];
                    }
            if (e != p.ent_base[(size_t)wv * (p.NBLK + 1) + c + 1]) return 3;
        }
    for (int g = 0; g < G; ++g)
        if (seen[(size_t)g] != (bucket[(size_t)g] >= 0 ? 1 : 0)) return 4;
    return 0;
}

// the offsets tile [0, perm_doubles) without gap or overlap, and a block holding its own indices unpacks into arrays that are exactly
// as long as their slices (a copy that runs over ends in a redzone), each receiving its slice
static int check_spatial_sums(int K) {
    const SpatialSumsLayout L(K);
    const size_t k = (size_t)K, kk = k * k;
    const size_t at[] = {L.mean, L.m2, L.C, L.deg_sums, L.m4, L.count_ge, L.count_le, L.sum_d, L.sumsq_d, L.perm_doubles};
    const size_t len[] = {k, k, kk, 2, k, kk, kk, kk, kk};
    if (at[0] != 0 || L.observed_doubles != L.m4) return 1;
    for (int i = 0; i < 9; ++i)
        if (at[i] + len[i] != at[i + 1]) return 2;
    std::vector<double> h(L.perm_doubles), mean(k), m2(k), C(kk), m4(k), sd(kk), sq(kk);
    std::vector<int64_t> deg(2), ge(kk), le(kk);
    for (size_t i = 0; i < h.size(); ++i) {
        const bool is_int = (i >= L.deg_sums && i < L.m4) || (i >= L.count_ge && i < L.sum_d);
        const int64_t v = (int64_t)i;
        if (is_int) std::memcpy(&h[i], &v, 8);
        else h[i] = (double)i;
    }
    L.unpack(h.data(), mean.data(), m2.data(), C.data(), deg.data(), m4.data(), ge.data(), le.data(), sd.data(), sq.data());
    for (size_t i = 0; i < k; ++i)
        if (mean[i] != (double)(L.mean + i) || m2[i] != (double)(L.m2 + i) || m4[i] != (double)(L.m4 + i)) return 3;
    for (size_t i = 0; i < kk; ++i)
        if (C[i] != (double)(L.C + i) || sd[i] != (double)(L.sum_d + i) || sq[i] != (double)(L.sumsq_d + i) ||
            ge[i] != (int64_t)(L.count_ge + i) || le[i] != (int64_t)(L.count_le + i))
            return 4;
    if (deg[0] != (int64_t)L.deg_sums || deg[1] != (int64_t)L.deg_sums + 1) return 5;
    h.resize(L.observed_doubles);                      // an observed block alone, C left out; then the answers without spots
    L.unpack(h.data(), mean.data(), m2.data(), nullptr, deg.data());
    L.fill_empty(mean.data(), m2.data(), C.data(), m4.data());
    return mean[0] == mean[0] || m2[k - 1] != 0.0 || C[kk - 1] != 0.0 || m4[k - 1] != 0.0 ? 6 : 0;
}

// wl = b / 2, wr = b - wl with b = max(2, bit_length(n - 1))
static int check_feistel_widths() {
    std::vector<long long> ns = {1, 2, 3, 4, 5, (1LL << 31) - 129};
    for (int k : {3, 16, 30})
        for (long long d : {-1, 0, 1}) ns.push_back((1LL << k) + d);
    for (long long n : ns) {
        int b = 0;
        while (b < 62 && (1LL << b) <= n - 1) ++b;                 // bit_length(n - 1): the least b with n - 1 < 2^b
        b = b < 2 ? 2 : b;
        int wl = -1, wr = -1;
        ss_feistel_widths(n, &wl, &wr);
        if (wl != b / 2 || wr != b - b / 2) return 1;
    }
    return 0;
}

// the clamp against its rule written out step by step, over a grid that reaches every branch; the result always lies in [1, cap]
static int check_perm_batch() {
    for (long long fit : {0LL, 1LL, 7LL, 512LL, 1000000LL})
        for (long long cap : {1LL, 512LL, 65535LL})
            for (long long max_batch : {0LL, 1LL, 5LL, 1000000LL})
                for (long long n_perm : {0LL, 1LL, 6LL, 999LL}) {
                    long long want = fit;
                    if (cap < want) want = cap;
                    if (max_batch > 0) {
                        if (max_batch < want) want = max_batch;
                    }
                    if (n_perm < 1) {
                        if (1 < want) want = 1;
                    } else if (n_perm < want) {
                        want = n_perm;
                    }
                    if (want < 1) want = 1;
                    const long long got = perm_batch(fit, cap, max_batch, n_perm);
                    if (got != want || got < 1 || got > cap) return 1;
                }
    return 0;
}

// the four slices tile [base, end) without gap or overlap; a block holding its own indices unpacks into arrays exactly as long as
// their slices (a copy that runs over ends in a redzone); fill_empty gives n_perm, n_perm, 0, 0
static int check_null_sums(size_t X) {
    const size_t base = 5;
    const NullSumsLayout L(X, base);
    const size_t at[] = {L.count_ge, L.count_le, L.sum_d, L.sumsq_d, L.end};
    if (L.X != X || at[0] != base) return 1;
    for (int i = 0; i < 4; ++i)
        if (at[i] + X != at[i + 1]) return 2;
    std::vector<double> h(L.end), sd(X), sq(X);
    std::vector<int64_t> ge(X), le(X);
    for (size_t i = 0; i < h.size(); ++i) {
        const int64_t v = (int64_t)i;
        if (i < L.sum_d) std::memcpy(&h[i], &v, 8);
        else h[i] = (double)i;
    }
    L.unpack(h.data(), ge.data(), le.data(), sd.data(), sq.data());
    for (size_t i = 0; i < X; ++i)
        if (ge[i] != (int64_t)(L.count_ge + i) || le[i] != (int64_t)(L.count_le + i) || sd[i] != (double)(L.sum_d + i) ||
            sq[i] != (double)(L.sumsq_d + i))
            return 3;
    L.fill_empty(7, ge.data(), le.data(), sd.data(), sq.data());
    for (size_t i = 0; i < X; ++i)
        if (ge[i] != 7 || le[i] != 7 || sd[i] != 0.0 || sq[i] != 0.0) return 4;
    return 0;
}

int main() {
    int bad = 0;
    if (check_feistel_widths()) { std::printf("Feistel widths: error\n"); ++bad; }
    if (check_perm_batch()) { std::printf("permutation batch clamp: error\n"); ++bad; }
    for (size_t X : {(size_t)1, (size_t)16, (size_t)33 * 33}) {
        const int rc = check_null_sums(X);
        if (rc) { std::printf("null sums layout X=%zu: error %d\n", X, rc); ++bad; }
    }
    for (int K : {1, 4, 33}) {
        const int rc = check_spatial_sums(K);
        if (rc) { std::printf("spatial sums layout K=%d: error %d\n", K, rc); ++bad; }
    }
    const int shapes[][5] = {{2000, 512, 16, 8, 768}, {2000, 512, 12, 11, 1024}, {5000, 1024, 12, 22, 736}, {5003, 1024, 8, 32, 512},
                             {300, 64, 16, 8, 512}, {40, 7, 16, 8, 256}, {1001, 500, 8, 16, 256}, {2000, 600, 12, 11, 1024}};
    for (const auto& s : shapes)
        for (unsigned seed = 1; seed <= 3; ++seed) {
            const int rc = check_tile(s[0], s[1], s[2], s[3], s[4], seed);
            if (rc) { std::printf("tile plan G=%d d=%d NW=%d JW=%d GB=%d seed=%u: error %d\n", s[0], s[1], s[2], s[3], s[4], seed, rc); ++bad; }
        }
    std::printf(bad ? "FAILED\n" : "plan builders and sums layout: ok under the sanitizers\n");
    return bad ? 1 : 0;
}
