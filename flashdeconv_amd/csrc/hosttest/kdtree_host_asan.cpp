// Host-only exerciser of the restated cKDTree (kdtree_host.cpp) and its thread pool (host_threads.cpp) for the sanitizer builds:
// `make -C flashdeconv_amd/csrc asan-host` compiles the three files with g++ -fsanitize=address,undefined, and once more with
// -fsanitize=thread, and runs them.  No HIP, no GPU, no scipy: the SERIAL build (one thread: scipy's algorithm step by step, which
// tests/test_host.py holds against scipy itself) is the reference, and every parallel form of the build - the passes of large
// nodes cut into pool tasks, subtrees as tasks, subtrees on a contiguous copy - has to give its index array and its k-nearest
// lists element for element; on a tie-free cloud the lists are also those of a brute-force search.  (No fork() here: in a
// sanitised multi-threaded program that tests the sanitizer; test_ckdtree_thread_pool_survives_a_fork has it.)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "../fdx_env.h"
#include "../kdtree_host.h"

namespace {
const char* g_par_depth = nullptr;      // what FDX_KDTREE_PAR_DEPTH reads as (set between builds only)
}
namespace fdx {
const char* env(const char* name) { return std::strcmp(name, "FDX_KDTREE_PAR_DEPTH") == 0 ? g_par_depth : nullptr; }
}

using namespace fdx;

namespace {

struct Input {
    const char* name;
    int dim;
    std::vector<double> c;
    long long n() const { return (long long)c.size() / dim; }
    // of the serial build
    std::vector<int64_t> order, k5, k7;
};

unsigned g_seed = 12345u;
unsigned rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

Input lattice(const char* name, int nx, int ny) {
    Input in{name, 2, {}, {}, {}, {}};
    for (int x = 0; x < nx; ++x) for (int y = 0; y < ny; ++y) { in.c.push_back(x); in.c.push_back(y); }
    return in;
}
Input hex(int rows, int cols) {
    Input in{"hex", 2, {}, {}, {}, {}};
    for (int r = 0; r < rows; ++r) for (int c = 0; c < cols; ++c) { in.c.push_back(c + 0.5 * (r & 1)); in.c.push_back(r * std::sqrt(3.0) / 2.0); }
    return in;
}
Input cube(int side) {
    Input in{"cube", 3, {}, {}, {}, {}};
    for (int x = 0; x < side; ++x) for (int y = 0; y < side; ++y) for (int z = 0; z < side; ++z) { in.c.push_back(x); in.c.push_back(y); in.c.push_back(z); }
    return in;
}
Input integers(long long n, int dim, unsigned values) {               // the median is often the node's minimum: the split just above it
    Input in{"integers", dim, {}, {}, {}, {}};
    for (long long i = 0; i < n * dim; ++i) in.c.push_back((double)(rnd() % values));
    return in;
}
Input cloud(long long n) {                                            // 24 random bits per coordinate: no two distances alike
    Input in{"cloud", 2, {}, {}, {}, {}};
    for (long long i = 0; i < n * 2; ++i) in.c.push_back((double)rnd() / 16777216.0 * 60.0);
    return in;
}

struct Lists { std::vector<int64_t> order, k5, k7; };

// one build; its index array and the lists of every point for kk 5 and 7
// (query_threads: the serial build's tree is queried on several threads - the queries only read the tree)
bool build_and_query(const Input& in, Lists* out, int query_threads = 0) {
    KdTree t;
    kd_build_tree(t, in.c.data(), in.n(), in.dim);
    if (query_threads) kd_set_threads(query_threads);
    out->order.assign((size_t)in.n(), -2);
    out->k5.assign((size_t)in.n() * 5, -2);
    out->k7.assign((size_t)in.n() * 7, -2);
    return ckdtree_query_host(t, 5, nullptr, 0, out->k5.data(), out->order.data()) &&
           ckdtree_query_host(t, 7, nullptr, 0, out->k7.data(), nullptr);
}

void settings(int threads, long long team_min, long long local_max, const char* par_depth) {
    kd_set_threads(threads);
    kd_set_team_min(team_min);
    kd_set_local_max(local_max);
    g_par_depth = par_depth;
}

#define CHECK(cond, ...) do { if (!(cond)) { std::printf("kdtree host: line %d: %s: ", __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); return 1; } } while (0)

int same_as_serial(const Input& in, const char* what) {
    Lists got;
    CHECK(build_and_query(in, &got), "%s %s", in.name, what);
    CHECK(got.order == in.order, "%s (%lld points, %d-D) %s: index array", in.name, in.n(), in.dim, what);
    CHECK(got.k5 == in.k5 && got.k7 == in.k7, "%s (%lld points, %d-D) %s: lists", in.name, in.n(), in.dim, what);
    return 0;
}

// Every setting the Python tests use, crossed: 2 team_min x 3 local_max x 3 thread shares = 18 builds, the par depth rotating
// through default / 0 / 2 against the share.  The inputs below the fork threshold take all 18 (those under 4096 points the 9 with
// team_min 64: at 5000 kd_build_tree gives them no pool), index array and both lists (kk 5 and 7) compared on each.  The large lattice takes every fourth combination - 4 is coprime to the 3 shares and local_max values,
// so its five builds are (team_min, local_max, share, par depth) = (64, 0, 2, default), (64, 300, 5, 2), (64, default, 11, 0),
// (5000, 300, 2, 0), (5000, default, 5, default) - with the index array and both lists compared on each.
int every_setting(const Input& in, bool large) {
    const long long team_mins[2] = {64, 5000}, local_maxes[3] = {0, 300, -1};
    const int shares[3] = {2, 5, 11};
    const char* depths[3] = {nullptr, "0", "2"};
    int combo = -1;
    for (long long team_min : team_mins)
        for (long long local_max : local_maxes)
            for (int share : shares) {
                ++combo;
                if (large && combo % 4 != 0) continue;
                if (team_min == 5000 && in.n() < 4096) continue;   // (no pool below 4096 points at this team_min: the serial build again)
                const char* depth = depths[(combo + combo / 3) % 3];
                settings(share, team_min, local_max, depth);
                char what[96];
                std::snprintf(what, sizeof what, "team_min %lld local_max %lld threads %d par_depth %s", team_min, local_max, share, depth ? depth : "default");
                if (same_as_serial(in, what)) return 1;
            }
    return 0;
}

// the tie-free cloud's first 2000 points: the lists are the kk nearest by distance, whatever the tree's order
int brute_force(const Input& all) {
    Input in{"cloud subset", 2, std::vector<double>(all.c.begin(), all.c.begin() + 2 * 2000), {}, {}, {}};
    const long long n = in.n();
    settings(5, 64, 300, nullptr);
    Lists got;
    CHECK(build_and_query(in, &got), "cloud subset");
    std::vector<std::pair<double, int64_t>> d((size_t)n);
    for (long long i = 0; i < n; ++i) {
        for (long long j = 0; j < n; ++j) {
            double s = 0.0;
            for (int a = 0; a < 2; ++a) { const double diff = in.c[(size_t)(j * 2 + a)] - in.c[(size_t)(i * 2 + a)]; s += diff * diff; }
            d[(size_t)j] = {s, j};
        }
        std::partial_sort(d.begin(), d.begin() + 8, d.end());
        CHECK(d[6].first < d[7].first, "cloud subset: distances tie at point %lld", i);
        for (int k = 0; k < 7; ++k) {
            CHECK(got.k7[(size_t)(i * 7 + k)] == d[(size_t)k].second, "cloud subset: point %lld neighbour %d of 7", i, k);
            if (k < 5) CHECK(got.k5[(size_t)(i * 5 + k)] == d[(size_t)k].second, "cloud subset: point %lld neighbour %d of 5", i, k);
        }
    }
    // the entry's own form (build + queries of some rows) on the same points
    const int64_t rows[3] = {1999, 0, 777};
    int64_t ids[3 * 7];
    CHECK(ckdtree_knn_impl(in.c.data(), n, 2, 7, rows, 3, ids, nullptr), "cloud subset: rows");
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 7; ++k) CHECK(ids[r * 7 + k] == got.k7[(size_t)(rows[r] * 7 + k)], "cloud subset: row %d neighbour %d", r, k);
    return 0;
}

// three threads build different inputs at once, all through the one pool (the C++ form of
// test_ckdtree_builds_from_several_threads_share_the_pool), at the largest share: the large lattice's forks on 22 members
int concurrent(const std::vector<Input>& inputs) {
    settings(11, 64, -1, nullptr);
    int bad[3] = {0, 0, 0};
    std::vector<std::thread> th;
    for (int w = 0; w < 3; ++w)
        th.emplace_back([&, w] {
            for (size_t i = (size_t)w; i < inputs.size(); i += 3) bad[w] += same_as_serial(inputs[i], "beside two other builds");
        });
    for (auto& x : th) x.join();
    CHECK(bad[0] + bad[1] + bad[2] == 0, "%d builds differ", bad[0] + bad[1] + bad[2]);
    return 0;
}

}  // namespace

int main() {
    std::vector<Input> inputs;
    inputs.push_back(lattice("square lattice", 60, 50));
    inputs.push_back(hex(45, 45));
    inputs.push_back(cube(11));
    for (int dim = 1; dim <= 3; ++dim)
        for (unsigned values : {2u, 5u, 30u}) inputs.push_back(integers(2000 + 100 * dim + 7 * values, dim, values));
    inputs.push_back(cloud(4200));                                   // (4096 points and more: pooled at team_min 5000 too)
    inputs.push_back(lattice("large lattice", 310, 300));            // above the 32768 points from which subtrees become pool tasks
    int bad = 0;
    for (Input& in : inputs) {
        settings(1, 0, -1, nullptr);                                  // one thread: the serial build
        Lists ref;
        if (!build_and_query(in, &ref, 8)) { std::printf("kdtree host: %s: serial build\n", in.name); return 1; }
        in.order = ref.order; in.k5 = ref.k5; in.k7 = ref.k7;
        std::vector<int64_t> sorted(in.order);
        std::sort(sorted.begin(), sorted.end());
        for (long long i = 0; i < in.n(); ++i)
            if (sorted[(size_t)i] != i || in.k5[(size_t)i * 5] < 0 || in.k7[(size_t)i * 7 + 6] < 0) { std::printf("kdtree host: %s: the serial build's index array or lists\n", in.name); return 1; }
        bad += every_setting(in, in.n() > 32768);
    }
    bad += brute_force(inputs[inputs.size() - 2]);
    bad += concurrent(inputs);
    settings(0, 0, -1, nullptr);
    std::printf(bad ? "FAILED\n" : "kdtree host: ok under the sanitizers\n");
    return bad ? 1 : 0;
}
