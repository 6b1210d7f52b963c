// Host-only exerciser of the graph cache's container (graph_cache.h: key equality on every scalar, least-recently-used order,
// per-device capacity, the reference count that handles and entries share) for the sanitizer build: `make -C flashdeconv_amd/csrc
// asan-host` compiles this file with g++ -fsanitize=address,undefined and runs it.  No HIP, no GPU: the coordinates, which the
// library compares on the device, are a host vector here and the "graph" is a counted object.
#include <atomic>
#include <cmath>
#include <cstdio>
#include <thread>
#include <vector>

#include "../graph_cache.h"

using namespace fdx;

namespace {

std::atomic<int> g_graphs{0};           // graphs not yet destroyed
struct Graph {
    RefCount refs;
    int tag = 0;
    explicit Graph(int t) : tag(t) { ++g_graphs; }
    ~Graph() { --g_graphs; }
};
void release(Graph* g) { if (g && g->refs.release()) delete g; }

struct Entry {
    GraphCacheKey key;
    long long bytes = 0;
    std::vector<double> coords;         // the entry's own copy
    Graph* g = nullptr;
    ~Entry() { release(g); }
};

GraphCacheKey key_of(long long n, int dim, int k = 6, int method = 1, double radius = 0.0, int dev = 0,
                     const char* switches = "") {
    GraphCacheKey q;
    q.n = n; q.dim = dim; q.k = k; q.method = method; q.radius = radius; q.dev = dev; q.switches = switches;
    return q;
}

// what fdx_graph_build_dev does: the candidates by scalars, the contents as bytes, hit (one more holder) or miss
Graph* find(GraphCache<Entry>& c, const GraphCacheKey& q, const std::vector<double>& coords) {
    for (const auto& e : c.candidates(q))
        if (e->coords.size() == coords.size() && std::memcmp(e->coords.data(), coords.data(), coords.size() * sizeof(double)) == 0) {
            c.hit(e);
            e->g->refs.retain();
            return e->g;
        }
    c.miss();
    return nullptr;
}

// a build that missed: the handle the caller gets (the creator's reference); the entry takes its own
Graph* build_and_publish(GraphCache<Entry>& c, const GraphCacheKey& q, const std::vector<double>& coords, int tag) {
    Graph* g = new Graph(tag);
    auto e = std::make_shared<Entry>();
    e->key = q;
    e->coords = coords;
    e->bytes = (long long)(coords.size() * sizeof(double));
    g->refs.retain();
    e->g = g;
    c.insert(std::move(e));
    return g;
}

std::vector<double> points(long long n, int dim, unsigned seed) {
    std::vector<double> v((size_t)(n * dim));
    unsigned s = seed * 2654435761u + 1u;
    for (double& x : v) { s = s * 1664525u + 1013904223u; x = (double)(s >> 8) * 0.125; }
    return v;
}

#define CHECK(cond) do { if (!(cond)) { std::printf("graph cache: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int keys() {
    GraphCache<Entry> c(2);
    const std::vector<double> P = points(100, 2, 1);
    const GraphCacheKey q = key_of(100, 2);
    CHECK(!find(c, q, P));
    Graph* first = build_and_publish(c, q, P, 1);
    std::vector<double> same = P;                               // another address, the same content
    Graph* hit = find(c, q, same);
    CHECK(hit == first && hit->refs.n == 3);
    release(hit);
    // every scalar of the key, one at a time
    CHECK(c.candidates(key_of(200, 1)).empty());                // the same bytes, another shape
    CHECK(c.candidates(key_of(50, 4)).empty());
    CHECK(c.candidates(key_of(100, 2, 5)).empty());
    CHECK(c.candidates(key_of(100, 2, 6, 2)).empty());
    CHECK(c.candidates(key_of(100, 2, 6, 1, 1.5)).empty());
    CHECK(c.candidates(key_of(100, 2, 6, 1, -0.0)).empty());    // the radius by its bits
    CHECK(c.candidates(key_of(100, 2, 6, 1, 0.0, 1)).empty());
    CHECK(c.candidates(key_of(100, 2, 6, 1, 0.0, 0, "1")).empty());
    CHECK(c.candidates(q).size() == 1);
    // the contents as bytes: one ulp at the first, a middle and the last word; -0.0 for 0.0
    for (size_t at : {(size_t)0, P.size() / 2, P.size() - 1}) {
        std::vector<double> Q = P;
        Q[at] = std::nextafter(Q[at], 1e300);
        CHECK(!find(c, q, Q));
    }
    std::vector<double> Z = P;
    Z[7] = 0.0;
    Graph* z = build_and_publish(c, q, Z, 2);
    Z[7] = -0.0;
    CHECK(!find(c, q, Z));
    CHECK(c.candidates(q).size() == 2 && c.candidates(q)[0]->g == z);   // most recently used first
    long long st[4];
    c.stats(st);
    CHECK(st[0] == 1 && st[1] == 5 && st[2] == 2 && st[3] == 2 * 200 * 8);
    release(first);
    release(z);
    CHECK(g_graphs == 2);                                       // the entries' references keep them
    c.clear();
    CHECK(g_graphs == 0);
    return 0;
}

int order_capacity_and_references() {
    {
        GraphCache<Entry> c(2);
        const GraphCacheKey q = key_of(40, 2);
        std::vector<std::vector<double>> P;
        for (unsigned i = 0; i < 4; ++i) P.push_back(points(40, 2, 10 + i));
        Graph* a = build_and_publish(c, q, P[0], 0);
        Graph* b = build_and_publish(c, q, P[1], 1);
        release(a);                                             // the handles go, the entries hold
        release(b);
        CHECK(g_graphs == 2);
        Graph* a2 = find(c, q, P[0]);                           // a is the most recently used now: b is the oldest
        CHECK(a2 && a2->tag == 0);
        Graph* d = build_and_publish(c, q, P[2], 2);            // evicts b, which nobody holds: gone
        CHECK(g_graphs == 2 && !find(c, q, P[1]));
        Graph* e = build_and_publish(c, q, P[3], 3);            // evicts a, which a2 still holds: lives on
        CHECK(g_graphs == 3 && !find(c, q, P[0]) && a2->tag == 0 && a2->refs.n == 1);
        release(a2);
        CHECK(g_graphs == 2);
        // the capacity is per device
        Graph* f = build_and_publish(c, key_of(40, 2, 6, 1, 0.0, 1), P[0], 4);
        long long st[4];
        c.stats(st);
        CHECK(st[2] == 3);
        Graph* d2 = find(c, q, P[2]);
        CHECK(d2 == d);
        release(d2);
        // a held handle outlives clear; both orders of letting go
        c.clear();
        c.stats(st);
        CHECK(st[2] == 0 && st[3] == 0 && g_graphs == 3 && d->tag == 2 && e->tag == 3 && f->tag == 4);
        release(e);
        release(d);
        release(f);
        CHECK(g_graphs == 0);
        Graph* g = build_and_publish(c, q, P[0], 5);
        Graph* g2 = find(c, q, P[0]);
        CHECK(g2 == g && g->refs.n == 3);
        release(g);                                             // the first handle first ...
        CHECK(g2->tag == 5 && g2->refs.n == 2);
        release(g2);
        g = find(c, q, P[0]);
        g2 = find(c, q, P[0]);
        release(g2);                                            // ... and the second first
        CHECK(g->tag == 5 && g->refs.n == 2);
        release(g);
    }
    CHECK(g_graphs == 0);                                       // the cache's own destructor releases what is left
    GraphCache<Entry> none(0);
    Graph* g = build_and_publish(none, key_of(3, 1), points(3, 1, 9), 0);
    CHECK(g_graphs == 1 && g->refs.n == 1);                     // (the entry that was never kept has let go)
    release(g);
    CHECK(g_graphs == 0);
    return 0;
}

// four threads, two coordinate sets, lookups, publications and clears interleaved: every hit is the right graph, the capacity
// holds, every graph dies exactly once
int threads() {
    {
        GraphCache<Entry> c(2);
        const GraphCacheKey q = key_of(64, 2);
        const std::vector<double> A = points(64, 2, 7), B = points(64, 2, 8);
        int bad[4] = {0, 0, 0, 0};
        std::vector<std::thread> th;
        for (int t = 0; t < 4; ++t)
            th.emplace_back([&, t]() {
                for (int it = 0; it < 400; ++it) {
                    const bool is_a = ((t + it) & 1) != 0;
                    std::vector<double> mine = is_a ? A : B;
                    Graph* g = find(c, q, mine);
                    if (!g) g = build_and_publish(c, q, mine, is_a ? 1 : 2);
                    if (g->tag != (is_a ? 1 : 2)) ++bad[t];
                    if (it % 97 == 0) c.clear();
                    long long st[4];
                    c.stats(st);
                    if (st[2] > 2) ++bad[t];
                    release(g);
                }
            });
        for (auto& w : th) w.join();
        CHECK(bad[0] + bad[1] + bad[2] + bad[3] == 0);
    }
    CHECK(g_graphs == 0);
    return 0;
}

}  // namespace

int main() {
    const int bad = keys() + order_capacity_and_references() + threads();
    std::printf(bad ? "FAILED\n" : "graph cache: ok under the sanitizers\n");
    return bad ? 1 : 0;
}
