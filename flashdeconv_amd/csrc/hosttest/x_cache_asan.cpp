// Host-only exerciser of the X caches' lookup (x_cache.h: key compare, least-recently-used order, capacity, shared ownership) for
// the sanitizer build: `make -C flashdeconv_amd/csrc asan-host` compiles this file with g++ -fsanitize=address,undefined and runs
// it.  No HIP, no GPU.
#include <atomic>
#include <cmath>
#include <cstdio>
#include <random>
#include <thread>
#include <vector>

#include "../x_cache.h"

using namespace fdx;

namespace {

std::atomic<int> g_alive{0};            // entries not yet destroyed
struct Entry {
    XCacheKey key;
    std::vector<double> X;
    int tag = 0;
    Entry() { ++g_alive; }
    ~Entry() { --g_alive; }
};

std::vector<double> matrix(int K, int G, unsigned seed) {
    std::mt19937 rng(seed);
    std::vector<double> X((size_t)K * G);
    for (double& v : X) v = (double)(rng() % 10000) * 0.25;
    return X;
}

XCacheKey key_of(const std::vector<double>& X, int K, int G, double reg = 1e-6, int dev = 0) {
    XCacheKey k;
    k.dev = dev; k.K = K; k.G = G; k.reg = reg; k.X = X.data();
    return k;
}

std::shared_ptr<Entry> entry_of(const std::vector<double>& X, int K, int G, int tag, double reg = 1e-6, int dev = 0) {
    auto e = std::make_shared<Entry>();
    e->X = X;
    e->key = key_of(e->X, K, G, reg, dev);
    e->tag = tag;
    return e;
}

#define CHECK(cond) do { if (!(cond)) { std::printf("x cache: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int keys() {
    XCache<Entry> c(4);
    const int K = 5, G = 300;
    const std::vector<double> X = matrix(K, G, 1);
    CHECK(!c.find(key_of(X, K, G)));
    c.insert(entry_of(X, K, G, 1));
    std::vector<double> same = X;                               // another address, the same content
    auto hit = c.find(key_of(same, K, G));
    CHECK(hit && hit->tag == 1 && hit->key.X == hit->X.data());
    for (size_t at : {(size_t)0, (size_t)777, X.size() - 1}) {  // one ulp, at a sampled word and between two
        std::vector<double> Y = X;
        Y[at] = std::nextafter(Y[at], 1e300);
        CHECK(!c.find(key_of(Y, K, G)));
    }
    std::vector<double> Z = X;
    Z[3] = 0.0;
    c.insert(entry_of(Z, K, G, 2));
    Z[3] = -0.0;                                                // compared as bytes
    CHECK(!c.find(key_of(Z, K, G)));
    CHECK(!c.find(key_of(X, K, G, 1e-5)));                      // another regularisation
    CHECK(!c.find(key_of(X, G, K)));                            // the same bytes, transposed shape
    CHECK(!c.find(key_of(X, K, G, 1e-6, 1)));                   // another device
    XCacheKey k = key_of(X, K, G);
    k.plan = &c;
    CHECK(!c.find(k));
    k = key_of(X, K, G);
    k.d = 64;
    CHECK(!c.find(k));
    k = key_of(X, K, G);
    k.mode = 1;
    CHECK(!c.find(k));
    k = key_of(X, K, G);
    k.KP = 128;
    CHECK(!c.find(k));
    k = key_of(X, K, G);
    k.route = 1;
    CHECK(!c.find(k));
    const std::vector<double> one = {2.5};                      // a single word: every sample is word 0
    c.insert(entry_of(one, 1, 1, 3));
    CHECK(c.find(key_of(one, 1, 1)));
    long long h = 0, m = 0;
    c.stats(&h, &m);
    CHECK(h == 2 && m == 13);
    return 0;
}

int order_and_capacity() {
    {
        XCache<Entry> c(4);
        const int K = 3, G = 40;
        std::vector<std::vector<double>> Xs;
        for (int i = 0; i < 6; ++i) Xs.push_back(matrix(K, G, 100 + (unsigned)i));
        for (int i = 0; i < 4; ++i) c.insert(entry_of(Xs[(size_t)i], K, G, i));
        CHECK(c.size() == 4 && g_alive == 4);
        CHECK(c.find(key_of(Xs[0], K, G)));                     // 0 is the most recently used now: 1 is the oldest
        c.insert(entry_of(Xs[4], K, G, 4));
        CHECK(c.size() == 4 && g_alive == 4);
        CHECK(!c.find(key_of(Xs[1], K, G)));
        CHECK(c.find(key_of(Xs[0], K, G)) && c.find(key_of(Xs[2], K, G)) && c.find(key_of(Xs[3], K, G)) && c.find(key_of(Xs[4], K, G)));
        // the later insert of an equal key wins, and does not count against the capacity
        c.insert(entry_of(Xs[2], K, G, 22));
        CHECK(c.size() == 4 && g_alive == 4);
        auto e = c.find(key_of(Xs[2], K, G));
        CHECK(e && e->tag == 22);
        e.reset();
        // the capacity is per device: four more on device 1 evict nothing of device 0, a fifth the oldest of device 1
        for (int i = 0; i < 4; ++i) c.insert(entry_of(Xs[(size_t)i], K, G, 10 + i, 1e-6, 1));
        CHECK(c.size() == 8);
        c.insert(entry_of(Xs[4], K, G, 14, 1e-6, 1));
        CHECK(c.size() == 8 && !c.find(key_of(Xs[0], K, G, 1e-6, 1)) && c.find(key_of(Xs[0], K, G)));
        // an owner outside the cache keeps an entry alive through eviction and clear
        auto held = c.find(key_of(Xs[3], K, G));
        CHECK(held);
        c.clear();
        CHECK(c.size() == 0 && g_alive == 1 && held->X == Xs[3] && held->key.X == held->X.data());
        CHECK(!c.find(key_of(Xs[3], K, G)));
        held.reset();
        CHECK(g_alive == 0);
        c.insert(entry_of(Xs[5], K, G, 5));
    }
    CHECK(g_alive == 0);                                        // the cache's own destructor releases what is left
    XCache<Entry> none(0);
    none.insert(entry_of(matrix(2, 2, 9), 2, 2, 0));
    CHECK(none.size() == 0 && g_alive == 0);
    return 0;
}

// four threads, two matrices, lookups and inserts interleaved: every hit is the right matrix, the capacity holds
int threads() {
    XCache<Entry> c(4);
    const int K = 4, G = 64;
    const std::vector<double> A = matrix(K, G, 7), B = matrix(K, G, 8);
    int bad[4] = {0, 0, 0, 0};
    std::vector<std::thread> th;
    for (int t = 0; t < 4; ++t)
        th.emplace_back([&, t]() {
            for (int it = 0; it < 400; ++it) {
                const std::vector<double>& X = ((t + it) & 1) ? A : B;
                std::vector<double> mine = X;
                auto e = c.find(key_of(mine, K, G));
                if (!e) c.insert(entry_of(mine, K, G, t));
                else if (e->X != X) ++bad[t];
                if (it % 97 == 0) c.clear();
                if (c.size() > 4) ++bad[t];
            }
        });
    for (auto& q : th) q.join();
    CHECK(bad[0] + bad[1] + bad[2] + bad[3] == 0);
    return 0;
}

}  // namespace

int main() {
    const int bad = keys() + order_and_capacity() + threads();
    std::printf(bad ? "FAILED\n" : "x caches: ok under the sanitizers\n");
    return bad ? 1 : 0;
}
