// Content-keyed cache of whole spatial graphs: what depends only on the coordinates (graph_cache.cpp, fdx_graph_build_dev).  One
// slide is fitted more than once - a coarse and a fine annotation, several references, several seeds of the sketch - and every such
// fit used to rebuild the graph it had just thrown away.  Sibling of x_cache.h with one difference: the content lives on the
// DEVICE, so the lookup here ends at the scalars (candidates) and the caller compares the coordinates with a kernel, then reports
// hit() or miss().  This header holds the key, the least-recently-used order, the capacity and the reference count that graph
// handles share - no HIP, so that hosttest/graph_cache_asan.cpp runs it under the sanitizers on the CPU.  Internal.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace fdx {

// Holders of one object: the cache's entry is one, every handle handed out is one.  Starts at one (the creator).
struct RefCount {
    std::atomic<int> n{1};
    void retain() { n.fetch_add(1, std::memory_order_relaxed); }
    bool release() { return n.fetch_sub(1, std::memory_order_acq_rel) == 1; }   // true: that was the last holder
};

// What a graph was built from, except the coordinates themselves (n * dim doubles on the device: compared by the caller, as bytes).
// switches: the value of every environment switch that changes what a build produces or which route it takes - tests build one
// coordinate set under different switches and compare the routes; with a key that ignored them they would compare a graph with itself.
struct GraphCacheKey {
    int dev = 0, dim = 0, method = 0, k = 0;
    long long n = 0;
    double radius = 0.0;
    std::string switches;
};

inline bool graph_cache_key_equal(const GraphCacheKey& a, const GraphCacheKey& b) {
    return a.dev == b.dev && a.dim == b.dim && a.method == b.method && a.k == b.k && a.n == b.n &&
           std::memcmp(&a.radius, &b.radius, sizeof(double)) == 0 && a.switches == b.switches;
}

// At most `cap` entries per device, least recently used out, one mutex.  Entry: anything with members `GraphCacheKey key` and
// `long long bytes`.  Entries are shared: one that is evicted (or dropped by clear) while a caller still holds it dies with its
// last owner.
template <class Entry>
class GraphCache {
  public:
    explicit GraphCache(size_t cap) : cap_(cap) {}
    // the entries whose scalars equal k, most recently used first; not counted - the caller compares the contents and reports
    std::vector<std::shared_ptr<Entry>> candidates(const GraphCacheKey& k) const {
        std::vector<std::shared_ptr<Entry>> out;
        std::lock_guard<std::mutex> lk(mu_);
        for (size_t i = v_.size(); i-- > 0;)
            if (graph_cache_key_equal(v_[i]->key, k)) out.push_back(v_[i]);
        return out;
    }
    // e's contents matched: now the most recently used (if it is still here - another thread may have evicted it meanwhile)
    void hit(const std::shared_ptr<Entry>& e) {
        std::lock_guard<std::mutex> lk(mu_);
        ++hits_;
        for (size_t i = 0; i < v_.size(); ++i)
            if (v_[i] == e) {
                v_.erase(v_.begin() + (long)i);
                v_.push_back(e);
                return;
            }
    }
    void miss() {
        std::lock_guard<std::mutex> lk(mu_);
        ++misses_;
    }
    // e becomes the most recently used entry; the oldest of its device leave until it fits.  Two threads that missed on the same
    // coordinates both built and both insert: the copies are equal, the older one ages out.
    void insert(std::shared_ptr<Entry> e) {
        if (!e || cap_ == 0) return;
        std::vector<std::shared_ptr<Entry>> dropped;   // released after the lock: an entry's destructor frees a graph
        {
            std::lock_guard<std::mutex> lk(mu_);
            size_t same_dev = 0;
            for (const auto& q : v_) same_dev += q->key.dev == e->key.dev ? 1 : 0;
            for (size_t i = 0; i < v_.size() && same_dev >= cap_;)
                if (v_[i]->key.dev == e->key.dev) {
                    dropped.push_back(v_[i]);
                    v_.erase(v_.begin() + (long)i);
                    --same_dev;
                } else {
                    ++i;
                }
            v_.push_back(std::move(e));
        }
    }
    void clear() {
        std::vector<std::shared_ptr<Entry>> dropped;
        {
            std::lock_guard<std::mutex> lk(mu_);
            dropped.swap(v_);
        }
    }
    // out: hits, misses, entries, bytes held by the entries
    void stats(long long out[4]) const {
        std::lock_guard<std::mutex> lk(mu_);
        out[0] = hits_;
        out[1] = misses_;
        out[2] = (long long)v_.size();
        out[3] = 0;
        for (const auto& q : v_) out[3] += q->bytes;
    }

  private:
    const size_t cap_;
    mutable std::mutex mu_;
    std::vector<std::shared_ptr<Entry>> v_;   // least recently used first
    long long hits_ = 0, misses_ = 0;
};

}  // namespace fdx
