// Content-keyed caches of what depends only on the signature matrix X: the leverage scores (fit.cpp) and the X side of a fit
// (prepare.cpp: X_sketch, XtX).  One study deconvolves many slides against one single-cell reference, so every fit of it passes
// the same X.  This header holds the lookup, the least-recently-used order and the capacity - no HIP, like the schedule builders
// (tile_plan.h), so that hosttest/x_cache_asan.cpp runs it under the sanitizers on the CPU.  Internal.
#pragma once
#include <cstddef>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

namespace fdx {

// What an entry was computed from.  X: K * G doubles that the OWNER of the key keeps alive (an entry: its own copy).  Fields a
// cache does not use stay zero.  No identity by pointer: X is compared by content (`plan` is the identity of a shared SketchPlan,
// which is itself content-keyed and which the entry keeps alive, so the address cannot be recycled under it).
struct XCacheKey {
    int dev = 0, K = 0, KP = 0, G = 0, d = 0, mode = 0, route = 0;
    double reg = 0.0;
    const void* plan = nullptr;
    const double* X = nullptr;
    size_t words() const { return (size_t)K * (size_t)G; }
};

// The cheap part first: the scalars, then a few sampled words of X (two references of one shape differ almost everywhere), then
// the whole matrix - a memcmp, which costs about what the memcpy of X into pinned memory costs that a hit saves.  No hash: a
// byte-serial one over 480 KB would cost 0.5 ms.  Doubles are compared as bytes (a one-ulp change is another matrix, -0.0 is not 0.0).
inline bool x_cache_key_equal(const XCacheKey& a, const XCacheKey& b) {
    if (a.dev != b.dev || a.K != b.K || a.KP != b.KP || a.G != b.G || a.d != b.d || a.mode != b.mode || a.route != b.route ||
        a.plan != b.plan || std::memcmp(&a.reg, &b.reg, sizeof(double)) != 0)
        return false;
    const size_t n = a.words();
    if (n == 0 || !a.X || !b.X) return false;
    constexpr size_t kSamples = 8;
    for (size_t s = 0; s < kSamples; ++s) {
        const size_t i = (n - 1) * s / (kSamples - 1);
        if (std::memcmp(a.X + i, b.X + i, sizeof(double)) != 0) return false;
    }
    return std::memcmp(a.X, b.X, n * sizeof(double)) == 0;
}

// At most `cap` entries per device, least recently used out, one mutex.  Entry: anything with a member `XCacheKey key` whose X
// points into memory the entry owns.  Entries are shared: one that is evicted (or dropped by clear) while a caller still holds it
// dies with its last owner.
template <class Entry>
class XCache {
  public:
    explicit XCache(size_t cap) : cap_(cap) {}
    // the entry of an equal key (now the most recently used), or null; counted as a hit / a miss
    std::shared_ptr<Entry> find(const XCacheKey& k) {
        std::lock_guard<std::mutex> lk(mu_);
        for (size_t i = 0; i < v_.size(); ++i)
            if (x_cache_key_equal(v_[i]->key, k)) {
                std::shared_ptr<Entry> e = v_[i];
                v_.erase(v_.begin() + (long)i);
                v_.push_back(e);
                ++hits_;
                return e;
            }
        ++misses_;
        return nullptr;
    }
    // e becomes the most recently used entry.  Two threads that missed on the same key both computed: the later insert wins.
    void insert(std::shared_ptr<Entry> e) {
        if (!e || cap_ == 0) return;
        std::vector<std::shared_ptr<Entry>> dropped;   // released after the lock: an entry's destructor may take other locks
        {
            std::lock_guard<std::mutex> lk(mu_);
            for (size_t i = 0; i < v_.size(); ++i)
                if (x_cache_key_equal(v_[i]->key, e->key)) {
                    dropped.push_back(v_[i]);
                    v_.erase(v_.begin() + (long)i);
                    break;
                }
            size_t same_dev = 0;
            for (const auto& q : v_) same_dev += q->key.dev == e->key.dev ? 1 : 0;
            for (size_t i = 0; i < v_.size() && same_dev >= cap_;)   // the oldest of this device first
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
    size_t size() const {
        std::lock_guard<std::mutex> lk(mu_);
        return v_.size();
    }
    void stats(long long* hits, long long* misses) const {
        std::lock_guard<std::mutex> lk(mu_);
        *hits = hits_;
        *misses = misses_;
    }

  private:
    const size_t cap_;
    mutable std::mutex mu_;
    std::vector<std::shared_ptr<Entry>> v_;   // least recently used first
    long long hits_ = 0, misses_ = 0;
};

}  // namespace fdx
