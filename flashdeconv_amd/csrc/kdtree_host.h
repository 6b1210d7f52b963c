// The host restatement of scipy.spatial.cKDTree's build and k-nearest query ORDER (kdtree_host.cpp has the rules): the tree, its
// build, the host queries and the tuning state.  Pure C++17 - no HIP, nothing of fdx_internal.h -, so hosttest/kdtree_host_asan.cpp
// compiles it with plain g++ under the sanitizers.
#pragma once
#include <atomic>
#include <cstdint>
#include <deque>
#include <memory>
#include <mutex>
#include <new>
#include <utility>
#include <vector>

namespace fdx {

struct KdNode {
    long long split_dim = -1;     // -1: leaf
    double split = 0.0;
    long long start = 0, end = 0;
    long long less = -1, greater = -1;
};

// std::vector that leaves new elements uninitialised (the index array is written in full right after its resize - by several
// threads, each touching its own pages first)
template <class T>
struct KdRawAlloc : std::allocator<T> {
    template <class U> struct rebind { using other = KdRawAlloc<U>; };
    template <class U> void construct(U* p) noexcept { ::new ((void*)p) U; }
    template <class U, class... A> void construct(U* p, A&&... a) { ::new ((void*)p) U(std::forward<A>(a)...); }
};

struct KdTree {
    const double* data = nullptr;
    long long n = 0;
    int m = 0;
    long long leafsize = 16;
    std::vector<long long, KdRawAlloc<long long>> indices;
    // all nodes, root first: raw storage that the threads of the build's last pass fill (and touch first) in parallel
    struct Nodes {
        KdNode* p = nullptr;
        size_t n = 0;
        Nodes() = default;
        Nodes(const Nodes&) = delete;
        Nodes& operator=(const Nodes&) = delete;
        ~Nodes() { ::operator delete(p); }
        void raw(size_t count) { ::operator delete(p); p = static_cast<KdNode*>(::operator new(count * sizeof(KdNode))); n = count; }
        size_t size() const { return n; }
        const KdNode& operator[](size_t i) const { return p[i]; }
    } nodes;
    std::vector<double> maxes, mins;   // of the whole data set
    // build only: the node vectors of the subtrees that were built on threads of their own (kd_children), until kd_build_tree
    // lays them out behind one another in `nodes`
    std::mutex seg_mu;
    std::deque<std::vector<KdNode>> segs;
    bool pooled = false;                 // the build may cut its work into tasks of the thread pool (more than one thread to its name)
    std::atomic<bool> failed{false};     // a task ran out of memory
    std::vector<int32_t, KdRawAlloc<int32_t>> lpos, rpos;   // the partition passes' position lists, by index-array position
};

// Tree of the n points at coords (n x dim doubles, dim 1-8; the tree reads them for as long as it lives).  Throws std::bad_alloc.
void kd_build_tree(KdTree& t, const double* coords, int64_t n, int32_t dim);
// The k-nearest queries of `rows` (NULL: every point, in order) on the host's threads: idx_out row j holds the answer for rows[j],
// nearest first, self included, -1 padded; tree_indices_out (may be NULL): the tree's index array.  False: out of memory in the
// query loop (the caller reports it).
bool ckdtree_query_host(const KdTree& t, int32_t kk, const int64_t* rows, int64_t n_rows, int64_t* idx_out, int64_t* tree_indices_out);
// build, then queries (FDX_TRACE_HOST: the time of either); false and throws as the two above
bool ckdtree_knn_impl(const double* coords, int64_t n, int32_t dim, int32_t kk, const int64_t* rows, int64_t n_rows, int64_t* idx_out,
                      int64_t* tree_indices_out);

// Tuning state (fdx_kdtree_set_threads, fdx_kdtree_tune).  Setters: 0 (local_max: negative) puts the default back.
void kd_set_threads(int threads);
void kd_set_team_min(long long points);
void kd_set_local_max(long long points);
// Host threads the restated cKDTree may use (build forks, host queries): the process's budget (host_threads.h), or the share the
// caller set with fdx_kdtree_set_threads (the ranks of one host each build the tree of the replicated coordinates: they share its
// cores), or FDX_KDTREE_THREADS.
unsigned kd_thread_share();
// Members of the pool a build may keep busy: twice the caller's share of the host's CPUs where the hardware has the threads, 32
// at most.  The share is a CPU-TIME quota (host_cpu_budget), a build is a burst of ~10 ms: 32 threads for that long are a fifth
// of what 16 CPUs may spend per scheduler period, and the 32 subtrees of a million points run side by side instead of in two rounds.
int kd_pool_members();
long long kd_team_min();      // points from which a node's passes are cut into tasks of the pool (400000)
long long kd_local_max();     // points up to which a subtree is built on a contiguous copy of its points (65536; 0: never)

}  // namespace fdx
