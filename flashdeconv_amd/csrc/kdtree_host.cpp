// Which of several EXACTLY equidistant points does the reference's k-nearest-neighbour query return?
//
// flashdeconv/utils/graph.py:60-63 builds `cKDTree(coords)` and calls `tree.query(coords, k = k + 1)`; on a regular lattice
// (Visium-HD bins: four neighbours at distance 1, four at sqrt 2, k = 6) the k-th neighbour is one of several at the same
// distance, and which ones come back is decided by nothing but the order in which scipy's tree visits the points.  The
// device build (graph_knn.cpp) breaks such ties by spot index; with knn_ties="ckdtree" the Python driver asks the entries of
// kdtree_order.cpp instead whenever fdx_graph_knn_ties() reports ties, and gets the reference's neighbour lists index for index.
//
// This is a host restatement of the published algorithm of scipy.spatial.cKDTree (third-party dependency of the reference,
// scipy >= 1.7 per its pyproject; checked here against scipy 1.15.3, the version of the build container) for exactly that
// call: tree construction with the constructor's defaults (leafsize 16, compact_nodes, balanced_tree) and the k-nearest
// query with p = 2, eps = 0, no distance bound.  What has to be reproduced is ORDER, so the restatement keeps every
// order-defining detail:
//   build   - recursive; bounds of a node recomputed from its points; split dimension = largest spread (first wins);
//             median by std::nth_element over the node's index range, compared by the coordinate alone, at
//             position n/2; split value = coordinate of that element; then a Hoare-style pass moving "< split" left and
//             ">= split" right (on a lattice many points equal the split: they all go right); when nothing is below the
//             split (the median is the node's minimum) the split moves to nextafter(minimum, +inf) and the pass is repeated;
//             children [start, p) and [p, end).  The index array after all of this is the order
//             in which a leaf's points are tested.  (std::nth_element is libstdc++'s introselect here as in scipy's
//             manylinux wheels.)
//   query   - best-first over nodes with scipy's own binary heap (strict comparisons: ties keep insertion structure),
//             near child followed directly, far child pushed when its distance <= the current k-th distance; a leaf's
//             points are tested in index-array order and accepted when d < bound (strict), the bound being the k-th
//             distance once k neighbours are known - so among equidistant candidates the ones met FIRST stay.
//             Squared distances accumulated coordinate by coordinate from zero, side distances updated incrementally
//             (min_distance += new - old) exactly as the library does, because equality decides here.
// tests/test_host.py compares fdx_ckdtree_knn with scipy itself (index arrays of the tree and query results) on lattices,
// duplicated points, random clouds in 1-3 dimensions - no GPU involved; hosttest/kdtree_host_asan.cpp runs this file and
// host_threads.cpp under the sanitizers.
//
// The build in parallel.  par_depth > 0: the `less` subtree of a large node is built as a task of the thread pool (host_threads.h)
// into a node vector of its own, which joins the tree's list of segments; the parent's link to it is the segment's tag until kd_build_tree lays all segments out in one
// vector (appending every subtree to its parent's vector on the way up copied the nodes once per level: 2 of 12 ms per million
// points).  The index array is partitioned in place - disjoint ranges; the NUMBERING of the nodes differs from a serial build,
// which nothing reads: queries follow the less / greater links.  The serial build was 130 of the 145 ms the tie remedy spent on
// the host for a million lattice points: its top levels are cache-missing passes over all points.
#include "kdtree_host.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "fdx_env.h"
#include "host_threads.h"

namespace fdx {

static std::atomic<int> g_kd_threads{0};
static std::atomic<long long> g_kd_team_min{0};
static std::atomic<long long> g_kd_local_max{-1};
void kd_set_threads(int threads) { g_kd_threads.store(threads > 0 ? threads : 0); }
void kd_set_team_min(long long points) { g_kd_team_min.store(points > 0 ? std::max<long long>(points, 64) : 0); }
void kd_set_local_max(long long points) { g_kd_local_max.store(points); }
unsigned kd_thread_share() {
    if (const char* e = fdx::env("FDX_KDTREE_THREADS")) return (unsigned)std::max(1, atoi(e));
    const int v = g_kd_threads.load();
    return v > 0 ? (unsigned)v : host_cpu_budget();
}
int kd_pool_members() {
    const unsigned share = kd_thread_share();
    if (share <= 1) return 1;
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    return (int)std::min(std::min(hw, 2u * share), 32u);
}
long long kd_team_min() {                                            // fdx_kdtree_tune(0, points): the tests send small nodes through the team
    const long long v = g_kd_team_min.load();
    return v > 0 ? v : 400000;                                        // (a million points: the root and its two children; 250000-point nodes do as well on one thread each)
}
long long kd_local_max() {                                           // fdx_kdtree_tune(1, points); 0 switches the copy off
    const long long v = g_kd_local_max.load();
    return v >= 0 ? v : 65536;
}

namespace {

// chunks a pass over `len` of the tree's n points is cut into: the node's share of the pool (the root all members, its children
// half each: the nodes of a level have their passes under way together), at least two, never chunks under 256 points
int kd_pass_chunks(const KdTree& t, long long len) {
    const long long members = KdPool::get().size();
    const long long share = (members * len + t.n - 1) / std::max<long long>(1, t.n);
    return (int)std::max<long long>(1, std::min<long long>(std::min<long long>(members, std::max<long long>(2, share)), len / 256));
}

// libstdc++'s __unguarded_partition(lo, hi, pivot) over the index range [lo, hi), keys read through the index array - by the whole
// team, with the result of the serial scan, swap for swap.  The serial scan stops its left pointer on every key >= pivot and its
// right pointer on every key <= pivot and swaps the two; between the pointers the array is still as it was, so the k-th swap
// is (k-th key >= pivot from the left, k-th key <= pivot from the right), for as long as the former lies left of the latter,
// and the returned cut is where the left pointer stops next: the next such key from the left, or the right partner of the
// last swap (which now holds a key >= pivot), whichever comes first.  (The pivot - moved to lo - 1 by the median step -
// and the median's other two samples guarantee both lists are non-empty inside the range.)
template <class Key>
long long team_unguarded_partition(KdTree& t, long long* idx, long long lo, long long hi, double pv, const Key& key) {
    KdPool& team = KdPool::get();
    const long long len = hi - lo;
    const int nt = kd_pass_chunks(t, len);
    int32_t* lp = t.lpos.data() + lo;                                // (the ranges of two nodes are disjoint: so are their lists)
    int32_t* rp = t.rpos.data() + lo;
    std::vector<long long> cb((size_t)nt + 1), cl((size_t)nt + 1, 0), cr((size_t)nt + 1, 0);
    for (int t = 0; t <= nt; ++t) cb[(size_t)t] = len * t / nt;
    team.parallel(nt, [&](int tid, int) {
        const long long b = cb[(size_t)tid], e = cb[(size_t)tid + 1];
        long long nl = 0, nr = 0;
        for (long long i = b; i < e; ++i) {
            const double v = key(idx[lo + i]);
            lp[b + nl] = (int32_t)i;
            nl += !(v < pv);
            rp[b + nr] = (int32_t)i;
            nr += !(pv < v);
        }
        cl[(size_t)tid + 1] = nl;
        cr[(size_t)tid + 1] = nr;
    }, &t.failed);
    // pl[t]: left-list entries before chunk t; sr[t]: right-list entries (counted from the right) after chunk t
    std::vector<long long> pl((size_t)nt + 1, 0), sr((size_t)nt + 1, 0);
    for (int t = 0; t < nt; ++t) pl[(size_t)t + 1] = pl[(size_t)t] + cl[(size_t)t + 1];
    for (int t = nt - 1; t >= 0; --t) sr[(size_t)t] = sr[(size_t)t + 1] + cr[(size_t)t + 1];
    const long long nL = pl[(size_t)nt], nR = sr[0];
    auto L = [&](long long k) {
        int t = (int)(std::upper_bound(pl.begin(), pl.end(), k) - pl.begin()) - 1;
        return (long long)lp[cb[(size_t)t] + (k - pl[(size_t)t])];
    };
    auto R = [&](long long k) {                                       // chunk t holds the k with sr[t + 1] <= k < sr[t]
        int t = nt - 1;
        while (sr[(size_t)t] <= k) --t;
        return (long long)rp[cb[(size_t)t] + (cr[(size_t)t + 1] - 1 - (k - sr[(size_t)t + 1]))];
    };
    long long a = 0, b = std::min(nL, nR);                            // K = number of k with L(k) < R(k): those come first
    while (a < b) {
        const long long mid = (a + b) / 2;
        if (L(mid) < R(mid)) a = mid + 1; else b = mid;
    }
    const long long K = a;
    if (K > 0)
        team.parallel(nt, [&](int tid, int n_t) {
            const long long k0 = K * tid / n_t, k1 = K * (tid + 1) / n_t;
            if (k0 >= k1) return;
            int tl = (int)(std::upper_bound(pl.begin(), pl.end(), k0) - pl.begin()) - 1;
            long long il = k0 - pl[(size_t)tl];
            int tr = nt - 1;
            while (sr[(size_t)tr] <= k0) --tr;
            long long ir = cr[(size_t)tr + 1] - 1 - (k0 - sr[(size_t)tr + 1]);
            for (long long k = k0; k < k1; ++k) {
                while (il >= cl[(size_t)tl + 1]) { ++tl; il = 0; }
                while (ir < 0) { --tr; ir = cr[(size_t)tr + 1] - 1; }
                std::swap(idx[lo + lp[cb[(size_t)tl] + il]], idx[lo + rp[cb[(size_t)tr] + ir]]);
                ++il;
                --ir;
            }
        }, &t.failed);
    long long cut = -1;
    if (K < nL) cut = L(K);
    if (K > 0) { const long long r = R(K - 1); cut = cut < 0 ? r : std::min(cut, r); }
    return lo + cut;
}

// std::nth_element(idx + first, idx + nth, idx + last, key(a) < key(b)) - libstdc++'s introselect with the partition passes of the
// long ranges done by the team; below `team_min` libstdc++'s own routine continues with the depth budget that is left.
template <class Key>
void team_nth_element(KdTree& t, long long* idx, long long first, long long nth, long long last, const Key& key, long long team_min) {
    auto cmp = [&key](long long a, long long b) { return key(a) < key(b); };
    auto icmp = __gnu_cxx::__ops::__iter_comp_iter(cmp);
    if (first == last || nth == last) return;
    long long depth = 2 * (long long)std::__lg(last - first);
    while (last - first > 3) {
        if (last - first < team_min || depth == 0) {
            std::__introselect(idx + first, idx + nth, idx + last, depth, icmp);
            return;
        }
        --depth;
        const long long mid = first + (last - first) / 2;
        std::__move_median_to_first(idx + first, idx + first + 1, idx + mid, idx + last - 1, icmp);
        const long long cut = team_unguarded_partition(t, idx, first + 1, last, key(idx[first]), key);
        if (cut <= nth) first = cut; else last = cut;
    }
    std::__insertion_sort(idx + first, idx + last, icmp);
}

constexpr long long kKdForkMin = 32768;   // points from which a node's `less` child becomes a task of the pool

// The two children of a node, the `less` one as a task of the pool when the node is large and forks are left (see the note at
// the head of the file): build(nodes, lesser) appends the subtree of that child to `nodes` and returns its root's index there.  The parent
// builds the other child, then runs pool tasks until its own has finished (its stack holds what the task works on).
inline long long kd_seg_tag(long long seg) { return -(2 + seg); }     // a link to the root (node 0) of segment `seg`
template <class Build>
void kd_children(KdTree& t, std::vector<KdNode>& nodes, bool fork, const Build& build, long long& less, long long& greater) {
    if (fork && t.pooled) {
        std::vector<KdNode>* sub = nullptr;
        long long seg = -1;
        {
            std::lock_guard<std::mutex> lk(t.seg_mu);
            t.segs.emplace_back();                                    // (a deque: the element stays where it is)
            sub = &t.segs.back();
            seg = (long long)t.segs.size() - 1;
        }
        std::atomic<int> pending{0};
        KdPool& pool = KdPool::get();
        pool.spawn([&build, &t, sub] { try { (void)build(*sub, true); } catch (...) { t.failed.store(true); } }, &pending);   // (its root is node 0 of `sub`)
        less = kd_seg_tag(seg);
        try {
            greater = build(nodes, false);
        } catch (...) {
            pool.wait_help(pending);
            throw;
        }
        pool.wait_help(pending);
        return;
    }
    less = build(nodes, true);
    greater = build(nodes, false);
}

// A subtree small enough for a core's cache is built on a contiguous copy of its points - records {coordinates, index} in
// index-array order - instead of through the index array: the same comparisons, hence the same swaps on the same positions and
// the same index order when the records' indices are written back, but bounds, selection and partition stream through 24-byte
// records that sit in L2 instead of chasing 8-byte indices into the coordinate array (the build is throughput-bound once its
// subtrees have threads of their own: ~150 ms of core time per million points, 16 levels of three passes).
template <int M>
struct KdRec {
    double c[M];
    long long i;
};

// std::nth_element(r, r + nth, r + last, key d ascending) with the partition passes of libstdc++'s introselect done WITHOUT the
// data-dependent branches of its two-pointer scan (half of them mispredicted on a median pivot - the larger part of a
// subtree's build time): one pass lists the positions with key >= pivot and the positions with key <= pivot - the stops of the
// scan's left and right pointer -, the k-th swap is (k-th of the first list, k-th from the end of the second) while the former
// lies left of the latter, the cut is where the left pointer would stop next (team_unguarded_partition above has the argument).
// Short ranges go to libstdc++'s own routine with the depth budget that is left.
template <int M>
void rec_nth_element(KdRec<M>* r, long long nth, long long last, int d, int32_t* scratch) {
    auto cmp = [d](const KdRec<M>& a, const KdRec<M>& b) { return a.c[d] < b.c[d]; };
    auto icmp = __gnu_cxx::__ops::__iter_comp_iter(cmp);
    long long first = 0;
    if (first == last || nth == last) return;
    long long depth = 2 * (long long)std::__lg(last - first);
    while (last - first > 3) {
        if (last - first < 192 || depth == 0) {
            std::__introselect(r + first, r + nth, r + last, depth, icmp);
            return;
        }
        --depth;
        const long long mid = first + (last - first) / 2;
        std::__move_median_to_first(r + first, r + first + 1, r + mid, r + last - 1, icmp);
        const double pv = r[first].c[d];
        const long long lo = first + 1, len = last - lo;
        int32_t* lp = scratch;
        int32_t* rp = scratch + len;
        long long nl = 0, nr = 0;
        for (long long i = 0; i < len; ++i) {
            const double v = r[lo + i].c[d];
            lp[nl] = (int32_t)i;
            nl += !(v < pv);
            rp[nr] = (int32_t)i;
            nr += !(pv < v);
        }
        long long a = 0, b = std::min(nl, nr);
        while (a < b) {
            const long long m2 = (a + b) / 2;
            if (lp[m2] < rp[nr - 1 - m2]) a = m2 + 1; else b = m2;
        }
        const long long K = a;
        for (long long k = 0; k < K; ++k) std::swap(r[lo + lp[k]], r[lo + rp[nr - 1 - k]]);
        long long cut = K < nl ? lp[K] : len;
        if (K > 0) cut = std::min<long long>(cut, rp[nr - K]);
        cut += lo;
        if (cut <= nth) first = cut; else last = cut;
    }
    std::__insertion_sort(r + first, r + last, icmp);
}

template <int M>
long long kd_build_local(KdTree& t, std::vector<KdNode>& nodes, KdRec<M>* rec, long long base, long long start, long long end,
                         int32_t* scratch, int par_depth) {
    nodes.emplace_back();
    const long long node_index = (long long)nodes.size() - 1;
    nodes[(size_t)node_index].start = start;
    nodes[(size_t)node_index].end = end;
    const long long n = end - start;
    if (n <= t.leafsize) return node_index;
    KdRec<M>* r = rec + (start - base);
    double mx[M], mn[M];
    for (int i = 0; i < M; ++i) mx[i] = mn[i] = r[0].c[i];
    for (long long j = 1; j < n; ++j)
        for (int i = 0; i < M; ++i) {
            const double v = r[j].c[i];
            mx[i] = mx[i] > v ? mx[i] : v;
            mn[i] = mn[i] < v ? mn[i] : v;
        }
    int d = 0;
    double size = 0.0;
    for (int i = 0; i < M; ++i)
        if (mx[i] - mn[i] > size) { d = i; size = mx[i] - mn[i]; }
    if (mx[d] == mn[d]) return node_index;
    const long long half = n / 2;
    rec_nth_element<M>(r, half, n, d, scratch);
    double split = r[half].c[d];
    long long p = 0, q = half - 1;                                    // (see kd_build for the pass and its shortcut)
    while (p <= q) {
        if (r[p].c[d] < split) ++p;
        else if (r[q].c[d] >= split) --q;
        else { std::swap(r[p], r[q]); ++p; --q; }
    }
    if (p == 0) {
        split = std::nextafter(split, HUGE_VAL);
        q = n - 1;
        while (p <= q) {
            if (r[p].c[d] < split) ++p;
            else if (r[q].c[d] >= split) --q;
            else { std::swap(r[p], r[q]); ++p; --q; }
        }
    }
    long long less = -1, greater = -1;
    const bool fork = par_depth > 0 && n > kKdForkMin;
    kd_children(t, nodes, fork, [&](std::vector<KdNode>& into, bool lesser) {
        if (!lesser) return kd_build_local<M>(t, into, rec, base, start + p, end, scratch, par_depth - 1);
        if (!fork) return kd_build_local<M>(t, into, rec, base, start, start + p, scratch, par_depth - 1);
        std::vector<int32_t, KdRawAlloc<int32_t>> own((size_t)(2 * p));   // on another thread: list scratch of its own
        return kd_build_local<M>(t, into, rec, base, start, start + p, own.data(), par_depth - 1);
    }, less, greater);
    KdNode& nd = nodes[(size_t)node_index];
    nd.split_dim = d;
    nd.split = split;
    nd.less = less;
    nd.greater = greater;
    return node_index;
}

template <int M>
long long kd_build_on_copy(KdTree& t, std::vector<KdNode>& nodes, long long start, long long end, int par_depth) {
    const long long n = end - start;
    std::vector<KdRec<M>, KdRawAlloc<KdRec<M>>> rec((size_t)n);
    long long* indices = t.indices.data();
    for (long long j = 0; j < n; ++j) {
        const long long i = indices[start + j];
        for (int c = 0; c < M; ++c) rec[(size_t)j].c[c] = t.data[i * M + c];
        rec[(size_t)j].i = i;
    }
    std::vector<int32_t, KdRawAlloc<int32_t>> scratch((size_t)(2 * n));
    const long long root = kd_build_local<M>(t, nodes, rec.data(), start, start, end, scratch.data(), par_depth);
    for (long long j = 0; j < n; ++j) indices[start + j] = rec[(size_t)j].i;
    return root;
}

long long kd_build(KdTree& t, std::vector<KdNode>& nodes, long long start, long long end, double* maxes, double* mins, int par_depth,
                   int level) {
    const int m = t.m;
    if (end - start > t.leafsize && end - start <= kd_local_max()) {
        if (m == 1) return kd_build_on_copy<1>(t, nodes, start, end, par_depth);
        if (m == 2) return kd_build_on_copy<2>(t, nodes, start, end, par_depth);
        if (m == 3) return kd_build_on_copy<3>(t, nodes, start, end, par_depth);
    }
    const double* data = t.data;
    long long* indices = t.indices.data();
    nodes.emplace_back();
    const long long node_index = (long long)nodes.size() - 1;
    nodes[(size_t)node_index].start = start;
    nodes[(size_t)node_index].end = end;
    if (end - start <= t.leafsize) return node_index;                 // leaf
    // compact nodes: bounds from the node's own points
    // the large nodes' passes are cut into tasks of the pool (KdPool, host_threads.h): same bounds, same permutation
    const bool teamed = end - start >= kd_team_min() && end - start < 0x7fffffffLL && t.pooled && m <= 8;   // (32-bit positions in the lists)
    KdPool& team = KdPool::get();
    if (teamed) {
        const int nt = kd_pass_chunks(t, end - start);
        std::vector<double> bmx((size_t)nt * 8), bmn((size_t)nt * 8);
        team.parallel(nt, [&](int tid, int n_t) {
            const long long b = start + (end - start) * tid / n_t, e = start + (end - start) * (tid + 1) / n_t;
            double mx[8], mn[8];
            for (int i = 0; i < m; ++i) mx[i] = mn[i] = data[indices[b] * m + i];
            for (long long j = b + 1; j < e; ++j)
                for (int i = 0; i < m; ++i) {
                    const double v = data[indices[j] * m + i];
                    mx[i] = mx[i] > v ? mx[i] : v;
                    mn[i] = mn[i] < v ? mn[i] : v;
                }
            for (int i = 0; i < m; ++i) { bmx[(size_t)tid * 8 + i] = mx[i]; bmn[(size_t)tid * 8 + i] = mn[i]; }
        }, &t.failed);
        for (int i = 0; i < m; ++i) {
            maxes[i] = bmx[(size_t)i];
            mins[i] = bmn[(size_t)i];
            for (int t2 = 1; t2 < nt; ++t2) {
                const double a = bmx[(size_t)t2 * 8 + i], b2 = bmn[(size_t)t2 * 8 + i];
                maxes[i] = maxes[i] > a ? maxes[i] : a;
                mins[i] = mins[i] < b2 ? mins[i] : b2;
            }
        }
    } else {
        for (int i = 0; i < m; ++i) maxes[i] = mins[i] = data[indices[start] * m + i];
        for (long long j = start + 1; j < end; ++j)
            for (int i = 0; i < m; ++i) {
                const double v = data[indices[j] * m + i];
                maxes[i] = maxes[i] > v ? maxes[i] : v;
                mins[i] = mins[i] < v ? mins[i] : v;
            }
    }
    int d = 0;
    double size = 0.0;
    for (int i = 0; i < m; ++i)
        if (maxes[i] - mins[i] > size) { d = i; size = maxes[i] - mins[i]; }
    if (maxes[d] == mins[d]) return node_index;                       // all points identical: leaf
    // median split (balanced tree)
    const long long half = (end - start) / 2;
    // (Selection and partition on contiguous (coordinate, index) pairs instead of through the index array - the same comparison
    // results, hence the same permutation - was tried for the large nodes: no faster, 23 vs 21 ms per million points.)
    // the comparator of scipy 1.15.3 is the coordinate alone (no index tie-break: checked against the library's index array
    // on lattices - with one the leaves come out in another order), so equal coordinates fall where introselect leaves them
    auto cmp = [data, m, d](long long a, long long b) { return data[a * m + d] < data[b * m + d]; };
    auto key = [data, m, d](long long a) { return data[a * m + d]; };
    if (teamed) team_nth_element(t, indices, start, start + half, end, key, std::max<long long>(kd_team_min() / 4, 16));
    else std::nth_element(indices + start, indices + start + half, indices + end, cmp);
    double split = data[indices[start + half] * m + d];
    // scipy's two-pointer pass "< split | >= split" over the whole range.  After the selection everything from position `half` on
    // is >= split (std::nth_element's postcondition): the pass would walk q down through that half without a swap - it starts
    // where that walk ends.  Same swaps, same result, half the pass.
    long long p = start, q = start + half - 1;
    if (teamed) {
        // the same pass in tasks: its k-th swap is (k-th key >= split from the left, k-th key < split from the right) while the
        // former lies left of the latter, and it ends with p on the first key >= split - the number of keys below the split.
        // After a selection only keys EQUAL to the split stand left of position `half`, so the left list is short: the
        // team counts and lists, one thread pairs.
        const int nt = kd_pass_chunks(t, half);
        std::vector<std::vector<long long>> lefts((size_t)nt);
        std::vector<long long> below((size_t)nt, 0);
        team.parallel(nt, [&](int tid, int n_t) {
            const long long b = start + half * tid / n_t, e = start + half * (tid + 1) / n_t;
            long long nb = 0;
            for (long long i = b; i < e; ++i) {
                if (data[indices[i] * m + d] < split) ++nb;
                else lefts[(size_t)tid].push_back(i);
            }
            below[(size_t)tid] = nb;
        }, &t.failed);
        long long n_below = 0;
        for (int t2 = 0; t2 < nt; ++t2) n_below += below[(size_t)t2];
        long long r = q;                                              // walks down over the keys < split
        bool crossed = false;
        for (int t2 = 0; t2 < nt && !crossed; ++t2)
            for (long long l : lefts[(size_t)t2]) {
                while (r > l && !(data[indices[r] * m + d] < split)) --r;
                if (r <= l) { crossed = true; break; }
                std::swap(indices[l], indices[r]);
                --r;
            }
        p = start + n_below;
    } else
    while (p <= q) {
        if (data[indices[p] * m + d] < split) ++p;
        else if (data[indices[q] * m + d] >= split) --q;
        else { std::swap(indices[p], indices[q]); ++p; --q; }
    }
    if (p == start) {
        // Nothing below the split: the median IS the node's minimum along d (more than half of its points share it - duplicated
        // spots, or a ragged tissue edge).  scipy 1.15.3 then splits just ABOVE the minimum - the tree reports
        // split == nextafter(minimum, +inf), with every point at the minimum in the lesser child - by the same two-pointer
        // pass over the whole range.  (Rounds 1-5 restated the older "slide one point over" rule here; it never fired on a
        // full lattice, and did on heavily duplicated coordinates - caught by the duplicates sweep of tests/test_host.py.)
        split = std::nextafter(split, HUGE_VAL);
        q = end - 1;
        while (p <= q) {
            if (data[indices[p] * m + d] < split) ++p;
            else if (data[indices[q] * m + d] >= split) --q;
            else { std::swap(indices[p], indices[q]); ++p; --q; }
        }
    }
    long long less = -1, greater = -1;
    kd_children(t, nodes, par_depth > 0 && end - start > kKdForkMin, [&](std::vector<KdNode>& into, bool lesser) {
        if (!lesser) return kd_build(t, into, p, end, maxes, mins, par_depth - 1, level + 1);
        std::vector<double> mx((size_t)m), mn((size_t)m);            // (possibly on another thread: bounds scratch of its own)
        return kd_build(t, into, start, p, mx.data(), mn.data(), par_depth - 1, level + 1);
    }, less, greater);
    KdNode& nd = nodes[(size_t)node_index];                           // (the vector may have moved)
    nd.split_dim = d;
    nd.split = split;
    nd.less = less;
    nd.greater = greater;
    return node_index;
}

// scipy's heap (ckdtree/src/ordered.h): binary min-heap on `priority`, strict comparisons
struct HeapItem {
    double priority;
    long long payload;
};
struct Heap {
    std::vector<HeapItem> h;
    long long n = 0;
    void push(const HeapItem& item) {
        ++n;
        if ((long long)h.size() < n) h.resize((size_t)(2 * h.size() + 1));
        long long i = n - 1;
        h[(size_t)i] = item;
        while (i > 0 && h[(size_t)i].priority < h[(size_t)((i - 1) / 2)].priority) {
            std::swap(h[(size_t)((i - 1) / 2)], h[(size_t)i]);
            i = (i - 1) / 2;
        }
    }
    const HeapItem& peek() const { return h[0]; }
    void remove() {
        h[0] = h[(size_t)(n - 1)];
        --n;
        const long long nn = n;
        long long i = 0, j = 1, k = 2;
        while ((j < nn && h[(size_t)i].priority > h[(size_t)j].priority) || (k < nn && h[(size_t)i].priority > h[(size_t)k].priority)) {
            const long long l = (k < nn && h[(size_t)j].priority > h[(size_t)k].priority) ? k : j;
            std::swap(h[(size_t)l], h[(size_t)i]);
            i = l;
            j = 2 * i + 1;
            k = 2 * i + 2;
        }
    }
    HeapItem pop() {
        const HeapItem it = h[0];
        remove();
        return it;
    }
};

struct NodeInfo {
    long long node;
    double min_distance;
    double side[8];
};

void kd_query_one(const KdTree& t, const double* x, int kmax, int64_t* out_idx, std::vector<NodeInfo>& pool, Heap& q,
                  Heap& neighbors) {
    const int m = t.m;
    pool.clear();
    q.n = 0;
    neighbors.n = 0;
    double upper = HUGE_VAL;
    pool.push_back(NodeInfo{0, 0.0, {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}});
    {
        NodeInfo& r = pool[0];
        for (int i = 0; i < m; ++i) {
            // distance from x to the interval [min, max] of the whole data set, to the power p = 2
            double sd = std::max(0.0, std::max(t.mins[(size_t)i] - x[i], x[i] - t.maxes[(size_t)i]));
            sd = sd * sd;
            r.min_distance += sd - r.side[i];
            r.side[i] = sd;
        }
    }
    long long cur = 0;                                                // index into pool
    for (;;) {
        const KdNode& nd = t.nodes[(size_t)pool[(size_t)cur].node];
        if (nd.split_dim == -1) {
            for (long long i = nd.start; i < nd.end; ++i) {
                const double* y = t.data + t.indices[(size_t)i] * m;
                double d = 0.0;
                for (int a = 0; a < m; ++a) {
                    const double diff = y[a] - x[a];
                    d += diff * diff;
                }
                if (d < upper) {
                    if (neighbors.n == kmax) neighbors.remove();
                    neighbors.push(HeapItem{-d, t.indices[(size_t)i]});
                    if (neighbors.n == kmax) upper = -neighbors.peek().priority;
                }
            }
            if (q.n == 0) break;
            cur = q.pop().payload;
        } else {
            if (pool[(size_t)cur].min_distance > upper) break;         // the nearest remaining cell is too far: done
            pool.push_back(pool[(size_t)cur]);                         // ni2 = copy of ni1 (side distances included)
            long long far = (long long)pool.size() - 1;
            const int sd_dim = (int)nd.split_dim;
            double side_distance;
            if (x[sd_dim] < nd.split) {
                pool[(size_t)cur].node = nd.less;
                pool[(size_t)far].node = nd.greater;
                side_distance = nd.split - x[sd_dim];
            } else {
                pool[(size_t)cur].node = nd.greater;
                pool[(size_t)far].node = nd.less;
                side_distance = x[sd_dim] - nd.split;
            }
            side_distance = side_distance * side_distance;
            NodeInfo& f = pool[(size_t)far];
            f.min_distance += side_distance - f.side[sd_dim];
            f.side[sd_dim] = side_distance;
            if (pool[(size_t)cur].min_distance > pool[(size_t)far].min_distance) std::swap(cur, far);   // ni1 = the closer one
            if (pool[(size_t)far].min_distance <= upper) q.push(HeapItem{pool[(size_t)far].min_distance, far});
        }
    }
    // neighbours, nearest first (heap order decides among equal distances, as in the library)
    const long long nnb = neighbors.n;
    std::vector<HeapItem> sorted((size_t)kmax);
    for (long long i = neighbors.n - 1; i >= 0; --i) sorted[(size_t)i] = neighbors.pop();
    for (int i = 0; i < kmax; ++i) out_idx[i] = i < nnb ? sorted[(size_t)i].payload : -1;
}

}  // namespace

bool ckdtree_knn_impl(const double* coords, int64_t n, int32_t dim, int32_t kk, const int64_t* rows, int64_t n_rows, int64_t* idx_out,
                      int64_t* tree_indices_out) {
    KdTree t;
    const bool trace = fdx::env("FDX_TRACE_HOST") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    kd_build_tree(t, coords, n, dim);
    const auto t1 = std::chrono::steady_clock::now();
    const bool ok = ckdtree_query_host(t, kk, rows, n_rows, idx_out, tree_indices_out);
    if (trace)
        std::fprintf(stderr, "[fdx-host] ckdtree: build %.1f ms (%lld nodes), %lld queries %.1f ms\n",
                     std::chrono::duration<double, std::milli>(t1 - t0).count(), (long long)t.nodes.size(), (long long)(rows ? n_rows : n),
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count());
    return ok;
}

void kd_build_tree(KdTree& t, const double* coords, int64_t n, int32_t dim) {
    t.data = coords;
    t.n = n;
    t.m = dim;
    t.indices.resize((size_t)n);
    t.maxes.assign((size_t)dim, 0.0);
    t.mins.assign((size_t)dim, 0.0);
    // identity index array and the bounds of the whole set: 3 ms of passes per million points when one thread makes them
    auto span = [&](long long b, long long e, double* mx, double* mn) {
        for (int a = 0; a < dim; ++a) mx[a] = mn[a] = coords[b * dim + a];
        for (long long i = b; i < e; ++i) {
            t.indices[(size_t)i] = i;
            for (int a = 0; a < dim; ++a) {
                const double v = coords[i * dim + a];
                mx[a] = std::max(mx[a], v);
                mn[a] = std::min(mn[a], v);
            }
        }
    };
    // the pool's threads are asked for where they can pay: from a few thousand points (the forks start at 32768, the passes'
    // tasks at 200000)
    KdPool& pool = KdPool::get();
    t.pooled = kd_thread_share() > 1 && n >= std::min<long long>(4096, kd_team_min()) && dim <= 8;
    if (t.pooled) pool.want(kd_pool_members());
    if (t.pooled && n >= kd_team_min()) {
        t.lpos.resize((size_t)n);                                     // (uninitialised: first touched by the tasks that fill them)
        t.rpos.resize((size_t)n);
        const int nt = pool.size();
        std::vector<double> bmx((size_t)nt * 8), bmn((size_t)nt * 8);
        pool.parallel(nt, [&](int tid, int n_t) { span(n * tid / n_t, n * (tid + 1) / n_t, &bmx[(size_t)tid * 8], &bmn[(size_t)tid * 8]); }, &t.failed);
        for (int a = 0; a < dim; ++a) {
            t.maxes[(size_t)a] = bmx[(size_t)a];
            t.mins[(size_t)a] = bmn[(size_t)a];
            for (int t2 = 1; t2 < nt; ++t2) {
                t.maxes[(size_t)a] = std::max(t.maxes[(size_t)a], bmx[(size_t)t2 * 8 + a]);
                t.mins[(size_t)a] = std::min(t.mins[(size_t)a], bmn[(size_t)t2 * 8 + a]);
            }
        }
    } else {
        span(0, n, t.maxes.data(), t.mins.data());
    }
    std::vector<double> mx(t.maxes), mn(t.mins);
    // the `less` child of every node above 32768 points becomes a task, five levels deep at most: 32 subtrees for a million points
    int par = t.pooled ? 5 : 0;
    if (const char* e = fdx::env("FDX_KDTREE_PAR_DEPTH")) par = t.pooled ? std::max(0, std::min(10, atoi(e))) : 0;
    std::vector<KdNode> top;
    top.reserve(1024);
    kd_build(t, top, 0, n, mx.data(), mn.data(), par, 0);
    // one vector: the top nodes, then the segments in the order they were handed in; tags become indices
    const size_t ns = t.segs.size();
    std::vector<long long> off(ns + 2, 0);
    off[1] = (long long)top.size();
    for (size_t i = 0; i < ns; ++i) off[i + 2] = off[i + 1] + (long long)t.segs[i].size();
    t.nodes.raw((size_t)off[ns + 1]);
    KdNode* flat = t.nodes.p;
    auto lay = [&](size_t si) {                                       // si = 0: the top nodes, else segment si - 1
        const std::vector<KdNode>& src = si == 0 ? top : t.segs[si - 1];
        const long long o = off[si];
        auto link = [&](long long l) { return l >= 0 ? l + o : l == -1 ? -1 : off[(size_t)(-l - 2) + 1]; };
        for (size_t i = 0; i < src.size(); ++i) {
            KdNode nd = src[i];
            nd.less = link(nd.less);
            nd.greater = link(nd.greater);
            ::new (flat + (size_t)o + i) KdNode(nd);
        }
    };
    if (t.failed.load()) throw std::bad_alloc();
    if (ns > 0 && t.pooled) pool.parallel(pool.size(), [&](int tid, int n_t) { for (size_t si = (size_t)tid; si < ns + 1; si += (size_t)n_t) lay(si); }, &t.failed);
    else for (size_t si = 0; si < ns + 1; ++si) lay(si);
    t.lpos = decltype(t.lpos)();
    t.rpos = decltype(t.rpos)();
    t.segs.clear();
}

bool ckdtree_query_host(const KdTree& t, int32_t kk, const int64_t* rows, int64_t n_rows, int64_t* idx_out, int64_t* tree_indices_out) {
    const double* coords = t.data;
    const long long n = t.n;
    const int dim = t.m;
    if (tree_indices_out) std::memcpy(tree_indices_out, t.indices.data(), (size_t)n * sizeof(int64_t));
    // the queries are independent (the tree is read-only; every thread has its own node pool and heaps): contiguous ranges of a
    // few thousand points and more per host thread.  1000 x 1000 lattice points on 8 cores: 2.2 -> 0.8-1.0 s, of which 0.29 s the
    // serial build (its top levels are full passes over the points - bounds, introselect, partition; building the subtrees below
    // the second level on four threads was tried and returned nothing measurable).
    const long long nq = rows ? n_rows : n;
    auto run = [&](long long i0, long long i1) {
        std::vector<NodeInfo> pool;
        Heap q, nb;
        q.h.resize(12);
        nb.h.resize((size_t)kk);
        for (long long i = i0; i < i1; ++i) {
            const long long p = rows ? rows[i] : i;
            kd_query_one(t, coords + p * dim, kk, idx_out + i * kk, pool, q, nb);
        }
    };
    unsigned nt = kd_thread_share();
    nt = (unsigned)std::min<long long>(std::max(1u, std::min(nt, 128u)), std::max<long long>(1, nq / 4096));
    // a thread that cannot be started (process limits, W ranks x 32 threads) or a failed allocation inside a worker must not end
    // the process: what was started is joined, the rest of the range runs here
    std::vector<std::thread> th;
    std::vector<int> failed(nt, 0);
    const long long per = (nq + nt - 1) / std::max(1u, nt);
    long long next = 0;
    if (nt > 1) {
        for (unsigned k = 0; k < nt; ++k) {
            const long long i0 = (long long)k * per, i1 = std::min<long long>(nq, i0 + per);
            if (i0 >= i1) break;
            try {
                th.emplace_back([&, i0, i1, k] {
                    try { run(i0, i1); } catch (...) { failed[k] = 1; }
                });
            } catch (...) {
                break;                                   // this and the following ranges: serially below
            }
            next = i1;
        }
    }
    bool ok = true;
    try {
        if (next < nq) run(next, nq);
    } catch (...) {
        ok = false;
    }
    for (auto& x : th) x.join();
    for (unsigned k = 0; k < nt; ++k) {
        if (!failed[k]) continue;
        const long long i0 = (long long)k * per, i1 = std::min<long long>(nq, i0 + per);
        try { run(i0, i1); } catch (...) { ok = false; }
    }
    return ok;
}

}  // namespace fdx
