// The reference's k-nearest lists where distances tie exactly - scipy.spatial.cKDTree's ORDER, restated: orchestration and entries.
//
// kdtree_host.cpp has the restatement itself (what is restated, the build rules, the query rules) and its host queries,
// kdtree_build_dev.cpp the same build on the device, kdtree_query_dev.cpp the queries on the device.  Here: which of them serves a
// call (ckdtree_lists_device: device build and device queries for 1-3 coordinates; else a host tree, uploaded, and device queries;
// else host queries), the tree whose build was started ahead (fdx_ckdtree_prebuild), and the entries of include/fdx.h.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <memory>
#include <mutex>
#include <system_error>
#include <thread>
#include <vector>

#include "fdx_env.h"
#include "fdx_internal.h"
#include "graph_build.h"
#include "host_threads.h"
#include "kdtree_dev.h"
#include "kdtree_host.h"

namespace fdx {
namespace {

const char* const kQueryLoopOom = "fdx_ckdtree_knn: out of memory in the query loop";

std::atomic<int> g_kd_device_build{1};   // fdx_kdtree_tune(2, 0): the tree of 1-3 coordinates is built on the host even where the device could (kdtree_build_dev.cpp)

// A tree whose build was started ahead (fdx_ckdtree_prebuild): the tie remedy of a fit knows it will need the tree the moment the
// device reports ties, ~4 ms before it gets round to asking for the lists (the device's own lists come first, behind the still
// running sketch) - the 21-24 ms host build runs beside that.  One pending build per process, matched by its coordinates.
struct KdPrebuilt {
    const double* key_host = nullptr;
    const double* key_dev = nullptr;
    long long n = 0;
    int dim = 0;
    PinnedScope pin;                     // coordinates fetched from the device (key_host == NULL)
    KdTree t;
    std::thread th;
    bool failed = false;
    // A build nobody asked the lists of: replaced, or pending when the process ends.  One that is still RUNNING at process exit
    // outlives what it works with - the thread pool (a function-local static, made after g_pre, so destroyed before it) and,
    // with key_host, the caller's coordinates, which this object does not own: the join keeps the exit from std::terminate,
    // it does not make such a build safe.
    ~KdPrebuilt() { if (th.joinable()) th.join(); }
};
std::mutex g_pre_mu;
std::unique_ptr<KdPrebuilt> g_pre;

bool kd_device_build_serves(const double* coords_dev, long long n, int dim) {
    return coords_dev && dim <= 3 && n < 0x3fffffffLL && g_kd_device_build.load() != 0 && !fdx::env("FDX_KDTREE_HOST_QUERIES");
}

// A host-built tree (1-3 coordinates, fewer than 2^31 nodes and points) in the layout of the query kernel: staged in `stage` as
// [meta | split | indices], the three uploads queued on st.  `stage` is the caller's: it has to live until st has consumed the
// copies (kd_queries_device waits for the stream).
int kd_upload_tree(const KdTree& t, KdDeviceTree* dt, PinnedScope* stage, hipStream_t st) {
    const size_t nn = t.nodes.size();
    const long long n = t.n;
    const size_t o_split = nn * sizeof(int4), o_idx = o_split + nn * sizeof(double);
    FDX_TRY(stage->get(o_idx + (((size_t)n * 4 + 15) & ~(size_t)15) + 64));
    char* sp = static_cast<char*>(stage->p);
    int4* meta = reinterpret_cast<int4*>(sp);
    double* split = reinterpret_cast<double*>(sp + o_split);
    int* idx32 = reinterpret_cast<int*>(sp + o_idx);
    auto stage_span = [&](int tid, int n_t) {                         // (1 ms per million points on one thread)
        for (size_t i = nn * (size_t)tid / (size_t)n_t, e = nn * ((size_t)tid + 1) / (size_t)n_t; i < e; ++i) {
            const KdNode& nd = t.nodes[i];
            const bool leaf = nd.split_dim == -1;
            meta[i] = make_int4(leaf ? -1 : (int)nd.split_dim, (int)(leaf ? nd.start : nd.less), (int)(leaf ? nd.end : nd.greater), 0);
            split[i] = nd.split;
        }
        for (long long i = n * tid / n_t, e = n * (tid + 1) / n_t; i < e; ++i) idx32[(size_t)i] = (int)t.indices[(size_t)i];
    };
    if (n >= kd_team_min() && kd_thread_share() > 1) {
        KdPool& pool = KdPool::get();
        pool.want(kd_pool_members());
        std::atomic<bool> stage_failed{false};                       // (nothing in the span allocates)
        pool.parallel(pool.size(), stage_span, &stage_failed);
    } else {
        stage_span(0, 1);
    }
    FDX_TRY(dt->meta.alloc(nn * sizeof(int4)));
    FDX_TRY(dt->split.alloc(nn * sizeof(double)));
    FDX_TRY(dt->idx.alloc((size_t)n * 4));
    FDX_HIP(hipMemcpyAsync(dt->meta.p, meta, nn * sizeof(int4), hipMemcpyHostToDevice, st));
    FDX_HIP(hipMemcpyAsync(dt->split.p, split, nn * sizeof(double), hipMemcpyHostToDevice, st));
    FDX_HIP(hipMemcpyAsync(dt->idx.p, idx32, (size_t)n * 4, hipMemcpyHostToDevice, st));
    dt->n_nodes = (int)nn;
    for (int a = 0; a < t.m; ++a) { dt->mins[a] = t.mins[(size_t)a]; dt->maxes[a] = t.maxes[(size_t)a]; }
    return 0;
}

int ckdtree_prebuild(const double* coords_host, const double* coords_dev, long long n, int dim) {
    if (kd_device_build_serves(coords_dev, n, dim)) return 0;          // the tree is built on the device when the lists are asked for
    {
        std::unique_ptr<KdPrebuilt> old;
        std::lock_guard<std::mutex> lk(g_pre_mu);
        old = std::move(g_pre);
    }                                                                  // (joined, outside the lock)
    auto p = std::make_unique<KdPrebuilt>();
    p->key_host = coords_host; p->key_dev = coords_dev; p->n = n; p->dim = dim;
    const double* src = coords_host;
    if (!src) {
        // on the library's side stream: the caller's stream may still be busy (the sketch of the stopped fit), the coordinates
        // are nobody's output
        hipStream_t ss = library_side_stream();
        const auto tf0 = std::chrono::steady_clock::now();
        FDX_TRY(p->pin.get((size_t)n * dim * sizeof(double)));
        FDX_HIP(hipMemcpyAsync(p->pin.p, coords_dev, (size_t)n * dim * sizeof(double), hipMemcpyDeviceToHost, ss));
        FDX_HIP(hipStreamSynchronize(ss));
        src = static_cast<const double*>(p->pin.p);
        if (fdx::env("FDX_TRACE_HOST"))
            std::fprintf(stderr, "[fdx-host] ckdtree prebuild: coordinates fetched in %.2f ms\n",
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tf0).count());
    }
    KdPrebuilt* raw = p.get();
    try {
        p->th = std::thread([raw, src, n, dim] {
            const auto tb0 = std::chrono::steady_clock::now();
            try { kd_build_tree(raw->t, src, n, dim); } catch (...) { raw->failed = true; }
            if (fdx::env("FDX_TRACE_HOST"))
                std::fprintf(stderr, "[fdx-host] ckdtree prebuild: tree of %lld points built in %.2f ms\n", n,
                             std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb0).count());
        });
    } catch (const std::system_error&) {
        return 0;                        // no thread: the lists call builds the tree itself
    }
    std::lock_guard<std::mutex> lk(g_pre_mu);
    g_pre = std::move(p);
    return 0;
}

}  // namespace

// graph_build.h.  coords_dev: the same (n, dim) float64 array as coords_host.  Queries on the device for 1-3 coordinates
// (FDX_KDTREE_HOST_QUERIES=1 or a deeper far-node heap than the work area holds: on the host's threads, then uploaded).
int ckdtree_lists_device(const double* coords_host_in, const double* coords_dev, long long n, int dim, int kk, const long long* rows_host,
                         long long n_rows, long long* ids_dev, hipStream_t st) {
    const long long nq = rows_host ? n_rows : n;
    if (nq == 0) return 0;
    const bool trace = fdx::env("FDX_TRACE_HOST") != nullptr;
    if (kd_device_build_serves(coords_dev, n, dim)) {
        // tree AND queries on the device (kdtree_build_dev.cpp); a selection that would leave introselect's partition loop, or a
        // tree deeper than the level cap, sends the call down the host build below
        const auto t0 = std::chrono::steady_clock::now();
        KdDeviceTree dt;
        FDX_TRY(kd_build_device(coords_dev, n, dim, &dt, st));
        const auto t1 = std::chrono::steady_clock::now();
        if (!dt.overflow) {
            int over = 0;
            FDX_TRY(kd_queries_device(coords_dev, dim, kk, dt, rows_host, nq, ids_dev, &over, st));
            if (trace)
                std::fprintf(stderr, "[fdx-host] ckdtree: tree built on the device in %.2f ms (%d nodes, %d levels), %lld queries %.2f ms%s\n",
                             std::chrono::duration<double, std::milli>(t1 - t0).count(), dt.n_nodes, dt.levels, nq,
                             std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count(),
                             over ? " (far-node heap too deep: repeated on the host)" : "");
            if (!over) return 0;
        } else if (trace) {
            std::fprintf(stderr, "[fdx-host] ckdtree: the device build gave up (selection depth / level cap): host build\n");
        }
    }
    std::unique_ptr<KdPrebuilt> pre;
    {
        std::lock_guard<std::mutex> lk(g_pre_mu);
        if (g_pre && g_pre->key_host == coords_host_in && g_pre->key_dev == coords_dev && g_pre->n == n && g_pre->dim == dim) pre = std::move(g_pre);
    }
    const auto tj0 = std::chrono::steady_clock::now();
    if (pre) {
        pre->th.join();
        if (pre->failed) pre.reset();
    }
    const double join_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tj0).count();
    // coords_host NULL: the coordinates are fetched here, into pinned memory
    PinnedScope pin_coords;
    const double* coords_host = coords_host_in;
    if (pre && !coords_host) coords_host = static_cast<const double*>(pre->pin.p);
    if (!coords_host) {
        FDX_TRY(pin_coords.get((size_t)n * dim * sizeof(double)));
        FDX_HIP(hipMemcpyAsync(pin_coords.p, coords_dev, (size_t)n * dim * sizeof(double), hipMemcpyDeviceToHost, st));
        FDX_HIP(hipStreamSynchronize(st));
        coords_host = static_cast<const double*>(pin_coords.p);
    }
    const auto t0 = std::chrono::steady_clock::now();
    KdTree t_own;
    if (!pre) kd_build_tree(t_own, coords_host, n, dim);
    KdTree& t = pre ? pre->t : t_own;
    const auto t1 = std::chrono::steady_clock::now();
    const bool on_device = dim <= 3 && n < 0x7fffff00LL && (long long)t.nodes.size() < 0x7fffff00LL && !fdx::env("FDX_KDTREE_HOST_QUERIES");
    if (on_device) {
        PinnedScope stage;                                            // (released after kd_queries_device has waited for the stream)
        KdDeviceTree dt;
        FDX_TRY(kd_upload_tree(t, &dt, &stage, st));
        const auto ts1 = std::chrono::steady_clock::now();
        int over = 0;
        FDX_TRY(kd_queries_device(coords_dev, dim, kk, dt, rows_host, nq, ids_dev, &over, st));
        if (trace)
            std::fprintf(stderr, "[fdx-host] ckdtree: waited %.1f ms for the tree, build here %.1f ms (%lld nodes), staging + uploads queued %.2f ms, %lld queries on the device %.2f ms%s\n",
                         join_ms, std::chrono::duration<double, std::milli>(t1 - t0).count(), (long long)dt.n_nodes,
                         std::chrono::duration<double, std::milli>(ts1 - t1).count(), nq,
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ts1).count(),
                         over ? " (far-node heap too deep: repeated on the host)" : "");
        if (!over) return 0;
    }
    std::vector<int64_t> ids((size_t)nq * kk);
    if (!ckdtree_query_host(t, kk, (const int64_t*)rows_host, nq, ids.data(), nullptr)) return fail(FDX_ERR_INVALID, kQueryLoopOom);
    FDX_HIP(hipMemcpyAsync(ids_dev, ids.data(), ids.size() * 8, hipMemcpyHostToDevice, st));
    FDX_HIP(hipStreamSynchronize(st));
    return 0;
}

}  // namespace fdx

// include/fdx.h
extern "C" int fdx_ckdtree_prebuild(const double* coords_host, const double* coords_dev, int64_t n, int32_t dim) {
    using namespace fdx;
    FDX_REQUIRE((coords_host || coords_dev) && n >= 1 && dim >= 1 && dim <= 8, "fdx_ckdtree_prebuild: bad arguments (1 to 8 coordinates)");
    try {
        return ckdtree_prebuild(coords_host, coords_dev, n, dim);
    } catch (...) {
        return fail(FDX_ERR_INVALID, "fdx_ckdtree_prebuild: out of memory");
    }
}

extern "C" int fdx_kdtree_set_threads(int32_t threads) {
    fdx::kd_set_threads(threads);
    return 0;
}

extern "C" int fdx_kdtree_tune(int32_t what, int64_t points) {
    FDX_REQUIRE(what >= 0 && what <= 2, "fdx_kdtree_tune: what is 0 (team_min), 1 (local_max) or 2 (device build)");
    if (what == 0) fdx::kd_set_team_min(points);
    else if (what == 1) fdx::kd_set_local_max(points);
    else fdx::g_kd_device_build.store(points != 0 ? 1 : 0);
    return 0;
}

extern "C" int fdx_ckdtree_indices_dev(const double* coords_dev, int64_t n, int32_t dim, int64_t* indices_out, int32_t* info_out, void* stream) {
    using namespace fdx;
    FDX_REQUIRE(coords_dev && indices_out && n >= 1 && dim >= 1 && dim <= 3, "fdx_ckdtree_indices_dev: bad arguments (1 to 3 coordinates)");
    hipStream_t st = (hipStream_t)stream;
    PoolStream pool_stream(st);
    KdDeviceTree dt;
    FDX_TRY(kd_build_device(coords_dev, n, dim, &dt, st));
    std::vector<int> h((size_t)n);
    FDX_HIP(hipMemcpyAsync(h.data(), dt.idx.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
    FDX_HIP(hipStreamSynchronize(st));
    for (int64_t i = 0; i < n; ++i) indices_out[i] = h[(size_t)i];
    if (info_out) { info_out[0] = dt.n_nodes; info_out[1] = dt.levels; info_out[2] = dt.overflow ? 1 : 0; }
    return 0;
}

extern "C" int fdx_ckdtree_knn(const double* coords, int64_t n, int32_t dim, int32_t kk, int64_t* idx_out, int64_t* tree_indices_out) {
    using namespace fdx;
    FDX_REQUIRE(coords && idx_out && n >= 1 && dim >= 1 && dim <= 8 && kk >= 1, "fdx_ckdtree_knn: bad arguments (1 to 8 coordinates)");
    try {
        return ckdtree_knn_impl(coords, n, dim, kk, nullptr, 0, idx_out, tree_indices_out) ? 0 : fail(FDX_ERR_INVALID, kQueryLoopOom);
    } catch (...) {
        return fail(FDX_ERR_INVALID, "fdx_ckdtree_knn: out of memory");
    }
}

extern "C" int fdx_ckdtree_knn_rows(const double* coords, int64_t n, int32_t dim, int32_t kk, const int64_t* rows, int64_t n_rows,
                                    int64_t* idx_out) {
    using namespace fdx;
    FDX_REQUIRE(coords && n >= 1 && dim >= 1 && dim <= 8 && kk >= 1 && n_rows >= 0 && (n_rows == 0 || (rows && idx_out)),
                "fdx_ckdtree_knn_rows: bad arguments (1 to 8 coordinates)");
    for (int64_t j = 0; j < n_rows; ++j) FDX_REQUIRE(rows[j] >= 0 && rows[j] < n, "fdx_ckdtree_knn_rows: row index out of range");
    if (n_rows == 0) return 0;
    try {
        return ckdtree_knn_impl(coords, n, dim, kk, rows, n_rows, idx_out, nullptr) ? 0 : fail(FDX_ERR_INVALID, kQueryLoopOom);
    } catch (...) {
        return fail(FDX_ERR_INVALID, "fdx_ckdtree_knn_rows: out of memory");
    }
}
