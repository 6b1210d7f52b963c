// The cache of whole spatial graphs by content of the coordinates: the device half of graph_cache.h (compare kernel, entries,
// publication) and its C entries.  fdx_graph_build_dev (capi_dev.cpp) looks a build up here before it queues anything else.
#include <algorithm>

#include "fdx_env.h"
#include "fdx_graph.h"
#include "graph_build.h"
#include "graph_cache.h"

namespace fdx {

// What the cache keeps of one build: its own copy of the coordinates (the caller's tensor may be overwritten or freed) and one
// reference on the graph.
struct GraphCacheEntry {
    GraphCacheKey key;
    long long bytes = 0;            // the copy and the graph's arrays, as the pool rounds them
    DevBuf coords;                  // key.n * key.dim doubles
    fdx_graph* g = nullptr;         // set at publication
    ~GraphCacheEntry() { if (g) graph_release(g); }
};

namespace {

// (on the heap, never destroyed: at process exit the pool's statics may be gone before this translation unit's)
GraphCache<GraphCacheEntry>& cache() {
    static GraphCache<GraphCacheEntry>* const c = new GraphCache<GraphCacheEntry>(2);
    return *c;
}

// The caller's coordinates against an entry's copy as 64-bit words - bytes, not values: a one-ulp change is another slide, -0.0 is
// not 0.0.  Every thread that sees a difference stores the same 1 into the (zeroed) word of the pinned block: no atomics.
__global__ __launch_bounds__(256) void coords_differ_kernel(const unsigned long long* __restrict__ a,
                                                            const unsigned long long* __restrict__ b, long long words,
                                                            long long* __restrict__ flag) {
    const long long stride = (long long)gridDim.x * 256;
    bool differ = false;
#pragma unroll 4
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < words; i += stride) differ |= a[i] != b[i];
    if (differ) *flag = 1;
}

long long graph_bytes(const fdx_graph* g) {
    const DevBuf* bufs[] = {&g->ell, &g->slice_off, &g->deg, &g->perm, &g->rank, &g->rows, &g->row_extra, &g->tile_halo,
                            &g->tile_hcnt, &g->ell_local, &g->ties_dev};
    long long b = 0;
    for (const DevBuf* q : bufs) b += (long long)q->cap;
    return b;
}

bool cacheable_graph(const fdx_graph* g, long long n) {   // whole graphs built from coordinates only: no shard, no CSR upload
    return g && g->n == n && g->n_total == n && g->shard_world == 0 && !g->shard_pending && !g->identity_order;
}

}  // namespace

bool graph_cache_enabled() { return fdx::env("FDX_NO_PLAN_CACHE") == nullptr; }

GraphCacheKey graph_cache_key(long long n, int dim, int method, int k, double radius) {
    GraphCacheKey key;
    (void)hipGetDevice(&key.dev);
    key.n = n; key.dim = dim; key.method = method; key.k = k; key.radius = radius;
    for (const char* name : {"FDX_GRAPH_SORT", "FDX_GRAPH_SYNC", "FDX_GRAPH_WCAP", "FDX_GRAPH_WCAP_RANK", "FDX_GRAPH_TWO_ELL_KERNELS",
                             "FDX_NO_TILED"}) {
        const char* v = fdx::env(name);
        key.switches += v ? v : "\x01";   // unset is not the empty string
        key.switches += '\x02';
    }
    return key;
}

// *out: the graph of an entry with these scalars and these coordinates (one more holder), or NULL.  With an entry that matches
// on the scalars the compare kernels are queued, alone, and their flags read after one wait: a hit needs no bounding box, and a
// repeated slide is the case the cache is there for.  A miss behind such an entry (another slide of the same size) builds as a
// build without a candidate does and so pays a second round trip, for its box.  No such entry: nothing is queued.
int graph_cache_lookup(const GraphCacheKey& key, const double* d_coords, hipStream_t st, fdx_graph** out) {
    *out = nullptr;
    std::vector<std::shared_ptr<GraphCacheEntry>> cand = cache().candidates(key);
    if (cand.empty()) {
        cache().miss();
        return 0;
    }
    if (cand.size() > 4) cand.resize(4);             // four flag words
    const long long words = key.n * key.dim;
    const int nblk = (int)std::min<long long>(1024, (words + 255) / 256);
    const std::function<int(long long*)> compare = [&](long long* flags_dev) -> int {
        for (size_t c = 0; c < cand.size(); ++c)
            hipLaunchKernelGGL(coords_differ_kernel, dim3(nblk), dim3(256), 0, st, (const unsigned long long*)d_coords,
                               cand[c]->coords.as<unsigned long long>(), words, flags_dev + c);
        FDX_CHECK_LAUNCH();
        return 0;
    };
    long long flags[4] = {0, 0, 0, 0};
    FDX_TRY(flag_words(st, compare, flags));
    for (size_t c = 0; c < cand.size(); ++c)
        if (flags[c] == 0) {
            cache().hit(cand[c]);
            cand[c]->g->refs.retain();
            *out = cand[c]->g;
            return 0;
        }
    cache().miss();
    return 0;
}

// A build that missed: the entry-to-be with room for its copy of the coordinates.  graph_cache_queue_copy fills it on the build's
// stream; it rides on the graph (cache_pending) until graph_cache_publish.
int graph_cache_entry_new(const GraphCacheKey& key, std::shared_ptr<GraphCacheEntry>* out) {
    auto e = std::make_shared<GraphCacheEntry>();
    e->key = key;
    FDX_TRY(e->coords.alloc((size_t)key.n * (size_t)key.dim * sizeof(double)));
    *out = std::move(e);
    return 0;
}

int graph_cache_queue_copy(GraphCacheEntry* e, const double* d_coords, hipStream_t st) {
    FDX_HIP(hipMemcpyAsync(e->coords.p, d_coords, (size_t)e->key.n * (size_t)e->key.dim * sizeof(double), hipMemcpyDeviceToDevice, st));
    return 0;
}

// The graph is complete - the deferred numbers have arrived (graph_meta_sync), or the build ended synchronously - and so is the
// copy queued ahead of it on the same stream: from here on other holders, on any stream, may take it.  A graph destroyed before it
// was consumed, or whose build failed, never gets here.
void graph_cache_publish(fdx_graph* g) {
    if (!g || !g->cache_pending) return;
    std::shared_ptr<GraphCacheEntry> e = std::move(g->cache_pending);
    g->cache_pending.reset();
    if (!graph_cache_enabled() || !cacheable_graph(g, e->key.n)) return;
    g->refs.retain();
    e->g = g;
    e->bytes = (long long)e->coords.cap + graph_bytes(g);
    cache().insert(std::move(e));
}

void graph_cache_clear() { cache().clear(); }

void graph_release(fdx_graph* g) {
    if (g && g->refs.release()) delete g;
}

}  // namespace fdx

using namespace fdx;

extern "C" {

int fdx_graph_cache_stats(int64_t out[4]) {
    FDX_REQUIRE(out != nullptr, "fdx_graph_cache_stats: null output");
    long long v[4] = {0, 0, 0, 0};
    cache().stats(v);
    for (int i = 0; i < 4; ++i) out[i] = v[i];
    return 0;
}

}  // extern "C"
