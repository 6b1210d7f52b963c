// The registry of libfdx's runtime switches (fdx_env.h).  Each selects an alternative, TESTED kernel path or a diagnostic - none
// is a CPU fallback (the reference has no switches).
#include "fdx_env.h"

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>
#include <string>

#include "fdx_internal.h"

namespace fdx {
namespace {

// value: what env() returns - NULL (unset) or a string that lives as long as the process.  Readers load the pointer and never
// touch a string that is being written; a reload publishes a NEW string for a value that changed and keeps the old one.
struct Switch {
    const char* name;
    const char* what;
    std::atomic<const char*> value{nullptr};
};

Switch g_switches[] = {
    {"FDX_TRACE_HOST", "host time between the marked points of a fit / a graph build (stderr)"},
    {"FDX_DEBUG", "one-line reports of the routes taken (leverage route, ELL rebuilds)"},
    {"FDX_NO_LOG_TABLE", "log1p without the per-row table of the 64 small counts (bit-identical: tests)"},
    {"FDX_GRAPH_WCAP", "ELL width bound of a graph build: forces the 'bound too small' rebuild / remedy (tests)"},
    {"FDX_GRAPH_WCAP_RANK", "... on this rank of a shard plan only"},
    {"FDX_NO_TILED", "global-gather sweep instead of the LDS-tiled one"},
    {"FDX_NO_INIT_SWEEP", "first sweep reads a written start vector instead of the constant 1/K"},
    {"FDX_SPLIT_MIN_TILES", "tiles from which a shard sweeps boundary and interior separately"},
    {"FDX_NO_OVERLAP", "sharded loop: one sweep launch per iteration, halo on the compute stream"},
    {"FDX_NO_FUSED", "two-kernel sketch -> H (scatter + contraction) instead of the tile kernel"},
    {"FDX_NO_TILE_WIDE", "no wide tile kernel (K > 32 / d > 704): the two-kernel path takes those shapes"},
    {"FDX_TILE_LOGV", "0: float64 log1p chain for float32 rows in the tile kernel"},
    {"FDX_SKETCH_GATHER", "gather form of the row sketch kernel"},
    {"FDX_GRAPH_SORT", "Morton order by a radix sort instead of by counting"},
    {"FDX_GRAPH_SYNC", "graph build completed inside the call (no deferred counts)"},
    {"FDX_GRAPH_TWO_ELL_KERNELS", "fill_ell + tile_halo as two kernels"},
    {"FDX_NO_FUSED_PACK", "sharded loop: halo_pack_kernel instead of the sweep writing the send staging"},
    {"FDX_LEV_ONE_WG", "leverage scores by the single-workgroup route"},
    {"FDX_KDTREE_HOST_QUERIES", "tie remedy: cKDTree queries on host threads instead of kd_query_kernel"},
    {"FDX_KDTREE_THREADS", "host threads of the restated cKDTree (build forks, host queries)"},
    {"FDX_KDTREE_PAR_DEPTH", "fork depth of the restated cKDTree build"},
    {"FDX_NO_PLAN_CACHE", "sketch plans / tile schedules, leverage scores, the X side and the spatial graph recomputed every fit (bench.py: cold_ms)"},
    {"FDX_NO_SIDE_STREAM", "everything on the caller's stream"},
    {"FDX_CSR_KEEP_CAP", "entries per wave of the fused CSR sketch's keep buffer (tests: rows that overflow it)"},
    {"FDX_EXPR_STRIPE_SEGMENTS", "segments per workgroup of the weighted gene sums and of the gene spatial sums (bit-identical: tests)"},
};
constexpr int kSwitches = sizeof(g_switches) / sizeof(g_switches[0]);
std::once_flag g_once;
std::mutex g_mu;                          // serialises load_all()
std::atomic<bool> g_trace_host{false};   // FDX_TRACE_HOST as load_all() last saw it: a trace point that is off costs this load, not a walk of the registry

const char* lookup(const char* name) {
    for (const Switch& s : g_switches)
        if (std::strcmp(s.name, name) == 0) return s.value.load(std::memory_order_acquire);
    return nullptr;          // not a runtime switch (tests/test_host.py checks the sources against the registry)
}

void load_all() {
    // every value ever published, never destroyed (a library thread may hold a pointer past exit()); it grows only when a value
    // changes between reloads - the tests, and bench.py around its cold fit
    static std::deque<std::string>* const kept = new std::deque<std::string>();
    std::lock_guard<std::mutex> lk(g_mu);
    for (Switch& s : g_switches) {
        const char* v = getenv(s.name);
        const char* cur = s.value.load(std::memory_order_relaxed);
        if (v && cur && std::strcmp(v, cur) == 0) continue;
        if (v) {
            kept->emplace_back(v);
            v = kept->back().c_str();
        }
        s.value.store(v, std::memory_order_release);
    }
    g_trace_host.store(lookup("FDX_TRACE_HOST") != nullptr, std::memory_order_relaxed);
}

}  // namespace

const char* env(const char* name) {
    std::call_once(g_once, load_all);
    return lookup(name);
}

void trace_host(const char* scope, const char* what) {
    std::call_once(g_once, load_all);
    if (!g_trace_host.load(std::memory_order_relaxed)) return;
    thread_local auto t_prev = std::chrono::steady_clock::now();
    const auto t = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[fdx-host] +%7.1f us  %s%s%s\n", std::chrono::duration<double, std::micro>(t - t_prev).count(),
                 scope ? scope : "", scope ? ": " : "", what);
    t_prev = t;
}

void env_reload() {
    std::call_once(g_once, load_all);
    load_all();
}

}  // namespace fdx

extern "C" int fdx_env_reload(void) {
    fdx::env_reload();
    return 0;
}

// name / description of runtime switch i (NULL past the end): lets the tests and the docs list the registry
extern "C" const char* fdx_env_switch(int32_t i, const char** what_out) {
    if (i < 0 || i >= fdx::kSwitches) return nullptr;
    if (what_out) *what_out = fdx::g_switches[i].what;
    return fdx::g_switches[i].name;
}
