// Device-resident fit pipeline: steps 2-6 of FlashDeconv.fit (flashdeconv/core/deconv.py:326-398) behind one C call.
//   graph (utils/graph.py) -> X_sketch, XtX -> Y_sketch chunks -> H, YtY -> lambda (core/spatial.py:144-192)
//   -> BCD solve (core/solver.py:287-428) -> beta / proportions in the caller's spot order (core/solver.py:431-452).
// Everything between "Y, coords resident in HBM" and "beta_, proportions_ resident in HBM" stays on the device; the
// host only sees a handful of scalars (bounding box, XtX, rel_change trace).
#include "fdx_env.h"
#include <algorithm>
#include <cstdio>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <vector>

#include "fdx_graph.h"
#include "fdx_internal.h"
#include "fdx_kernels.h"
#include "graph_build.h"
#include "prepare.h"
#include "sketch_plan.h"
#include "solver.h"
#include "x_cache.h"

using namespace fdx;

namespace {

int build_csc_from_tables(const int32_t* bucket, const double* weight, int G, int d, std::vector<long long>* col_ptr,
                          std::vector<int>* gene_idx, std::vector<double>* w) {
    col_ptr->assign((size_t)d + 1, 0);
    for (int g = 0; g < G; ++g) {
        FDX_REQUIRE(bucket[g] >= 0 && bucket[g] < d, "fit: bucket index out of range");
        (*col_ptr)[(size_t)bucket[g] + 1]++;
    }
    for (int c = 0; c < d; ++c) (*col_ptr)[(size_t)c + 1] += (*col_ptr)[(size_t)c];
    gene_idx->assign((size_t)G, 0);
    w->assign((size_t)G, 0.0);
    std::vector<long long> cur(col_ptr->begin(), col_ptr->end() - 1);
    for (int g = 0; g < G; ++g) {   // ascending gene order inside every bucket
        const long long e = cur[(size_t)bucket[g]]++;
        (*gene_idx)[(size_t)e] = g;
        (*w)[(size_t)e] = weight[g];
    }
    return 0;
}

}  // namespace

// The leverage scores depend on (X, regularization) alone, and a study passes one reference X to every fit: they are kept by
// content (x_cache.h), so that a repeated X costs one comparison instead of an upload, three kernels and the host's wait for them.
// An entry is what the first computation produced, so a hit returns the same bits.  FDX_NO_PLAN_CACHE bypasses the cache.
struct LevEntry {
    XCacheKey key;                  // K, G, reg, route = the route the job starts on (FDX_LEV_ONE_WG changes it); key.X -> X
    // the signatures, in ordinary memory: the missed job's pinned buffer goes back to its pool (kept here, the next job that misses
    // would find that pool one buffer short and allocate a new one); end_keep uploads a hit's device copy from this one
    std::vector<double> X;
    std::vector<double> scores;
    int route = LEV_ROUTE_SVD;      // the route that settled
    int dbg[8] = {0};
};
// (on the heap, never destroyed: at process exit the pool's statics may be gone before this translation unit's)
static XCache<LevEntry>& lev_cache() {
    static XCache<LevEntry>* const c = new XCache<LevEntry>(4);
    return *c;
}
namespace fdx {
void leverage_cache_clear() { lev_cache().clear(); }
void leverage_cache_stats(long long* hits, long long* misses) { lev_cache().stats(hits, misses); }
}  // namespace fdx

// The Jacobi SVD runs in ONE workgroup, so it occupies one CU for ~1.6 ms while the other 255 idle.  begin/end let the
// caller put the spatial-graph build (many short, latency-bound kernels on the caller's stream) under it: the job runs
// on a library-owned non-blocking side stream.
struct fdx_leverage_job {
    // the scores and the status words travel to pinned memory right behind the kernels (queued by begin): end only waits for
    // the event - collecting a finished job cost 70 us of two pageable copies and a stream synchronisation
    double* pin = nullptr;          // G doubles, then 8 ints
    size_t pin_cap = 0;
    Event done;
    double* hX = nullptr;           // pinned copy of the signatures (the caller may drop X once begin returns; the upload does not stage)
    size_t hX_cap = 0;
    ~fdx_leverage_job() {
        if (pin) fdx::pinned_buffer_put(pin, pin_cap);
        if (hX) fdx::pinned_buffer_put(hX, hX_cap);
    }
    DevBuf dX, dW, dS, dL, dDbg, dScratch;
    int K = 0, G = 0, route = LEV_ROUTE_SVD;
    double reg = 0.0;
    hipStream_t st = nullptr;
    std::shared_ptr<fdx::HelperTicket> ticket;   // begin's launches were handed to the helper thread: end waits for them first
    std::shared_ptr<LevEntry> hit;               // a cached X: the job was complete when begin returned, nothing above is in use
    bool cacheable = false;                      // a miss: end inserts the entry (route0: the route the key names)
    int route0 = LEV_ROUTE_SVD;
    bool fallback = true;                        // a refusal of the Cholesky-QR route is answered with the Jacobi SVD passes
};

namespace fdx {
// the library's per-device side stream (leverage job, the X-side preamble of a fit / a shard's prepare, the export)
hipStream_t library_side_stream() {
    static hipStream_t streams[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    if (!streams[dev]) {
        // A priority of its own keeps the side stream off the hardware queue the caller's streams share (HIP multiplexes
        // same-priority streams over a few queues; with RCCL's streams around, aliasing with the caller's stream
        // serialised the SVD with the graph build).
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        if (hipStreamCreateWithPriority(&streams[dev], hipStreamNonBlocking, hi) != hipSuccess &&
            hipStreamCreateWithFlags(&streams[dev], hipStreamNonBlocking) != hipSuccess)
            streams[dev] = nullptr;
    }
    return streams[dev];
}
}  // namespace fdx

extern "C" int fdx_leverage_begin(const double* X, int32_t K, int32_t G, double regularization, fdx_leverage_job** out) {
    return fdx_leverage_begin_opt(X, K, G, regularization, 1, out);
}

// queue_async = 0: the launches are queued by the calling thread (a caller that collects the scores at once gains nothing from the
// helper thread - and in the gene-selection flow of FlashDeconv.fit the hand-over measurably cost ~3 ms of wait on some boxes)
static int leverage_begin_impl(const double* X, int32_t K, int32_t G, double regularization, int32_t queue_async, int route,
                               bool use_cache, fdx_leverage_job** out);
extern "C" int fdx_leverage_begin_opt(const double* X, int32_t K, int32_t G, double regularization, int32_t queue_async,
                                      fdx_leverage_job** out) {
    return leverage_begin_impl(X, K, G, regularization, queue_async, -1, true, out);
}
// route < 0: the route a fit starts on (Cholesky-QR where it applies; FDX_LEV_ONE_WG: the one-workgroup Jacobi kernel), with the
// fallback; a LEV_ROUTE_* value: that route and nothing else (fdx_leverage_scores_route)
static int leverage_begin_impl(const double* X, int32_t K, int32_t G, double regularization, int32_t queue_async, int route,
                               bool use_cache, fdx_leverage_job** out) {
    FDX_REQUIRE(X && out && K > 0 && G > 0, "fdx_leverage_begin: bad arguments");
    *out = nullptr;
    auto* job = new fdx_leverage_job();
    job->K = K;
    job->G = G;
    job->reg = regularization;
    if (route < 0)
        job->route0 = fdx::env("FDX_LEV_ONE_WG") ? LEV_ROUTE_SVD_ONE_WG : leverage_qr_applies(K, G) ? LEV_ROUTE_QR : LEV_ROUTE_SVD;
    else {
        job->route0 = route;
        job->fallback = false;
    }
    if (use_cache && !fdx::env("FDX_NO_PLAN_CACHE")) {
        XCacheKey key;
        key.K = K; key.G = G; key.reg = regularization; key.route = job->route0; key.X = X;
        job->hit = lev_cache().find(key);
        if (job->hit) {                          // no device work, no helper thread, no side stream
            *out = job;
            return 0;
        }
        job->cacheable = true;
    }
    job->st = library_side_stream();
    job->hX = (double*)pinned_buffer_get((size_t)K * G * sizeof(double), &job->hX_cap);
    if (!job->hX) { delete job; return fail(FDX_ERR_HIP, "fdx_leverage_begin: pinned host buffer"); }
    std::memcpy(job->hX, X, (size_t)K * G * sizeof(double));
    // the upload (a pageable copy: the host waits for it) and the launches cost ~75 us of host time that the caller - on its way to
    // a graph build, with the scores not needed before the sketch tables - has better uses for: the helper thread queues them
    const bool async = queue_async != 0;
    auto run = [job, K, G, regularization]() -> int {
        PoolStream pool_stream(job->st);
        FDX_TRY(job->dX.alloc((size_t)K * G * sizeof(double)));
        FDX_TRY(job->dW.alloc((size_t)K * G * sizeof(double)));
        FDX_TRY(job->dS.alloc((size_t)K * sizeof(double)));
        FDX_TRY(job->dL.alloc((size_t)G * sizeof(double)));
        FDX_TRY(job->dDbg.alloc(8 * sizeof(int)));
        FDX_HIP(hipMemcpyAsync(job->dX.p, job->hX, (size_t)K * G * sizeof(double), hipMemcpyHostToDevice, job->st));
        FDX_TRY(job->dScratch.alloc(leverage_scratch_doubles(K, G) * sizeof(double)));
        job->route = job->route0;
        FDX_TRY(launch_leverage(job->dX.as<double>(), K, G, regularization, job->dW.as<double>(), job->dS.as<double>(),
                                job->dL.as<double>(), job->dDbg.as<int>(), job->dScratch.as<double>(), job->st, job->route));
        job->pin = (double*)pinned_buffer_get((size_t)G * sizeof(double) + 64, &job->pin_cap);
        FDX_REQUIRE(job->pin != nullptr, "fdx_leverage_begin: pinned host buffer");
        FDX_HIP(hipMemcpyAsync(job->pin, job->dL.p, (size_t)G * sizeof(double), hipMemcpyDeviceToHost, job->st));
        FDX_HIP(hipMemcpyAsync(job->pin + G, job->dDbg.p, 8 * sizeof(int), hipMemcpyDeviceToHost, job->st));
        return job->done.record(job->st);
    };
    if (async) {
        job->ticket = helper_submit(run);
        *out = job;
        return 0;
    }
    const int rc = run();
    if (rc) {
        (void)hipStreamSynchronize(job->st);
        delete job;
        return rc;
    }
    *out = job;
    return 0;
}

static int leverage_end_impl(fdx_leverage_job* job, double* lev_out, double** x_dev_out, int32_t* info = nullptr);
extern "C" int fdx_leverage_end(fdx_leverage_job* job, double* lev_out) { return leverage_end_impl(job, lev_out, nullptr); }
extern "C" int fdx_leverage_end_keep(fdx_leverage_job* job, double* lev_out, double** x_dev_out) {
    FDX_REQUIRE(x_dev_out != nullptr, "fdx_leverage_end_keep: null output");
    *x_dev_out = nullptr;
    return leverage_end_impl(job, lev_out, x_dev_out);
}
static int leverage_end_impl(fdx_leverage_job* job, double* lev_out, double** x_dev_out, int32_t* info) {
    FDX_REQUIRE(job != nullptr, "fdx_leverage_end: null job");
    if (job->hit) {
        std::unique_ptr<fdx_leverage_job> owner(job);
        const LevEntry& c = *job->hit;
        FDX_REQUIRE(lev_out != nullptr, "fdx_leverage_end: null output");
        std::memcpy(lev_out, c.scores.data(), (size_t)job->G * sizeof(double));
        if (x_dev_out) {                         // a fresh device copy of X for the caller, from the entry's copy
            hipStream_t st = library_side_stream();
            PoolStream pool_stream(st);
            DevBuf dX;
            FDX_TRY(dX.alloc(c.key.words() * sizeof(double)));
            FDX_TRY(copy_h2d(dX.p, c.X.data(), c.key.words() * sizeof(double), st));
            FDX_HIP(hipStreamSynchronize(st));
            dX.mark_idle();
            *x_dev_out = dX.as<double>();
            dX.p = nullptr;
            dX.bytes = dX.cap = 0;
        }
        if (fdx::env("FDX_DEBUG"))
            std::fprintf(stderr, "[fdx] leverage: K=%d G=%d route=%s passes/sweeps=%d converged=%d (cached)\n", job->K, job->G,
                         c.route == LEV_ROUTE_QR ? "cholesky-qr" : "jacobi-svd", c.dbg[0], c.dbg[6]);
        return 0;
    }
    if (job->ticket) {
        const int qrc = helper_wait(job->ticket);
        job->ticket.reset();
        if (qrc) {
            (void)hipStreamSynchronize(job->st);
            delete job;
            return qrc;
        }
    }
    int rc = 0;
    int dbg[8] = {0};
    auto run = [&]() -> int {
        FDX_REQUIRE(lev_out != nullptr, "fdx_leverage_end: null output");
        FDX_HIP(hipMemcpyAsync(lev_out, job->dL.p, (size_t)job->G * sizeof(double), hipMemcpyDeviceToHost, job->st));
        FDX_HIP(hipMemcpyAsync(dbg, job->dDbg.p, sizeof(dbg), hipMemcpyDeviceToHost, job->st));
        return 0;
    };
    hipError_t e = hipSuccess;
    if (lev_out == nullptr) rc = fail(FDX_ERR_INVALID, "fdx_leverage_end: null output");
    if (job->done && job->pin) {
        // the job's kernels and its copies are the last work of the job on its stream: behind the event nothing of it is in flight
        e = hipEventSynchronize(job->done.e);
        if (!rc && e == hipSuccess) {
            std::memcpy(lev_out, job->pin, (size_t)job->G * sizeof(double));
            std::memcpy(dbg, job->pin + job->G, sizeof(dbg));
        }
    } else {
        if (!rc) rc = run();
        e = hipStreamSynchronize(job->st);          // always drain before the buffers go back to the pool
    }
    const bool refused = !rc && e == hipSuccess && job->route == LEV_ROUTE_QR && dbg[7] != 1;
    if (refused && job->fallback) {
        // the Cholesky-QR route refused the matrix (rank-deficient or cond above ~3e4): the Jacobi SVD passes, as before
        PoolStream pool_stream(job->st);
        job->route = LEV_ROUTE_SVD;
        rc = launch_leverage(job->dX.as<double>(), job->K, job->G, job->reg, job->dW.as<double>(), job->dS.as<double>(),
                             job->dL.as<double>(), job->dDbg.as<int>(), job->dScratch.as<double>(), job->st, LEV_ROUTE_SVD);
        if (!rc) rc = run();
        e = hipStreamSynchronize(job->st);
        if (!rc) dbg[5] = 1;                                   // for the debug line: fell back
    }
    if (!rc && e != hipSuccess) rc = fail(FDX_ERR_HIP, hipGetErrorString(e));
    if (e == hipSuccess)              // nothing of the job is in flight any more: the blocks may follow any stream
        for (DevBuf* b : {&job->dX, &job->dW, &job->dS, &job->dL, &job->dDbg, &job->dScratch}) b->mark_idle();
    if (!rc && e == hipSuccess && x_dev_out) {      // the device copy of X changes hands (the caller returns it with fdx_free)
        *x_dev_out = job->dX.as<double>();
        job->dX.p = nullptr;
        job->dX.bytes = job->dX.cap = 0;
    }
    if (!rc && e == hipSuccess && info) {
        // {route that produced the scores (fdx.h numbering), refused, passes or sweeps, done / converged, fell back, 0, 0, 0}
        const int form = job->route == LEV_ROUTE_QR ? LEV_ROUTE_QR : leverage_svd_form(job->K, job->route);
        const int settled = form == LEV_ROUTE_QR ? dbg[7] == 1 : form == LEV_ROUTE_SVD_STREAM ? dbg[6] != 0 : dbg[0] < LEV_ONE_WG_MAX_SWEEPS;
        const int32_t v[8] = {form, refused ? 1 : 0, dbg[0], settled, refused && job->fallback ? 1 : 0, 0, 0, 0};
        std::memcpy(info, v, sizeof(v));
    }
    if (!rc && e == hipSuccess && job->cacheable && job->hX) {
        // the scores have arrived and the route has settled
        auto ent = std::make_shared<LevEntry>();
        ent->X.assign(job->hX, job->hX + (size_t)job->K * job->G);
        ent->key.K = job->K; ent->key.G = job->G; ent->key.reg = job->reg; ent->key.route = job->route0; ent->key.X = ent->X.data();
        ent->scores.assign(lev_out, lev_out + job->G);
        ent->route = job->route;
        std::memcpy(ent->dbg, dbg, sizeof(dbg));
        lev_cache().insert(std::move(ent));
    }
    if (!rc && fdx::env("FDX_DEBUG"))   // phase stamps in 100 MHz ticks
        std::fprintf(stderr, "[fdx] leverage: K=%d G=%d route=%s passes/sweeps=%d converged=%d\n", job->K, job->G,
                     job->route == LEV_ROUTE_QR ? "cholesky-qr" : "jacobi-svd", dbg[0], dbg[6]);
    delete job;
    return rc;
}

extern "C" int fdx_leverage_scores(const double* X, int32_t K, int32_t G, double regularization, double* lev_out) {
    FDX_REQUIRE(X && lev_out && K > 0 && G > 0, "fdx_leverage_scores: bad arguments");
    fdx_leverage_job* job = nullptr;
    FDX_TRY(fdx_leverage_begin(X, K, G, regularization, &job));
    return fdx_leverage_end(job, lev_out);
}

extern "C" int fdx_leverage_scores_route(const double* X, int32_t K, int32_t G, double regularization, int32_t route, double* lev_out,
                                         int32_t* info) {
    FDX_REQUIRE(X && lev_out && info && K > 0 && G > 0, "fdx_leverage_scores_route: bad arguments");
    FDX_REQUIRE(route >= 0 && route <= 3, "fdx_leverage_scores_route: route must be 0 .. 3");
    FDX_REQUIRE(route != LEV_ROUTE_QR || leverage_qr_applies(K, G), "fdx_leverage_scores_route: the Cholesky-QR route needs 2 <= K <= 272");
    FDX_REQUIRE(route != LEV_ROUTE_SVD_STREAM || leverage_stream_applies(K), "fdx_leverage_scores_route: the streaming Jacobi passes need 2 <= K <= 64");
    fdx_leverage_job* job = nullptr;
    FDX_TRY(leverage_begin_impl(X, K, G, regularization, 0, route == 0 ? -1 : route, false, &job));
    return leverage_end_impl(job, lev_out, nullptr, info);
}

extern "C" int fdx_column_sums_dev(const void* Y_dev, int32_t dtype, int64_t n, int32_t G, int64_t ldy,
                                   double* sums_out_host, void* stream) {
    FDX_REQUIRE(dtype == FDX_F32 || dtype == FDX_F64, "fdx_column_sums_dev: dtype must be FDX_F32 or FDX_F64");
    FDX_REQUIRE(n >= 0 && G > 0 && sums_out_host && (n == 0 || Y_dev), "fdx_column_sums_dev: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    PoolStream pool_stream(st);
    DevBuf dPart, dOut;
    FDX_TRY(dPart.alloc((size_t)column_sums_parts(n) * G * sizeof(double)));
    FDX_TRY(dOut.alloc((size_t)G * sizeof(double)));
    FDX_TRY(launch_column_sums(Y_dev, dtype, ldy, n, G, dPart.as<double>(), dOut.as<double>(), st));
    FDX_TRY(copy_d2h(sums_out_host, dOut.p, (size_t)G * sizeof(double), st));
    FDX_HIP(hipStreamSynchronize(st));
    return 0;
}

// What a fit that stopped on k-NN ties leaves behind for the fit that follows on the rebuilt graph: the sketch -> H stage (the
// rebuilt graph keeps the Morton order, so H's columns are where the second fit wants them) with everything the still-running
// kernel reads, and an event behind it.  The stopped call returns at once instead of draining ~3 ms of sketch that the tie remedy's
// host work (a kd-tree build of ~20 ms) then runs beside.
struct fdx_fit_carry {
    fdx::DevBuf dH, dRowSq;
    std::shared_ptr<fdx::XSideBufs> xs;           // X_sketch, read by the fused kernels (shared with the X-side cache when published)
    fdx::YTables tables;
    fdx::Event done;
    long long n = 0, ld = 0;
    int K = 0, KP = 0, d = 0, G = 0, mode_y = 0;
    const void* y_id = nullptr;
    bool fused = false;
    double gram_ms = 0.0;                         // (sketch_ms: the stage's events belong to the stopped call, the second fit reports the stage as carried)
    ~fdx_fit_carry() {
        if (done) (void)hipEventSynchronize(done.e);
    }
};

extern "C" int fdx_fit_carry_free(void* carry) {
    delete static_cast<fdx_fit_carry*>(carry);
    return 0;
}

namespace {

// The caller has let go of prm->carry when it makes the call: it is owned here ahead of every check, so that an early return
// waits for the carry's kernel and releases its buffers
std::unique_ptr<fdx_fit_carry> adopt_carry(const fdx_fit_params* prm) {
    return std::unique_ptr<fdx_fit_carry>(prm ? static_cast<fdx_fit_carry*>(prm->carry) : nullptr);
}

int fit_impl(const YSource& ysrc, int64_t n, int32_t G, const double* X, int32_t K, const int32_t* bucket,
             const double* weight_y, const double* weight_x, const double* coords_dev, int32_t dim,
             const fdx_fit_params* prm_in, std::unique_ptr<fdx_fit_carry> carry_in, fdx_graph** graph_inout, double* beta_out_dev,
             double* prop_out_dev, double* objectives_out, double* rel_changes_out, fdx_fit_info* info, void* stream) {
    FDX_REQUIRE(info != nullptr && prm_in != nullptr && graph_inout != nullptr, "fdx_fit_dev: null argument");
    fdx_fit_params prm_local = *prm_in;
    prm_local.mode_y &= 0xff;
    const fdx_fit_params* prm = &prm_local;
    TileF64Math f64_math((prm_in->mode_y & FDX_PRE_F64_MATH) != 0);
    std::memset(info, 0, sizeof(*info));
    const int32_t y_dtype = ysrc.row_dtype();
    FDX_REQUIRE(y_dtype == FDX_F32 || y_dtype == FDX_F64, "fdx_fit_dev: Y dtype must be FDX_F32 or FDX_F64");
    FDX_REQUIRE(n > 0 && G > 0 && K > 0, "fdx_fit_dev: empty problem");
    FDX_REQUIRE(n < 0x7fffff00LL, "fdx_fit_dev: n too large for one device");
    FDX_REQUIRE(ysrc.csr || ysrc.ldy >= G, "fdx_fit_dev: ldy < G");
    FDX_REQUIRE((ysrc.dense || ysrc.csr) && X && bucket && weight_y && weight_x, "fdx_fit_dev: null array");
    const int d = prm->sketch_dim;
    FDX_REQUIRE(d > 0, "fdx_fit_dev: sketch_dim must be positive");
    FDX_REQUIRE(prm->max_iter >= 0, "fdx_fit_dev: max_iter must be non-negative");
    hipStream_t st = (hipStream_t)stream;
    PoolStream pool_stream(st);
    // contiguous intervals on the caller's stream: [begin, eS0) prologue, [eS0, eS1) sketch -> H, [eS1, solved) solve + objective,
    // [solved, end) what is left of the export
    Event t_begin(true), t_graph(true), eS0(true), eS1(true), t_solved(true), t_end(true);
    FDX_TRY(t_begin.record(st));
    trace_host("fit", "entry");

    // ---- spatial graph (core/deconv.py:358)
    fdx_graph* g = nullptr;
    if (prm->graph_method == FDX_GRAPH_GIVEN) {
        g = *graph_inout;
        FDX_REQUIRE(g != nullptr && g->n == n, "fdx_fit_dev: given graph does not match n");
    } else {
        FDX_REQUIRE(coords_dev != nullptr, "fdx_fit_dev: null coords");
        g = new fdx_graph();
        int rc = (prm->graph_method == FDX_GRAPH_KNN)
                     ? graph_build_knn(coords_dev, n, dim, prm->k_neighbors, g, st)
                     : graph_build_radius(coords_dev, n, dim, prm->radius, 0, n, g, st);
        if (rc) { delete g; return rc; }
        *graph_inout = g;
    }
    // the build's start event serves this one fit (a later fit on the same handle starts its own clock; a cached graph gets a
    // new one with every hit): taken over here, under the graph's lock - the graph may have other holders
    Event build_begin(true);
    if (prm->graph_method == FDX_GRAPH_GIVEN) {
        std::lock_guard<std::mutex> lk(g->mu);
        if (g->begin_event && g->begin_stream == st) {
            build_begin.e = g->begin_event;
            g->begin_event = nullptr;
            g->begin_stream = nullptr;
        }
    }
    // a deferred build (graph_ell.cpp) queued on ANOTHER stream: everything below reads the graph's arrays (perm first)
    if (g->meta_pending && g->meta_event && g->meta_stream != st) FDX_HIP(hipStreamWaitEvent(st, g->meta_event, 0));
    FDX_TRY(t_graph.record(st));

    // ---- Everything that does not depend on the graph or on Y goes to the library's side stream and runs beside the graph build
    // queued on the caller's stream just before: beta0 = 1/K (core/solver.py:372) and the cleared pad rows, the sketch tables
    // (Omega comes from the host: hash/sign from numpy's RandomState, core/sketching.py:58-59; plans are shared through a
    // content-keyed cache, so a repeated fit builds nothing), X, X_sketch (K, d) and XtX (core/sketching.py:202-204,
    // core/solver.py:346).  The buffers are allocated with the side stream as their pool stream (a block last used elsewhere
    // orders it behind that work); the caller's stream waits for ONE event before the sketch.  (Queued on the caller's stream
    // these ~120 us of small launches and copies sat between the end of the graph build and the start of the sketch, and a new
    // plan's table upload made the host wait for the whole graph build.)
    const long long ld = round_up(n + 1, 64);
    const int KP = solver_padded_K(K);             // 65 - 128 cell types: planes of the next instantiated sweep, pad types all zero
    // declared ABOVE the drains: on an early return both streams are drained before any of these goes back to the pool
    // (the rows' squared norms and dSum are read on the side stream)
    DevBuf dB0, dB1, dH, dSum;
    XSide x;
    YTables tables;                 // the Y side's plan, or a CSR source's selected columns with their {weight, bucket}
    RowsToH rows;
    struct SideDrain { hipStream_t s = nullptr; ~SideDrain() { if (s) (void)hipStreamSynchronize(s); } } side_drain;   // before buffers are released
    // an early return leaves work on the caller's stream that uses the side-stream buffers above: wait for it before they go
    struct AbortDrain { hipStream_t s; bool armed = true; ~AbortDrain() { if (armed) (void)hipStreamSynchronize(s); } } abort_drain{st};
    Event evInit, evG;
    hipStream_t side = fdx::env("FDX_NO_SIDE_STREAM") ? nullptr : library_side_stream();
    if (side == st) side = nullptr;
    const hipStream_t xs = side ? side : st;
    if (side) side_drain.s = side;
    for (int g_ = 0; g_ < G; ++g_) FDX_REQUIRE(bucket[g_] >= 0 && bucket[g_] < d, "fit: bucket index out of range");
    double* Gh = (double*)pinned_scratch(0, (size_t)K * K * sizeof(double));   // pinned: the copy of XtX must not hold the host back
    FDX_REQUIRE(Gh != nullptr, "fit: pinned host buffer");
    const bool beta0_virtual = side && KP == K && K <= FDX_MAX_K_FAST && prm->max_iter > 0 && !prm->verbose && !fdx::env("FDX_NO_INIT_SWEEP");
    {
        PoolStream pool_xs(xs);
        FDX_TRY(tables.build(ysrc, G, d, K, bucket, weight_y, xs, "fdx_fit_csr_dev"));
    }
    if (weight_x == weight_y) x.plan = tables.plan;   // (a CSR source has none)
    FDX_TRY(queue_x_side(&x, X, nullptr, K, KP, G, d, prm->mode_x, bucket, weight_x, nullptr, Gh, &evG, xs));
    // A repeated fit: the X side came from its cache (no event: nothing was queued for it) and is complete, and the Y side's plan
    // is the one that entry was computed with, so its tables were uploaded before the entry was published.  The sketch then reads
    // nothing that is in flight on the side stream: it is launched first, and what it does not read - the abundance buffers with
    // their pad fills - is queued while it runs instead of ahead of it (~35 us of host path per fit).  In every other case the
    // sketch waits for evInit as ever.  Not for a call that may stop on ties (counts still pending, or known ties): the pad fills
    // find no free compute unit until the sketch ends, and the stopped call would wait for them where it returns at once today.
    const bool may_stop = prm->stop_on_ties && (g->meta_pending || g->knn_ties > 0);
    const bool sketch_first = side && !carry_in && !may_stop && !evG && x.b->published && tables.plan && tables.plan == x.plan;
    const double* XtX_dev = x.XtX(K, KP);
    const int* row_map = g->identity_order ? nullptr : g->perm.as<int>();
    // the abundance buffers (beta0 = 1/K, core/solver.py:372, and the cleared pad rows); on the side stream everything queued there
    // so far is behind evInit, which the caller's stream waits for
    auto queue_solver_buffers = [&]() -> int {
        {
            PoolStream pool_xs(xs);
            FDX_TRY(dB0.alloc((size_t)KP * ld * sizeof(double)));
            FDX_TRY(dB1.alloc((size_t)KP * ld * sizeof(double)));
            if (side) {
                // no pad types: the uniform start vector is a constant of the first sweep and is not written (solver.cpp: beta0_virtual)
                if (beta0_virtual) FDX_TRY(solver_zero_pad(dB0.as<double>(), ld, g->n_total, KP, xs));
                else FDX_TRY(solver_init_beta(dB0.as<double>(), ld, g->n_total, K, xs, KP));
                FDX_TRY(solver_zero_pad(dB1.as<double>(), ld, g->n_total, KP, xs));
            }
        }
        if (side) {
            FDX_TRY(evInit.record(side));
            // tables, X_sketch, XtX, beta0: all behind this one.  (Behind a sketch launched first only the solve needs it, and the
            // solve waits for it itself, below: a second barrier between the sketch and the first sweep costs the device ~7 us.)
            if (!sketch_first) FDX_TRY(evInit.wait_on(st));
        }
        return 0;
    };
    // Y_sketch in solver order, contracted into H (K, ld) as it is produced
    auto queue_sketch = [&]() -> int {
        FDX_TRY(dH.alloc((size_t)KP * ld * sizeof(double)));
        if (KP != K) FDX_HIP(hipMemsetAsync(dH.as<double>() + (size_t)K * ld, 0, (size_t)(KP - K) * ld * sizeof(double), st));   // pad types
        FDX_TRY(solver_zero_pad(dH.as<double>(), ld, n, K, st));   // columns of real spots are all written by the sketch -> H stage
        FDX_TRY(eS0.record(st));                  // the prologue (graph chain, X-side preamble) ends here
        FDX_TRY(queue_rows_to_h(ysrc, tables, n, G, d, K, prm->mode_y, row_map, x.Xs(), dH.as<double>(), ld, true, &rows, st));
        return eS1.record(st);                    // read at the end of the fit, no wait here
    };
    if (sketch_first) {
        FDX_TRY(queue_sketch());
        trace_host("fit", "sketch queued ahead of the side-stream preamble");
        FDX_TRY(queue_solver_buffers());
        FDX_TRY(dSum.alloc(sizeof(double)));
    } else {
        FDX_TRY(queue_solver_buffers());
        // ---- ... or a carry: the sketch -> H stage of a call that stopped on ties for these inputs (the rebuilt graph keeps the
        // spot order)
        if (carry_in)
            FDX_REQUIRE(carry_in->n == n && carry_in->ld == ld && carry_in->K == K && carry_in->KP == KP && carry_in->d == d &&
                            carry_in->G == G && carry_in->mode_y == prm->mode_y && carry_in->y_id == ysrc.id(),
                        "fdx_fit_dev: the carry belongs to a different problem");
        FDX_TRY(dSum.alloc(sizeof(double)));
        trace_host("fit", "side-stream preamble queued, buffers allocated");
        if (carry_in) {                           // H and the rows' squared norms as the stopped call left them, behind its event
            FDX_TRY(eS0.record(st));
            FDX_TRY(carry_in->done.wait_on(st));
            dH.take(carry_in->dH);
            rows.dRowSq.take(carry_in->dRowSq);
            rows.fused = carry_in->fused;
            rows.gram_ms = carry_in->gram_ms;
            FDX_TRY(eS1.record(st));
        } else {
            FDX_TRY(queue_sketch());
        }
    }
    // ---- the graph's counts (a build that was only queued has long finished behind the sketch launch).  Ties under stop_on_ties: the
    // caller wants the reference's choice among equidistant neighbours - nothing is solved on this graph, and the sketch -> H stage
    // that is already running goes to the caller as a carry for the fit on the rebuilt graph (tie-free inputs never pay for the
    // question; lattices no longer pay a second sketch and the wait for the first)
    // (a cached X side is complete: no event.  A new one is published now that its last copy has arrived)
    if (!prm->verbose && evG) FDX_TRY(evG.sync());
    if (!prm->verbose) x_side_publish(&x, X, Gh);
    FDX_TRY(graph_meta_sync(g));
    info->knn_ties = g->knn_ties;
    info->nnz = g->nnz;
    if (prm->stop_on_ties && g->knn_ties > 0) {
        info->status = FDX_FIT_TIES;
        if (carry_in) return 0;                   // (a carry on a graph that still has ties: dropped, drained by the guards)
        auto carry = std::make_unique<fdx_fit_carry>();
        FDX_TRY(carry->done.record(st));
        carry->dH.take(dH);
        carry->dRowSq.take(rows.dRowSq);
        carry->xs = x.b;                          // (X_sketch is read by the fused kernels)
        carry->tables = std::move(tables);
        carry->n = n; carry->ld = ld; carry->K = K; carry->KP = KP; carry->d = d; carry->G = G; carry->mode_y = prm->mode_y;
        carry->y_id = ysrc.id();
        carry->fused = rows.fused;
        carry->gram_ms = rows.gram_ms;
        if (!rows.fused) FDX_HIP(hipStreamSynchronize(st));   // the chunked path's Y_sketch buffer goes back to the pool with this call
        info->carry = carry.release();
        abort_drain.armed = false;                // everything the running kernel reads lives in the carry (Y and the graph: the caller's)
        return 0;
    }
    // YtY (core/solver.py:348) only enters the objective: its two small reductions and the read-back go to the side stream (behind the
    // sketch, beside the first sweep) instead of standing between the sketch and the sweeps; the verbose trace needs it at once
    double* YtY_h = (double*)pinned_scratch(1, sizeof(double));   // pinned: the host runs ahead and queues the solve behind the sketch
    FDX_REQUIRE(YtY_h != nullptr, "fit: pinned host buffer");
    *YtY_h = 0.0;
    Event evY;                                    // YtY has arrived (the export is queued on the same stream later)
    FDX_TRY(queue_yty(rows.dRowSq.as<double>(), n, dSum.as<double>(), YtY_h, &evY, st, (side && !prm->verbose) ? side : st));
    if (prm->verbose) {
        FDX_HIP(hipStreamSynchronize(st));
        x_side_publish(&x, X, Gh);
    }
    trace_host("fit", "sketch queued, XtX on the host");
    const double diag_mean = xtx_diag_mean(Gh, K);
    const double lambda = prm->lambda_auto ? auto_lambda(diag_mean, (double)g->nnz / (double)n) : prm->lambda_spatial;

    // ---- solve
    SolveProblem p;
    p.graph = g; p.H = dH.as<double>(); p.ldh = ld; p.XtX = XtX_dev;
    p.beta[0] = dB0.as<double>(); p.beta[1] = dB1.as<double>(); p.ld = ld; p.K = KP; p.K_real = K; p.YtY = prm->verbose ? *YtY_h : 0.0;   // verbose: the stream was synchronised above
    p.lambda = lambda; p.rho_eff = prm->rho_sparsity * diag_mean; p.max_iter = prm->max_iter; p.tol = prm->tol;
    p.verbose = prm->verbose;
    p.compute_objective = prm->verbose ? 1 : 0;
    SolveResult r;
    if (evInit) {
        p.init_beta = 0;                     // done on the side stream at the top
        p.beta0_virtual = beta0_virtual ? 1 : 0;
        FDX_TRY(evInit.wait_on(st));
    }
    FDX_TRY(solver_run(p, &r, st));          // its chunked read-backs synchronise the stream: YtY has arrived after it
    // The export of the result (type-major solver order -> row-major caller order, 0.25 ms at 1M x 30) and the objective pass
    // (0.2 ms) both only read the final abundances: the export goes to the library's side stream (idle here - the leverage
    // job was collected before this call) and runs beside the objective pass instead of after it.
    Event evSolved, evExported;
    if ((beta_out_dev || prop_out_dev) && !prm->verbose && side) {
        FDX_TRY(evSolved.record(st));
        FDX_TRY(evSolved.wait_on(side));
        FDX_TRY(launch_normalize_export(p.beta[r.result_buffer], ld, row_map, (int)n, g->n_slices, K, beta_out_dev,
                                        prop_out_dev, side));
        FDX_TRY(evExported.record(side));
    }
    if (!prm->verbose) {
        DevBuf objp, objo;
        FDX_TRY(objp.alloc((size_t)std::max(objective_partials_count(g->n_slices), g->n_tiles) * 4 * sizeof(double)));
        FDX_TRY(objo.alloc(4 * sizeof(double)));
        if (prm->max_iter == 0) FDX_HIP(hipStreamSynchronize(st));
        if (evY) FDX_TRY(evY.sync());   // long there
        FDX_TRY(solver_objective(*g, p.beta[r.result_buffer], ld, p.H, ld, p.XtX, KP, *YtY_h, lambda, p.rho_eff, objp.as<double>(),
                                 objo.as<double>(), &r.final_objective, st));
    }
    FDX_TRY(t_solved.record(st));
    if (evExported) FDX_TRY(evExported.wait_on(st));
    else if (beta_out_dev || prop_out_dev)
        FDX_TRY(launch_normalize_export(p.beta[r.result_buffer], ld, row_map, (int)n, g->n_slices, K, beta_out_dev,
                                        prop_out_dev, st));
    // per-spot diagnostics on request: one more launch behind the objective pass and the export, inside finish_ms / span_ms.  It
    // reads the K real types only (the bordered XtX of a padded solve with its own row stride)
    Event t_diag0(true), t_diag1(true);
    if (prm->spot_diag_out_dev) {
        FDX_TRY(t_diag0.record(st));
        FDX_TRY(launch_spot_diagnostics(p.beta[r.result_buffer], ld, p.H, ld, XtX_dev, KP, rows.dRowSq.as<double>(), g->ell.as<int>(),
                                        g->slice_off.as<int>(), g->deg.as<int>(), row_map, (int)n, g->n_slices, K,
                                        prm->spot_diag_out_dev, st));
        FDX_TRY(t_diag1.record(st));
    }
    FDX_TRY(t_end.record(st));
    FDX_HIP(hipStreamSynchronize(st));
    abort_drain.armed = false;

    info->solve.converged = r.converged;
    info->solve.n_iterations = r.n_iterations;
    info->solve.final_objective = r.final_objective;
    info->solve.final_change = r.final_change;
    info->solve.n_objectives = (int32_t)r.objectives.size();
    info->solve.sweep_ms = r.sweep_ms;
    info->lambda_used = lambda;
    info->rho_effective = p.rho_eff;
    info->YtY = *YtY_h;
    info->nnz = g->nnz;
    info->graph_ms = t_graph.ms_since(t_begin.e);
    info->sketch_ms = rows.fused ? eS1.ms_since(eS0.e) : rows.sketch_ms;   // the chunked path keeps its per-chunk split of the same interval
    info->gram_ms = rows.gram_ms;
    const hipEvent_t t0 = build_begin ? build_begin.e : t_begin.e;
    info->prologue_ms = eS0.ms_since(t0);
    info->span_ms = t_end.ms_since(t0);
    info->solve_ms = t_solved.ms_since(eS1.e);
    info->finish_ms = t_end.ms_since(t_solved.e);
    info->diag_ms = t_diag1.ms_since(t_diag0.e);
    info->total_ms = t_end.ms_since(t_begin.e);
    info->solve.total_ms = info->total_ms;
    if (objectives_out)
        for (size_t t = 0; t < r.objectives.size(); ++t) objectives_out[t] = r.objectives[t];
    if (rel_changes_out)
        for (size_t t = 0; t < r.rel_changes.size(); ++t) rel_changes_out[t] = r.rel_changes[t];
    return 0;
}

}  // namespace

extern "C" int fdx_fit_dev(const void* Y_dev, int32_t y_dtype, int64_t n, int32_t G, int64_t ldy, const double* X, int32_t K,
                           const int32_t* bucket, const double* weight_y, const double* weight_x, const double* coords_dev,
                           int32_t dim, const fdx_fit_params* prm, fdx_graph** graph_inout, double* beta_out_dev,
                           double* prop_out_dev, double* objectives_out, double* rel_changes_out, fdx_fit_info* info,
                           void* stream) {
    auto carry = adopt_carry(prm);
    FDX_REQUIRE(Y_dev != nullptr, "fdx_fit_dev: null array");
    YSource ys;
    ys.dense = Y_dev;
    ys.dtype = y_dtype;
    ys.ldy = ldy;
    return fit_impl(ys, n, G, X, K, bucket, weight_y, weight_x, coords_dev, dim, prm, std::move(carry), graph_inout, beta_out_dev,
                    prop_out_dev, objectives_out, rel_changes_out, info, stream);
}

static int csr_view_ok(const fdx_csr_view* Y, const char* who) {
    FDX_REQUIRE(Y != nullptr, std::string(who) + ": null matrix");
    FDX_REQUIRE(Y->n >= 0 && Y->nnz >= 0 && Y->G > 0, std::string(who) + ": bad CSR shape");
    FDX_REQUIRE(Y->indptr != nullptr && (Y->nnz == 0 || (Y->indices && Y->data)), std::string(who) + ": null CSR array");
    FDX_REQUIRE(Y->dtype == FDX_F32 || Y->dtype == FDX_F64, std::string(who) + ": dtype must be FDX_F32 or FDX_F64");
    return 0;
}

extern "C" int fdx_csr_check_dev(const fdx_csr_view* Y, void* stream) {
    FDX_TRY(csr_view_ok(Y, "fdx_csr_check_dev"));
    hipStream_t st = (hipStream_t)stream;
    PoolStream pool_stream(st);
    DevBuf flag;
    FDX_TRY(flag.alloc(sizeof(int)));
    FDX_TRY(launch_csr_check((const long long*)Y->indptr, Y->indices, Y->n, Y->nnz, Y->G, Y->sorted_rows, flag.as<int>(), st));
    int bad = 0;
    FDX_HIP(hipMemcpyAsync(&bad, flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
    FDX_HIP(hipStreamSynchronize(st));
    FDX_REQUIRE((bad & 1) == 0, "CSR matrix is malformed (indptr not monotone from 0 to nnz, or a column index outside [0, G))");
    FDX_REQUIRE((bad & 2) == 0, "CSR matrix claims sorted_rows but a row's column indices are not ascending");
    return 0;
}

extern "C" int fdx_csr_gene_moments_dev(const fdx_csr_view* Y, double* mean_out_host, double* var_out_host,
                                        double* colsum_out_host, void* stream) {
    FDX_TRY(csr_view_ok(Y, "fdx_csr_gene_moments_dev"));
    FDX_REQUIRE(Y->n > 0, "fdx_csr_gene_moments_dev: empty matrix");
    hipStream_t st = (hipStream_t)stream;
    PoolStream pool_stream(st);
    const size_t G = (size_t)Y->G;
    DevBuf scale, part, out;
    const int ns = colsum_out_host ? 3 : 2;
    FDX_TRY(scale.alloc((size_t)Y->n * sizeof(double)));
    FDX_TRY(part.alloc((size_t)csr_moment_stripes(Y->n) * ns * G * sizeof(double)));
    FDX_TRY(out.alloc(3 * G * sizeof(double)));
    double* o = out.as<double>();
    FDX_TRY(launch_csr_moments((const long long*)Y->indptr, Y->indices, Y->data, Y->dtype, Y->n, Y->nnz, Y->G, scale.as<double>(),
                               part.as<double>(), o, o + G, colsum_out_host ? o + 2 * G : nullptr, Y->sorted_rows != 0, st));
    if (mean_out_host) FDX_TRY(copy_d2h(mean_out_host, o, G * sizeof(double), st));
    if (var_out_host) FDX_TRY(copy_d2h(var_out_host, o + G, G * sizeof(double), st));
    if (colsum_out_host) FDX_TRY(copy_d2h(colsum_out_host, o + 2 * G, G * sizeof(double), st));
    FDX_HIP(hipStreamSynchronize(st));
    return 0;
}

extern "C" int fdx_fit_csr_dev(const fdx_csr_view* Y, const int32_t* gene_idx, int32_t G, const double* X, int32_t K,
                               const int32_t* bucket, const double* weight_y, const double* weight_x,
                               const double* coords_dev, int32_t dim, const fdx_fit_params* prm, fdx_graph** graph_inout,
                               double* beta_out_dev, double* prop_out_dev, double* objectives_out, double* rel_changes_out,
                               fdx_fit_info* info, void* stream) {
    auto carry = adopt_carry(prm);
    FDX_TRY(csr_view_ok(Y, "fdx_fit_csr_dev"));
    FDX_REQUIRE(gene_idx != nullptr || G == Y->G, "fdx_fit_csr_dev: gene_idx may be NULL only when G equals the matrix width");
    FDX_REQUIRE(prm != nullptr, "fdx_fit_csr_dev: null argument");
    FDX_REQUIRE(prm->mode_y == FDX_PRE_RAW || prm->mode_y == FDX_PRE_LOG_CPM_SPARSE,
                "fdx_fit_csr_dev: mode_y must be FDX_PRE_RAW or FDX_PRE_LOG_CPM_SPARSE");
    YSource ys;
    ys.csr = Y;
    ys.gene_idx = gene_idx;
    return fit_impl(ys, Y->n, G, X, K, bucket, weight_y, weight_x, coords_dev, dim, prm, std::move(carry), graph_inout,
                    beta_out_dev, prop_out_dev, objectives_out, rel_changes_out, info, stream);
}
