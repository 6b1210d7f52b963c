// The sketch -> H stage of a fit and of a shard's prepare (prepare.h): core/sketching.py:194-204, core/solver.py:346-348.
#include "prepare.h"

#include <algorithm>
#include <cstring>
#include <vector>

#include "fdx_env.h"
#include "fdx_kernels.h"
#include "solver.h"

namespace fdx {

int YTables::build(const YSource& y, int G, int d, int K, const int32_t* bucket, const double* weight_y, hipStream_t xs,
                   const char* who) {
    if (!y.csr) return sketch_plan_cached(bucket, weight_y, G, d, xs, &plan);
    csr_fused = csr_contract_ok(d, K, (y.csr->G + 31) / 32, G);
    return sel.build(y.gene_idx, G, y.csr->G, bucket, weight_y, d, csr_fused, xs, who);
}

namespace {
// (on the heap, never destroyed: the entries own pooled device buffers - see sketch_plan.cpp)
XCache<XSideBufs>& x_side_cache() {
    static XCache<XSideBufs>* const c = new XCache<XSideBufs>(4);
    return *c;
}
}  // namespace

void x_side_cache_clear() { x_side_cache().clear(); }
void x_side_cache_stats(long long* hits, long long* misses) { x_side_cache().stats(hits, misses); }

int queue_x_side(XSide* x, const double* X, const double* X_dev, int K, int KP, int G, int d, int mode_x, const int32_t* bucket,
                 const double* weight_x, double* XtX_dev, double* XtX_host, Event* done, hipStream_t xs) {
    PoolStream pool_xs(xs);
    // The schedules of an Omega are built once per content and device (sketch_plan.cpp); a new Omega's tables are uploaded on xs
    if (!x->plan) FDX_TRY(sketch_plan_cached(bucket, weight_x, G, d, xs, &x->plan));
    if (!XtX_dev && XtX_host && !fdx::env("FDX_NO_PLAN_CACHE")) {
        XCacheKey& k = x->key;
        FDX_HIP(hipGetDevice(&k.dev));
        k.K = K; k.KP = KP; k.G = G; k.d = d; k.mode = mode_x;
        k.route = fdx::env("FDX_SKETCH_GATHER") ? 1 : 0;      // (the other form of sketch_rows adds in another order)
        k.plan = x->plan.get();
        k.X = X;
        x->b = x_side_cache().find(k);
        if (x->b) {
            std::memcpy(XtX_host, x->b->XtX.data(), (size_t)K * K * sizeof(double));
            return 0;
        }
        x->cacheable = true;
    }
    x->b = std::make_shared<XSideBufs>();
    XSideBufs& b = *x->b;
    if (!X_dev) FDX_TRY(x->dX.alloc((size_t)K * G * sizeof(double)));
    FDX_TRY(b.dXs.alloc((size_t)K * d * sizeof(double)));
    if (!XtX_dev) {
        FDX_TRY(b.dG.alloc((size_t)K * K * sizeof(double)));
        XtX_dev = b.dG.as<double>();
    }
    if (!X_dev) {                                   // (else: already there - the leverage job's copy, complete)
        FDX_TRY(copy_h2d(x->dX.p, X, (size_t)K * G * sizeof(double), xs));
        X_dev = x->dX.as<double>();
    }
    double* Xs = b.dXs.as<double>();
    FDX_TRY(launch_sketch_rows(X_dev, FDX_F64, G, nullptr, K, G, d, mode_x, x->plan->dev(), Xs, d, nullptr, xs));
    FDX_TRY(launch_xyt(Xs, Xs, d, K, d, K, XtX_dev, K, nullptr, xs));
    if (KP != K) {
        FDX_TRY(b.dGp.alloc((size_t)KP * KP * sizeof(double)));
        FDX_TRY(solver_pad_square(XtX_dev, K, b.dGp.as<double>(), KP, xs));
    }
    // XtX goes to the host NOW: lambda and the scaled rho are host scalars of the sweeps, and with them known early the solve
    // is queued behind the sketch without the host waiting for it
    if (XtX_host) FDX_HIP(hipMemcpyAsync(XtX_host, XtX_dev, (size_t)K * K * sizeof(double), hipMemcpyDeviceToHost, xs));
    if (done) FDX_TRY(done->record(xs));
    return 0;
}

void x_side_publish(XSide* x, const double* X, const double* XtX_host) {
    if (!x->cacheable || !x->b || x->b->published || !X || !XtX_host) return;
    XSideBufs& b = *x->b;
    const size_t K = (size_t)x->key.K;
    b.X.assign(X, X + x->key.words());
    b.XtX.assign(XtX_host, XtX_host + K * K);
    b.plan = x->plan;
    b.key = x->key;
    b.key.X = b.X.data();
    b.published = true;
    x->cacheable = false;
    x_side_cache().insert(x->b);
}

int queue_rows_to_h(const YSource& y, const YTables& t, long long n, int G, int d, int K, int mode_y, const int* row_map,
                    const double* Xs, double* H, long long ldh, bool time_chunks, RowsToH* out, hipStream_t st) {
    const int32_t dtype = y.row_dtype();
    const SketchPlanDev plan = t.plan ? t.plan->dev() : SketchPlanDev();
    FDX_TRY(out->dRowSq.alloc((size_t)n * sizeof(double)));
    double* row_sq = out->dRowSq.as<double>();
    // The same choice for a fit and for a shard: shards start on multiples of 256, so the fused kernels' groups of 16 spots
    // coincide with those of an unsharded run and H keeps the same bits
    out->fused = y.csr ? t.csr_fused : fused_sketch_contract_ok(dtype, y.ldy, y.dense, G, d, K, mode_y, plan);
    if (out->fused) {
        if (y.csr)     // CSR rows -> LDS accumulators -> MFMA contraction -> H  (csr_kernels.cpp)
            return launch_sketch_csr_contract((const long long*)y.csr->indptr, y.csr->indices, y.csr->data, dtype, row_map, n, d,
                                              mode_y, t.sel, Xs, K, H, ldh, row_sq, st);
        // one kernel, no Y_sketch: rows -> LDS tile -> bucket sums -> MFMA contraction -> H  (tile_sketch_kernel.h)
        return launch_sketch_contract(y.dense, dtype, y.ldy, row_map, n, G, d, mode_y, plan, Xs, K, H, ldh, row_sq, st);
    }
    // Y_sketch is produced and consumed in chunks of 256k rows (1 GB at d = 512): measured on MI355X, smaller chunks
    // (down to Infinity-Cache size) under-fill the chip and are slower, larger ones gain nothing.
    const long long chunk = std::min<long long>(n, SKETCH_CHUNK_ROWS);
    FDX_TRY(out->dYs.alloc((size_t)chunk * d * sizeof(double)));
    double* Ys = out->dYs.as<double>();
    const int n_chunks = (int)((n + chunk - 1) / chunk);
    const int n_timed = time_chunks ? std::min(n_chunks, 64) : 0;             // stage timing from up to 64 chunks, scaled
    std::vector<Event> ev;
    for (int j = 0; j < n_timed * 3; ++j) ev.emplace_back(true);
    int ci = 0;
    for (long long r0 = 0; r0 < n; r0 += chunk, ++ci) {
        const long long nr = std::min(chunk, n - r0);
        if (ci < n_timed) FDX_TRY(ev[(size_t)ci * 3].record(st));
        // with a row map the chunk gathers rows perm[r0..]; without one it reads rows r0.. of Y directly
        if (y.csr) {
            FDX_TRY(launch_sketch_csr((const long long*)y.csr->indptr, y.csr->indices, y.csr->data, dtype,
                                      row_map ? row_map + r0 : nullptr, r0, nr, d, mode_y, t.sel.slots.p, t.sel.bits.as<unsigned>(),
                                      t.sel.sel_words, Ys, d, row_sq + r0, st));
        } else {
            const unsigned char* ybase = static_cast<const unsigned char*>(y.dense);
            if (!row_map) ybase += (size_t)r0 * (size_t)y.ldy * (dtype == FDX_F32 ? 4 : 8);
            FDX_TRY(launch_sketch_rows(ybase, dtype, y.ldy, row_map ? row_map + r0 : nullptr, nr, G, d, mode_y, plan, Ys, d,
                                       row_sq + r0, st));
        }
        if (ci < n_timed) FDX_TRY(ev[(size_t)ci * 3 + 1].record(st));
        FDX_TRY(launch_xyt(Xs, Ys, d, nr, d, K, H + r0, ldh, nullptr, st));
        if (ci < n_timed) FDX_TRY(ev[(size_t)ci * 3 + 2].record(st));
    }
    if (n_timed == 0) return 0;
    FDX_HIP(hipStreamSynchronize(st));
    for (int c = 0; c < n_timed; ++c) {
        out->sketch_ms += ev[(size_t)c * 3 + 1].ms_since(ev[(size_t)c * 3].e);
        out->gram_ms += ev[(size_t)c * 3 + 2].ms_since(ev[(size_t)c * 3 + 1].e);
    }
    const double scale = (double)n_chunks / (double)n_timed;
    out->sketch_ms *= scale;
    out->gram_ms *= scale;
    return 0;
}

int queue_yty(const double* row_sq, long long n, double* sum_dev, double* yty_host, Event* done, hipStream_t st, hipStream_t ys) {
    if (ys != st) {
        Event sketched;                             // released once the wait has consumed it
        FDX_TRY(sketched.record(st));
        FDX_TRY(sketched.wait_on(ys));
    }
    FDX_TRY(launch_sum_partials(row_sq, n, sum_dev, 1, 1, ys));
    if (yty_host) FDX_HIP(hipMemcpyAsync(yty_host, sum_dev, sizeof(double), hipMemcpyDeviceToHost, ys));
    if (done && ys != st) FDX_TRY(done->record(ys));
    return 0;
}

int prepare_queue(PrepareJob* job, const void* Y_dev, int y_dtype, long long n, int G, long long ldy, const int* row_map_dev,
                  const double* X, int K, const int* bucket, const double* weight_y, const double* weight_x, int d, int mode_y_in,
                  int mode_x, double* H_out_dev, long long ldh, double* XtX_host, hipStream_t st, const double* X_dev) {
    const int32_t mode_y = mode_y_in & 0xff;
    TileF64Math f64_math((mode_y_in & FDX_PRE_F64_MATH) != 0);
    FDX_REQUIRE(y_dtype == FDX_F32 || y_dtype == FDX_F64, "fdx_prepare_dev: Y dtype must be FDX_F32 or FDX_F64");
    FDX_REQUIRE(n >= 0 && G > 0 && K > 0 && d > 0, "fdx_prepare_dev: bad shape");
    FDX_REQUIRE(X && bucket && weight_y && weight_x && H_out_dev, "fdx_prepare_dev: null array");
    FDX_REQUIRE(ldh >= n && ldy >= G, "fdx_prepare_dev: leading dimension too small");
    YSource ysrc;
    ysrc.dense = Y_dev;
    ysrc.dtype = y_dtype;
    ysrc.ldy = ldy;
    // The X side (upload of the signatures - a pageable copy: the host waits for it -, X_sketch, XtX and its copy to the host) runs
    // on the library's side stream: queued on the caller's stream behind a shard plan that is still executing, the upload made
    // the host wait for the whole plan and the launches behind it arrived on an idle device (70 us of a 125k-spot rank's 1.6 ms).
    hipStream_t side = fdx::env("FDX_NO_SIDE_STREAM") ? nullptr : library_side_stream();
    if (side == st) side = nullptr;
    job->side = side;
    const hipStream_t xs = side ? side : st;
    {
        PoolStream pool_xs(xs);
        FDX_TRY(job->y.build(ysrc, G, d, K, bucket, weight_y, xs, "fdx_prepare_dev"));
    }
    if (weight_x == weight_y) job->x.plan = job->y.plan;
    FDX_TRY(queue_x_side(&job->x, X, X_dev, K, K, G, d, mode_x, bucket, weight_x, nullptr, XtX_host, &job->evX, xs));
    if (side && job->evX) FDX_TRY(job->evX.wait_on(st));   // the tables, X_sketch, XtX: all behind this one (a cached X side: complete)
    if (n == 0) return 0;
    FDX_REQUIRE(Y_dev != nullptr, "fdx_prepare_dev: null Y");
    FDX_TRY(job->dSum.alloc(sizeof(double)));
    FDX_TRY(queue_rows_to_h(ysrc, job->y, n, G, d, K, mode_y, row_map_dev, job->x.Xs(), H_out_dev, ldh, false,
                            &job->rows, st));
    // the shard's partial YtY only enters the objective: its reduction goes to the side stream (behind the sketch, beside the
    // first sweep) instead of standing between the sketch and the sweeps
    return queue_yty(job->rows.dRowSq.as<double>(), n, job->dSum.as<double>(), nullptr, &job->evSum, st, xs);
}

}  // namespace fdx
