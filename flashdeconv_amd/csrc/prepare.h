// The sketch -> H stage (prepare.cpp), one copy for the single-GPU fit (fit.cpp) and for a shard's prepare (capi_dev.cpp, comm.cpp):
// a sharded run is bit-identical to one GPU because both queue the same kernels through these routines.  Internal.
#pragma once
#include <memory>
#include <vector>

#include "fdx_internal.h"
#include "sketch_plan.h"
#include "x_cache.h"

namespace fdx {

// Where the spot rows come from: a dense (n, G) device matrix, or a CSR matrix over csr->G columns of which gene_idx
// (host, G entries; NULL = all columns in order) are the selected genes.
struct YSource {
    const void* dense = nullptr;
    int32_t dtype = FDX_F32;
    int64_t ldy = 0;
    const fdx_csr_view* csr = nullptr;
    const int32_t* gene_idx = nullptr;
    int32_t row_dtype() const { return csr ? csr->dtype : dtype; }
    const void* id() const { return csr ? (const void*)csr->data : dense; }   // whose rows these are (the carry of a stopped fit)
};

// The CountSketch of the Y side on the device: the cached plan of a dense source, or a CSR source's column selection (in the form
// of the fused kernel when that one serves the shape)
struct YTables {
    std::shared_ptr<SketchPlan> plan;
    CsrSelection sel;
    bool csr_fused = false;
    int build(const YSource& y, int G, int d, int K, const int32_t* bucket, const double* weight_y, hipStream_t xs, const char* who);
};

// What the X-side preamble leaves for the rest of a fit: X_sketch (K, d), XtX (K, K), its bordered form (KP, KP) when KP != K, and
// XtX on the host.  It depends on (device, K, KP, G, d, mode_x, the sketch plan, X) and not on Y or the coordinates, so a complete
// one is published in a small content-keyed cache (x_cache.h; FDX_NO_PLAN_CACHE bypasses it) and shared by the fits that follow
// with the same reference X.  Shared ownership: the fit, the carry of a fit that stopped on ties, the cache - an entry evicted
// while in use dies with its last owner.  A published entry is complete (its last event has been waited for), so nothing ever
// waits for one, and its blocks go back to the pool idle: any stream may take them.
struct XSideBufs {
    XCacheKey key;                                 // valid once published; key.X -> X
    std::vector<double> X, XtX;                    // host copies: the key's content, XtX (K, K)
    DevBuf dXs, dG, dGp;
    std::shared_ptr<SketchPlan> plan;              // (keeps the identity the key names alive)
    bool published = false;
    ~XSideBufs() {
        if (published)
            for (DevBuf* b : {&dXs, &dG, &dGp}) b->mark_idle();
    }
};

// X side: plan for weight_x (x->plan when the caller has set it: the Y side's plan for equal weights), upload of the signatures
// unless X_dev has them, X_sketch (K, d), XtX (K, K) into XtX_dev (NULL: b->dG), bordered with zeros to (KP, KP) in b->dGp when
// KP != K, copied to XtX_host when given, `done` recorded when given - all queued on xs, whose pool stream the buffers get.
// With XtX_dev NULL and XtX_host given the cache is asked first.  A hit: x->b is the cached entry, XtX_host is filled before the
// call returns, NOTHING is queued and `done` stays unrecorded.  A miss queues all of it as ever; the caller publishes the entry
// (x_side_publish) once `done` has been waited for.
struct XSide {
    DevBuf dX;
    std::shared_ptr<XSideBufs> b;
    std::shared_ptr<SketchPlan> plan;
    bool cacheable = false;                        // a miss of the cache: to be published
    XCacheKey key;                                 // (key.X: the caller's X, valid during the call only)
    const double* Xs() const { return b->dXs.as<double>(); }
    const double* XtX(int K, int KP) const { return KP != K ? b->dGp.as<double>() : b->dG.as<double>(); }
};
int queue_x_side(XSide* x, const double* X, const double* X_dev, int K, int KP, int G, int d, int mode_x, const int32_t* bucket,
                 const double* weight_x, double* XtX_dev, double* XtX_host, Event* done, hipStream_t xs);
// XtX_host: what queue_x_side filled, now complete.  No-op for a hit, a bypassed cache or an entry already published.
void x_side_publish(XSide* x, const double* X, const double* XtX_host);
void x_side_cache_clear();
void x_side_cache_stats(long long* hits, long long* misses);
// (fit.cpp)
void leverage_cache_clear();
void leverage_cache_stats(long long* hits, long long* misses);

// Rows -> H: columns [0, n) of H (K, ldh) = X_sketch . sketch(row)^T and the rows' squared norms, queued on st.  One kernel where
// the shape has a fused form, else Y_sketch in chunks (dYs) contracted as it is produced.  row_map: optional gather (the fit's
// spot permutation).  time_chunks: the two-kernel path records events per chunk, WAITS for the stream and fills sketch_ms /
// gram_ms (the fit's stage timing); without it nothing is waited for.
struct RowsToH {
    DevBuf dRowSq, dYs;
    bool fused = false;
    double sketch_ms = 0.0, gram_ms = 0.0;
};
int queue_rows_to_h(const YSource& y, const YTables& t, long long n, int G, int d, int K, int mode_y, const int* row_map,
                    const double* Xs, double* H, long long ldh, bool time_chunks, RowsToH* out, hipStream_t st);

// YtY = sum of the rows' squared norms into sum_dev, queued on ys behind the work of st (ys may be st), copied to yty_host and
// `done` recorded on ys where given
int queue_yty(const double* row_sq, long long n, double* sum_dev, double* yty_host, Event* done, hipStream_t st, hipStream_t ys);

// Queued form of a dense shard's "prepare" step: X side on the library's side stream, sketch -> H of the own rows on the
// caller's, the partial ||Y_s||^2 on the side stream again - nothing waited for.
struct PrepareJob {
    XSide x;                                       // x.b->dG: XtX (K, K)
    YTables y;
    RowsToH rows;
    DevBuf dSum;                                   // the shard's partial YtY (one double, valid behind evSum)
    hipStream_t side = nullptr;                    // nullptr: everything on the caller's stream
    Event evX;                                     // X side done (XtX in x.b->dG, and on the host when asked for); unrecorded on a cache hit
    Event evSum;                                   // dSum written (on the side stream when there is one: consumers on another stream wait for it)
};

// Y_dev: (n, G) rows of this shard in solver order (row_map_dev: optional gather).  XtX_host: pinned or pageable, K*K doubles or
// NULL - filled behind job->evX (pageable, or a cached X side: before this returns).  H_out_dev (K, ldh): columns [0, n) written.
int prepare_queue(PrepareJob* job, const void* Y_dev, int y_dtype, long long n, int G, long long ldy, const int* row_map_dev,
                  const double* X, int K, const int* bucket, const double* weight_y, const double* weight_x, int d, int mode_y_in,
                  int mode_x, double* H_out_dev, long long ldh, double* XtX_host, hipStream_t st, const double* X_dev = nullptr);

}  // namespace fdx
