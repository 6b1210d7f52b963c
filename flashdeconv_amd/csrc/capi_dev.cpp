// Device-pointer C-ABI building blocks used by the spot-sharded multi-GPU driver and the stage tests (see include/fdx.h): graph
// builds and their queries, and the stages of a fit one by one - gene moments / column gather, prepare, sweep, objective, spot
// diagnostics, normalise / export.  The analysis entries stand beside their kernels (spatial_stats_kernels.cpp,
// local_stats_kernels.cpp, correlogram_kernels.cpp, niche_kernels.cpp, metrics_kernels.cpp, expression_kernels.cpp).
#include "fdx_env.h"
#include <memory>
#include <vector>

#include "fdx_graph.h"
#include "fdx_internal.h"
#include "fdx_kernels.h"
#include "graph_build.h"
#include "prepare.h"
#include "sketch_plan.h"
#include "solver.h"

using namespace fdx;

extern "C" {

// The graph depends on the coordinates, the method and k / radius and on nothing else of a fit, and one slide is fitted more than
// once: the build is looked up by content first (graph_cache.cpp).  Hit: the entry's graph with one more holder - no binning, no
// k-NN, no symmetrise / ELL / tile kernels, no allocations and no bounding box: the compare kernel is all that runs.  Miss: built
// as before, with an own copy of the coordinates queued on the way and published once the graph is complete.
int fdx_graph_build_dev(const double* coords_dev, int64_t n, int32_t dim, int32_t method, int32_t k, double radius,
                        void* stream, fdx_graph** out) {
    hipStream_t st = (hipStream_t)stream;
    PoolStream pool_stream(st);
    FDX_REQUIRE(out != nullptr, "fdx_graph_build_dev: null output");
    *out = nullptr;
    FDX_REQUIRE(n == 0 || coords_dev != nullptr, "fdx_graph_build_dev: null coords");
    FDX_REQUIRE(method == FDX_GRAPH_KNN || method == FDX_GRAPH_RADIUS, "fdx_graph_build_dev: unknown method");
    hipEvent_t begin = nullptr;                                  // the fit's prologue timer (fdx_fit_info.prologue_ms) starts here
    if (hipEventCreate(&begin) != hipSuccess || hipEventRecord(begin, st) != hipSuccess) {
        if (begin) (void)hipEventDestroy(begin);
        begin = nullptr;
        (void)hipGetLastError();
    }
    struct BeginGuard { hipEvent_t* e; ~BeginGuard() { if (*e) (void)hipEventDestroy(*e); } } begin_guard{&begin};   // until a graph takes it
    const bool cached = n > 0 && dim >= 1 && dim <= 8 && graph_cache_enabled();
    GraphCacheKey key;
    if (cached) {
        key = graph_cache_key(n, dim, method, k, radius);
        fdx_graph* hit = nullptr;
        FDX_TRY(graph_cache_lookup(key, coords_dev, st, &hit));
        if (hit) {
            std::lock_guard<std::mutex> lk(hit->mu);            // re-recorded on every hit: prologue_ms keeps its meaning (build call -> sketch)
            if (hit->begin_event) (void)hipEventDestroy(hit->begin_event);
            hit->begin_event = begin;
            hit->begin_stream = begin ? st : nullptr;
            begin = nullptr;
            *out = hit;
            return 0;
        }
    }
    std::shared_ptr<GraphCacheEntry> entry;
    if (cached) FDX_TRY(graph_cache_entry_new(key, &entry));
    // the entry's copy of the coordinates: queued under the host's wait for the bounding box (no host time on the build's path)
    const std::function<int()> copy = [&]() -> int { return entry ? graph_cache_queue_copy(entry.get(), coords_dev, st) : 0; };
    GraphBuildHooks hooks;
    hooks.under_wait = &copy;
    fdx_graph* g = new fdx_graph();
    g->begin_event = begin;
    g->begin_stream = begin ? st : nullptr;
    begin = nullptr;
    int rc;
    if (method == FDX_GRAPH_KNN) rc = graph_build_knn(coords_dev, n, dim, k, g, st, &hooks);
    else rc = graph_build_radius(coords_dev, n, dim, radius, 0, n, g, st, &hooks);
    if (rc) { delete g; return rc; }                             // (fail() has drained the device: the copy can go)
    g->cache_pending = std::move(entry);
    if (!g->meta_pending) graph_cache_publish(g);                // built to the end here; a queued build: graph_meta_sync publishes
    *out = g;
    return 0;
}

int fdx_side_stream(void** stream_out) {
    FDX_REQUIRE(stream_out != nullptr, "fdx_side_stream: null output");
    *stream_out = (void*)library_side_stream();
    FDX_REQUIRE(*stream_out != nullptr, "fdx_side_stream: the side stream could not be created");
    return 0;
}

int fdx_stream_wait_stream(void* waiter, void* producer) {
    Event ev;                                       // released once the wait has consumed it
    FDX_TRY(ev.record((hipStream_t)producer));
    return ev.wait_on((hipStream_t)waiter);
}

int fdx_graph_build_radius_rows_dev(const double* coords_dev, int64_t n, int32_t dim, double radius, int64_t lo, int64_t hi,
                                    void* stream, fdx_graph** out) {
    PoolStream pool_stream((hipStream_t)stream);
    FDX_REQUIRE(out != nullptr, "fdx_graph_build_radius_rows_dev: null output");
    *out = nullptr;
    FDX_REQUIRE(n == 0 || coords_dev != nullptr, "fdx_graph_build_radius_rows_dev: null coords");
    fdx_graph* g = new fdx_graph();
    const int rc = graph_build_radius(coords_dev, n, dim, radius, lo, hi, g, (hipStream_t)stream);
    if (rc) { delete g; return rc; }
    *out = g;
    return 0;
}

int fdx_graph_knn_lists_dev(const double* coords_dev, int64_t n, int32_t dim, int32_t k, int64_t lo, int64_t hi,
                            int32_t* nbr_dev, int32_t* cnt_dev, void* stream, fdx_graph_plan** plan) {
    PoolStream pool_stream((hipStream_t)stream);
    FDX_REQUIRE(plan != nullptr, "fdx_graph_knn_lists_dev: null output");
    *plan = nullptr;
    FDX_REQUIRE(coords_dev && nbr_dev && cnt_dev, "fdx_graph_knn_lists_dev: null argument");
    return graph_knn_lists(coords_dev, n, dim, k, lo, hi, nbr_dev, cnt_dev, plan, (hipStream_t)stream);
}

int fdx_graph_knn_lists_band_dev(const double* coords_dev, int64_t n, int32_t dim, int32_t k, int64_t lo, int64_t hi,
                                 int32_t* nbr_dev, int32_t* cnt_dev, void* stream, fdx_graph_plan** plan) {
    PoolStream pool_stream((hipStream_t)stream);
    FDX_REQUIRE(plan != nullptr, "fdx_graph_knn_lists_band_dev: null output");
    *plan = nullptr;
    FDX_REQUIRE(coords_dev && nbr_dev && cnt_dev, "fdx_graph_knn_lists_band_dev: null argument");
    return graph_knn_lists(coords_dev, n, dim, k, lo, hi, nbr_dev, cnt_dev, plan, (hipStream_t)stream, true);
}

int fdx_graph_plan_order_dev(const fdx_graph_plan* plan, int32_t* perm_out_dev, int32_t* rank_out_dev, void* stream) {
    FDX_REQUIRE(plan != nullptr, "fdx_graph_plan_order_dev: null plan");
    return graph_plan_order(plan, perm_out_dev, rank_out_dev, (hipStream_t)stream);
}

int fdx_graph_plan_set_lists_dev(fdx_graph_plan* plan, const int64_t* ids_host, const int64_t* rows_host, int64_t n_rows,
                                 int32_t* nbr_dev, int32_t* cnt_dev, void* stream) {
    PoolStream pool_stream((hipStream_t)stream);
    FDX_REQUIRE(plan && nbr_dev && cnt_dev && (n_rows == 0 || ids_host), "fdx_graph_plan_set_lists_dev: null argument");
    return graph_plan_set_lists(plan, (const long long*)ids_host, (const long long*)rows_host, n_rows, nbr_dev, cnt_dev, (hipStream_t)stream);
}

int fdx_graph_plan_set_ckdtree_lists_dev(fdx_graph_plan* plan, const double* coords_host, const double* coords_dev, int64_t n,
                                         int32_t dim, const int64_t* rows_host, int64_t n_rows, int32_t* nbr_dev, int32_t* cnt_dev,
                                         void* stream) {
    hipStream_t st = (hipStream_t)stream;
    PoolStream pool_stream(st);
    FDX_REQUIRE(plan && coords_dev && nbr_dev && cnt_dev, "fdx_graph_plan_set_ckdtree_lists_dev: null argument");   // coords_host NULL: fetched from coords_dev
    FDX_REQUIRE(n >= 1 && dim >= 1 && dim <= 8 && n_rows >= 0 && (n_rows == 0 || rows_host),
                "fdx_graph_plan_set_ckdtree_lists_dev: bad arguments (1 to 8 coordinates)");
    const int kk = graph_plan_kk(plan);
    const long long nq = rows_host ? n_rows : n;
    if (rows_host)
        for (int64_t j = 0; j < n_rows; ++j) FDX_REQUIRE(rows_host[j] >= 0 && rows_host[j] < n, "fdx_graph_plan_set_ckdtree_lists_dev: row index out of range");
    if (nq == 0) return graph_plan_lists_replaced(plan);
    DevBuf d_ids;
    FDX_TRY(d_ids.alloc((size_t)nq * kk * 8));
    try {
        FDX_TRY(ckdtree_lists_device(coords_host, coords_dev, n, dim, kk, (const long long*)rows_host, nq, d_ids.as<long long>(), st));
    } catch (...) {
        return fail(FDX_ERR_INVALID, "fdx_graph_plan_set_ckdtree_lists_dev: out of memory");
    }
    return graph_plan_set_lists_device(plan, d_ids.as<long long>(), (const long long*)rows_host, nq, nbr_dev, cnt_dev, st);
}

int fdx_graph_plan_lists_replaced(fdx_graph_plan* plan) {
    FDX_REQUIRE(plan != nullptr, "fdx_graph_plan_lists_replaced: null plan");
    return graph_plan_lists_replaced(plan);
}

int fdx_graph_knn_far(const fdx_graph* g, int32_t* far) {
    FDX_REQUIRE(g != nullptr && far != nullptr, "fdx_graph_knn_far: null argument");
    FDX_TRY(fdx::graph_meta_sync(g));
    *far = g->knn_far;
    return 0;
}

int fdx_graph_from_knn_lists_dev(fdx_graph_plan* plan, const int32_t* nbr_dev, const int32_t* cnt_dev, int64_t lo, int64_t hi,
                                 void* stream, fdx_graph** out) {
    PoolStream pool_stream((hipStream_t)stream);
    FDX_REQUIRE(plan != nullptr, "fdx_graph_from_knn_lists_dev: null plan");
    int rc = 0;
    fdx_graph* g = nullptr;
    if (!out || !nbr_dev || !cnt_dev) {
        rc = fail(FDX_ERR_INVALID, "fdx_graph_from_knn_lists_dev: null argument");
    } else {
        *out = nullptr;
        g = new fdx_graph();
        rc = graph_from_knn_lists(plan, nbr_dev, cnt_dev, lo, hi, g, (hipStream_t)stream);
    }
    graph_plan_destroy(plan);                      // consumed either way
    if (rc) { delete g; return rc; }
    *out = g;
    return 0;
}

int fdx_graph_perm_dev(const fdx_graph* g, int32_t* perm_out_dev, void* stream) {
    PoolStream pool_stream((hipStream_t)stream);
    if (!(g && g->shard_pending)) FDX_TRY(fdx::graph_meta_sync(g));   // a queued shard build: the copy below is ordered behind it on the stream
    FDX_REQUIRE(g && (g->n == 0 || perm_out_dev), "fdx_graph_perm_dev: null argument");
    return graph_copy_perm(g, perm_out_dev, (hipStream_t)stream);
}

int fdx_graph_localize(const fdx_graph* full, int32_t n_ranks, const int64_t* bounds, int32_t my_rank, void* stream,
                       fdx_graph** local) {
    PoolStream pool_stream((hipStream_t)stream);
    FDX_TRY(fdx::graph_meta_sync(full));
    FDX_REQUIRE(full && bounds && local, "fdx_graph_localize: null argument");
    FDX_REQUIRE(n_ranks >= 1 && my_rank >= 0 && my_rank < n_ranks, "fdx_graph_localize: bad rank");
    FDX_REQUIRE(bounds[0] == 0 && bounds[n_ranks] == full->n, "fdx_graph_localize: bounds must cover [0, n]");
    for (int r = 0; r < n_ranks; ++r) {
        FDX_REQUIRE(bounds[r + 1] >= bounds[r], "fdx_graph_localize: bounds must be non-decreasing");
        FDX_REQUIRE(bounds[r] % 256 == 0, "fdx_graph_localize: range starts must be multiples of 256");
    }
    *local = nullptr;
    fdx_graph* g = new fdx_graph();
    std::vector<long long> b(bounds, bounds + n_ranks + 1);
    const int rc = graph_localize(full, b[(size_t)my_rank], b[(size_t)my_rank + 1], n_ranks, b.data(), my_rank, g,
                                  (hipStream_t)stream);
    if (rc) { delete g; return rc; }
    *local = g;
    return 0;
}

int fdx_graph_shard_knn_dev(const double* coords_dev, int64_t n, int32_t dim, int32_t k, int32_t n_ranks, const int64_t* bounds,
                            int32_t my_rank, void* stream, fdx_graph** local) {
    PoolStream pool_stream((hipStream_t)stream);
    FDX_REQUIRE(coords_dev && bounds && local, "fdx_graph_shard_knn_dev: null argument");
    FDX_REQUIRE(n_ranks >= 1 && my_rank >= 0 && my_rank < n_ranks, "fdx_graph_shard_knn_dev: bad rank");
    *local = nullptr;
    fdx_graph* g = new fdx_graph();
    std::vector<long long> b(bounds, bounds + n_ranks + 1);
    const int rc = graph_shard_knn(coords_dev, n, dim, k, n_ranks, b.data(), my_rank, g, (hipStream_t)stream);
    if (rc) { delete g; return rc; }
    *local = g;
    return 0;
}

int fdx_graph_shard_status(const fdx_graph* local, int64_t* own_nnz, int64_t* knn_ties, int32_t* far, int32_t* overflow) {
    FDX_REQUIRE(local != nullptr, "fdx_graph_shard_status: null graph");
    FDX_TRY(fdx::graph_meta_sync(local));
    if (own_nnz) *own_nnz = local->nnz;
    if (knn_ties) *knn_ties = local->knn_ties;
    if (far) *far = local->knn_far;
    if (overflow) *overflow = local->shard_overflow;
    return 0;
}

// test hook: the stored neighbour indices of one row (positions of this graph's own order; for a local graph own rows are
// 0..n-1 and halo slots n..n_total-1), as the sweeps read them
int fdx_graph_row_indices(const fdx_graph* g, int64_t row, int32_t* idx_out, int32_t cap, int32_t* deg_out) {
    FDX_REQUIRE(g && idx_out && deg_out && row >= 0 && row < g->n, "fdx_graph_row_indices: bad arguments");
    int so = 0, dg = 0;
    FDX_HIP(hipMemcpy(&so, g->slice_off.as<int>() + (row >> 6), 4, hipMemcpyDeviceToHost));
    FDX_HIP(hipMemcpy(&dg, g->deg.as<int>() + row, 4, hipMemcpyDeviceToHost));
    *deg_out = dg;
    for (int m = 0; m < dg && m < cap; ++m)
        FDX_HIP(hipMemcpy(idx_out + m, g->ell.as<int>() + ((size_t)so + m) * 64 + (row & 63), 4, hipMemcpyDeviceToHost));
    return 0;
}

// test hook: which traversal the sweep and the objective take on this graph (tiled = the LDS-tiled kernels of bcd_sweep_inst.cpp)
int fdx_graph_tile_info(const fdx_graph* g, int32_t* n_tiles, int32_t* halo_max, int32_t* tiled) {
    FDX_REQUIRE(g != nullptr, "fdx_graph_tile_info: null graph");
    FDX_TRY(fdx::graph_meta_sync(g));
    if (n_tiles) *n_tiles = g->n_tiles;
    if (halo_max) *halo_max = g->halo_max;
    if (tiled) *tiled = g->tiled ? 1 : 0;
    return 0;
}

int fdx_graph_halo_info(const fdx_graph* local, int64_t* n_halo, int32_t* send_counts, int32_t* recv_counts) {
    FDX_REQUIRE(local != nullptr, "fdx_graph_halo_info: null graph");
    FDX_TRY(fdx::graph_meta_sync(local));
    if (n_halo) *n_halo = local->n_total - local->n;
    const size_t R = local->send_off.empty() ? 0 : local->send_off.size() - 1;
    for (size_t r = 0; r < R; ++r) {
        if (send_counts) send_counts[r] = local->send_off[r + 1] - local->send_off[r];
        if (recv_counts) recv_counts[r] = local->recv_off[r + 1] - local->recv_off[r];
    }
    return 0;
}

int fdx_graph_send_indices_dev(const fdx_graph* local, int32_t* idx_out_dev, void* stream) {
    FDX_REQUIRE(local != nullptr, "fdx_graph_send_indices_dev: null graph");
    FDX_TRY(fdx::graph_meta_sync(local));
    const int total = local->send_off.empty() ? 0 : local->send_off.back();
    if (total == 0) return 0;
    FDX_REQUIRE(idx_out_dev != nullptr, "fdx_graph_send_indices_dev: null output");
    FDX_HIP(hipMemcpyAsync(idx_out_dev, local->send_idx.p, (size_t)total * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

int fdx_prepare_dev(const void* Y_dev, int32_t y_dtype, int64_t n, int32_t G, int64_t ldy, const int32_t* row_map_dev,
                    const double* X, int32_t K, const int32_t* bucket, const double* weight_y, const double* weight_x,
                    int32_t d, int32_t mode_y_in, int32_t mode_x, double* H_out_dev, int64_t ldh, double* XtX_out_dev,
                    double* XtX_out_host, double* YtY_partial_out, void* stream) {
    FDX_REQUIRE(XtX_out_dev != nullptr, "fdx_prepare_dev: null array");
    hipStream_t st = (hipStream_t)stream;
    PoolStream pool_stream(st);
    PrepareJob job;
    // on any return both streams are idle before the job's buffers go back to the pool
    struct Drain { PrepareJob* j; hipStream_t s; ~Drain() { if (j->side) (void)hipStreamSynchronize(j->side); (void)hipStreamSynchronize(s); } } drain{&job, st};
    FDX_TRY(prepare_queue(&job, Y_dev, y_dtype, n, G, ldy, row_map_dev, X, K, bucket, weight_y, weight_x, d, mode_y_in, mode_x,
                          H_out_dev, ldh, XtX_out_host, st));
    // the caller's XtX buffer belongs to the caller's stream: filled there (the stream already waits for the X side)
    FDX_HIP(hipMemcpyAsync(XtX_out_dev, job.x.b->dG.p, (size_t)K * K * sizeof(double), hipMemcpyDeviceToDevice, st));
    double yty = 0.0;
    if (n > 0 && job.evSum) FDX_TRY(job.evSum.wait_on(st));
    if (n > 0) FDX_HIP(hipMemcpyAsync(&yty, job.dSum.p, sizeof(double), hipMemcpyDeviceToHost, st));
    FDX_HIP(hipStreamSynchronize(st));
    if (job.side) FDX_HIP(hipStreamSynchronize(job.side));
    x_side_publish(&job.x, X, XtX_out_host);        // both streams are idle: the X side is complete
    if (YtY_partial_out) *YtY_partial_out = yty;
    return 0;
}

// The same for a CSR shard (core/deconv.py:181-188 sparse log-CPM rule, core/sketching.py:194-199): the own rows stay
// sparse in HBM; gene_idx selects G of the matrix's columns (NULL = all, in order).
int fdx_prepare_csr_dev(const fdx_csr_view* Y, const int32_t* gene_idx, int32_t G, const double* X, int32_t K,
                        const int32_t* bucket, const double* weight_y, const double* weight_x, int32_t d, int32_t mode_y,
                        int32_t mode_x, double* H_out_dev, int64_t ldh, double* XtX_out_dev, double* XtX_out_host,
                        double* YtY_partial_out, void* stream) {
    return fdx_prepare_csr_ex_dev(Y, gene_idx, G, X, K, bucket, weight_y, weight_x, d, mode_y, mode_x, H_out_dev, ldh, XtX_out_dev,
                                  XtX_out_host, YtY_partial_out, nullptr, Y ? Y->n : 0, stream);
}

// ... for n_rows rows of the matrix in the order of row_map_dev (NULL: rows 0..n_rows-1), as a fit passes the graph's solver order
// and a shard a subset; the values of the map are the caller's responsibility, as for fdx_prepare_dev
int fdx_prepare_csr_ex_dev(const fdx_csr_view* Y, const int32_t* gene_idx, int32_t G, const double* X, int32_t K,
                           const int32_t* bucket, const double* weight_y, const double* weight_x, int32_t d, int32_t mode_y,
                           int32_t mode_x, double* H_out_dev, int64_t ldh, double* XtX_out_dev, double* XtX_out_host,
                           double* YtY_partial_out, const int32_t* row_map_dev, int64_t n_rows, void* stream) {
    FDX_REQUIRE(Y != nullptr && Y->n >= 0 && Y->G > 0, "fdx_prepare_csr_dev: bad matrix");
    FDX_REQUIRE(Y->dtype == FDX_F32 || Y->dtype == FDX_F64, "fdx_prepare_csr_dev: dtype must be FDX_F32 or FDX_F64");
    FDX_REQUIRE(G > 0 && K > 0 && d > 0 && (gene_idx || G == Y->G), "fdx_prepare_csr_dev: bad shape");
    FDX_REQUIRE(X && bucket && weight_y && weight_x && H_out_dev && XtX_out_dev, "fdx_prepare_csr_dev: null array");
    FDX_REQUIRE(mode_y == FDX_PRE_RAW || mode_y == FDX_PRE_LOG_CPM_SPARSE, "fdx_prepare_csr_dev: mode_y must be FDX_PRE_RAW or FDX_PRE_LOG_CPM_SPARSE");
    const long long n = n_rows;
    FDX_REQUIRE(n >= 0 && (row_map_dev || n <= Y->n), "fdx_prepare_csr_dev: bad number of rows");
    FDX_REQUIRE(ldh >= n, "fdx_prepare_csr_dev: leading dimension too small");
    hipStream_t st = (hipStream_t)stream;
    PoolStream pool_stream(st);
    YSource ysrc;
    ysrc.csr = Y;
    ysrc.gene_idx = gene_idx;
    YTables tables;
    XSide x;
    RowsToH rows;
    DevBuf dSum;
    // everything on the caller's stream; XtX straight into the caller's buffer
    FDX_TRY(tables.build(ysrc, G, d, K, bucket, weight_y, st, "fdx_prepare_csr_dev"));
    FDX_TRY(queue_x_side(&x, X, nullptr, K, K, G, d, mode_x, bucket, weight_x, XtX_out_dev, nullptr, nullptr, st));
    double yty = 0.0;
    if (n > 0) {
        FDX_TRY(dSum.alloc(sizeof(double)));
        FDX_TRY(queue_rows_to_h(ysrc, tables, n, G, d, K, mode_y, row_map_dev, x.Xs(), H_out_dev, ldh, false, &rows, st));
        FDX_TRY(queue_yty(rows.dRowSq.as<double>(), n, dSum.as<double>(), &yty, nullptr, st, st));
    }
    if (XtX_out_host)
        FDX_HIP(hipMemcpyAsync(XtX_out_host, XtX_out_dev, (size_t)K * K * sizeof(double), hipMemcpyDeviceToHost, st));
    FDX_HIP(hipStreamSynchronize(st));      // the host tables above are stack objects
    if (YtY_partial_out) *YtY_partial_out = yty;
    return 0;
}

int fdx_init_beta_dev(double* beta_dev, int64_t ld, int64_t n_fill, int32_t K, void* stream) {
    FDX_REQUIRE(beta_dev && ld > 0 && K > 0 && n_fill <= ld, "fdx_init_beta_dev: bad arguments");
    return solver_init_beta(beta_dev, ld, n_fill, K, (hipStream_t)stream);
}

int fdx_bcd_sweep_dev(const fdx_graph* g, const double* H_dev, int64_t ldh, const double* XtX_dev, const double* beta_in,
                      double* beta_out, int64_t ld, int32_t K, double lambda, double rho_eff, double tol, int32_t it,
                      void* stats_dev, double* rel_change_dev, void* stream) {
    return fdx_bcd_sweep_ex_dev(g, H_dev, ldh, XtX_dev, beta_in, beta_out, ld, K, lambda, rho_eff, tol, it, stats_dev, rel_change_dev,
                                0.0, nullptr, 0, stream);
}

// test hook: the same sweep with the two forms of the tiled kernel that only whole solves reach otherwise - the first sweep from a
// constant start (INIT) and the sweep over a list of tiles
int fdx_bcd_sweep_ex_dev(const fdx_graph* g, const double* H_dev, int64_t ldh, const double* XtX_dev, const double* beta_in,
                         double* beta_out, int64_t ld, int32_t K, double lambda, double rho_eff, double tol, int32_t it,
                         void* stats_dev, double* rel_change_dev, double init_uniform, const int32_t* tile_list_dev, int32_t n_list,
                         void* stream) {
    FDX_TRY(fdx::graph_meta_sync(g));
    FDX_REQUIRE(g && H_dev && XtX_dev && beta_in && beta_out && stats_dev && rel_change_dev, "fdx_bcd_sweep_dev: null argument");
    FDX_REQUIRE(ld >= g->n_total + 1, "fdx_bcd_sweep_dev: ld must cover own + halo + zero row");
    FDX_REQUIRE(K >= 1 && (sweep_instantiated(K) || K > FDX_MAX_K_PAD),
                "fdx_bcd_sweep_dev: K must be in 1..64, fdx_solver_padded_k of 65..96 cell types, or above 96");
    if (g->n == 0) return 0;
    // above 96 types the whole shard goes in one launch of the LDS-resident or the generic sweep, its scratch prepared per call
    DevBuf scratch;
    size_t scratch_ld = 0;
    {
        PoolStream pool_stream((hipStream_t)stream);
        FDX_TRY(sweep_scratch_prepare(XtX_dev, K, g->n_slices, &scratch, &scratch_ld, (hipStream_t)stream));
    }
    BcdSweepArgs a = sweep_args_for_graph(*g, false);   // (this entry does not look at FDX_NO_TILED)
    a.H = H_dev; a.XtX = XtX_dev; a.beta_in = beta_in; a.beta_out = beta_out;
    a.stats = (unsigned long long*)stats_dev; a.rel_change = rel_change_dev;
    a.lambda = lambda; a.rho = rho_eff; a.tol = tol; a.ldh = (int)ldh; a.ld = (int)ld; a.K = K; a.it = it;
    if (init_uniform != 0.0 || tile_list_dev != nullptr || n_list != 0) {
        // only the tiled kernel knows these forms (launch_k): elsewhere the launch would sweep every spot from beta_in, or not run
        FDX_REQUIRE(bcd_sweep_uses_tiles(a), "fdx_bcd_sweep_ex_dev: init_uniform and tile lists need the tiled sweep");
        FDX_REQUIRE(init_uniform == 0.0 || K <= FDX_MAX_K_FAST, "fdx_bcd_sweep_ex_dev: init_uniform needs K <= 64");
        FDX_REQUIRE((tile_list_dev != nullptr) == (n_list > 0) && (init_uniform == 0.0 || tile_list_dev == nullptr),
                    "fdx_bcd_sweep_ex_dev: a tile list comes with its length, and not together with init_uniform");
        a.init_uniform = init_uniform; a.tile_list = tile_list_dev; a.n_list = n_list;
    }
    return launch_bcd_sweep(a, scratch.as<double>(), scratch_ld, (hipStream_t)stream);
}

int fdx_bcd_fold_dev(void* stats_dev, double* rel_change_dev, int32_t it, void* stream) {
    FDX_REQUIRE(stats_dev && rel_change_dev && it >= 0, "fdx_bcd_fold_dev: bad arguments");
    return launch_bcd_fold_last((const unsigned long long*)stats_dev, rel_change_dev, it, (hipStream_t)stream);
}

int fdx_objective_partials_dev(const fdx_graph* g, const double* beta_dev, int64_t ld, const double* H_dev, int64_t ldh,
                               const double* XtX_dev, int32_t K, double* out4_host, void* stream) {
    FDX_TRY(fdx::graph_meta_sync(g));
    FDX_REQUIRE(g && beta_dev && H_dev && XtX_dev && out4_host, "fdx_objective_partials_dev: null argument");
    hipStream_t st = (hipStream_t)stream;
    PoolStream pool_stream(st);
    out4_host[0] = out4_host[1] = out4_host[2] = out4_host[3] = 0.0;
    if (g->n == 0) return 0;
    DevBuf part, out;
    const int nblk = objective_partials_count(g->n_slices);
    FDX_TRY(part.alloc((size_t)nblk * 4 * sizeof(double)));
    FDX_TRY(out.alloc(4 * sizeof(double)));
    FDX_TRY(solver_objective_partials(*g, beta_dev, ld, H_dev, ldh, XtX_dev, K, part.as<double>(), out.as<double>(), st));
    FDX_HIP(hipMemcpyAsync(out4_host, out.p, 4 * sizeof(double), hipMemcpyDeviceToHost, st));
    FDX_HIP(hipStreamSynchronize(st));
    return 0;
}

int fdx_spot_diagnostics_dev(const fdx_graph* g, const double* beta_dev, int64_t ld, const double* H_dev, int64_t ldh,
                             const double* XtX_dev, int32_t ldg, int32_t K, const double* row_sq_dev, double* out_dev,
                             void* stream) {
    FDX_TRY(fdx::graph_meta_sync(g));
    FDX_REQUIRE(g && beta_dev && H_dev && XtX_dev && row_sq_dev && out_dev, "fdx_spot_diagnostics_dev: null argument");
    FDX_REQUIRE(K >= 1 && ldg >= K, "fdx_spot_diagnostics_dev: K must be positive and ldg at least K");
    FDX_REQUIRE(ld >= g->n_total + 1, "fdx_spot_diagnostics_dev: ld must cover own + halo + zero row");
    FDX_REQUIRE(ldh >= g->n, "fdx_spot_diagnostics_dev: ldh must cover the own spots");
    if (g->n == 0) return 0;
    // a shard's local graph keeps GLOBAL ids in perm: its rows stay in the graph's own order
    const int* perm = g->world_n > 0 ? nullptr : caller_order_perm(g);
    return launch_spot_diagnostics(beta_dev, ld, H_dev, ldh, XtX_dev, ldg, row_sq_dev, g->ell.as<int>(), g->slice_off.as<int>(),
                                   g->deg.as<int>(), perm, (int)g->n, g->n_slices, K, out_dev, (hipStream_t)stream);
}

int fdx_export_dev(const fdx_graph* g, const double* beta_dev, int64_t ld, int32_t K, double* beta_out_dev, double* prop_out_dev,
                   void* stream) {
    FDX_TRY(fdx::graph_meta_sync(g));
    FDX_REQUIRE(g && beta_dev && K > 0, "fdx_export_dev: bad arguments");
    FDX_REQUIRE(ld >= g->n, "fdx_export_dev: ld must cover the own spots");
    FDX_REQUIRE(g->world_n == 0 && g->n_total == g->n, "fdx_export_dev: a shard's local graph is refused (its perm holds global ids)");
    if (g->n == 0) return 0;
    // the export of a fit (fit.cpp): the graph's own perm, null for a graph in the caller's order
    return launch_normalize_export(beta_dev, ld, caller_order_perm(g), (int)g->n, g->n_slices, K, beta_out_dev, prop_out_dev,
                                   (hipStream_t)stream);
}

int fdx_normalize_dev(const double* beta_dev, int64_t ld, int64_t n, int32_t K, double* beta_out_dev, double* prop_out_dev,
                      void* stream) {
    FDX_REQUIRE(beta_dev && n >= 0 && K > 0, "fdx_normalize_dev: bad arguments");
    if (n == 0) return 0;
    return launch_normalize_export(beta_dev, ld, nullptr, (int)n, (int)((n + 63) / 64), K, beta_out_dev, prop_out_dev,
                                   (hipStream_t)stream);
}

}  // extern "C"

extern "C" int fdx_gene_moments_dev(const void* Y_dev, int32_t dtype, int64_t n, int32_t G, int64_t ldy, double* mean_out_host,
                                    double* var_out_host, void* stream) {
    FDX_REQUIRE(Y_dev && mean_out_host && var_out_host && n > 0 && G > 0, "fdx_gene_moments_dev: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    PoolStream pool_stream(st);
    DevBuf scale, part, mean, var;
    FDX_TRY(scale.alloc((size_t)n * 8));
    FDX_TRY(part.alloc((size_t)column_sums_parts(n) * 2 * G * 8));
    FDX_TRY(mean.alloc((size_t)G * 8));
    FDX_TRY(var.alloc((size_t)G * 8));
    FDX_TRY(launch_gene_moments(Y_dev, dtype, ldy, n, G, scale.as<double>(), part.as<double>(), mean.as<double>(), var.as<double>(), st));
    FDX_TRY(copy_d2h(mean_out_host, mean.p, (size_t)G * 8, st));
    FDX_TRY(copy_d2h(var_out_host, var.p, (size_t)G * 8, st));
    return 0;
}

extern "C" int fdx_gather_columns_dev(const void* Y_dev, int32_t dtype, int64_t n, int32_t G, int64_t ldy, const int32_t* idx_host,
                                      int32_t G_sel, void* out_dev, void* stream) {
    FDX_REQUIRE(n >= 0 && G > 0 && G_sel > 0 && idx_host && (n == 0 || (Y_dev && out_dev)), "fdx_gather_columns_dev: bad arguments");
    for (int j = 0; j < G_sel; ++j) FDX_REQUIRE(idx_host[j] >= 0 && idx_host[j] < G, "fdx_gather_columns_dev: column index out of range");
    hipStream_t st = (hipStream_t)stream;
    PoolStream pool_stream(st);
    DevBuf di;
    FDX_TRY(di.alloc((size_t)G_sel * 4));
    FDX_TRY(copy_h2d(di.p, idx_host, (size_t)G_sel * 4, st));
    FDX_TRY(launch_gather_columns(Y_dev, dtype, ldy, n, G, di.as<int>(), G_sel, out_dev, st));
    FDX_HIP(hipStreamSynchronize(st));
    return 0;
}
