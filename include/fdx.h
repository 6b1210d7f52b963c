/*
 * fdx.h -- C ABI of libfdx.so, the MI355X (gfx950) implementation of FlashDeconv's
 * sketched graph-regularised NNLS hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.  Each entry names the
 * reference function it replaces (paths under flashdeconv/ of cafferychen777/flashdeconv v0.1.6).
 * The reference is pure Python (numpy/scipy/numba); a maintainer binds these with ctypes (see
 * INTEGRATION.md), and flashdeconv_amd/_lib.py is exactly such a binding.
 *
 * Conventions
 *   - Every function returns 0 on success, <0 on failure (FDX_ERR_*); fdx_last_error() returns the
 *     message of the last failure on the calling thread.
 *   - "host" pointers are ordinary C-contiguous arrays owned by the caller; "dev" pointers are HIP device
 *     pointers on the current device (e.g. torch.Tensor.data_ptr()).  The library never frees caller memory.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Device-pointer entry points
 *     only enqueue work on that stream unless stated otherwise; host-pointer entry points are synchronous.
 *   - Device layout of abundances and of H is TYPE-MAJOR: element (type k, spot i) lives at [k*ld + i].
 *     Host-visible results (beta, proportions) are (n_spots, n_types) row-major like the reference.
 *   - Not thread-safe per handle; distinct handles may be used from distinct threads.
 */
#ifndef FDX_H
#define FDX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FDX_OK 0
#define FDX_ERR_INVALID (-1)
#define FDX_ERR_HIP (-2)
#define FDX_ERR_UNSUPPORTED (-3)
#define FDX_ERR_INTERNAL (-4)

/* dtype codes for the spot-by-gene matrix Y */
#define FDX_F32 0
#define FDX_F64 1

/* preprocess modes (core/deconv.py:147-235) */
#define FDX_PRE_RAW 0
#define FDX_PRE_LOG_CPM 1       /* dense rule: log1p(y / (rowsum + 1e-10) * 1e4)   (core/deconv.py:190-191) */
#define FDX_PRE_LOG_CPM_SPARSE 2 /* sparse rule: rowsum 0 -> 1, log1p on stored values (core/deconv.py:183-188) */
/* OR-ed into the mode of a dense FDX_F32 matrix whose values are float32 in STORAGE only (integer counts converted
 * exactly): numpy promotes integer input to float64 in core/deconv.py:190-191, so the transform must stay float64-accurate.
 * Without the flag float32 rows get a float32-class log1p, which is what the reference computes for float32 input. */
#define FDX_PRE_F64_MATH 0x100

int fdx_version(void);
/* Runtime switches (environment variables FDX_*: alternative tested kernel paths and diagnostics, csrc/fdx_env.cpp) are read once,
 * when the library first asks; fdx_env_reload re-reads them.  fdx_env_switch(i, &what): name and description of switch i, NULL
 * past the end of the registry. */
int fdx_env_reload(void);
const char* fdx_env_switch(int32_t i, const char** what_out);
const char* fdx_last_error(void);
int fdx_device_count(int* count);
int fdx_set_device(int device);
int fdx_device_name(char* buf, int buflen);

/* ---- plain device memory helpers (so a ctypes-only binding needs no other GPU runtime) ---------------- */
int fdx_malloc(void** dev_ptr, size_t bytes);
int fdx_free(void* dev_ptr);
/* Device scratch is recycled through a caching pool; fdx_trim() returns every cached block to the driver (and drops the
 * caches below and the graph cache of fdx_graph_build_dev, whose entries own device blocks). */
int fdx_trim(void);
/* What depends on the signature matrix X alone is kept by content, at most 4 entries each: the leverage scores (fdx_leverage_*)
 * and the X side of a fit (X_sketch, XtX: fdx_fit_dev, fdx_fit_csr_dev, fdx_prepare_dev, fdx_shard_fit_dev).  A hit returns what
 * the first computation produced, bit for bit; FDX_NO_PLAN_CACHE bypasses both.  out: {leverage hits, leverage misses, X-side
 * hits, X-side misses} since the library was loaded (bypassed calls count as neither). */
int fdx_x_cache_stats(int64_t out[4]);
int fdx_memcpy_h2d(void* dev_dst, const void* host_src, size_t bytes, void* stream);
int fdx_memcpy_d2h(void* host_dst, const void* dev_src, size_t bytes, void* stream);
int fdx_memset(void* dev_dst, int value, size_t bytes, void* stream);
int fdx_stream_sync(void* stream);

/* ---- caller (pageable) memory <-> HBM for the matrices a fit is handed (core/deconv.py:237-243: Y is an ndarray or a scipy
 * matrix of any numeric dtype; core/deconv.py:190-191, 229: numpy promotes it to float64 on the host) --------------------------- */
/* element type of a host source array */
#define FDX_SRC_F32 0
#define FDX_SRC_F64 1
#define FDX_SRC_I8 2
#define FDX_SRC_U8 3
#define FDX_SRC_I16 4
#define FDX_SRC_U16 5
#define FDX_SRC_I32 6
#define FDX_SRC_U32 7
#define FDX_SRC_I64 8
#define FDX_SRC_U64 9
/* `count` elements of type src_code at src_host -> FDX_F32 / FDX_F64 elements at dst_dev: a team of host threads copies (integer
 * counts: converts - the reference's astype on the host) chunk by chunk into recycled pinned buffers, every chunk's DMA queued as
 * soon as it is filled.  max_abs_out (may be NULL): largest |value| of an integer source (is float32 exact?).  Returns with the
 * data in HBM; work queued on `stream` before the call is waited for first. */
int fdx_upload_convert_dev(void* dst_dev, int32_t dst_dtype, const void* src_host, int32_t src_code, int64_t count,
                           double* max_abs_out, void* stream);
/* bytes from HBM to caller memory through the same ring (beta_ / proportions_: core/deconv.py:395-398 are host arrays) */
int fdx_download_dev(void* dst_host, const void* src_dev, size_t bytes, void* stream);
/* GB/s of ONE pinned copy of `bytes` over the box's link (to_device != 0: host to device) - the yardstick for the two above */
int fdx_pinned_copy_rate(size_t bytes, int32_t to_device, double* gbps_out);

/* ---- preprocess + sketch (replaces core/deconv.py:147-235 and core/sketching.py:160-206) ------------- */
/* Y_sketch = f(Y) @ Omega for host arrays.  Y is (n, G) row-major of `dtype`; Omega (G x d) is given in CSC form
 * (col_ptr int64[d+1], gene_idx int32[nnz] ascending per column, weight f64[nnz]); `mode` is FDX_PRE_*.
 * For "pearson" pass FDX_PRE_RAW with the weights already divided by sigma_g (core/deconv.py:199-225).
 * Ys_out is (n, d) f64.  This is project_to_sketch(Y_tilde, ., Omega) when mode = FDX_PRE_RAW. */
int fdx_sketch(const void* Y, int32_t dtype, int64_t n, int32_t G, const int64_t* col_ptr, const int32_t* gene_idx,
               const double* weight, int32_t d, int32_t mode, double* Ys_out);
/* Host-only inspection of the gather schedule the tile kernel (csrc/tile_sketch_kernel.h) runs for a CountSketch
 * (core/sketching.py:58-74: gene g -> bucket gene_bucket[g] with weight gene_w[g]; -1 = gene not in Omega): buckets are
 * dealt to NW waves x JW groups x 4 lane classes, genes are cut into column blocks of GB.  No device call is made, so
 * tests can replay the schedule on the CPU.  dims_out[4] = {blocks, table entries, steps, steps of the busiest wave};
 * the tables are returned when slot_bucket_out is non-NULL: slot_bucket (NW*JW*4), len (NW*blocks*JW),
 * ent_base (NW*(blocks+1)), w / off (entries; cap_entries = capacity of w_out and off_out). */
int fdx_tile_schedule(const int32_t* gene_bucket, const double* gene_w, int32_t G, int32_t d, int32_t NW, int32_t JW,
                      int32_t GB, int32_t* dims_out, int32_t* slot_bucket_out, uint8_t* len_out, int32_t* ent_base_out,
                      double* w_out, uint16_t* off_out, int64_t cap_entries);
/* Which kernels fdx_prepare_dev / fdx_fit_dev run for the sketch -> H stage of a DENSE matrix with these arguments (Y_dev
 * may be NULL: only its 16-byte alignment matters; mode_y as for fdx_prepare_dev): *path_out = 0 the two-kernel path
 * (sketch_rows_* + contraction), 1 the narrow and 2 the wide form of the tile kernel.  For the tile forms dims_out[6]
 * (may be NULL) = {consumer waves, loader waves, groups per wave, type tiles, genes per column block, column blocks}.
 * The answer comes from the functions the launch itself calls (the cached plan of the Omega, the runtime switches), so
 * it builds and caches that plan; no kernel is launched.  Tests state the path they mean to cover with it. */
int fdx_sketch_path(int32_t y_dtype, const void* Y_dev, int64_t ldy, int32_t G, int32_t d, int32_t K, int32_t mode_y,
                    const int32_t* bucket, const double* weight_y, int32_t* path_out, int32_t* dims_out);
/* The same question for a CSR matrix (fdx_prepare_csr_dev / fdx_fit_dev with sparse rows) of G_all columns, n_sel of them selected,
 * values of `dtype`, mode FDX_PRE_RAW or FDX_PRE_LOG_CPM_SPARSE: *path_out = 0 the scatter kernel (rows -> Y_sketch) and the
 * contraction, 1 the fused kernel.  dims_out[8]: path 1 {blocks of 256 buckets, type tiles, 64-entry register slots of a row, slots
 * fetched ahead of the contraction, keep-buffer entries per wave (follows FDX_CSR_KEEP_CAP), weight / bucket by rank in LDS?, spots
 * of one trip of the whole grid, LDS bytes}; path 0 {rows (waves) per workgroup, rows of one trip of the whole grid, rows per
 * Y_sketch chunk, LDS bytes, 0...}.  Answered by the functions the dispatch and the launches call; no device is needed. */
int fdx_sketch_csr_path(int32_t dtype, int32_t G_all, int32_t n_sel, int32_t d, int32_t K, int32_t mode, int32_t* path_out,
                        int32_t* dims_out);
/* out[i] = log1p(y[i] * scale) exactly as the fused sketch kernel evaluates the log-CPM transform (core/deconv.py:190-191)
 * for FLOAT32 rows with every argument in [0, 32000): float32-class (the reference computes this step in float32 for
 * float32 input, numpy dtype rules), v_log_f32 plus a first-order correction of the rounding of 1 + x.  Host arrays;
 * accuracy tests call this, nothing else does. */
int fdx_log1p_f32(const float* y, float scale, int64_t n, float* out);
/* Per-gene column sums of a host (n, G) matrix (pearson's mean: core/deconv.py:207-214). */
int fdx_column_sums(const void* Y, int32_t dtype, int64_t n, int32_t G, double* sums_out);

/* Same column sums for a matrix already resident on the device (ld = row stride in elements). */
int fdx_column_sums_dev(const void* Y_dev, int32_t dtype, int64_t n, int32_t G, int64_t ldy, double* sums_out_host,
                        void* stream);

/* ---- gene selection support (utils/genes.py:18-145 select_hvg, core/deconv.py:321 gene subset) --------------- */
/* Per-gene mean and ddof-1 variance of log1p(y / max(rowsum,1) * 1e4) over the n spots of a device matrix (the
 * statistics select_hvg ranks genes by; utils/genes.py:85-102 and :52-83).  Host outputs of G doubles each. */
int fdx_gene_moments_dev(const void* Y_dev, int32_t dtype, int64_t n, int32_t G, int64_t ldy, double* mean_out_host,
                         double* var_out_host, void* stream);
/* out[r, j] = Y[r, idx[j]]: the gene subset Y[:, gene_idx] (core/deconv.py:321) as a dense (n, G_sel) device matrix of
 * the same dtype.  idx_host: G_sel int32 column indices. */
int fdx_gather_columns_dev(const void* Y_dev, int32_t dtype, int64_t n, int32_t G, int64_t ldy, const int32_t* idx_host,
                           int32_t G_sel, void* out_dev, void* stream);

/* ---- leverage scores (replaces utils/genes.py:238-290 compute_leverage_scores) ------------------------ */
/* X is the HOST (K, G) row-major reference signature matrix restricted to the selected genes; lev_out (G) receives
 * the normalised leverage scores.  One-sided Jacobi SVD of the centred G x K matrix on the device. */
int fdx_leverage_scores(const double* X, int32_t K, int32_t G, double regularization, double* lev_out);
/* Split form: begin enqueues the job on a library-owned side stream and returns; end waits, copies the scores to
 * lev_out and frees the job.  The kernel is a single workgroup, so a caller can build the spatial graph on its own
 * stream between the two calls (core/deconv.py:305-318 and :358 have no data dependence).  X may be released after
 * begin returns. */
typedef struct fdx_leverage_job fdx_leverage_job;
int fdx_leverage_begin(const double* X, int32_t K, int32_t G, double regularization, fdx_leverage_job** job);
int fdx_leverage_end(fdx_leverage_job* job, double* lev_out);
/* fdx_leverage_end that hands the job's device copy of X to the caller instead of releasing it (*x_dev_out: K x G float64, to be
 * returned with fdx_free): a fit that follows needs the same matrix on the device (fdx_shard_fit_params.X_dev). */
int fdx_leverage_end_keep(fdx_leverage_job* job, double* lev_out, double** x_dev_out);
/* fdx_leverage_begin with a choice of who queues the job's upload and launches: queue_async != 0 - the library's helper thread (the
 * caller returns at once and has ~75 us more for its own launches: fdx_leverage_begin does this); 0 - the calling thread (for a caller
 * that collects the scores right away). */
int fdx_leverage_begin_opt(const double* X, int32_t K, int32_t G, double regularization, int32_t queue_async, fdx_leverage_job** job);
/* fdx_leverage_scores on a chosen kernel route (for tests and measurements; neither reads nor fills the content cache):
 *   0  what fdx_leverage_begin + fdx_leverage_end do: Cholesky-QR where it applies, the Jacobi SVD when it refuses the matrix
 *   1  Cholesky-QR alone (2 <= K <= 272); when it refuses, info says so and lev_out is unspecified
 *   2  the streaming Jacobi passes (2 <= K <= 64)
 *   3  the one-workgroup Jacobi kernel (any K)
 * A route that does not apply to K is FDX_ERR_INVALID.  info (8 ints): [0] the route (1, 2 or 3) that produced the scores,
 * [1] 1 when Cholesky-QR refused the matrix, [2] Jacobi passes (route 2) or sweeps (route 3), 0 for Cholesky-QR, [3] 1 when that
 * route finished (Cholesky-QR stood / the passes found nothing left to rotate / the sweeps converged), [4] 1 when route 0 fell back
 * to the Jacobi SVD, [5..7] 0. */
int fdx_leverage_scores_route(const double* X, int32_t K, int32_t G, double regularization, int32_t route, double* lev_out,
                              int32_t* info);

/* ---- spatial graph (replaces utils/graph.py:25-212 and the CSR handling of core/solver.py:363-365) ---- */
typedef struct fdx_graph fdx_graph;

/* From an existing adjacency structure (the `A` argument of core/solver.py:287 bcd_solve): host CSR,
 * int64 indptr (n+1) / indices (nnz); values are ignored (structure only, core/solver.py:157-159).
 * Spots keep their order. */
int fdx_graph_from_csr(const int64_t* indptr, const int64_t* indices, int64_t n, fdx_graph** out);
/* From coordinates, entirely on the device: coords is a HOST (n, dim) row-major f64 array, dim in {1,2,3}.
 *   fdx_graph_build_knn    <- utils/graph.py:25-83  build_knn_graph(coords, k)   (k clamped to n-1, union symmetrised)
 *   fdx_graph_build_radius <- utils/graph.py:86-133 build_radius_graph(coords, radius)
 * Spots are reordered internally (grid-cell order) for locality; every host-visible result uses the caller's order. */
int fdx_graph_build_knn(const double* coords, int64_t n, int32_t dim, int32_t k, fdx_graph** out);
int fdx_graph_build_radius(const double* coords, int64_t n, int32_t dim, double radius, fdx_graph** out);
/* Distance from every spot to its nearest other spot (host in/out, n >= 2): the quantity whose median sets the
 * radius of build_grid_graph (utils/graph.py:163-170). */
int fdx_nearest_distance(const double* coords, int64_t n, int32_t dim, double* dist_out);
/* Adjacency as CSR in the caller's labels: indptr int64[n+1], indices int32[nnz] ascending per row (host outputs;
 * all values of the reference's matrix are 1.0).  Call fdx_graph_info first to size `indices`. */
int fdx_graph_export_csr(const fdx_graph* g, int64_t* indptr, int32_t* indices);
int fdx_graph_destroy(fdx_graph* g);
/* n spots, structural nnz, maximum degree */
int fdx_graph_info(const fdx_graph* g, int64_t* n, int64_t* nnz, int32_t* max_deg);
/* k-NN graphs: the number of spots (of the rows this graph was built for) whose k-th and (k+1)-th nearest neighbours
 * lie at EXACTLY the same distance.  The k-NN set of such a spot is not unique: the reference inherits whatever
 * scipy's cKDTree.query meets first (utils/graph.py:60-63), which depends on the order the spots are listed in; this
 * library keeps the lower spot index.  Regular lattices (Visium-HD bins, k = 6) tie on every spot.  0 for graphs
 * built from a radius or a given adjacency, and for k_neighbors = 63 (no spare slot). */
int fdx_graph_knn_ties(const fdx_graph* g, int64_t* ties);
/* The host tail of select_hvg (utils/genes.py:104-145) on a G-vector of per-gene moments, with numpy's arithmetic (percentile
 * interpolation, pairwise sums): 20 percentile bins of the positive means, z-score of the variance per bin, the mean / dispersion
 * filters, the n_top genes of largest dispersion - ascending indices in idx_out (room for n_top), their number in *n_out.
 * sorted_pos: the n_pos positive means in ascending order (the caller's np.sort).
 * *ambiguous = 1 (nothing written): exactly equal dispersions straddle the cut, or one is NaN - the order numpy's sort leaves them
 * in decides, so the caller runs numpy itself.  Pure host code. */
int fdx_hvg_from_moments(const double* mean, const double* var, int32_t G, const double* sorted_pos, int32_t n_pos, int32_t n_top,
                         double min_mean, double max_mean, double min_disp, int64_t* idx_out, int32_t* n_out, int32_t* ambiguous);
/* Starts the host build of the restated cKDTree of these coordinates (utils/graph.py:60) in a thread of the library's own and
 * returns: the next fdx_graph_plan_set_ckdtree_lists_dev on the SAME coordinates (same pointers, n, dim) takes the tree over
 * instead of building it.  coords_host may be NULL (fetched from coords_dev on the library's side stream).  One pending build per
 * process; the coordinates must stay valid until that call. */
int fdx_ckdtree_prebuild(const double* coords_host, const double* coords_dev, int64_t n, int32_t dim);
/* Host threads the restated cKDTree may use from now on (0: the process's budget): the ranks of one host, each building the tree
 * of the replicated coordinates (utils/graph.py:60), share its cores. */
int fdx_kdtree_set_threads(int32_t threads);
/* Two sizes of the restated tree's build, for the host tests and probes - the tree is the same whatever they are.
 * what 0: nodes of at least `points` points have their passes (bounds, median selection, partition) cut into tasks of the library's
 *         pool of host threads instead of made by one thread (0: the default, 400000);
 * what 1: subtrees of at most `points` points are built on a contiguous copy of their points (negative: the default, 65536;
 *         0: never);
 * what 2: 0 = fdx_graph_plan_set_ckdtree_lists_dev builds the tree on the host's threads even for 1-3 coordinates (default 1: ON
 *         THE DEVICE, csrc/kdtree_build_dev.cpp - the same tree, level by level, a team of threads per node; a tree deeper than
 *         128 levels falls back to the host build by itself). */
int fdx_kdtree_tune(int32_t what, int64_t points);
/* The index array of that tree as the DEVICE build makes it (1-3 coordinates; coords_dev: n x dim doubles on the device):
 * indices_out (host, n) must equal scipy.spatial.cKDTree(coords).indices.  info_out[3] (may be NULL) = {nodes, levels of split
 * nodes, 1 when the build gave up - a selection past introselect's depth budget or a tree deeper than the level cap; the product
 * then builds on the host}.  Tests call this; the fit uses the same build through fdx_graph_plan_set_ckdtree_lists_dev. */
int fdx_ckdtree_indices_dev(const double* coords_dev, int64_t n, int32_t dim, int64_t* indices_out, int32_t* info_out, void* stream);
/* The neighbour lists the REFERENCE gets on such inputs: a host restatement of scipy.spatial.cKDTree(coords) with the
 * constructor's defaults followed by tree.query(coords, k = kk) with p = 2 (utils/graph.py:60-63), reproducing the order in
 * which the library meets equidistant points - hence which of them it returns.  coords: HOST (n, dim) row-major f64,
 * dim 1..8; idx_out: HOST (n, kk) int64, row i = the kk nearest of point i (itself included), nearest first, -1 padded
 * when n < kk; tree_indices_out: optional HOST int64[n], the tree's index array (tests compare it with scipy's).  Pure
 * host code, serial, O(n log n): for the opt-in knn_ties="ckdtree" of the Python driver when fdx_graph_knn_ties() > 0. */
int fdx_ckdtree_knn(const double* coords, int64_t n, int32_t dim, int32_t kk, int64_t* idx_out, int64_t* tree_indices_out);
/* The same tree, queried for the listed points only (rows: HOST int64[n_rows], idx_out: HOST (n_rows, kk), row j = the answer for
 * point rows[j]) - a spot shard asks for its own rows and its band instead of all n.  dim 1..8 for both entries. */
int fdx_ckdtree_knn_rows(const double* coords, int64_t n, int32_t dim, int32_t kk, const int64_t* rows, int64_t n_rows,
                         int64_t* idx_out);

/* ---- solver (replaces core/solver.py:287-428 bcd_solve and everything it calls) ---------------------- */
typedef struct fdx_solve_info {
    int32_t converged;        /* info['converged']        */
    int32_t n_iterations;     /* info['n_iterations']     */
    double final_objective;   /* info['final_objective']  */
    double final_change;      /* info['final_change']     */
    int32_t n_objectives;     /* len(info['objectives']) (0 unless verbose) */
    int32_t reserved;
    double sweep_ms;          /* GPU time of the BCD sweeps (hipEvent), additive diagnostics */
    double total_ms;
} fdx_solve_info;

/* Host-pointer form of bcd_solve(Y_sketch, X_sketch, A, lambda_, rho, max_iter, tol, verbose):
 *   Y_sketch (n, d) row-major f64, X_sketch (K, d) row-major f64, graph built from A.
 *   beta_out (n, K) row-major f64.  rho is the user-facing fraction; it is scaled by mean(diag XtX)
 *   inside, as core/solver.py:359-360 does.  objectives_out (max_iter doubles, may be NULL) receives the
 *   verbose objective trace (core/solver.py:399-404); rel_changes_out (max_iter doubles, may be NULL)
 *   receives rel_change of every executed iteration. */
int fdx_bcd_solve(const fdx_graph* g, const double* Y_sketch, const double* X_sketch, int64_t n, int32_t d,
                  int32_t K, double lambda, double rho, int32_t max_iter, double tol, int32_t verbose,
                  double* beta_out, double* objectives_out, double* rel_changes_out, fdx_solve_info* info);

/* Function-level seams of the solver the reference's own tests import (tests/test_solver.py:7-14):
 *   fdx_gram_xty  <- precompute_gram_matrix (core/solver.py:187-201) and precompute_XtY (:204-223): XtX = Xs Xs^T (K, K),
 *                    H = Xs Ys^T (K, n) row-major; either output may be NULL.  Host arrays, f64 MFMA on the device.
 *   fdx_objective <- compute_objective (core/solver.py:226-284) for host beta (n, K) / H (K, n) and a graph built with
 *                    fdx_graph_from_csr from the structure of A (L = D - A); rho is passed as given (already scaled). */
int fdx_gram_xty(const double* X_sketch, const double* Y_sketch, int64_t n, int32_t d, int32_t K, double* XtX_out,
                 double* H_out);
int fdx_objective(const fdx_graph* g, const double* beta, const double* H, const double* XtX, int64_t n, int32_t K,
                  double YtY, double lambda, double rho, double* obj_out);

/* ---- whole fit (replaces steps 2-6 of FlashDeconv.fit, core/deconv.py:326-398) -------------------------- */
#define FDX_GRAPH_KNN 0
#define FDX_GRAPH_RADIUS 1
#define FDX_GRAPH_GIVEN 2   /* use the fdx_graph passed in */

typedef struct fdx_fit_params {
    int32_t sketch_dim;      /* d */
    int32_t mode_y;          /* FDX_PRE_* applied to Y rows */
    int32_t mode_x;          /* FDX_PRE_RAW or FDX_PRE_LOG_CPM applied to X rows (X always uses the dense rule) */
    int32_t graph_method;    /* FDX_GRAPH_* */
    int32_t k_neighbors;
    int32_t lambda_auto;     /* 1: lambda = 0.005*mean(diag XtX)/max(mean degree,1)  (core/spatial.py:144-192) */
    int32_t max_iter;
    int32_t verbose;
    double radius;
    double lambda_spatial;   /* used when lambda_auto == 0 */
    double rho_sparsity;     /* user-facing fraction, scaled by mean(diag XtX) inside */
    double tol;
    int32_t stop_on_ties;    /* k-NN graphs: 1 = return with info->status = FDX_FIT_TIES before the solve when some spot's k-th neighbour is
                                tied (the caller then rebuilds the graph on the reference's choice, utils/graph.py:60-63, and calls again) */
    int32_t reserved;
    void* carry;             /* NULL, or the info->carry of a call that stopped on ties for the SAME inputs: its sketch -> H stage is taken
                                over instead of being run again (the rebuilt graph keeps the spot order); consumed by the call */
    double* spot_diag_out_dev; /* NULL (a zeroed struct): off.  Otherwise 3 * n doubles on the device: the per-spot diagnostics of
                                fdx_spot_diagnostics_dev for the fitted abundances, planes [residual_sq | sketch_sq | neighbor_sq] in
                                the caller's spot order, queued behind the objective pass and the export (a call that stops on
                                ties writes nothing) */
} fdx_fit_params;
#define FDX_FIT_TIES 3

typedef struct fdx_fit_info {
    fdx_solve_info solve;
    double lambda_used;
    double rho_effective;
    double YtY;
    int64_t nnz;             /* structural non-zeros of the adjacency */
    double graph_ms, sketch_ms, gram_ms, solve_ms, finish_ms, total_ms;   /* hipEvent stage timings */
    /* contiguous device intervals: prologue_ms runs from the first kernel of the graph build (the event fdx_graph_build_dev
     * records at its top, when the graph was built on this stream; otherwise from the top of this call) to the start of the
     * sketch stage; span_ms from that same point to the end of the export, so that
     * prologue_ms + (sketch stage) + solve_ms + finish_ms = span_ms up to event granularity */
    double prologue_ms, span_ms;
    int64_t knn_ties;        /* spots whose k-th and (k+1)-th nearest neighbours are exactly equidistant (k-NN graphs built on the device) */
    int32_t status;          /* 0: fitted; FDX_FIT_TIES: stopped before the solve (stop_on_ties) - nothing but knn_ties / nnz / carry is valid */
    int32_t reserved;
    void* carry;             /* FDX_FIT_TIES: the stopped call's sketch -> H stage, still running on the device when the call returns - hand
                                it to the next fit of the same inputs (params->carry) or release it with fdx_fit_carry_free */
    double diag_ms;          /* hipEvent time of the per-spot diagnostics launch (part of finish_ms and span_ms); 0 when
                                params->spot_diag_out_dev is NULL */
} fdx_fit_info;
/* Releases a carry that no fit consumed (waits for the work it holds). */
int fdx_fit_carry_free(void* carry);

/* Device-resident fit.  Y_dev: (n, G) matrix of `y_dtype` on the device, row stride ldy elements.  X: HOST (K, G)
 * f64 raw signatures (selected genes).  Omega as per-gene tables on the HOST: bucket int32[G] and the two weight
 * vectors weight_y / weight_x f64[G] (they differ only for "pearson", where each carries its own 1/sigma_g).
 * coords_dev: (n, dim) f64 on the device (ignored for FDX_GRAPH_GIVEN).  graph_inout: in for FDX_GRAPH_GIVEN,
 * otherwise receives the graph built here (caller destroys it).  beta_out_dev / prop_out_dev: (n, K) row-major f64
 * on the device in the caller's spot order (either may be NULL).  objectives_out / rel_changes_out: HOST arrays of
 * max_iter doubles (may be NULL).  Synchronous: results are complete on return. */
int fdx_fit_dev(const void* Y_dev, int32_t y_dtype, int64_t n, int32_t G, int64_t ldy, const double* X, int32_t K,
                const int32_t* bucket, const double* weight_y, const double* weight_x, const double* coords_dev,
                int32_t dim, const fdx_fit_params* params, fdx_graph** graph_inout, double* beta_out_dev,
                double* prop_out_dev, double* objectives_out, double* rel_changes_out, fdx_fit_info* info, void* stream);

/* ---- CSR (sparse) spot matrix on the device --------------------------------------------------------------- *
 * The reference accepts scipy.sparse Y and keeps it sparse through gene statistics, log-CPM and the sketch product
 * (utils/genes.py:52-83, core/deconv.py:181-188, core/sketching.py:194-199).  A view holds DEVICE pointers of a
 * canonical CSR matrix with G columns: indptr int64[n+1], indices int32[nnz], data dtype[nnz].                    */
typedef struct fdx_csr_view {
    const int64_t* indptr;
    const int32_t* indices;
    const void* data;
    int32_t dtype;           /* FDX_F32 or FDX_F64 */
    int64_t n;
    int64_t nnz;
    int32_t G;
    int32_t sorted_rows;     /* 1: column indices ascend within every row (canonical CSR) - verified by fdx_csr_check_dev;
                                lets the gene statistics read the indices once instead of once per gene tile */
} fdx_csr_view;

/* Structure check (monotone indptr from 0 to nnz, columns inside [0, G), and the sorted_rows claim if made); call once
 * after an upload, before any kernel indexes with the arrays.  FDX_ERR_INVALID with a message on violation. */
int fdx_csr_check_dev(const fdx_csr_view* Y, void* stream);
/* select_hvg statistics of the sparse branch (utils/genes.py:52-83): z = log1p(y * 1e4 / max(rowsum, 1)) on the stored
 * entries, mean_g = sum z / n, var_g = n/(n-1) * (sum z^2 / n - mean_g^2) clipped at 0; colsum_g = sum y (the "pearson"
 * means of core/deconv.py:207-212 are colsum / n).  HOST outputs of G doubles each; any may be NULL. */
int fdx_csr_gene_moments_dev(const fdx_csr_view* Y, double* mean_out_host, double* var_out_host, double* colsum_out_host,
                             void* stream);
/* fdx_fit_dev for a CSR matrix.  gene_idx: HOST int32[G] selected columns of Y (Y[:, gene_idx], core/deconv.py:321;
 * NULL = all G == Y->G columns); X, bucket, weight_y, weight_x are indexed by position in gene_idx as in fdx_fit_dev.
 * params->mode_y must be FDX_PRE_RAW or FDX_PRE_LOG_CPM_SPARSE (library size over the selected genes, 0 -> 1). */
int fdx_fit_csr_dev(const fdx_csr_view* Y, const int32_t* gene_idx, int32_t G, const double* X, int32_t K,
                    const int32_t* bucket, const double* weight_y, const double* weight_x, const double* coords_dev,
                    int32_t dim, const fdx_fit_params* params, fdx_graph** graph_inout, double* beta_out_dev,
                    double* prop_out_dev, double* objectives_out, double* rel_changes_out, fdx_fit_info* info, void* stream);

/* Per-cell-type signatures from a single-cell reference resident on the device (io/loader.py:114-135 load_reference):
 * X[k, :] = sum (mean = 0) or mean (mean = 1) over the cells of type k.  rows_dev: int32[n] the cell rows sorted by type and,
 * inside a type, ascending (a stable sort of the host-side labels); type_off_dev: int32[K + 1] the ranges of the types in
 * rows_dev.  Rows are added in that order (numpy's axis-0 order) in float64.  X_out_dev: (K, G) float64 on the device. */
int fdx_type_sums_dev(const void* Y_dev, int32_t dtype, int64_t n, int32_t G, int64_t ldy, const int32_t* rows_dev,
                      const int32_t* type_off_dev, int32_t K, int32_t mean, double* X_out_dev, void* stream);
int fdx_type_sums_csr_dev(const fdx_csr_view* Y, const int32_t* rows_dev, const int32_t* type_off_dev, int32_t K, int32_t mean,
                          double* X_out_dev, void* stream);

/* ---- evaluation metrics (replaces utils/metrics.py:12-266; csrc/metrics_kernels.cpp) --------------------------------------- *
 * pred_dev / true_dev: (n, K) row-major device matrices of the same `dtype` (FDX_F32 / FDX_F64), row strides ld_pred / ld_true
 * in elements; arithmetic is float64.  1 <= n, 1 <= K, n * K <= 2^31 - 1.  The results come back to host arrays, so these
 * entries return after the device work is done (one device-to-host copy at the end).  Workspace comes from the library's
 * caching pool (about 1.2 GB at 1M x 30 float64 when Spearman is asked for); fdx_trim() returns it to the driver.
 *
 * stats_host: (K + 1) rows of FDX_METRICS_FIELDS doubles; row k < K is column k, row K is all n * K entries.  Fields: */
#define FDX_MX_SSE 0        /* sum of (pred - true)^2 (metrics.py:36-41) */
#define FDX_MX_SAE 1        /* sum of |pred - true| (metrics.py:63-68) */
#define FDX_MX_SUM_P 2      /* sums of pred / true (the means of metrics.py:208-209) */
#define FDX_MX_SUM_T 3
#define FDX_MX_MIN_P 4      /* min / max ignoring NaN: ptp of _safe_corr (metrics.py:100-103) is max - min unless a NaN ... */
#define FDX_MX_MAX_P 5
#define FDX_MX_MIN_T 6
#define FDX_MX_MAX_T 7
#define FDX_MX_NAN_P 8      /* ... which these flags (1.0 / 0.0) report */
#define FDX_MX_NAN_T 9
#define FDX_MX_N_RARE 10    /* rare-cell counts as exact integers (metrics.py:245-257); also in rare_host */
#define FDX_MX_TP 11
#define FDX_MX_FP 12
#define FDX_MX_FN 13
#define FDX_MX_JSD_SUM 14   /* row K only: sum of the per-spot JSD when jsd_out_dev was given (metrics.py:141-157) */
#define FDX_MX_C_PT 15      /* centred sums of np.corrcoef (metrics.py:110): about the column means (rows < K) or the overall */
#define FDX_MX_C_PP 16      /* means (row K): sum (p - mp)(t - mt), sum (p - mp)^2, sum (t - mt)^2 */
#define FDX_MX_C_TT 17
#define FDX_METRICS_FIELDS 18
/* Spearman selection (metrics.py:104-106, 112-122): per column and / or over pred.flatten() vs true.flatten() */
#define FDX_SPEARMAN_OVERALL 1
#define FDX_SPEARMAN_PER_TYPE 2

/* Moments of a pred / true pair (metrics.py:36-41 compute_rmse, :63-68 compute_mae, :107-122 Pearson compute_correlation,
 * :141-157 compute_jsd, :245-257 compute_rare_cell_detection): stats_host as above; rare_host (may be NULL): int64
 * {n_rare, TP, FP, FN} for `threshold` (rare: 0 < true < threshold; present: pred > threshold / 2); jsd_out_dev (n doubles on
 * the device, NULL = skip the JSD) receives the per-spot JSD with clipping bound `epsilon`. */
int fdx_metrics_moments_dev(const void* pred_dev, const void* true_dev, int32_t dtype, int64_t n, int32_t K, int64_t ld_pred,
                            int64_t ld_true, double threshold, double epsilon, double* jsd_out_dev, double* stats_host,
                            int64_t* rare_host, void* stream);
/* Spearman correlation (metrics.py:104-106 scipy.stats.spearmanr: Pearson of average ranks, ties averaged, -0.0 == +0.0):
 * rho_host[k] for column k (flags & FDX_SPEARMAN_PER_TYPE), rho_host[K] over all entries (flags & FDX_SPEARMAN_OVERALL), NaN
 * where not asked for; clipped to [-1, 1].  The constant / NaN rules of _safe_corr (metrics.py:100-103) are the caller's: a
 * constant column gives NaN here. */
int fdx_metrics_spearman_dev(const void* pred_dev, const void* true_dev, int32_t dtype, int64_t n, int32_t K, int64_t ld_pred,
                             int64_t ld_true, int32_t flags, double* rho_host, void* stream);
/* Both in one device sequence and one copy back (metrics.py:160-217 evaluate_deconvolution). */
int fdx_metrics_evaluate_dev(const void* pred_dev, const void* true_dev, int32_t dtype, int64_t n, int32_t K, int64_t ld_pred,
                             int64_t ld_true, double threshold, double epsilon, int32_t flags, double* jsd_out_dev,
                             double* stats_host, int64_t* rare_host, double* rho_host, void* stream);

/* ---- device-pointer building blocks (spot-sharded multi-GPU driver, flashdeconv_amd/distributed.py) ------- *
 * One process per GPU; the host side (torch.distributed over RCCL) owns the buffers and the halo exchange, these
 * entry points only enqueue kernels on `stream`.  Same reference lines as the single-GPU entries above.           */

/* Graph from coordinates already on the device (method FDX_GRAPH_KNN / FDX_GRAPH_RADIUS).  A k-NN build may return with its
 * last kernels still queued on `stream`; every entry point that takes the graph waits for them (the fit entries order their
 * own stream behind the build when it differs). */
int fdx_graph_build_dev(const double* coords_dev, int64_t n, int32_t dim, int32_t method, int32_t k, double radius,
                        void* stream, fdx_graph** out);
/* The graph depends on the coordinates, the method and k / radius alone, and one slide is fitted more than once: whole graphs are
 * kept by CONTENT of the coordinates (compared on the device as bytes: one ulp, or -0.0 for 0.0, is another slide; never by
 * pointer), at most 2 per device, least recently used out.  fdx_graph_build_dev looks there first: a hit returns the graph the
 * first build produced - the same bits - and queues no build; a miss builds as before and publishes the graph, with an own copy
 * of the coordinates, once it is complete.  Handles are counted: fdx_graph_destroy drops one reference, the cache holds one, and
 * an entry that is evicted or trimmed dies with its last handle.  FDX_NO_PLAN_CACHE bypasses the cache, fdx_trim() drops it.
 * Graphs of spot shards and of fdx_graph_from_csr never enter it.
 * fdx_graph_cache_stats: {hits, misses, entries, device bytes the entries hold}; bypassed calls count as neither hit nor miss. */
int fdx_graph_cache_stats(int64_t out[4]);
/* The library's own non-blocking side stream of the current device (hipStream_t): a graph build queued there runs beside whatever
 * the caller's stream is doing (FlashDeconv.fit with gene selection: beside the gene statistics and the host's ranking). */
int fdx_side_stream(void** stream_out);
/* Work queued on `waiter` from now on starts after everything queued on `producer` so far (event record + stream wait). */
int fdx_stream_wait_stream(void* waiter, void* producer);
/* Spot shards, radius / grid graphs (utils/graph.py:84-212): rows [lo, hi) (solver positions, lo a multiple of 64) of the
 * radius graph, all other rows left empty - the shard's part of fdx_graph_build_dev(FDX_GRAPH_RADIUS).  A radius graph is
 * symmetric by construction (query_pairs, graph.py:115-121), so a shard's own rows need nothing from the other shards; the
 * result goes to fdx_graph_localize like the one of fdx_graph_from_knn_lists_dev. */
int fdx_graph_build_radius_rows_dev(const double* coords_dev, int64_t n, int32_t dim, double radius, int64_t lo, int64_t hi,
                                    void* stream, fdx_graph** out);
/* The same k-NN graph in two phases, so that a spot shard builds only its own rows (utils/graph.py:25-83):
 *   1. knn_lists: every rank bins ALL coordinates (replicated; the Morton order fixes the solver positions) and finds
 *      the k nearest neighbours of solver positions [lo, hi) only.  Rows [lo, hi) of nbr_dev (n x kk int32 solver
 *      positions, -1 padded, kk = min(k, n-1) + 1) and of cnt_dev (n int32) are written; needs n >= 2, k >= 1.
 *   2. the caller all-gathers the rows of the other ranks into the same two arrays (RCCL) - the symmetrisation
 *      A + A^T (graph.py:80-81) needs the lists of every spot that points at an own spot;
 *   3. from_knn_lists: symmetrise, sort and lay out rows [lo, hi) (lo a multiple of 64); rows outside keep degree 0.
 *      The result is a full-size graph that fdx_graph_localize can cut for this rank.  The plan is consumed.
 * With [lo, hi) = [0, n) and no exchange this is fdx_graph_build_dev(FDX_GRAPH_KNN). */
typedef struct fdx_graph_plan fdx_graph_plan;
int fdx_graph_knn_lists_dev(const double* coords_dev, int64_t n, int32_t dim, int32_t k, int64_t lo, int64_t hi,
                            int32_t* nbr_dev, int32_t* cnt_dev, void* stream, fdx_graph_plan** plan);
int fdx_graph_from_knn_lists_dev(fdx_graph_plan* plan, const int32_t* nbr_dev, const int32_t* cnt_dev, int64_t lo, int64_t hi,
                                 void* stream, fdx_graph** out);
/* Phase 1 WITHOUT the exchange ("recompute, don't communicate"): besides the lists of rows [lo, hi) the rank finds the lists of
 * its BAND - the rows outside [lo, hi) that live in grid cells within two cells of a cell holding an own row - and marks every
 * other row of cnt_dev empty.  A row whose k-NN walk stayed within two shells of its own cell (at ~4 points per cell: all but
 * freak rows) can only point at rows at most two cells away, so the band holds every row that can point at an own row, and
 * fdx_graph_from_knn_lists_dev (called directly, step 2 skipped) yields the same rows [lo, hi) bit for bit.  The condition is
 * checked where it can be: every rank reports through fdx_graph_knn_far() of the graph it built whether a walk of one of its
 * OWN rows went further (or its band list overflowed); if any rank reports it (one integer more in the all-reduce of the edge
 * counts), the ranks rebuild by the three steps above.  Cost: own rows + band, plus one 4-byte fill per spot. */
int fdx_graph_knn_lists_band_dev(const double* coords_dev, int64_t n, int32_t dim, int32_t k, int64_t lo, int64_t hi,
                                 int32_t* nbr_dev, int32_t* cnt_dev, void* stream, fdx_graph_plan** plan);
int fdx_graph_knn_far(const fdx_graph* g, int32_t* far);
/* Spot order of a plan of fdx_graph_knn_lists[_band]_dev: perm_out_dev[p] = caller's id at solver position p, rank_out_dev[id] = its
 * position (int32, n entries each, device; either may be NULL).  A band plan lays out only the neighbourhood of its own rows
 * (positions / ids elsewhere are not data). */
int fdx_graph_plan_order_dev(const fdx_graph_plan* plan, int32_t* perm_out_dev, int32_t* rank_out_dev, void* stream);
/* The caller has REPLACED rows of nbr_dev / cnt_dev (e.g. by the reference's choice among equidistant neighbours,
 * fdx_ckdtree_knn): call this before fdx_graph_from_knn_lists_dev so that the symmetrisation counts the lists it is given
 * (a whole-graph plan carries counts its k-NN kernel drew for its own lists). */
int fdx_graph_plan_lists_replaced(fdx_graph_plan* plan);
/* The usual replacement in one call: ids_host (n_rows, kk) int64 = the answers of a k-nearest query in CALLER ids (the point itself
 * usually among them, -1 padded: fdx_ckdtree_knn / fdx_ckdtree_knn_rows), row r for caller id rows_host[r] (NULL: r).  Uploaded and
 * written on the device where the symmetrisation expects them - the row's solver position, neighbours as solver positions, the
 * point itself dropped (utils/graph.py:70-74), -1 padded; includes fdx_graph_plan_lists_replaced.  Rows not listed keep their lists. */
int fdx_graph_plan_set_lists_dev(fdx_graph_plan* plan, const int64_t* ids_host, const int64_t* rows_host, int64_t n_rows,
                                 int32_t* nbr_dev, int32_t* cnt_dev, void* stream);
/* The reference's choice among equidistant neighbours for rows_host (n_rows caller ids; NULL: every spot) in one call: scipy
 * cKDTree's build restated on the host (coords_host), its k-nearest queries answered on the device for 1-3 coordinates (coords_dev:
 * the same (n, dim) float64 array; 4-8 coordinates: on the host's threads), the answers written where the symmetrisation expects
 * them as by fdx_graph_plan_set_lists_dev.  Replaces utils/graph.py:60-74 for those rows. */
int fdx_graph_plan_set_ckdtree_lists_dev(fdx_graph_plan* plan, const double* coords_host, const double* coords_dev, int64_t n,
                                         int32_t dim, const int64_t* rows_host, int64_t n_rows, int32_t* nbr_dev, int32_t* cnt_dev,
                                         void* stream);
/* perm_out_dev[p] = caller's spot id at solver position p (int32, n entries, device). */
int fdx_graph_perm_dev(const fdx_graph* g, int32_t* perm_out_dev, void* stream);
/* Shard of a full graph for rank `my_rank`: own spots are solver positions [bounds[my_rank], bounds[my_rank+1])
 * (range starts must be multiples of 256).  The local graph indexes own spots first, then the halo. */
int fdx_graph_localize(const fdx_graph* full, int32_t n_ranks, const int64_t* bounds, int32_t my_rank, void* stream,
                       fdx_graph** local);
/* The three steps above (band lists -> own rows of the symmetrised graph -> local graph of rank `my_rank`) as ONE queued
 * pipeline: after the bounding box of the coordinates nothing returns to the host - the halo, the local sliced ELL, the tile
 * tables of the sweep, the send lists of every peer and the boundary / interior tile lists are produced on the device, with
 * allocations sized by bounds the host knows.  The call returns with the kernels queued on `stream`; fdx_graph_perm_dev may be
 * queued behind it at once, every other consumer of the graph (and fdx_graph_shard_status) waits for its counts first.
 * 2 <= n_ranks <= 32, 1 to 3 coordinates, this rank must own at least one row; bounds as for fdx_graph_localize.
 * fdx_graph_shard_status: structural non-zeros of the own rows, own rows with a tied k-th neighbour, `far` (a k-NN walk of an own
 * row left its block or the band list overflowed: all-reduce it, and if any rank reports it every rank rebuilds by
 * fdx_graph_knn_lists_dev + exchange), `overflow` (a bound of this pipeline was too small, e.g. hub rows: rebuild this rank's graph
 * by the three stepwise calls - same rows, same order).  Reference: utils/graph.py:25-83 (the rows), core/solver.py:157-166
 * (what makes a shard's halo sufficient). */
int fdx_graph_shard_knn_dev(const double* coords_dev, int64_t n, int32_t dim, int32_t k, int32_t n_ranks, const int64_t* bounds,
                            int32_t my_rank, void* stream, fdx_graph** local);
int fdx_graph_shard_status(const fdx_graph* local, int64_t* own_nnz, int64_t* knn_ties, int32_t* far, int32_t* overflow);
/* Halo bookkeeping of a local graph: n_halo; send_counts[r] own rows rank r needs; recv_counts[r] halo rows owned by r. */
/* test hook: the stored neighbour indices of one row as the sweeps read them (positions in this graph's own order; local graph:
 * own rows 0..n-1, halo slots n..n_total-1); at most cap are written, *deg_out is the row's degree */
int fdx_graph_row_indices(const fdx_graph* g, int64_t row, int32_t* idx_out, int32_t cap, int32_t* deg_out);
/* test hook: the workgroup tiles of the LDS-tiled sweep and objective (tile = 256 consecutive solver positions): their number, the
 * largest halo of a tile, and whether the graph takes the tiled kernels at all (0: every traversal gathers from global memory).
 * Waits for a deferred build.  Any output may be NULL. */
int fdx_graph_tile_info(const fdx_graph* g, int32_t* n_tiles, int32_t* halo_max, int32_t* tiled);
int fdx_graph_halo_info(const fdx_graph* local, int64_t* n_halo, int32_t* send_counts, int32_t* recv_counts);
/* Own local indices to send, grouped by destination rank ascending (sum(send_counts) int32 entries, device). */
int fdx_graph_send_indices_dev(const fdx_graph* local, int32_t* idx_out_dev, void* stream);

/* X_sketch, XtX (device K*K and host copy), H (K, ldh) for `n` rows of Y (row_map_dev: int32 row ids or NULL),
 * and this shard's part of YtY.  core/sketching.py:160-206, core/solver.py:187-223,348. */
int fdx_prepare_dev(const void* Y_dev, int32_t y_dtype, int64_t n, int32_t G, int64_t ldy, const int32_t* row_map_dev,
                    const double* X, int32_t K, const int32_t* bucket, const double* weight_y, const double* weight_x,
                    int32_t d, int32_t mode_y, int32_t mode_x, double* H_out_dev, int64_t ldh, double* XtX_out_dev,
                    double* XtX_out_host, double* YtY_partial_out, void* stream);
/* The same for a shard kept sparse in HBM (scipy.sparse / torch CSR input: core/deconv.py:181-188, core/sketching.py:194-199):
 * Y = the own rows as an fdx_csr_view, gene_idx = the G selected columns (NULL = all); mode_y FDX_PRE_RAW or
 * FDX_PRE_LOG_CPM_SPARSE. */
int fdx_prepare_csr_dev(const fdx_csr_view* Y, const int32_t* gene_idx, int32_t G, const double* X, int32_t K,
                        const int32_t* bucket, const double* weight_y, const double* weight_x, int32_t d, int32_t mode_y,
                        int32_t mode_x, double* H_out_dev, int64_t ldh, double* XtX_out_dev, double* XtX_out_host,
                        double* YtY_partial_out, void* stream);
/* fdx_prepare_csr_dev for n_rows rows of the matrix: column p of H (ldh >= n_rows) is row row_map_dev[p] (int32, device; a fit passes
 * the graph's solver order, a shard a subset).  NULL = rows 0..n_rows-1, n_rows <= Y->n.  The values of the map are the caller's
 * responsibility, as for fdx_prepare_dev.  With (NULL, Y->n) it is fdx_prepare_csr_dev. */
int fdx_prepare_csr_ex_dev(const fdx_csr_view* Y, const int32_t* gene_idx, int32_t G, const double* X, int32_t K,
                           const int32_t* bucket, const double* weight_y, const double* weight_x, int32_t d, int32_t mode_y,
                           int32_t mode_x, double* H_out_dev, int64_t ldh, double* XtX_out_dev, double* XtX_out_host,
                           double* YtY_partial_out, const int32_t* row_map_dev, int64_t n_rows, void* stream);
/* beta[k*ld + i] = 1/K for i < n_fill, 0 beyond (core/solver.py:372 plus the zero pad row). */
int fdx_init_beta_dev(double* beta_dev, int64_t ld, int64_t n_fill, int32_t K, void* stream);
/* One BCD sweep of the own spots of `g` (core/solver.py:104-184).  stats_dev: (max_iter, 128) uint64 slots zeroed by
 * the caller; rel_change_dev: (max_iter) doubles.  Sweep `it` tests sweep it-1's statistics on the device and
 * becomes a no-op once they are below tol, so the caller all-reduces (MAX) slot row it-1 across ranks first.  K: 1..64, the
 * fdx_solver_padded_k size of 65..96 cell types (pad planes all zero), or any number above 96.  A graph without own spots: no-op
 * (the caller folds such a rank's statistics itself: fdx_bcd_fold_dev after every all-reduce). */
int fdx_bcd_sweep_dev(const fdx_graph* g, const double* H_dev, int64_t ldh, const double* XtX_dev, const double* beta_in,
                      double* beta_out, int64_t ld, int32_t K, double lambda, double rho_eff, double tol, int32_t it,
                      void* stats_dev, double* rel_change_dev, void* stream);
/* test hook: fdx_bcd_sweep_dev with the two forms of the tiled sweep that otherwise only whole solves reach.  init_uniform != 0: every
 * old abundance IS that constant and beta_in is not read (the first sweep of a solve; K <= 64).  tile_list_dev (n_list int32 tile
 * numbers, device): only those tiles of 256 solver positions are swept and add to the statistics.  FDX_ERR_INVALID where the graph and
 * K do not take the tiled sweep (fdx_graph_tile_info), for init_uniform above 64 types, and for both extras at once.  With
 * (0, NULL, 0) it is fdx_bcd_sweep_dev. */
int fdx_bcd_sweep_ex_dev(const fdx_graph* g, const double* H_dev, int64_t ldh, const double* XtX_dev, const double* beta_in,
                         double* beta_out, int64_t ld, int32_t K, double lambda, double rho_eff, double tol, int32_t it,
                         void* stats_dev, double* rel_change_dev, double init_uniform, const int32_t* tile_list_dev, int32_t n_list,
                         void* stream);
int fdx_bcd_fold_dev(void* stats_dev, double* rel_change_dev, int32_t it, void* stream);
/* (cross, quad, spatial, l1) partial sums of the objective over the own spots (core/solver.py:269-284), to host. */
int fdx_objective_partials_dev(const fdx_graph* g, const double* beta_dev, int64_t ld, const double* H_dev, int64_t ldh,
                               const double* XtX_dev, int32_t K, double* out4_host, void* stream);
/* Per-spot terms of the objective for the own spots of `g` (additive, not in the reference).  out_dev: 3 * g->n doubles, planes
 *   residual_sq = max(0, row_sq_i - 2 beta_i . h_i + beta_i' XtX beta_i)   ( = ||s_i - beta_i Xs||^2, s_i the sketched row)
 *   sketch_sq   = row_sq_i                                                  ( = ||s_i||^2)
 *   neighbor_sq = 0.5 * sum_{j in N(i)} ||beta_i - beta_j||^2               (0 without neighbours)
 * so that 0.5 sum residual_sq + 0.5 lambda sum neighbor_sq + rho_eff sum beta is the objective of a symmetric graph.  beta_dev
 * (K, ld) and H_dev (K, ldh) type-major and row_sq_dev in the graph's solver order (halo columns of beta_dev are read for the
 * neighbours, ld >= own + halo + 1 as for the sweep; ldh >= own spots); XtX_dev with row stride ldg >= K (the bordered matrix of
 * a padded solve: pass the real K).  Rows of a whole graph are written in the caller's spot order (row perm[i] of
 * fdx_graph_perm_dev); a shard's local graph, whose perm holds global ids, writes its own order.  Asynchronous on `stream`. */
int fdx_spot_diagnostics_dev(const fdx_graph* g, const double* beta_dev, int64_t ld, const double* H_dev, int64_t ldh,
                             const double* XtX_dev, int32_t ldg, int32_t K, const double* row_sq_dev, double* out_dev,
                             void* stream);
/* Spatial autocorrelation of per-spot values over a whole graph (additive, not in the reference).  V_dev: (g->n, K) row-major with
 * row stride ldv >= K, rows in the caller's spot order.  With A the graph's symmetric binary adjacency, to HOST memory:
 *   mean_out[a] = (1/n) sum_i V_ia          m2_out[a] = sum_i Z_ia^2, Z = V - mean          C_out (K, K) row-major = Z' (A Z)
 *   counts_out  = { n, W = sum_i deg_i, sum_i deg_i^2 }
 * from which Moran's I is (n / W) C_aa / m2_a and the bivariate Moran matrix (n / W) C_ab / sqrt(m2_a m2_b).  neighbor_mean_dev
 * (may be NULL): (n, K) row-major DEVICE matrix in the caller's spot order, (sum_j A_ij V_ja) / deg_i, 0 where deg_i = 0.  float64
 * throughout, no floating-point atomics (two calls return the same bits), one host synchronisation.  A shard's local graph is
 * refused. */
int fdx_spatial_autocorr_dev(const fdx_graph* g, const double* V_dev, int64_t ldv, int32_t K, double* mean_out, double* m2_out,
                             double* C_out, int64_t* counts_out, double* neighbor_mean_dev, void* stream);
/* Permutation null of the statistics above (additive, not in the reference).  Permutation r of `seed` is the bijection pi_r of
 * [0, n) that flashdeconv_amd/utils/spatial_stats.py:permutation_indices defines (an 8-round unbalanced Feistel network on
 * max(2, bit_length(n - 1)) bits with the splitmix64 finaliser as round function, cycle-walked below n), evaluated in the kernels:
 * V_pi[i] = V[pi_r(i)] in the caller's spot order, C_r = Z_pi' (A Z_pi).  The call runs the observed pass (mean_out, m2_out, C_out,
 * counts_out as - and bit for bit what - fdx_spatial_autocorr_dev returns), m4_out[a] = sum_i Z_ia^4, then permutations
 * first_perm .. first_perm + n_perm - 1 in batches of B per launch chain (B from a scratch budget of 1 GiB, at most 512 and at
 * most max_batch when that is positive; *batch_out, may be NULL, reports it).  To HOST memory, (K, K) row-major each:
 *   count_ge_out / count_le_out = how many of the call's permutations have C_r >= C_obs / C_r <= C_obs
 *   sum_d_out / sumsq_d_out     = sum over them of d = C_r - C_obs and of d^2, added in permutation order
 * null_dev (may be NULL): (n_perm, K, K) DEVICE array that receives every C_r.  A permutation's C_r does not depend on B, on
 * first_perm or on the call it ran in, so counts of split calls add up exactly.  No floating-point atomics, two calls return the
 * same bits, one host synchronisation.  Refused: a shard's local graph, n >= 2^31 - 128, null pointers, negative counts. */
int fdx_spatial_perm_dev(const fdx_graph* g, const double* V_dev, int64_t ldv, int32_t K, uint64_t seed, int64_t first_perm,
                         int64_t n_perm, int32_t max_batch, double* null_dev, double* mean_out, double* m2_out, double* C_out,
                         int64_t* counts_out, double* m4_out, int64_t* count_ge_out, int64_t* count_le_out, double* sum_d_out,
                         double* sumsq_d_out, int32_t* batch_out, void* stream);
/* out_dev[i] (n int32, DEVICE) = pi_r(i) of `seed` for i < n, by the device function the kernels of fdx_spatial_perm_dev use.
 * Asynchronous on `stream`. */
int fdx_permutation_indices_dev(uint64_t seed, int64_t r, int64_t n, int32_t* out_dev, void* stream);
/* Neighbourhood enrichment of spot labels over a whole graph: join counts and their permutation null (additive, not in the
 * reference).  labels_dev: g->n int32 on the DEVICE in the caller's spot order, each in [-1, C), -1 = not counted; 1 <= C <= 64.
 * With A the graph's symmetric binary adjacency, to HOST memory:
 *   label_counts_out[a] = n_a = #{i : l_i = a}                 pair_out (C, C) row-major = N_ab = #{(i, j) : A_ij = 1, l_i = a, l_j = b}
 *   counts_out          = { n, W = sum_i deg_i, sum_i deg_i^2 }
 * (ordered pairs: N is symmetric and N_aa is twice the number of undirected a-a edges).  Then permutations
 * first_perm .. first_perm + n_perm - 1 of `seed` (pi_r as for fdx_spatial_perm_dev; n_perm = 0: the observed counts only): the
 * labels l^r_i = l[pi_r(i)] - spots labelled -1 are shuffled like any other and never counted - give N^r, in batches of B per
 * launch chain (groups of 8 or 16 permutations, one byte per spot and permutation, as many groups as a scratch budget of 1 GiB
 * holds, at most 64, and at most max_batch permutations when that is positive; *batch_out, may be NULL, reports B).  To HOST
 * memory, (C, C) row-major each:
 *   count_ge_out / count_le_out = how many of the call's permutations have N^r >= N / N^r <= N
 *   sum_d_out / sumsq_d_out     = the float64 sums over them of d = N^r - N and of d^2, added in permutation order
 * null_dev (may be NULL): (n_perm, C, C) int64 DEVICE array that receives every N^r.  Every count is exact; N^r does not depend on
 * B, on max_batch, on first_perm or on the call it ran in, so split calls add up exactly; no floating-point atomics, two calls
 * return the same bits, one host synchronisation.  Refused with a message: a shard's local graph, n >= 2^31 - 128, C outside
 * 1 .. 64, null pointers, negative counts, and - checked on the device, reported after the call - a label outside [-1, C). */
int fdx_label_pair_counts_dev(const fdx_graph* g, const int32_t* labels_dev, int32_t C, uint64_t seed, int64_t first_perm,
                              int64_t n_perm, int32_t max_batch, int64_t* null_dev, int64_t* label_counts_out, int64_t* pair_out,
                              int64_t* counts_out, int64_t* count_ge_out, int64_t* count_le_out, double* sum_d_out,
                              double* sumsq_d_out, int32_t* batch_out, void* stream);
/* Ligand-receptor test between spot groups: per-label gene sums and their label-permutation null (additive, not in the reference;
 * no graph).  Y (n, G) as for fdx_gene_group_sums_dev (dense FDX_F32 / FDX_F64 with row stride ldy on the DEVICE, or a CSR view with
 * rows in any order); labels_dev: n int32 on the DEVICE in [-1, C), -1 = not counted, 1 <= C <= 64; 1 <= n <= 2^24.  HOST inputs:
 * `genes`, S <= 4096 ascending distinct columns of Y, and `pairs` (P, 2) int32 columns (ligand, receptor), every one listed in
 * `genes`, P >= 1 and P * C^2 <= 2^22.  In float64 on the value converted from storage, to HOST memory:
 *   u_out (C, S) = u[c, s] = sum_{i : l_i = c} y[i, genes[s]]      nnz_out (C, S) = #{i : l_i = c, y != 0}      label_counts_out[c] = n_c
 * Then permutations first_perm .. first_perm + n_perm - 1 of `seed` (pi_r as for fdx_spatial_perm_dev; n_perm = 0: the observed
 * part only): the labels l^r_i = l[pi_r(i)] - a spot labelled -1 is shuffled like any other and never counted, so every n_c stays -
 * give u^r, and per (p, a, b) with T^r = (u^r[a, lig_p] / n_a + u^r[b, rec_p] / n_b) * 0.5 (one IEEE division per mean, one
 * addition, one multiplication) and T the same expression of u, to HOST memory, (P, C, C) row-major each:
 *   count_ge_out / count_le_out = how many of the call's permutations have T^r >= T / T^r <= T
 *   sum_d_out / sumsq_d_out     = the float64 sums over them of d = T^r - T and of d * d (the square rounded, then added: no fma),
 *                                 added in permutation order
 * all four 0 where n_a < 1 or n_b < 1.  null_dev (may be NULL): (n_perm, C, S) float64 DEVICE array that receives every u^r.
 * Permutations run in batches of B per launch chain (groups of 16, as many as a scratch budget of 1 GiB holds, at most 64 groups
 * and at most max_batch permutations when that is positive; *batch_out, may be NULL, reports B); the gathered copy of the columns
 * goes in stripes of whole tiles of 16 genes above max_gather_bytes (0: 1 GiB).  Order: a spot's value is added to the cell of its
 * label by a thread that owns the cell, the spots of a segment of 2,048 in ascending order, the segments in ascending order; an
 * exact zero is skipped, which changes no bit.  So u^r depends only on the labels, the column and the permutation - not on B,
 * max_batch, the stripe, the other genes or pairs, first_perm or the call it ran in; split calls add their counts exactly; no
 * floating-point atomics, two calls return the same bits, one host synchronisation.  Refused with a message: null pointers, a bad
 * view / ldy < G / dtype, n, C, S, P out of range, genes not ascending or outside [0, G), a pair's column missing from genes,
 * negative counts, and - checked on the device, reported after the call - a label outside [-1, C). */
int fdx_label_gene_sums_dev(const void* Y_dev, int32_t dtype, int64_t n, int32_t G, int64_t ldy, const int32_t* labels_dev, int32_t C,
                            const int32_t* genes, int32_t S, const int32_t* pairs, int32_t P, uint64_t seed, int64_t first_perm,
                            int64_t n_perm, int32_t max_batch, int64_t max_gather_bytes, double* null_dev, double* u_out, int64_t* nnz_out,
                            int64_t* label_counts_out, int64_t* count_ge_out, int64_t* count_le_out, double* sum_d_out, double* sumsq_d_out,
                            int32_t* batch_out, void* stream);
int fdx_label_gene_sums_csr_dev(const fdx_csr_view* Y, const int32_t* labels_dev, int32_t C, const int32_t* genes, int32_t S,
                                const int32_t* pairs, int32_t P, uint64_t seed, int64_t first_perm, int64_t n_perm, int32_t max_batch,
                                int64_t max_gather_bytes, double* null_dev, double* u_out, int64_t* nnz_out, int64_t* label_counts_out,
                                int64_t* count_ge_out, int64_t* count_le_out, double* sum_d_out, double* sumsq_d_out, int32_t* batch_out,
                                void* stream);
/* Local indicators of spatial association over a whole graph (additive, not in the reference): per spot and column the observed
 * neighbour sum and its conditional-permutation null.  V_dev as for fdx_spatial_autocorr_dev.  DEVICE outputs, rows in the
 * caller's spot order, overwritten:
 *   nbr_sum_dev (n, K) float64 = S_ia = sum_{j in N(i)} V_ja          deg_dev (n) int32 = deg_i
 * and over conditional permutations r = first_perm .. first_perm + n_perm - 1 of `seed`, in which spot i keeps its value and its
 * neighbours are replaced by the deg_i spots flashdeconv_amd/utils/local_stats.py:conditional_indices(seed, r, i, n, deg_i)
 * defines (the bijection of fdx_permutation_indices_dev under the key mix64(key_r + (i + 1) * 0x9e3779b97f4a7c15), the spot
 * itself skipped), S_ia,r their sum added in slot order:
 *   count_ge_dev / count_le_dev (n, K) int32 = #{r: S_r >= S} / #{r: S_r <= S}
 *   sum_d_dev / sumsq_d_dev (n, K) float64   = sum_r d and sum_r d^2, d = S_r - S
 * These four may be NULL if and only if n_perm == 0; n_perm < 2^31.  To HOST memory mean_out, m2_out (K) and counts_out =
 * { n, W, sum_i deg_i^2 }: bit for bit what fdx_spatial_autocorr_dev returns.  No floating-point atomics, no scratch memory, any
 * degree; the counts and sums do not depend on a launch parameter, and those of split calls add up (exactly where the sums are
 * exact).  One host synchronisation.  Refused: null pointers, K < 1, ldv < K, negative counts, a shard's local graph, a graph
 * without device tables, n >= 2^31 - 128. */
int fdx_local_stats_dev(const fdx_graph* g, const double* V_dev, int64_t ldv, int32_t K, uint64_t seed, int64_t first_perm,
                        int64_t n_perm, double* nbr_sum_dev, int32_t* deg_dev, int32_t* count_ge_dev, int32_t* count_le_dev,
                        double* sum_d_dev, double* sumsq_d_dev, double* mean_out, double* m2_out, int64_t* counts_out,
                        void* stream);
/* Spatial correlogram (additive, not in the reference): the sums of fdx_spatial_autocorr_dev per distance band, in one walk over
 * the pairs within the largest radius and with no graph built.  coords_dev: (n, dim) row-major DEVICE, 1 <= dim <= 3; V_dev as
 * for fdx_spatial_autocorr_dev, rows in the order of coords_dev; radii: B HOST values, 0 < r_1 < ... < r_B finite, 1 <= B <= 32.
 * With d_ij = sqrt((dx*dx + dy*dy) + dz*dz), every operation rounded, ordered pairs i != j fall into band 1 where d_ij <= r_1
 * (coincident spots among them) and into band b where r_{b-1} < d_ij <= r_b: the union of bands 1 .. b is the adjacency of the
 * radius graph of r_b, entry for entry.  To HOST memory: mean, m2, m4 (K; m4 may be NULL) as the other entries define them, and
 * per band b with adjacency A_b
 *   C (B, K, K) row-major = Z' A_b Z        W[b] = sum_i deg_{b,i}        sum_deg_sq[b] = sum_i deg_{b,i}^2
 * degree_dev (may be NULL): (n, B) int32 DEVICE, deg_{b,i} in the caller's spot order.  The lag planes of
 * *bands_per_pass_out (may be NULL) bands are in flight at once: what a scratch budget of 1 GiB holds, at most
 * max_bands_per_pass when that is positive; no output depends on it.  The walk examines sum over the grid cells (edge >= r_B)
 * of count(cell) * count(its 3^dim block) candidate pairs: that number is computed first, returned in *candidates_out (may be
 * NULL), and a call where it exceeds max_candidates fails with FDX_ERR_INVALID before any pair is walked.  The candidates are
 * walked once per group of columns and per chunk of bands (ceil(K / KC) * ceil(B / bands per pass) walks; KC columns fit the
 * 16 KB of LDS accumulators of bands-per-pass bands, 16 at the most), so max_candidates = 0 stands for
 * FDX_CORRELOGRAM_MAX_CANDIDATE_WALKS / walks: about ten seconds of walking whatever K and B are.  float64 throughout, no
 * floating-point atomics, grids are functions of the shapes only, two calls return the same bits.  Two host synchronisations
 * behind the binning's: the candidate count and the results. */
#define FDX_CORRELOGRAM_MAX_CANDIDATE_WALKS 1600000000000LL   /* measured: 1.5e11 candidate walks per second at 1M x 30 x 6 */
int fdx_spatial_correlogram_dev(const double* coords_dev, int64_t n, int32_t dim, const double* V_dev, int64_t ldv, int32_t K,
                                const double* radii, int32_t B, int32_t max_bands_per_pass, int64_t max_candidates, double* mean,
                                double* m2, double* m4, double* C, int64_t* W, int64_t* sum_deg_sq, int32_t* degree_dev,
                                int32_t* bands_per_pass_out, int64_t* candidates_out, void* stream);
/* Label co-occurrence by distance band (additive, not in the reference): the join counts of fdx_label_pair_counts_dev in every
 * distance band of fdx_spatial_correlogram_dev, with their label-permutation null, in walks over the pairs within the largest radius
 * and with no graph built.  coords_dev: (n, dim) row-major DEVICE, 1 <= dim <= 3; labels_dev: n int32 on the DEVICE in the order of
 * coords_dev, each in [-1, C), -1 = not counted (and still a spot: it counts in n and in the degrees); 1 <= C <= 64; radii: B HOST
 * values, 0 < r_1 < ... < r_B finite, 1 <= B <= 32.  Distances and bands are the correlogram's, bit for bit: band 1 holds
 * d_ij <= r_1 (d = 0 among them), band b holds r_{b-1} < d_ij <= r_b, ordered pairs i != j.  To HOST memory:
 *   label_counts_out[a] = n_a           pair_out (B, C, C) row-major = N_b[a][c] = #{(i, j) in band b : l_i = a, l_j = c}
 *   deg_sums_out (3, B) = W_b = sum_i deg_{b,i} | sum_i deg_{b,i}^2 | sum_i (sum_{b' <= b} deg_{b',i})^2 (the radius graph of r_b)
 * degree_dev (may be NULL): (n, B) int32 DEVICE, deg_{b,i} in the caller's spot order.  Then permutations
 * first_perm .. first_perm + n_perm - 1 of `seed` (pi_r and l^r_i = l[pi_r(i)] as for fdx_label_pair_counts_dev: the same
 * (seed, r) is the same relabelling) give N^r_b and the running sums Ncum^r_b = sum_{b' <= b} N^r_{b'}; to HOST memory, each
 * (2, B, C, C) row-major with [0] the bands and [1] the running sums, against N_b and Ncum_b:
 *   count_ge_out / count_le_out = how many of the call's permutations have N^r >= N / N^r <= N
 *   sum_d_out / sumsq_d_out     = the float64 sums over them of d = N^r - N and of d^2, added in permutation order
 * null_dev (may be NULL): (n_perm, B, C, C) int64 DEVICE array that receives every N^r_b.  Groups of 8 (C > 32) or 16 permutations
 * share one distance computation per pair; *bands_per_pass_out bands (what 128 KiB of 32-bit bins in LDS hold, at most
 * max_bands_per_pass when that is positive) are counted per walk, *batch_out permutations (what a scratch budget of 1 GiB holds,
 * at most 64 groups, at most max_batch when positive) per launch chain, in at most max_blocks workgroups a group when that is
 * positive (more where the 32-bit bins of a workgroup need them); either pointer may be NULL.  Every count is an exact integer:
 * no output depends on any of the three caps, on first_perm or on the call a permutation ran in, split calls add up exactly, no
 * floating-point atomics, two calls return the same bits.  The guard is the correlogram's: the candidate pairs of a walk are
 * computed first, returned in *candidates_out (may be NULL), and a call where they exceed max_candidates fails with
 * FDX_ERR_INVALID before any pair is walked; max_candidates = 0 stands for FDX_CORRELOGRAM_MAX_CANDIDATE_WALKS / walks with
 * walks = ceil(B / bands per pass) * (1 + ceil(n_perm / batch)).  n <= 1: zeros (count_ge = count_le = n_perm), nothing walked.
 * Refused with a message: null pointers, n >= 2^31 - 128, dim, C, B or the radii out of range, negative counts, a spot with 2^26
 * candidates or more, and - checked on the device, reported after the call - a label outside [-1, C).  Host synchronisations
 * behind the binning's: the candidate count and the results. */
int fdx_label_cooccurrence_dev(const double* coords_dev, int64_t n, int32_t dim, const int32_t* labels_dev, int32_t C,
                               const double* radii, int32_t B, uint64_t seed, int64_t first_perm, int64_t n_perm, int32_t max_batch,
                               int32_t max_bands_per_pass, int32_t max_blocks, int64_t max_candidates, int32_t* degree_dev,
                               int64_t* null_dev, int64_t* label_counts_out, int64_t* pair_out, int64_t* deg_sums_out,
                               int64_t* count_ge_out, int64_t* count_le_out, double* sum_d_out, double* sumsq_d_out,
                               int32_t* batch_out, int32_t* bands_per_pass_out, int64_t* candidates_out, void* stream);
/* out_dev[t] (count int32, DEVICE) = the t-th spot conditional permutation r of `seed` draws for `spot` among n, by the device
 * function the kernel of fdx_local_stats_dev uses; 0 <= spot < n, 0 <= count <= n - 1.  Asynchronous on `stream`. */
int fdx_conditional_indices_dev(uint64_t seed, int64_t r, int64_t spot, int64_t n, int64_t count, int32_t* out_dev, void* stream);
/* k-means of per-spot feature rows (spatial niches; additive, not in the reference).  F_dev: (n, D) row-major DEVICE matrix with
 * row stride ldf >= D (columns D .. ldf - 1 are never read); centres: (C, D) row-major, contiguous, 1 <= C <= 64.  Everywhere
 * d2(i, c) = sum_k (F_ik - M_ck)^2 with the difference formed first, accumulated by fma in ascending k.  float64 throughout, no
 * floating-point atomics, grids and summation orders are functions of the shapes only: two calls return the same bits.  Refused
 * with a message each: null pointers, D < 1, ldf < D, C outside 1 .. 64, n >= 2^31 - 128, and (where the centres are rows of F)
 * C > n.
 *
 * fdx_kmeans_assign_dev: labels_dev[i] (n int32, DEVICE, in/out) = the smallest c attaining min_c d2(i, c); min_d2_dev (n, DEVICE,
 *   may be NULL) that minimum; to HOST memory *changed_out = the rows whose label differs from the buffer's previous content
 *   (exact) and *inertia_out = sum_i d2(i, label_i).  One host synchronisation. */
int fdx_kmeans_assign_dev(const double* F_dev, int64_t ldf, int64_t n, int32_t D, const double* centres_dev, int32_t C,
                          int32_t* labels_dev, double* min_d2_dev, int64_t* changed_out, double* inertia_out, void* stream);
/* To HOST memory: sums_out (C, D) row-major, sums_out[c][k] = sum of F_ik over the rows with labels_dev[i] == c, and counts_out[c]
 * how many there are; a label that never occurs gives zero sums and count 0, labels outside 0 .. C - 1 are skipped.  Any n >= 0;
 * F need not be the matrix the labels came from (a niche's mean composition after clustering on other features). */
int fdx_label_sums_dev(const double* F_dev, int64_t ldf, int64_t n, int32_t D, const int32_t* labels_dev, int32_t C,
                       double* sums_out, int64_t* counts_out, void* stream);
/* One step of k-means++ seeding: d2_dev[i] (n, DEVICE, in/out; +inf before the first centre) = min(d2_dev[i], d2(i, m)) for the
 * new centre m = centre_dev (D doubles on the DEVICE: a row of F, say).  To HOST memory: *block_rows_out = R (a multiple of 256
 * and a function of n only), *n_blocks_out = ceil(n / R) <= 1024 and block_sums_out[b] (room for 1024) = the sum of d2 over rows
 * [b R, (b + 1) R). */
int fdx_kmeans_seed_dist_dev(const double* F_dev, int64_t ldf, int64_t n, int32_t D, const double* centre_dev, double* d2_dev,
                             double* block_sums_out, int64_t* block_rows_out, int32_t* n_blocks_out, void* stream);
/* Lloyd's loop on the caller's stream.  centres_dev (C, D) DEVICE, in: the initial centres, out: the final ones; labels_dev (n
 * int32, DEVICE, out).
 *     labels = -1
 *     for it = 1 .. max_iter:  labels, changed, inertia = assign(F, centres);  changed == 0: converged, stop;  it == max_iter: stop;
 *                              sums, counts = label_sums(F, labels);  centres[c] = sums[c] / counts[c] where counts[c] > 0
 * (an empty niche keeps its centre).  The labels returned are the arg-min of the centres returned; on convergence the centres are
 * also the means of their members.  To HOST memory: counts_out (C) of the labels returned, *inertia_out of the last assign pass,
 * *n_iter_out = assign passes made, *converged_out 1 / 0.  16 bytes are read back per iteration.  max_iter < 1 is refused. */
int fdx_kmeans_dev(const double* F_dev, int64_t ldf, int64_t n, int32_t D, int32_t C, int32_t max_iter, double* centres_dev,
                   int32_t* labels_dev, int64_t* counts_out, double* inertia_out, int32_t* n_iter_out, int32_t* converged_out,
                   void* stream);
/* ---- cell-type expression in tissue (additive, not in the reference; csrc/expression_kernels.cpp) ------------------------------ *
 * Sufficient statistics of the per-gene regressions Y[:, g] ~ W s_g, s_g >= 0, over groups of rows, and the solves.
 *
 * fdx_weighted_gene_sums_dev / _csr_dev: Y (n, G) dense FDX_F32 / FDX_F64 with row stride ldy, or a CSR view whose rows have
 * distinct columns (sorted or not); W_dev (n, K) float64 with row stride ldw >= K, 1 <= K <= 272.  rows_dev: int32 DEVICE, the
 * rows sorted by group and ascending inside a group (a stable sort of the labels), group_off: int32[C + 1] HOST, the ranges of the
 * C >= 1 groups in rows_dev (group_off[0] = 0, ascending; rows left out are simply not listed).  rows_dev == NULL: rows 0 .. n - 1
 * as ONE group (C must be 1, group_off is not read).  With R_c the rows of group c in that order, to DEVICE memory, float64:
 *   A (C, K, K) = sum_i w_i w_i'     B (C, K, G) = sum_i w_i y_i'     q (C, G) = sum_i y_ig^2     u (C, G) = sum_i y_ig
 * The order of every sum is fixed by the data alone: the rows of a group are cut into segments of FDX_EXPRESSION_SEGMENT_ROWS
 * rows, a segment is added row after row (a product and its addition are one fused operation), and the segment sums are added in
 * ascending order.  No floating-point atomics; two calls return the same bits, and so does a call whose launch gives a workgroup
 * more or fewer segments (FDX_EXPR_STRIPE_SEGMENTS) or the genes in more passes.  float32 Y is widened in registers; CSR entries
 * that are not stored add nothing.  Asynchronous on `stream`; the segment sums live in the library's pool (about 1 GiB at a time:
 * beyond that the segments go in batches and the sums continue from the previous batch's, the same bits again), beside a copy
 * of the listed rows of W padded to a multiple of 16 columns. */
#define FDX_EXPRESSION_SEGMENT_ROWS 2048
#define FDX_EXPRESSION_MAX_K 272
int fdx_weighted_gene_sums_dev(const void* Y_dev, int32_t dtype, int64_t n, int32_t G, int64_t ldy, const double* W_dev, int64_t ldw,
                               int32_t K, const int32_t* rows_dev, const int32_t* group_off, int32_t C, double* A_dev, double* B_dev,
                               double* q_dev, double* u_dev, void* stream);
int fdx_weighted_gene_sums_csr_dev(const fdx_csr_view* Y, const double* W_dev, int64_t ldw, int32_t K, const int32_t* rows_dev,
                                   const int32_t* group_off, int32_t C, double* A_dev, double* B_dev, double* q_dev, double* u_dev,
                                   void* stream);
/* Non-negative least squares from the sums, one problem per (group c, gene g): minimise s' A_c s - 2 s' B_c[:, g] over s >= 0 by
 * cyclic coordinate descent from s = 0 with D_k = A_c[k][k] + ridge * (A_c[0][0] + ... + A_c[K-1][K-1]) / K:
 *   sweep it = 1 .. max_iter:  for k = 0 .. K - 1:  new = D_k > 0 ? max(0, (b_k - sum_{j != k} A_c[k][j] s_j) / D_k) : 0
 *   converged after the sweep where max_k |new - s_k| <= tol * max_k s_k.
 * The kernel keeps t = A_c s - b and forms the numerator as A_c[k][k] s_k - t_k (fused), t += A_c[:, k] (new - s_k) (fused): the
 * iterates agree with the dot-product form up to rounding.  A_dev (C, K, K), B_dev (C, K, G), q_dev (C, G; may be NULL) on the
 * DEVICE; to DEVICE memory S (C, K, G), n_iter and converged (C, G) int32, and - where q_dev is given - rss (C, G) =
 * max(0, q - 2 s.b + s' A_c s) with A_c s formed afresh (no ridge in it).  1 <= K <= 272 (A_c in LDS up to 88 types, read through
 * L2 above), ridge >= 0, max_iter >= 1, tol > 0.  Asynchronous on `stream`. */
int fdx_nnls_gram_dev(const double* A_dev, const double* B_dev, const double* q_dev, int32_t C, int32_t K, int32_t G, double ridge,
                      int32_t max_iter, double tol, double* S_dev, int32_t* n_iter_dev, int32_t* converged_dev, double* rss_dev,
                      void* stream);
/* ---- spatially variable genes (additive, not in the reference; csrc/gene_spatial_kernels.cpp) ----------------------------------- *
 * Per gene of Y (n, G) - rows in the CALLER's spot order; dense FDX_F32 / FDX_F64 with row stride ldy >= G, or a CSR view whose rows
 * have distinct columns (sorted or not: sorted_rows is honoured, stored zeros are legal) - the sums from which Moran's I, Geary's
 * C and their moments are assembled, over a WHOLE graph g of n spots (a shard's local graph is refused): A its symmetric binary
 * adjacency, deg_i = sum_j A_ij.  sums_dev: (9, G) row-major float64 on the DEVICE, all arithmetic float64 on the value converted
 * from its storage type:
 *   0 u = sum_i y_i        1 q = sum_i y_i*y_i        2 c3 = sum_i (y_i*y_i)*y_i        3 c4 = sum_i (y_i*y_i)*(y_i*y_i)
 *   4 D = sum_i deg_i*y_i  5 H = sum_i deg_i*(y_i*y_i)
 *   6 P = sum_i y_i*lag_i, lag_i = sum_{j in N(i)} y_j added in the graph's stored neighbour order
 *   7 ymin = min_i y_i     8 ymax = max_i y_i
 * A CSR entry that is not stored is the value 0: it adds nothing to planes 0-6 and takes part in min / max exactly when its column
 * stores fewer than n entries.  deg_dev: NULL, or n int32 on the DEVICE, deg_i in the caller's order.  counts_out (HOST) =
 * {n, W = sum deg, sum deg^2}, what fdx_spatial_autocorr_dev returns.  n = 0: zeros, NaN in planes 7 and 8.
 * The order of every sum is fixed by the graph alone: its positions (position p holds the caller's spot perm[p]) are cut into
 * segments of FDX_GENE_SPATIAL_SEGMENT_POSITIONS, a segment is added position after position and the segment sums are added in
 * ascending order.  No floating-point atomics; two calls return the same bits, and so does a call whose launch gives a workgroup
 * more or fewer segments (FDX_EXPR_STRIPE_SEGMENTS) or keeps fewer segment sums in flight (they live in the library's pool, about
 * 1 GiB at a time: beyond that the segments go in batches and the sums continue from the previous batch's).  One host
 * synchronisation, for counts_out.  Refused with a message: null pointers, G < 1, ldy < G, n other than the graph's, n >= 2^31 - 128. */
#define FDX_GENE_SPATIAL_SEGMENT_POSITIONS 256
int fdx_gene_spatial_sums_dev(const fdx_graph* g, const void* Y_dev, int32_t dtype, int64_t n, int32_t G, int64_t ldy,
                              double* sums_dev, int32_t* deg_dev, int64_t* counts_out, void* stream);
int fdx_gene_spatial_sums_csr_dev(const fdx_graph* g, const fdx_csr_view* Y, double* sums_dev, int32_t* deg_dev, int64_t* counts_out,
                                  void* stream);
/* ---- gene-pair spatial co-expression (additive, not in the reference; csrc/gene_pair_kernels.cpp) -------------------------------- *
 * Per pair (a, b) of columns of Y (n, G) - Y, g, deg_i and counts_out as for fdx_gene_spatial_sums_dev; lag_g,i = sum_{j in N(i)} y_jg
 * added in the graph's stored neighbour order - the sums from which the bivariate Moran's R, Pearson's r and the exact permutation
 * variances of R are assembled.  pairs: P x 2 int32 on the HOST, row p = (a_p, b_p) with 0 <= a_p, b_p < G; a_p == b_p and
 * repeated rows are legal.  sums_dev: (17, P) row-major float64 on the DEVICE, all arithmetic float64 on the value converted from its
 * storage type:
 *   0 ua = sum_i y_a     1 ub = sum_i y_b     2 qa = sum_i y_a*y_a     3 qb = sum_i y_b*y_b     4 Da = sum_i deg_i*y_a     5 Db = sum_i deg_i*y_b
 *   6 S = sum_i y_a*y_b  7 Xab = sum_i y_a*lag_b                       8 Xba = sum_i y_b*lag_a
 *   9 La = sum_i lag_a*lag_a     10 Lb = sum_i lag_b*lag_b     11 DLa = sum_i deg_i*lag_a     12 DLb = sum_i deg_i*lag_b
 *   13 amin = min_i y_a     14 amax = max_i y_a     15 bmin = min_i y_b     16 bmax = max_i y_b
 * A CSR entry that is not stored is the value 0, a stored zero a value like any other.  n = 0: zeros, NaN in planes 13-16.
 * The order of every sum is that of fdx_gene_spatial_sums_dev (segments of FDX_GENE_SPATIAL_SEGMENT_POSITIONS positions, folded in
 * ascending order; no floating-point atomics; the same bits from two calls, from another FDX_EXPR_STRIPE_SEGMENTS and from fewer
 * segment sums in flight), and A PAIR'S SEVENTEEN NUMBERS DEPEND ONLY ON THE GRAPH AND ITS TWO COLUMNS: not on the other pairs of the
 * call, their order, or - CSR - on how the call was cut.  The CSR entries gather the distinct genes of a chunk of consecutive pairs
 * into a dense (n, S) matrix of the storage type in the library's pool and run the dense kernels on it; the chunks are cut so that
 * n * S * sizeof(dtype) <= max_gather_bytes (0: about 1 GiB), one pair a chunk at the least.
 * The local entries write, for every spot i (the CALLER's order) and pair p, to out_dev[i * ldo + p] (float64, DEVICE, ldo >= P)
 *   coef_p * [ (y_a,i - mean_a_p) (lag_b,i - mean_b_p deg_i) + (y_b,i - mean_b_p) (lag_a,i - mean_a_p deg_i) ]
 * from mean_a_dev, mean_b_dev, coef_dev (P float64 each, DEVICE); asynchronous on `stream`, no host synchronisation.
 * Refused with a message: what fdx_gene_spatial_sums_dev refuses, P < 1 ("P must be at least 1"), an index outside [0, G) ("pair
 * index out of range"), ldo < P. */
int fdx_gene_pair_sums_dev(const fdx_graph* g, const void* Y_dev, int32_t dtype, int64_t n, int32_t G, int64_t ldy, const int32_t* pairs,
                           int32_t P, double* sums_dev, int64_t* counts_out, void* stream);
int fdx_gene_pair_sums_csr_dev(const fdx_graph* g, const fdx_csr_view* Y, const int32_t* pairs, int32_t P, int64_t max_gather_bytes,
                               double* sums_dev, int64_t* counts_out, void* stream);
int fdx_gene_pair_local_dev(const fdx_graph* g, const void* Y_dev, int32_t dtype, int64_t n, int32_t G, int64_t ldy, const int32_t* pairs,
                            int32_t P, const double* mean_a_dev, const double* mean_b_dev, const double* coef_dev, double* out_dev,
                            int64_t ldo, void* stream);
int fdx_gene_pair_local_csr_dev(const fdx_graph* g, const fdx_csr_view* Y, const int32_t* pairs, int32_t P, int64_t max_gather_bytes,
                                const double* mean_a_dev, const double* mean_b_dev, const double* coef_dev, double* out_dev, int64_t ldo,
                                void* stream);
/* ---- spatial gene modules: all-pairs co-expression (additive, not in the reference; csrc/gene_module_kernels.cpp) ----------------- *
 * For S distinct columns `genes` (int32 on the HOST, 1 <= S <= 4096) of Y (n, G) - Y, g, deg_i, lag and counts_out as for
 * fdx_gene_pair_sums_dev - the raw sums of every pair of them, all arithmetic float64 on the value converted from its storage type:
 *   gene_sums_dev (6, S) row-major, DEVICE:   0 u = sum_i y    1 D = sum_i deg_i*y    2 L = sum_i lag*lag    3 DL = sum_i deg_i*lag
 *                                             4 ymin           5 ymax
 *   cross_dev (2, S, S) row-major, DEVICE:    0 S_ab = sum_i y_a,i*y_b,i           1 X_ab = sum_i y_a,i*lag_b,i
 * (a, b: places in `genes`), so sum y_a^2 = S_aa and sum y_a*lag_a = X_aa; entry for entry the planes S, Xab, Xba, ua, Da, La, DLa,
 * amin, amax of fdx_gene_pair_sums_dev.  A CSR entry that is not stored is the value 0.  n = 0: zeros, NaN in planes 4 and 5.
 * The columns are first gathered into a dense (n, S_pad) matrix of the storage type in the graph's order (S_pad: S rounded up to a
 * multiple of 64) - one matrix, never chunked, refused above max_gather_bytes (0: 16 GiB).  The graph's positions are then cut into
 * SPLITS of split_segments segments of FDX_GENE_SPATIAL_SEGMENT_POSITIONS positions (0: 16 segments); a split is summed position
 * after position - the matrices on the float64 matrix cores, four positions an instruction; the per-gene sums in four quarter sums,
 * quarter w over the positions [64 w, 64 w + 64) of every segment of the split, added in the order w = 0 .. 3 - and the split sums
 * are added in ascending order.
 * Order: no floating-point atomics; two calls return the same bits; so does a call with fewer split sums in flight; EVERY NUMBER
 * DEPENDS ONLY ON THE GRAPH, ITS ONE OR TWO COLUMNS AND split_segments - not on which other genes are listed or on their order; S is
 * bitwise symmetric.  Another split_segments moves the boundaries at which the sums are reassociated: other roundings, and no
 * change where every partial sum is exactly representable.
 * The score entries write, for every spot i (the CALLER's order) and module c < C, to out_dev[i * ldo + c] (float64, DEVICE)
 *   sum over the genes s with label[s] == c, in the order of `genes`, of  y_s,i * scale_dev[s] - shift_dev[s]
 * label: S int32 on the HOST, -1: the gene takes no part; scale_dev, shift_dev: S float64 each on the DEVICE; a module without
 * genes scores 0.  Asynchronous on `stream`.
 * Refused with a message: what fdx_gene_spatial_sums_dev refuses, then "S must be in [1, 4096]", "gene index out of range",
 * "gene listed twice", "gathered matrix needs <bytes> bytes, max_gather_bytes is <bytes>", and for the scores "ldo < C",
 * "C must be at least 1", "label outside [-1, C)". */
int fdx_gene_coexpr_sums_dev(const fdx_graph* g, const void* Y_dev, int32_t dtype, int64_t n, int32_t G, int64_t ldy, const int32_t* genes,
                             int32_t S, int32_t split_segments, int64_t max_gather_bytes, double* gene_sums_dev, double* cross_dev,
                             int64_t* counts_out, void* stream);
int fdx_gene_coexpr_sums_csr_dev(const fdx_graph* g, const fdx_csr_view* Y, const int32_t* genes, int32_t S, int32_t split_segments,
                                 int64_t max_gather_bytes, double* gene_sums_dev, double* cross_dev, int64_t* counts_out, void* stream);
int fdx_gene_module_scores_dev(const fdx_graph* g, const void* Y_dev, int32_t dtype, int64_t n, int32_t G, int64_t ldy, const int32_t* genes,
                               const int32_t* label, int32_t S, int32_t C, const double* scale_dev, const double* shift_dev,
                               double* out_dev, int64_t ldo, void* stream);
int fdx_gene_module_scores_csr_dev(const fdx_graph* g, const fdx_csr_view* Y, const int32_t* genes, const int32_t* label, int32_t S,
                                   int32_t C, int64_t max_gather_bytes, const double* scale_dev, const double* shift_dev, double* out_dev,
                                   int64_t ldo, void* stream);
/* ---- permutation test per gene for Moran's I and Geary's C (additive, not in the reference; csrc/gene_perm_kernels.cpp) ------------ *
 * For S distinct columns `genes` (int32 on the HOST, S >= 1) of Y (n, G) - Y, g, deg_i and counts_out = {n, W, sum deg^2} as for
 * fdx_gene_spatial_sums_dev - and the permutations pi_r of fdx_spatial_perm_dev (utils/spatial_stats.py:permutation_indices of
 * `seed`), r = first_perm .. first_perm + n_perm - 1, with v_i = y[pi_r(i)] in the CALLER's spot order, all arithmetic float64 on
 * the value converted from its storage type:
 *   null_dev (n_perm, 3, S) row-major, DEVICE (may be NULL when n_perm = 0):
 *       0 P_r = sum_i v_i * sum_{j in N(i)} v_j        1 D_r = sum_i deg_i*v_i        2 H_r = sum_i deg_i*v_i*v_i
 *   obs_dev (7, S) row-major, DEVICE:   0 u = sum y   1 q = sum y*y   2 D   3 H   4 P (the identity in place of pi_r)   5 ymin   6 ymax
 * A CSR entry that is not stored is the value 0.  n = 0: zeros, NaN in planes 5 and 6, and no permutation kernel is launched; nor
 * is one for n_perm = 0 (the observed planes only).
 * The columns are gathered once, in the storage type and the graph's order, into tiles of TILE genes (position-major inside a
 * tile; genes in STRIPES of whole tiles, one tile at the least, when the copy would exceed max_gather_bytes - 0: about 1 GiB);
 * per permutation of a BATCH a table of n int32 - the
 * position whose value lands at each position - is computed once and shared by every gene (max_batch caps the batch, 0: what
 * about 1 GiB of tables holds).  A workgroup owns a tile and a range of the batch's permutations; by how much LDS the tile needs
 * against max_lds_bytes (0: the device's 160 KiB per workgroup) a call takes one ROUTE:
 *   2  the tile's columns and the permutation's table in LDS (TILE = the largest of 4, 2, 1 - float64: of 2, 1 - with
 *      TILE*elem*n + 4*n bytes fitting)
 *   1  one column in LDS, the table read through L2        0  columns and table read through L2 (any n), TILE = 4 (float64: 2)
 * On route 2 the LDS left beside the tile holds up to four tables, and every 256 threads of a workgroup walk a permutation of their
 * own (WAYS); a workgroup takes CHUNK permutations of the batch, never fewer than it has ways.
 * info_out (6 int64 on the HOST, may be NULL): {TILE, batch, route, stripes, ways and chunk of the first permutation launch}.
 * Order: no floating-point atomics; thread t of 256 adds the graph's positions p = t, t + 256, ... in ascending order, a
 * neighbour sum in the stored neighbour order, and a fixed tree combines the 256 partial sums - so EVERY (gene, permutation) SUM
 * DEPENDS ONLY ON THE GRAPH, THE COLUMN AND THE PERMUTATION: not on the tile, the ways, the batch, the stripe, the route, the other genes,
 * their order or max_batch; two calls and a range of permutations split into several calls return the same bits.
 * One host synchronisation (the counts).  Refused with a message: what fdx_gene_spatial_sums_dev refuses ("null argument",
 * "ldy < G", "dtype must be FDX_F32 or FDX_F64", "G must be at least 1", "Y has <n> rows but the graph has <m> spots"), then
 * "S must be at least 1", "gene index out of range", "gene listed twice", "first_perm must not be negative", "n_perm must not be
 * negative", "max_batch must not be negative", "max_lds_bytes must not be negative", "max_gather_bytes must not be negative". */
int fdx_gene_spatial_perm_dev(const fdx_graph* g, const void* Y_dev, int32_t dtype, int64_t n, int32_t G, int64_t ldy, const int32_t* genes,
                              int32_t S, uint64_t seed, int64_t first_perm, int64_t n_perm, int64_t max_batch, int64_t max_lds_bytes,
                              int64_t max_gather_bytes, double* obs_dev, double* null_dev, int64_t* counts_out, int64_t* info_out,
                              void* stream);
int fdx_gene_spatial_perm_csr_dev(const fdx_graph* g, const fdx_csr_view* Y, const int32_t* genes, int32_t S, uint64_t seed,
                                  int64_t first_perm, int64_t n_perm, int64_t max_batch, int64_t max_lds_bytes, int64_t max_gather_bytes,
                                  double* obs_dev, double* null_dev, int64_t* counts_out, int64_t* info_out, void* stream);
/* ---- marker genes of spot groups: rank-sum and Welch sums per (group, gene) (additive, not in the reference; ----------------------- *
 * csrc/gene_group_kernels.cpp).  Y (n, G) as for fdx_weighted_gene_sums_dev (dense FDX_F32 / FDX_F64 with row stride ldy, or a CSR
 * view with rows in any order; an entry that is not stored is the value 0), n <= FDX_GENE_GROUP_MAX_ROWS; labels_dev: n int32 on the
 * DEVICE in [-1, C), -1 leaves the spot out; 1 <= C <= 256.  With N the number of used spots, n_c the size of group c and a gene's
 * values compared as converted to float64 from their storage type (all 64 bits of a float64 count), to DEVICE memory:
 *   u_dev, q_dev (C, G) float64   sum y, sum y*y over group c: the planes u and q of fdx_weighted_gene_sums_dev called with W = 1 and
 *                                 the rows sorted stably by label, bit for bit (the same pass runs)
 *   nnz_dev (C, G) int64          spots of group c with y != 0 (-0.0 and a stored zero are zeros)
 *   R2_dev (C, G) int64           sum over the spots i of group c of 2 * midrank_i, midrank_i the 1-based average rank of y_ig among
 *                                 the N used values of gene g (ties share the mean of their ranks)
 *   T_dev (G) int64               sum over the tie runs of gene g's N used values of t^3 - t, t the run's length
 * and to HOST memory n_c_out (C) and *N_out.  The integers are exact, so any accumulation order gives the same bits (integer
 * atomics carry them; no floating-point atomic anywhere).  Zeros are never sorted: the nonzeros of a STRIPE of consecutive genes are
 * compacted, sorted by value and then stably by gene (rocPRIM radix sorts), and the zero run's ranks follow from the counts.  The
 * stripes are cut from the per-gene counts so that keys, payloads and sort workspace - 24 bytes an entry for float32, 32 for float64,
 * plus rocPRIM's - stay within max_sort_bytes (0: about 1 GiB), one gene a stripe at the least; a stripe never changes a result.
 * info_out (HOST, may be NULL): {stripes, entries of the largest stripe, bytes of its ranking workspace}.  NaN in Y is not
 * supported.  Two host synchronisations (the group sizes, the per-gene counts).  Refused with a message: what
 * fdx_weighted_gene_sums_dev refuses of Y, "C must be 1 .. 256", "at most 2000000 rows" (sum t^3 - t stays below 2^63),
 * "max_sort_bytes < 0", "a label lies outside [-1, C)". */
#define FDX_GENE_GROUP_MAX_ROWS 2000000
int fdx_gene_group_sums_dev(const void* Y_dev, int32_t dtype, int64_t n, int32_t G, int64_t ldy, const int32_t* labels_dev, int32_t C,
                            int64_t max_sort_bytes, double* u_dev, double* q_dev, int64_t* nnz_dev, int64_t* R2_dev, int64_t* T_dev,
                            int64_t* n_c_out, int64_t* N_out, int64_t* info_out, void* stream);
int fdx_gene_group_sums_csr_dev(const fdx_csr_view* Y, const int32_t* labels_dev, int32_t C, int64_t max_sort_bytes, double* u_dev,
                                double* q_dev, int64_t* nnz_dev, int64_t* R2_dev, int64_t* T_dev, int64_t* n_c_out, int64_t* N_out,
                                int64_t* info_out, void* stream);
/* beta (K, ld) type-major -> beta_out / prop_out (n, K) row-major in solver order of the own spots. */
int fdx_normalize_dev(const double* beta_dev, int64_t ld, int64_t n, int32_t K, double* beta_out_dev, double* prop_out_dev,
                      void* stream);
/* The export pass of a fit on its own (core/solver.py:431-452 fused with the layout change): beta (K, ld) type-major in the solver
 * order of the whole graph `g` -> beta_out / prop_out (g->n, K) row-major at row perm[i] of fdx_graph_perm_dev, i.e. in the caller's
 * spot order (a graph in the caller's order: row i).  Either output may be NULL (not written).  A shard's local graph is refused:
 * fdx_normalize_dev serves it.  Asynchronous on `stream`. */
int fdx_export_dev(const fdx_graph* g, const double* beta_dev, int64_t ld, int32_t K, double* beta_out_dev, double* prop_out_dev,
                   void* stream);

/* ---- native sharded solve: the per-iteration loop on RCCL directly (csrc/comm.cpp) -------------------------- *
 * The reference has no distributed code; sharding spots is legal because the sweep is Jacobi across spots
 * (core/solver.py:157-166 reads only the previous iterate).  One process per GPU:
 *   rank 0:  fdx_comm_unique_id(id)  -> ship the 128 bytes to every rank (any side channel)
 *   all:     fdx_comm_init(id, rank, world, &comm)          (ncclCommInitRank; librccl is loaded with dlopen here)
 *            fdx_graph_localize(...) for `world` ranks, fdx_prepare_dev(...) for the own rows
 *            fdx_sharded_solve_dev(comm, local_graph, H, XtX, ...)
 * Per iteration: boundary tiles swept first, their rows packed (one kernel) and sent / received with grouped
 * ncclSend / ncclRecv on a communication stream while the interior tiles are swept, halo unpacked (one kernel),
 * ncclAllReduce(max) of the iteration's 128 convergence slots.  Same bits and iteration count as fdx_bcd_solve on the
 * unsharded problem.  fdx_local_world_* / fdx_comm_init_local: the same loop with host threads of ONE process as ranks
 * on one GPU (device copies through a shared mailbox) - for tests, no RCCL involved.  When one thread rank leaves a solve with
 * an error the world is marked aborted (the others return "another rank failed" instead of waiting for ever) and STAYS so:
 * destroy it and create a new one. */
typedef struct fdx_comm fdx_comm;
typedef struct fdx_local_world fdx_local_world;
int fdx_comm_unique_id(void* id_out_128);
int fdx_comm_init(const void* id_128, int32_t rank, int32_t world, fdx_comm** out);
int fdx_local_world_create(int32_t world, fdx_local_world** out);
/* One rank of a `world`-rank job ALONE: fdx_sharded_solve_dev runs its complete loop (boundary tiles, pack, interior tiles
 * beside the copy, unpack, stopping rule, chunked read-backs) with the exchange replaced by a device copy of the rank's own
 * staging and no all-reduce - the time of a rank's critical path without wire time (bench.py --virtual-ranks: the projected
 * speed-up of a job this build could not run on N GPUs).  The halo values are NOT those of the job: results are meaningless,
 * run it with tol = 0 and max_iter = the iteration count of the real solve. */
int fdx_comm_init_loopback(int32_t rank, int32_t world, fdx_comm** out);
int fdx_local_world_destroy(fdx_local_world* w);
int fdx_comm_init_local(fdx_local_world* w, int32_t rank, fdx_comm** out);
int fdx_comm_destroy(fdx_comm* comm);
int fdx_comm_info(const fdx_comm* comm, int32_t* rank, int32_t* world);
/* Ranks RCCL itself reports for this communicator (ncclCommCount); 0 for the in-process / loopback transports. */
int fdx_comm_rccl_count(const fdx_comm* comm, int32_t* count);
/* In-place sum over the ranks of `count` device doubles (YtY, objective partials, nnz, per-gene moment sums). */
int fdx_comm_allreduce_sum_dev(fdx_comm* comm, double* buf_dev, int32_t count, void* stream);
/* One rank's WHOLE fit behind a plan queued by fdx_graph_shard_knn_dev (or any local graph): X_sketch / XtX, sketch -> H of the
 * own rows (Y_dev: the own rows in the order of fdx_graph_perm_dev), the plan's counts all-reduced over the ranks while the sketch
 * runs, lambda (core/spatial.py:181-190), the iteration loop of fdx_sharded_solve_dev, the objective (its sums and YtY in one
 * all-reduce) and the export - core/deconv.py:326-398 for one shard, one call, no host round trip between the stages.
 * status != 0: nothing was solved and the caller applies the remedy - FDX_SHARD_FAR (some rank's k-NN walk left its block: every
 * rank rebuilds its graph by the list exchange), FDX_SHARD_OVERFLOW (a bound of some rank's queued plan was too small: the ranks
 * rebuild by the stepwise calls), FDX_SHARD_TIES (stop_on_ties set and some k-th neighbour is tied: the reference's order is the
 * caller's to establish).  nnz_total >= 0: the job's edge count (the graph was not built by the queued plan); 1 to 96 cell types. */
typedef struct {
    int32_t sketch_dim, mode_y, mode_x, lambda_auto, max_iter, stop_on_ties;
    double lambda_spatial, rho_sparsity, tol;
    int64_t n_total_spots, nnz_total;
    const double* X_dev;          /* optional: X already on the device (K x G row-major float64, e.g. from fdx_leverage_end_keep): not uploaded again */
} fdx_shard_fit_params;
typedef struct {
    int32_t status, reserved;
    int64_t nnz_total, knn_ties_total, own_nnz, n_halo;
    double lambda_used, rho_effective, YtY;
    fdx_solve_info solve;
} fdx_shard_fit_info;
#define FDX_SHARD_FAR 1
#define FDX_SHARD_OVERFLOW 2
#define FDX_SHARD_TIES 3
int fdx_shard_fit_dev(fdx_comm* comm, const fdx_graph* local, const void* Y_dev, int32_t y_dtype, int64_t n_own, int32_t G,
                      int64_t ldy, const double* X, int32_t K, const int32_t* bucket, const double* weight_y,
                      const double* weight_x, const fdx_shard_fit_params* prm, double* beta_out_dev, double* prop_out_dev,
                      double* rel_changes_out, fdx_shard_fit_info* info, void* stream);
/* The bcd_solve loop (core/solver.py:385-413) over this rank's shard.  beta0_dev / beta1_dev: (K, ld) type-major buffers
 * of the caller (initialised here: 1/K on own + halo, 0 on the pad); *result_buffer says which of the two holds the
 * final abundances.  info: n_iterations, converged, final_change, sweep_ms; rel_changes_out: max_iter doubles or NULL. */
int fdx_sharded_solve_dev(fdx_comm* comm, const fdx_graph* local, const double* H_dev, int64_t ldh, const double* XtX_dev,
                          int32_t K, double lambda, double rho_eff, double tol, int32_t max_iter, double* beta0_dev,
                          double* beta1_dev, int64_t ld, fdx_solve_info* info, double* rel_changes_out,
                          int32_t* result_buffer, void* stream);
/* More than 64 cell types on the sharded path (65..96): the solve runs the next instantiated sweep size fdx_solver_padded_k(K)
 * (72 / 80 / 88 / 96; = K up to 64) with all-zero pad types.  The caller provides H (zero planes K_real..K-1), XtX (K x K, zero
 * rows / columns for the pad types) and the two beta buffers with K = fdx_solver_padded_k(K_real) planes; the first K_real planes of
 * the result are the abundances.  fdx_sharded_solve_dev is this with K_real = K. */
int32_t fdx_solver_padded_k(int32_t K);
int fdx_sharded_solve_padded_dev(fdx_comm* comm, const fdx_graph* local, const double* H_dev, int64_t ldh, const double* XtX_dev,
                                 int32_t K, int32_t K_real, double lambda, double rho_eff, double tol, int32_t max_iter,
                                 double* beta0_dev, double* beta1_dev, int64_t ld, fdx_solve_info* info, double* rel_changes_out,
                                 int32_t* result_buffer, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FDX_H */
