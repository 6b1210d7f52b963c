"""``FlashDeconv`` estimator: the reference's ``flashdeconv/core/deconv.py`` surface on the MI355X path.

Constructor arguments, validation messages, fitted attributes (``beta_``, ``proportions_``, ``gene_idx_``, ``info_``,
``adjacency_``, ``lambda_used_``, ``n_spots_`` ...), getters and ``summary()`` follow core/deconv.py:88-512.  ``fit``
keeps the six steps of core/deconv.py:305-398 but runs steps 2-6 in one device-resident call (``fdx_fit_dev``).

Inputs may be NumPy arrays, SciPy sparse matrices, or CUDA (HIP) ``torch`` tensors that already live in HBM; with
``output="torch"`` the fitted arrays stay on the device as well.
"""
import ctypes
import os
import sys
import time

import numpy as np
from scipy import sparse

from .. import _lib
from ..utils import genes as _genes
from .sketching import sketch_tables

_PRE_MODES = ("log_cpm", "pearson", "raw")


def device_counts_as_float(Y):
    """A dense CUDA tensor as the float32 / float64 matrix the kernels stream, plus whether its transform must keep float64
    accuracy (``PRE_F64_MATH``).  Integer counts: numpy promotes them to float64 in the reference (core/deconv.py:190-191),
    so the log-CPM chain stays float64; float32 STORAGE is used when it holds every value exactly (below 2**24 - checked
    unless the dtype cannot exceed it), float64 otherwise.  Shared by FlashDeconv.fit and ShardedFlashDeconv.fit_transform."""
    import torch
    f64_math = False
    if Y.dtype not in (torch.float32, torch.float64):
        f64_math = not Y.dtype.is_floating_point
        small = Y.dtype in (torch.uint8, torch.int8, torch.int16, torch.bool, torch.float16, torch.bfloat16)
        exact = small or Y.numel() == 0
        if not exact:
            try:                                          # torch lacks min / max for some unsigned dtypes: float64 then
                hi = int(Y.max().item())
                lo = int(Y.min().item()) if Y.dtype.is_signed else 0
                exact = max(hi, -lo) < (1 << 24)
            except (RuntimeError, TypeError, NotImplementedError):
                exact = False
        Y = Y.to(torch.float32 if exact else torch.float64)
    return Y.contiguous(), f64_math


class _DeviceBuffer:
    """Plain device allocation through the C ABI (fdx_malloc / fdx_free)."""

    def __init__(self, nbytes):
        self.ptr = ctypes.c_void_p()
        self.nbytes = int(nbytes)
        _lib.check(_lib.load().fdx_malloc(ctypes.byref(self.ptr), self.nbytes))

    @classmethod
    def from_host(cls, arr):
        arr = np.ascontiguousarray(arr)
        buf = cls(arr.nbytes)
        _lib.upload_bytes(buf.ptr, arr)
        return buf

    @classmethod
    def adopt(cls, ptr, nbytes):
        """Takes over a block handed out by the library (fdx_malloc inside _lib.upload_matrix)."""
        buf = cls.__new__(cls)
        buf.ptr, buf.nbytes = ptr, int(nbytes)
        return buf

    def to_host(self, shape, dtype=np.float64, out=None):
        if out is None:
            out = np.empty(shape, dtype=dtype)
        _lib.download_bytes(out, self.ptr)
        return out

    def free(self):
        if self.ptr is not None and self.ptr.value:
            _lib.load().fdx_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def reference_tie_graph(c_ptr, coords_host, n, dim, k):
    """The k-NN graph on the REFERENCE's choice among exactly equidistant neighbours (regular lattices tie on every spot): the
    lists come from the restated cKDTree (utils/graph.py: ckdtree_knn_lists - scipy's build and traversal order, on the host),
    everything else stays on the device - the lists are put, in solver positions, where the device's own lists would be and
    symmetrised / laid out by fdx_graph_from_knn_lists_dev.  The graph therefore keeps the Morton order and the sweep tiles of
    any other device-built graph (the round-4 route went through a host adjacency in the caller's order: A + A^T in scipy, an
    untiled upload).  Reference: utils/graph.py:60-81."""
    from ..utils.graph import _ckdtree_restatement_matches_scipy
    lib = _lib.load()
    tr = [("start", time.perf_counter())] if os.environ.get("FDX_TRACE_HOST") else None

    def mark(name):
        if tr is not None:
            tr.append((name, time.perf_counter()))
    kk = min(int(k), n - 1) + 1
    nbr, cnt = _DeviceBuffer(n * kk * 4), _DeviceBuffer(n * 4)
    plan, h = ctypes.c_void_p(), ctypes.c_void_p()
    # where the tree is built on the host (4-8 coordinates, fdx_kdtree_tune(2, 0)) that build starts NOW, in the library's thread
    # pool, beside the device's own lists below, which wait ~3 ms behind the stopped fit's sketch; for 1-3 coordinates the tree is
    # built on the device when the lists are asked for and this call returns at once
    _ckdtree_restatement_matches_scipy()
    ch_arr = None if coords_host is None else np.ascontiguousarray(coords_host, dtype=np.float64)
    ch = None if ch_arr is None else _lib.ptr_f64(ch_arr)
    if dim <= 8:
        _lib.check(lib.fdx_ckdtree_prebuild(ch, c_ptr, n, dim))
    try:
        _lib.check(lib.fdx_graph_knn_lists_dev(c_ptr, n, dim, int(k), 0, n, nbr.ptr, cnt.ptr, None, ctypes.byref(plan)))
        try:
            mark("device lists + order")
            # the restated tree is built on the host, its queries run on the device (1-3 coordinates), and the answers go - as solver
            # positions, self dropped - to the rows' positions without leaving the device
            # coordinates that only exist on the device are fetched by the library into pinned memory (a pageable copy here would be
            # pinned by the driver, and unmapping it afterwards stalls the process's GPU queues: DESIGN appendix)
            _lib.check(lib.fdx_graph_plan_set_ckdtree_lists_dev(plan, ch, c_ptr, n, dim, None, 0, nbr.ptr, cnt.ptr, None))
            mark("tree (device, 1-3 coordinates; else the host's pool) + device queries + lists to positions")
        except Exception:
            dead = ctypes.c_void_p()                                           # the plan owns device buffers: consume it
            lib.fdx_graph_from_knn_lists_dev(plan, nbr.ptr, cnt.ptr, 0, 0, None, ctypes.byref(dead))
            if dead.value:
                _lib.Graph(dead.value).close()
            raise
        _lib.check(lib.fdx_graph_from_knn_lists_dev(plan, nbr.ptr, cnt.ptr, 0, n, None, ctypes.byref(h)))
        mark("symmetrise + ELL + tiles (device)")
        if tr is not None:
            print("[fdx-host] reference_tie_graph: " + ", ".join(f"{b[0]} {1e3 * (b[1] - a[1]):.1f} ms" for a, b in zip(tr[:-1], tr[1:])),
                  file=sys.stderr)
        return _lib.Graph(h.value)
    finally:
        for b in (nbr, cnt):
            b.free()


def _fit_timings(info, t_entry, t_graph, t_graph_end, select_s, t_lev, t_done, t_call, t_ret, ties_remedy_ms, span_from_call):
    """timings_ of a fit (additive, not in the reference): the per-stage GPU milliseconds the fit call reports (hipEvents) and
    the host intervals between the clock marks FlashDeconv.fit recorded - entry, the graph build call and its end, the wait for
    the leverage SVD (t_lev .. t_done), the fit call and its return."""
    t = {k: float(getattr(info, k)) for k in ("graph_ms", "sketch_ms", "gram_ms", "solve_ms", "finish_ms", "total_ms", "prologue_ms",
                                              "span_ms")}
    t["sweep_ms"] = float(info.solve.sweep_ms)
    # ties under "auto": the stopped first call + the reference's lists (host tree) + the rebuilt graph; ahead of the fit proper
    t["ties_remedy_ms"] = ties_remedy_ms
    # host wall of the graph build call, and of the wait for the leverage SVD that ran beside it
    t["graph_ms"] = (t_graph_end - t_graph) * 1e3
    t["select_ms"] = select_s * 1e3               # gene statistics on the device + HVG/marker ranking on the host
    t["leverage_wait_ms"] = (t_done - t_lev) * 1e3
    # the graph is built by its own call ahead of fdx_fit_dev, whose total_ms starts after it: one figure for the fit
    t["device_ms"] = t["total_ms"]
    # Accounting that tiles the wall time of the fit: host_pre_ms (entry -> the graph build call: conversions, gene selection,
    # leverage job set-up) + span_ms (device, hipEvents: first kernel of the graph build -> end of the export =
    # prologue_ms + sketch_ms + gram_ms + solve_ms + finish_ms) + host_post_ms (fit_dev's return -> here);
    # total_ms is their sum, and what the wall has beyond it is the host's last synchronisation.
    # span_from_call: the device span starts with the fit call - the graph was queued on the side stream FIRST (gene selection
    # active: gene statistics + ranking + leverage + tables all lie before the call; select_ms is the part that selects), or it
    # was rebuilt on the reference's tie order (first build, the stopped call, the host tree, the rebuild are host time)
    t["host_pre_ms"] = ((t_call if span_from_call else t_graph) - t_entry) * 1e3
    t["host_post_ms"] = (time.perf_counter() - t_ret) * 1e3
    t["total_ms"] = t["host_pre_ms"] + t["span_ms"] + t["host_post_ms"]
    return t


class FlashDeconv:
    """Fast spatial transcriptomics deconvolution with spatial regularisation (MI355X implementation).

    Parameters are those of the reference estimator (core/deconv.py:27-68): ``sketch_dim``, ``lambda_spatial``
    (float or "auto"), ``rho_sparsity``, ``n_hvg``, ``n_markers_per_type``, ``spatial_method`` ("knn" | "radius" |
    "grid"), ``k_neighbors``, ``radius``, ``max_iter``, ``tol``, ``preprocess`` ("log_cpm" | "pearson" | "raw"),
    ``random_state``, ``verbose``.
    """

    def __init__(self, sketch_dim=512, lambda_spatial="auto", rho_sparsity=0.01, n_hvg=2000, n_markers_per_type=50,
                 spatial_method="knn", k_neighbors=6, radius=None, max_iter=100, tol=1e-4, preprocess="log_cpm",
                 random_state=0, verbose=False, knn_ties="auto"):
        if sketch_dim <= 0:
            raise ValueError(f"sketch_dim must be positive, got {sketch_dim}")
        if k_neighbors < 0:
            raise ValueError(f"k_neighbors must be non-negative, got {k_neighbors}")
        if max_iter < 0:
            raise ValueError(f"max_iter must be non-negative, got {max_iter}")
        if tol <= 0:
            raise ValueError(f"tol must be positive, got {tol}")
        if isinstance(lambda_spatial, (int, float)) and lambda_spatial < 0:
            raise ValueError(f"lambda_spatial must be non-negative, got {lambda_spatial}")
        if rho_sparsity < 0:
            raise ValueError(f"rho_sparsity must be non-negative, got {rho_sparsity}")
        if n_hvg < 0:
            raise ValueError(f"n_hvg must be non-negative, got {n_hvg}")
        if n_markers_per_type < 0:
            raise ValueError(f"n_markers_per_type must be non-negative, got {n_markers_per_type}")
        if spatial_method == "radius" and radius is None:
            raise ValueError("radius must be specified when spatial_method='radius'")
        if radius is not None and radius <= 0:
            raise ValueError(f"radius must be positive, got {radius}")
        self.sketch_dim = sketch_dim
        self.lambda_spatial = lambda_spatial
        self.rho_sparsity = rho_sparsity
        self.n_hvg = n_hvg
        self.n_markers_per_type = n_markers_per_type
        self.spatial_method = spatial_method
        self.k_neighbors = k_neighbors
        self.radius = radius
        self.max_iter = max_iter
        self.tol = tol
        self.preprocess = preprocess
        self.random_state = random_state
        self.verbose = verbose
        # additive (not in the reference): how exactly equidistant candidates for the k-th neighbour are taken (regular lattices
        # tie on every spot).  "auto" (default): the device build's graph when it met no tie - every tie-free input, at no cost -
        # and otherwise the fit is repeated on the reference's own choice (cKDTree's traversal order, restated on the host:
        # csrc/kdtree_host.cpp), so the result is the reference's on lattices too; "ckdtree": the same, decided before the
        # first solve (one fit, but the graph build is waited for); "index": ascending spot index, the device rule, always
        # (fastest on lattices; a warning reports the ties, proportions a few 1e-4 from the reference's)
        if knn_ties not in ("auto", "index", "ckdtree"):
            raise ValueError(f"knn_ties must be 'auto', 'index' or 'ckdtree', got {knn_ties}")
        self.knn_ties = knn_ties

        self.beta_ = None
        self.proportions_ = None
        self.gene_idx_ = None
        self.info_ = None
        self.spot_diagnostics_ = None
        self._fitted = False
        self._graph = None
        self._adjacency = None

    # ------------------------------------------------------------------ adjacency_ (materialised on first access)
    @property
    def adjacency_(self):
        if self._adjacency is None and self._graph is not None:
            n = self.n_spots_
            indptr, indices = self._graph.to_csr_arrays()
            self._adjacency = sparse.csr_matrix((np.ones(len(indices), dtype=np.float64), indices,
                                                 indptr.astype(np.int32) if len(indices) < 2**31 - 1 else indptr),
                                                shape=(n, n))
        return self._adjacency

    @adjacency_.setter
    def adjacency_(self, value):
        self._adjacency = value

    # ------------------------------------------------------------------ fit
    def fit(self, Y, X, coords, cell_type_names=None, output="numpy", spot_diagnostics=False):
        """Fit the model (core/deconv.py:237-405).  ``output="torch"`` keeps ``beta_``/``proportions_`` in HBM.

        ``spot_diagnostics=True`` (additive, not in the reference) also keeps the per-spot terms of the objective in
        ``spot_diagnostics_``: ``residual_sq`` (squared sketch residual), ``sketch_sq`` (squared norm of the sketched row) and
        ``neighbor_sq`` (half the summed squared distance to the neighbours' abundances), each ``(n_spots,)`` float64 in the
        caller's spot order - see ``get_spot_residuals``.  One more kernel behind the fit; off, nothing is launched."""
        t_entry = time.perf_counter()
        if Y.shape[1] != X.shape[1]:
            raise ValueError(
                f"Gene dimension mismatch: Y has {Y.shape[1]} genes but X has {X.shape[1]} genes. They must share "
                f"the same gene space (align before calling fit).")
        if coords.shape[0] != Y.shape[0]:
            raise ValueError(
                f"Spot count mismatch: Y has {Y.shape[0]} spots but coords has {coords.shape[0]} rows. Each spot "
                f"needs exactly one coordinate.")
        if X.shape[0] == 0:
            raise ValueError(
                "Reference matrix X must contain at least one cell type (X.shape[0] > 0). Check your reference "
                "filtering and cell_type_key mapping.")
        if cell_type_names is not None and len(cell_type_names) != X.shape[0]:
            raise ValueError(
                f"cell_type_names length ({len(cell_type_names)}) does not match number of cell types in X "
                f"({X.shape[0]}).")
        if self.preprocess not in _PRE_MODES:
            raise ValueError(f"Unknown preprocess method: {self.preprocess}. Choose from 'log_cpm', 'pearson', or 'raw'.")
        if self.spatial_method not in ("knn", "radius", "grid"):
            raise ValueError(f"Unknown method: {self.spatial_method}")
        if len(coords.shape) != 2 or coords.shape[1] == 0:
            raise ValueError(f"coords must be 2D with at least 1 coordinate dimension, got shape {tuple(coords.shape)}")
        from ..utils.graph import check_coord_dims
        check_coord_dims(int(coords.shape[0]), int(coords.shape[1]), self.spatial_method == "knn")
        # the reference takes any k (utils/graph.py:51); the device's k-NN lists hold at most 64 entries per spot (self included):
        # above that the lists come from the restated cKDTree on the host (utils/graph.py: ckdtree_knn_adjacency - the reference's
        # own neighbours, ties included) and the adjacency is uploaded as given (caller's spot order, untiled sweep)
        big_k = self.spatial_method == "knn" and min(int(self.k_neighbors), int(coords.shape[0]) - 1) > 63
        _lib.require_gpu()
        lib = _lib.load()
        log = print if self.verbose else (lambda *a, **k: None)
        log("FlashDeconv: Starting deconvolution...")
        log(f"  Spatial data: {Y.shape[0]} spots x {Y.shape[1]} genes")
        log(f"  Reference: {X.shape[0]} cell types x {X.shape[1]} genes")

        n, G_all = int(Y.shape[0]), int(Y.shape[1])
        X = np.asarray(X.detach().cpu().numpy() if hasattr(X, "detach") else X, dtype=np.float64)
        K = X.shape[0]
        self.n_spots_, self.n_genes_, self.n_cell_types_ = n, G_all, K
        self.cell_type_names_ = cell_type_names
        if n == 0:
            raise ValueError("Y has no spots")

        # Y into HBM (full gene set), then Step 1: informative genes + leverage scores (core/deconv.py:305-318)
        owned = []
        try:
            if G_all == 0:
                raise ValueError("No genes selected. Increase n_hvg or n_markers_per_type.")
            csr = None
            y_f64_math = False
            if sparse.issparse(Y) or _lib.is_torch_sparse_csr(Y):
                # sparse stays sparse in HBM: gene statistics, log-CPM and the sketch read the stored entries only
                csr = _lib.CsrOnDevice.from_scipy(Y) if sparse.issparse(Y) else _lib.CsrOnDevice.from_torch(Y)
                owned.append(csr)
                y_ptr, y_code, y_sparse_rule = None, csr.view.dtype, True
            elif _lib.is_cuda_tensor(Y):
                Y, y_f64_math = device_counts_as_float(Y)
                y_ptr, y_code, y_sparse_rule = Y.data_ptr(), _lib.dtype_code(Y), False
            else:
                y_sparse_rule = False
                Yh = np.asarray(Y)
                y_f64_math = Yh.dtype.kind in "iub"
                y_ptr, y_code = _lib.upload_matrix(Yh)         # threaded, staged, integer counts narrowed on the way
                owned.append(_DeviceBuffer.adopt(y_ptr, Yh.size * (4 if y_code == _lib.FDX_F32 else 8)))
            csr_colsum = None
            # coordinates into HBM; with gene selection active (G > n_hvg) the spatial graph - which does not depend on the genes -
            # is queued FIRST: its ~0.7 ms of kernels then run under the gene statistics and the host's ranking of the G-vector
            # instead of after them (the device idled ~1.5 ms there)
            if _lib.is_cuda_tensor(coords):
                import torch
                cd = coords.to(torch.float64).contiguous()
                c_ptr = cd.data_ptr()
                coords_host = None
            else:
                coords_host = np.ascontiguousarray(np.asarray(coords), dtype=np.float64)
                cbuf = _DeviceBuffer.from_host(coords_host)
                owned.append(cbuf)
                c_ptr = cbuf.ptr
            dim = int(coords.shape[1])
            g_method, g_k, g_radius = self._graph_request(coords, coords_host)
            graph_early = G_all > self.n_hvg and not big_k
            t_graph = t_graph_done = None
            if self._graph is not None:
                self._graph.close()
                self._graph = None
            self._adjacency = None
            if graph_early:
                t_graph = time.perf_counter()
                gh = ctypes.c_void_p()
                side = ctypes.c_void_p()
                if os.environ.get("FDX_NO_SIDE_STREAM"):
                    side = None
                else:
                    # on the library's side stream, behind whatever produced the coordinates on the default stream so far
                    _lib.check(lib.fdx_side_stream(ctypes.byref(side)))
                    if _lib.is_cuda_tensor(coords):
                        _lib.check(lib.fdx_stream_wait_stream(side, _lib.current_stream()))
                _lib.check(lib.fdx_graph_build_dev(c_ptr, n, dim, g_method, g_k, g_radius, side, ctypes.byref(gh)))
                self._graph = _lib.Graph(gh.value)
                t_graph_done = time.perf_counter()
            log("Step 1: Selecting informative genes...")
            t_sel = time.perf_counter()
            if G_all <= self.n_hvg:
                # select_hvg returns every gene when the matrix has no more than n_hvg of them and the marker union is a
                # subset (utils/genes.py:135-145, 330) - no pass over Y needed.
                gene_idx = np.arange(G_all, dtype=np.intp)
            else:
                # the marker table depends on X only: a helper thread ranks it while the device reduces Y to its per-gene
                # moments (and, for CSR rows under "pearson", to the column sums of step 2)
                def moments():
                    nonlocal csr_colsum
                    if csr is None:
                        return _genes.gene_moments_device(y_ptr, y_code, n, G_all, G_all)
                    mean, var, csr_colsum = csr.gene_moments(want_colsum=self.preprocess == "pearson")
                    return mean, var
                gene_idx = _genes.select_gene_idx(X, self.n_hvg, self.n_markers_per_type, moments)
            self.gene_idx_ = gene_idx
            t_sel_end = time.perf_counter()
            t_sel = t_sel_end - t_sel
            G = len(gene_idx)
            log(f"  Selected {G} genes (HVG + markers)")
            Xsel = np.ascontiguousarray(X) if G == G_all else np.take(X, gene_idx, axis=1)          # (np.take: half the time of X[:, gene_idx] at 30 x 3300 of 20000)
            # The leverage SVD runs on the library's side stream beside the graph build.  Its job is set up FIRST: set up behind
            # the build call, its pooled buffers (last used on the caller's stream) order the side stream behind everything the
            # build has just queued - the SVD then starts when the graph is done (measured: the wait 0.6 -> 1.3 ms).
            t_x0 = time.perf_counter()
            lev_job = _genes.LeverageJob(Xsel, queue_async=not graph_early)   # graph already queued: the scores are collected next
            if os.environ.get("FDX_TRACE_HOST"):
                print(f"[fdx-host] python: select end -> Xsel {1e6 * (t_x0 - t_sel_end):.0f} us, leverage job set-up {1e6 * (time.perf_counter() - t_x0):.0f}",
                      file=sys.stderr)
            if G != G_all and csr is None:          # Y[:, gene_idx] (core/deconv.py:321) as a compact device matrix
                sub = _DeviceBuffer(n * G * (4 if y_code == _lib.FDX_F32 else 8))
                owned.append(sub)
                gi32 = np.ascontiguousarray(gene_idx, dtype=np.int32)
                _lib.check(lib.fdx_gather_columns_dev(y_ptr, y_code, n, G_all, G_all, _lib.ptr_i32(gi32), G, sub.ptr, None))
                y_ptr = sub.ptr
            ldy = G

            # Step 4 runs here, under the leverage SVD (no data dependence between core/deconv.py:318 and :358)
            if big_k:
                from ..utils.graph import ckdtree_knn_adjacency
                t_graph = time.perf_counter()
                A = ckdtree_knn_adjacency(coords_host if coords_host is not None else _lib.tensor_to_host(coords), int(self.k_neighbors))
                self._graph = _lib.Graph.from_csr(A.indptr, A.indices, n)
                self._adjacency = A                      # (adjacency_: the host matrix itself)
            elif not graph_early:
                t_graph = time.perf_counter()
                gh = ctypes.c_void_p()
                _lib.check(lib.fdx_graph_build_dev(c_ptr, n, dim, g_method, g_k, g_radius, None, ctypes.byref(gh)))
                self._graph = _lib.Graph(gh.value)
            n_ties = 0
            if self.spatial_method == "knn" and self.knn_ties == "ckdtree" and not big_k:
                # the reference's tie order, on request: only when the device build met ties (this question waits for the
                # build, which otherwise completes behind the sketch) the lists come from the host restatement of scipy's
                # tree (csrc/kdtree_host.cpp) and the graph is rebuilt from the reference's own adjacency
                n_ties = self._graph.knn_ties()
                if n_ties:
                    self._graph.close()
                    self._graph = None
                    self._graph = reference_tie_graph(c_ptr, coords_host, n, dim, int(self.k_neighbors))
            t_lev = time.perf_counter()
            leverage = lev_job.result()
            t_done = time.perf_counter()

            # Step 2+3 tables: preprocessing mode and CountSketch Omega (core/deconv.py:326-352)
            log(f"Step 2: Preprocessing with method='{self.preprocess}'...")

            def y_colsum():
                if csr is not None:
                    return (csr_colsum if csr_colsum is not None else csr.gene_moments(want_colsum=True)[2])[gene_idx]
                sums = np.empty(G, dtype=np.float64)
                _lib.check(lib.fdx_column_sums_dev(y_ptr, y_code, n, G, ldy, _lib.ptr_f64(sums), None))
                return sums
            bucket32, wy, wx, mode_y, mode_x = sketch_tables(
                G, self.sketch_dim, leverage, self.random_state, self.preprocess, Xsel, y_sparse=y_sparse_rule,
                f64_math=y_f64_math and csr is None and y_code == _lib.FDX_F32, y_colsum=y_colsum, n_spots=n)
            log({"log_cpm": "  Y and X normalized to log-CPM space", "pearson": "  Y and X transformed with uncentered Pearson residuals",
                 "raw": "  No preprocessing applied (raw)"}[self.preprocess])
            log(f"Step 3: Sketching to {self.sketch_dim} dimensions...")
            log(f"  Compressed {G} genes -> {self.sketch_dim} dims")

            prm = _lib.FitParams()
            prm.sketch_dim = int(self.sketch_dim)
            prm.mode_y, prm.mode_x = mode_y, mode_x
            prm.k_neighbors = int(self.k_neighbors)
            prm.max_iter, prm.tol, prm.verbose = int(self.max_iter), float(self.tol), 1 if self.verbose else 0
            prm.rho_sparsity = float(self.rho_sparsity)
            prm.lambda_auto = 1 if self.lambda_spatial == "auto" else 0
            prm.lambda_spatial = 0.0 if prm.lambda_auto else float(self.lambda_spatial)
            prm.radius = 0.0
            prm.graph_method = _lib.GRAPH_GIVEN
            # "auto": the question "is any k-th neighbour tied?" is answered inside the fit, where the graph's counts are taken
            # over anyway - tie-free inputs pay nothing; on ties the call returns before the solve and the graph is rebuilt on the
            # reference's choice
            prm.stop_on_ties = 1 if (self.spatial_method == "knn" and self.knn_ties == "auto" and not big_k) else 0
            log("Step 4: Building spatial graph...")

            if output == "torch":
                import torch
                dev = Y.device if _lib.is_cuda_tensor(Y) else torch.device("cuda", torch.cuda.current_device())
                beta_t = torch.empty((n, K), dtype=torch.float64, device=dev)
                prop_t = torch.empty((n, K), dtype=torch.float64, device=dev)
                b_ptr, p_ptr = beta_t.data_ptr(), prop_t.data_ptr()
            else:
                bbuf, pbuf = _DeviceBuffer(n * K * 8), _DeviceBuffer(n * K * 8)
                owned += [bbuf, pbuf]
                b_ptr, p_ptr = bbuf.ptr, pbuf.ptr

            diag_t = dbuf = None
            if spot_diagnostics:                 # one 3n block: [residual_sq | sketch_sq | neighbor_sq]
                if output == "torch":
                    diag_t = torch.empty(3 * n, dtype=torch.float64, device=dev)
                    prm.spot_diag_out_dev = diag_t.data_ptr()
                else:
                    dbuf = _DeviceBuffer(3 * n * 8)
                    owned.append(dbuf)
                    prm.spot_diag_out_dev = dbuf.ptr
            objs = np.zeros(max(int(self.max_iter), 1), dtype=np.float64)
            rels = np.zeros(max(int(self.max_iter), 1), dtype=np.float64)
            info = _lib.FitInfo()
            gh = ctypes.c_void_p(self._graph.handle.value)
            t_call = time.perf_counter()
            gi32 = np.ascontiguousarray(gene_idx, dtype=np.int32)

            def run_fit():
                if csr is not None:
                    _lib.check(lib.fdx_fit_csr_dev(ctypes.byref(csr.view), _lib.ptr_i32(gi32), G, _lib.ptr_f64(Xsel), K,
                                                   _lib.ptr_i32(bucket32), _lib.ptr_f64(wy), _lib.ptr_f64(wx), c_ptr, dim,
                                                   ctypes.byref(prm), ctypes.byref(gh), b_ptr, p_ptr, _lib.ptr_f64(objs),
                                                   _lib.ptr_f64(rels), ctypes.byref(info), None))
                else:
                    _lib.check(lib.fdx_fit_dev(y_ptr, y_code, n, G, ldy, _lib.ptr_f64(Xsel), K, _lib.ptr_i32(bucket32),
                                               _lib.ptr_f64(wy), _lib.ptr_f64(wx), c_ptr, dim, ctypes.byref(prm),
                                               ctypes.byref(gh), b_ptr, p_ptr, _lib.ptr_f64(objs), _lib.ptr_f64(rels),
                                               ctypes.byref(info), None))

            run_fit()
            ties_remedy_ms = 0.0
            if info.status == _lib.FIT_TIES:
                # ties under "auto": the reference's neighbour choice, then the fit proper.  The stopped call's sketch -> H stage is
                # still running on the device while the host builds the tree; the second call takes it over (info.carry) - the
                # rebuilt graph keeps the spot order.  The first graph stays alive until then: the running kernel reads its order.
                n_ties = int(info.knn_ties)
                log(f"k-NN ties on {n_ties} of {n} spots: rebuilding the graph on the reference's (cKDTree) neighbour choice")
                stale, carry = self._graph, info.carry
                self._graph = None
                try:
                    self._graph = reference_tie_graph(c_ptr, coords_host, n, dim, int(self.k_neighbors))
                    gh = ctypes.c_void_p(self._graph.handle.value)
                    prm.stop_on_ties = 0
                    prm.carry, carry = carry, None             # consumed by the call
                    ties_resolved_here = True
                    ties_remedy_ms = (time.perf_counter() - t_call) * 1e3
                    t_call = time.perf_counter()
                    run_fit()
                finally:
                    if carry:
                        lib.fdx_fit_carry_free(carry)
                    stale.close()
            else:
                ties_resolved_here = False
            t_ret = time.perf_counter()
            if os.environ.get("FDX_TRACE_HOST"):
                print(f"[fdx-host] python: entry->build {1e6 * (t_graph - t_entry):.0f} us, build call {1e6 * (t_lev - t_graph):.0f}, leverage wait "
                      f"{1e6 * (t_done - t_lev):.0f}, tables + setup {1e6 * (t_call - t_done):.0f}, fit call {1e6 * (t_ret - t_call):.0f}", file=sys.stderr)
            if output == "torch":
                self.beta_, self.proportions_ = beta_t, prop_t
            else:
                # A model that is fitted again and whose previous result arrays nobody else holds writes into them: releasing
                # 240 MB arrays and faulting in fresh ones costs ~25 ms of munmap / page zeroing per fit at 1M x 30 - more than
                # the device spends on the whole fit (unobservable: no other reference to the old arrays exists)
                self.beta_ = bbuf.to_host((n, K), out=self._recyclable("beta_", (n, K)))
                self.proportions_ = pbuf.to_host((n, K), out=self._recyclable("proportions_", (n, K)))
            self.spot_diagnostics_ = None
            if spot_diagnostics:
                planes = diag_t if diag_t is not None else dbuf.to_host((3 * n,))
                self.spot_diagnostics_ = {name: planes[j * n:(j + 1) * n]
                                          for j, name in enumerate(("residual_sq", "sketch_sq", "neighbor_sq"))}
        finally:
            for b in owned:
                b.free()

        log(f"  Average neighbors per spot: {info.nnz / max(n, 1):.1f}")
        self.lambda_used_ = float(info.lambda_used)
        log(f"Step 5: {'Auto-tuned' if prm.lambda_auto else 'Using'} lambda = {self.lambda_used_:.4f}")
        log("Step 6: Solving via Block Coordinate Descent...")
        n_it = int(info.solve.n_iterations)
        objectives = [float(v) for v in objs[:info.solve.n_objectives]]
        if self.verbose:
            its = [t for t in range(n_it) if t % 10 == 0 or t == self.max_iter - 1]
            for t, obj in zip(its, objectives):
                print(f"Iteration {t}: objective = {obj:.6f}, rel_change = {rels[t]:.6e}")
            if info.solve.converged:
                print(f"Converged at iteration {n_it - 1}")
        self.info_ = info.solve.as_dict()
        self.info_["objectives"] = objectives if self.verbose else []
        # additive (not in the reference): spots whose k-NN set is a choice - the k-th and (k+1)-th neighbours exactly
        # equidistant.  The reference takes whichever cKDTree.query meets first (utils/graph.py:60-63), which changes
        # with the order the spots are listed in; here the lower spot index wins.  Regular lattices tie on every spot.
        resolved = self.spatial_method == "knn" and (self.knn_ties == "ckdtree" or ties_resolved_here)
        self.info_["knn_ties"] = (n_ties if resolved else int(info.knn_ties)) if self.spatial_method == "knn" else 0
        if self.info_["knn_ties"] and not resolved:
            import warnings
            warnings.warn(
                f"k-NN ties: {self.info_['knn_ties']} of {n} spots have their k-th and (k+1)-th nearest neighbours at exactly "
                "the same distance (regular lattice?), so the neighbour graph depends on how ties are broken - here by "
                "spot index, in the reference by cKDTree's traversal, i.e. by the order the spots are listed in.  "
                "Proportions can differ from the reference's by a few 1e-4 (relative); knn_ties='auto' (the default) or "
                "'ckdtree' reproduce the reference's choice (host-side, about a second per million spots), "
                "spatial_method='grid' builds a tie-free graph on lattices.", UserWarning, stacklevel=2)
        # ties resolved: the graph was rebuilt on the reference's tie order, the device span starts with the fit call that used it
        self.timings_ = _fit_timings(info, t_entry, t_graph, t_graph_done if graph_early else t_lev, t_sel, t_lev, t_done, t_call, t_ret,
                                     ties_remedy_ms, span_from_call=graph_early or ties_resolved_here or bool(resolved and n_ties))
        if spot_diagnostics:
            self.timings_["diagnostics_ms"] = float(info.diag_ms)
        self._fitted = True
        log(f"  Converged: {self.info_['converged']}")
        log(f"  Iterations: {self.info_['n_iterations']}")
        log("FlashDeconv: Done!")
        return self

    def _recyclable(self, name, shape):
        """The model's previous result array `name` when it can take the new result in place: same shape, float64, owns its
        memory, and referenced by nobody but the model (attribute + this frame's variable + getrefcount's argument)."""
        old = getattr(self, name, None)
        ok = (isinstance(old, np.ndarray) and old.shape == tuple(shape) and old.dtype == np.float64 and old.flags.c_contiguous
              and old.flags.owndata and old.flags.writeable and sys.getrefcount(old) <= 3)
        return old if ok else None

    def _graph_request(self, coords, coords_host):
        """(method, k, radius) of the graph build for this model's spatial_method (utils/graph.py:175-212)."""
        if self.spatial_method == "knn":
            return _lib.GRAPH_KNN, int(self.k_neighbors), 0.0
        if self.spatial_method == "radius":
            if self.radius is None:
                raise ValueError("radius must be specified for radius method")
            return _lib.GRAPH_RADIUS, 0, float(self.radius)
        if self.spatial_method == "grid":  # radius = 1.5 x median nearest-neighbour distance (utils/graph.py:163-170)
            if coords.shape[0] < 2:
                return _lib.GRAPH_KNN, 0, 0.0
            from ..utils.graph import grid_radius
            ch = coords_host if coords_host is not None else _lib.tensor_to_host(coords)
            return _lib.GRAPH_RADIUS, 0, grid_radius(ch)
        raise ValueError(f"Unknown method: {self.spatial_method}. Choose from 'knn', 'radius', 'grid'.")

    def fit_transform(self, Y, X, coords, **kwargs):
        self.fit(Y, X, coords, **kwargs)
        return self.proportions_

    # ------------------------------------------------------------------ getters (core/deconv.py:436-512)
    def _require_fitted(self):
        if not self._fitted:
            raise RuntimeError("Model has not been fitted. Call fit() first.")

    def get_cell_type_proportions(self):
        self._require_fitted()
        return self.proportions_

    def get_abundances(self):
        self._require_fitted()
        return self.beta_

    def get_spot_residuals(self, relative=True):
        """Per-spot goodness of fit in sketch space (additive, not in the reference): ``sqrt(residual_sq / sketch_sq)`` - the share
        of a spot's sketched row the fitted mixture leaves unexplained, 0 where the row is all zero - or, with
        ``relative=False``, ``sqrt(residual_sq)``.  Needs ``fit(..., spot_diagnostics=True)``; same array kind as
        ``spot_diagnostics_``."""
        self._require_fitted()
        if self.spot_diagnostics_ is None:
            raise RuntimeError("No per-spot diagnostics: call fit(..., spot_diagnostics=True) first.")
        res, sq = self.spot_diagnostics_["residual_sq"], self.spot_diagnostics_["sketch_sq"]
        if isinstance(res, np.ndarray):
            if not relative:
                return np.sqrt(res)
            return np.sqrt(np.divide(res, sq, out=np.zeros_like(res), where=sq > 0))
        import torch
        if not relative:
            return torch.sqrt(res)
        return torch.sqrt(torch.where(sq > 0, res / torch.where(sq > 0, sq, torch.ones_like(sq)), torch.zeros_like(res)))

    def get_spatial_autocorrelation(self, what="proportions", neighbor_mean=False, n_permutations=0, random_state=None):
        """Moran's I per cell type, the K x K bivariate Moran matrix (neighbourhood co-localisation) and, with
        ``neighbor_mean=True``, each spot's neighbour-averaged composition, over the graph the fit used (additive, not in the
        reference): ``utils.spatial_stats.spatial_autocorrelation`` on ``proportions_`` (``what="proportions"``) or ``beta_``
        (``what="abundances"``) and the model's device graph.  Works for both ``output`` kinds of ``fit``.

        ``n_permutations=R`` > 0 adds the permutation test of ``utils.spatial_stats.spatial_permutation_test`` (p values and
        simulated z scores of I and of every pair, the randomisation variance), seeded by ``random_state`` (None: the model's)."""
        self._require_fitted()
        if what not in ("proportions", "abundances"):
            raise ValueError(f"Unknown what: {what}. Choose from 'proportions', 'abundances'.")
        from ..utils.spatial_stats import spatial_autocorrelation, spatial_permutation_test, spatial_sums
        values = self.proportions_ if what == "proportions" else self.beta_
        if isinstance(n_permutations, (bool, np.bool_)) or not isinstance(n_permutations, (int, np.integer)) or n_permutations < 0:
            raise ValueError(f"n_permutations must be an int >= 0, got {n_permutations!r}")
        if n_permutations == 0:
            return spatial_autocorrelation(values, self, neighbor_mean=neighbor_mean)
        out = spatial_permutation_test(values, self, n_permutations=n_permutations,
                                       random_state=self.random_state if random_state is None else random_state)
        if neighbor_mean:
            out["neighbor_mean"] = spatial_sums(values, self, neighbor_mean=True)["neighbor_mean"]
        return out

    def get_local_spatial_statistics(self, what="proportions", n_permutations=0, random_state=None):
        """Where a cell type is spatially clustered (additive, not in the reference): local Moran's I with its HH / LH / LL / HL
        quadrant and the Getis-Ord Gi* hot-spot score per spot and cell type, over the graph the fit used -
        ``utils.local_stats.local_spatial_statistics`` on ``proportions_`` (``what="proportions"``) or ``beta_``
        (``what="abundances"``) and the model's device graph.  Works for both ``output`` kinds of ``fit``.

        ``n_permutations=R`` > 0 adds the conditional-permutation p values and simulated z scores per spot, seeded by
        ``random_state`` (None: the model's)."""
        self._require_fitted()
        if what not in ("proportions", "abundances"):
            raise ValueError(f"Unknown what: {what}. Choose from 'proportions', 'abundances'.")
        from ..utils.local_stats import local_spatial_statistics
        return local_spatial_statistics(self.proportions_ if what == "proportions" else self.beta_, self,
                                        n_permutations=n_permutations,
                                        random_state=self.random_state if random_state is None else random_state)

    def get_spatial_correlogram(self, coords, radii=None, n_bands=10, what="proportions"):
        """Over what range cell types are clustered and co-localised (additive, not in the reference): Moran's I per cell type and
        the K x K bivariate Moran matrix in every distance band of ``radii`` (None: ``n_bands`` multiples of the grid radius) -
        ``utils.correlogram.spatial_correlogram`` on ``proportions_`` (``what="proportions"``) or ``beta_``
        (``what="abundances"``).  The model does not keep the coordinates: pass the ones the fit was given.  Works for both
        ``output`` kinds of ``fit``."""
        self._require_fitted()
        if what not in ("proportions", "abundances"):
            raise ValueError(f"Unknown what: {what}. Choose from 'proportions', 'abundances'.")
        from ..utils.correlogram import spatial_correlogram
        return spatial_correlogram(self.proportions_ if what == "proportions" else self.beta_, coords, radii=radii,
                                   n_bands=n_bands)

    def get_spatial_niches(self, n_niches, what="proportions", features="both", **kw):
        """Groups the spots into ``n_niches`` spatial niches (tissue domains) by k-means of their composition, of their
        neighbourhood's composition over the graph the fit used, or of both (additive, not in the reference):
        ``utils.niches.spatial_niches`` on ``proportions_`` (``what="proportions"``) or ``beta_`` (``what="abundances"``) and the
        model's device graph; further keywords (``neighbor_weight``, ``init``, ``max_iter``, ``random_state``) go there.  Works for
        both ``output`` kinds of ``fit``."""
        self._require_fitted()
        if what not in ("proportions", "abundances"):
            raise ValueError(f"Unknown what: {what}. Choose from 'proportions', 'abundances'.")
        from ..utils.niches import spatial_niches
        return spatial_niches(self.proportions_ if what == "proportions" else self.beta_, n_niches, graph=self, features=features,
                              **kw)

    def get_celltype_expression(self, Y, what="proportions", spot_scale=None, groups=None, **kw):
        """What each cell type expresses in this tissue and which genes the fitted composition explains (additive, not in the
        reference): per-gene non-negative least squares of ``Y`` on the fitted weights -
        ``utils.expression.celltype_expression`` on ``proportions_`` (``what="proportions"``) or ``beta_``
        (``what="abundances"``).  ``Y``: ``n_spots_`` rows, dense or CSR, ANY gene set - every column is regressed, not only
        ``gene_idx_``.  ``spot_scale``: (n_spots,) finite non-negative factors that multiply the rows of the weights (each spot's
        library size over the mean library size is the natural choice for counts).  ``groups``: labels per spot (the ``labels``
        of ``get_spatial_niches``, say; ``-1`` = left out) for one signature matrix per group.  Further keywords (``n_groups``,
        ``ridge``, ``max_iter``, ``tol``, ``output``) go to ``celltype_expression``.  Works for both ``output`` kinds of ``fit``."""
        from ..utils.expression import celltype_expression
        return celltype_expression(Y, self._weights_for(Y, what, spot_scale), groups=groups, **kw)

    def _weights_for(self, Y, what, spot_scale):
        """The fitted weights a per-gene analysis of ``Y`` regresses on: ``proportions_`` or ``beta_``, their rows multiplied by
        ``spot_scale`` where given; ``Y`` must have the fit's spots as rows."""
        self._require_fitted()
        if what not in ("proportions", "abundances"):
            raise ValueError(f"Unknown what: {what}. Choose from 'proportions', 'abundances'.")
        W = self.proportions_ if what == "proportions" else self.beta_
        n = int(W.shape[0])
        if not hasattr(Y, "shape") or len(Y.shape) != 2 or int(Y.shape[0]) != n:
            raise ValueError(f"Y must be a 2-D matrix with the {n} spots of the fit as rows, got shape {getattr(Y, 'shape', None)}")
        if spot_scale is not None:
            if _lib.is_cuda_tensor(spot_scale):
                sc = _lib.tensor_to_host(spot_scale).astype(np.float64)
            else:
                sc = np.asarray(spot_scale.detach().numpy() if hasattr(spot_scale, "detach") else spot_scale, dtype=np.float64)
            if sc.shape != (n,) or not np.all(np.isfinite(sc)) or np.any(sc < 0):
                raise ValueError(f"spot_scale must be {n} finite non-negative numbers, got shape {sc.shape}")
            if _lib.is_cuda_tensor(W):
                import torch
                W = W * torch.as_tensor(sc).to(device=W.device, dtype=W.dtype)[:, None]
            else:
                W = W * sc[:, None]
        return W

    def get_spatially_variable_genes(self, Y, residual=False, what="proportions", spot_scale=None, n_top=None, n_permutations=0,
                                     random_state=None, permutation_genes=None, **kw):
        """Which genes vary over this tissue, and which still do once the fitted composition is accounted for (additive, not in
        the reference): Moran's I and Geary's C per gene of ``Y`` over the graph the fit used, with z scores, p and q values -
        ``utils.spatial_genes.spatially_variable_genes``.  ``Y``: ``n_spots_`` rows, dense or CSR, ANY gene set, scored as it is
        passed.  ``residual=True`` also regresses every gene on ``proportions_`` (``what="proportions"``) or ``beta_``
        (``what="abundances"``), their rows multiplied by ``spot_scale`` as in ``get_celltype_expression``, and reports Moran's I
        of what the composition leaves (``residual_morans_i``, ``residual_z_score``, ``r2``, ``expression``): high for genes with
        a gradient or a state of their own inside a cell type.  ``n_top``: also ``top``, the first genes of ``order``.
        ``n_permutations=R`` > 0 also ranks Moran's I and Geary's C of the genes ``permutation_genes`` (column indices of ``Y``,
        None: every gene) against R random reassignments of each gene's values to the spots, on the GPU
        (``utils.gene_permutations.spatial_gene_permutation_test``, seeded by ``random_state``, None: the model's), and adds
        ``p_sim``, ``p_sim_less``, ``gearys_p_sim``, ``z_sim``, ``null_mean``, ``null_std``, ``q_sim`` (G,) - NaN for the genes
        that were not tested - and ``n_permutations``; with 0 the result is what it is without these arguments.  Further
        keywords (``ridge``, ``max_iter``, ``tol``) go to the solve.  Works for both ``output`` kinds of ``fit``."""
        if not isinstance(residual, (bool, np.bool_)):
            raise ValueError(f"residual must be True or False, got {residual!r}")
        from ..utils._device import check_count
        from ..utils.gene_permutations import STAT_KEYS, check_request, spatial_gene_permutation_test
        if check_count("n_permutations", n_permutations):      # (0: exactly today's call, today's errors in today's order)
            check_request(tuple(Y.shape) if hasattr(Y, "shape") else np.shape(Y), permutation_genes, n_permutations)
        W = self._weights_for(Y, what, spot_scale)
        from ..utils.spatial_genes import spatially_variable_genes
        out = spatially_variable_genes(Y, self, weights=W if residual else None, n_top=n_top, **kw)
        if n_permutations:
            seed = self.random_state if random_state is None else random_state
            perm = spatial_gene_permutation_test(Y, self, genes=permutation_genes, n_permutations=n_permutations, random_state=seed)
            for key in STAT_KEYS:
                full = np.full(out["morans_i"].shape[0], np.nan)
                full[perm["genes"]] = perm[key]
                out[key] = full
            out["n_permutations"] = int(n_permutations)
        return out

    def get_gene_pair_colocalisation(self, Y, pairs, local=False, n_top=None):
        """Which pairs of genes - a ligand and its receptor - are expressed next to each other in this tissue, and where (additive,
        not in the reference): the bivariate Moran's R of every pair of ``pairs`` ((P, 2) column indices of ``Y``) over the graph
        the fit used, with Pearson's r, z scores under the exact permutation variance, p and q values and, with ``local=True``,
        the per-spot score ``local`` (n_spots, P) - ``utils.gene_pairs.spatial_gene_pairs``.  ``Y``: ``n_spots_`` rows, dense or
        CSR, ANY gene set, scored as it is passed.  ``n_top``: also ``top``, the first pairs of ``order``.  After
        ``fit(output="torch")`` ``local`` stays a CUDA tensor."""
        self._weights_for(Y, "proportions", None)              # fitted, and Y has the fit's spots as rows
        from ..utils.gene_pairs import spatial_gene_pairs
        return spatial_gene_pairs(Y, self, pairs, local=local, n_top=n_top,
                                  output="torch" if _lib.is_cuda_tensor(self.proportions_) else "numpy")

    def get_spatial_gene_modules(self, Y, **kw):
        """Which genes vary together over this tissue, and where (additive, not in the reference): the spatial co-expression matrix
        of ``genes`` (None: the spatially variable genes of ``Y``, at most ``n_genes``) over the graph the fit used, the gene
        modules cut from it and every module's score per spot - ``utils.gene_modules.spatial_gene_modules``, which takes the
        keywords (``genes``, ``n_genes``, ``fdr``, ``n_modules``, ``min_module_size``, ``scores``).  ``Y``: ``n_spots_`` rows, dense
        or CSR, ANY gene set, scored as it is passed.  After ``fit(output="torch")`` ``scores`` stays a CUDA tensor."""
        self._weights_for(Y, "proportions", None)              # fitted, and Y has the fit's spots as rows
        from ..utils.gene_modules import spatial_gene_modules
        return spatial_gene_modules(Y, self, output="torch" if _lib.is_cuda_tensor(self.proportions_) else "numpy", **kw)

    def get_niche_genes(self, Y, groups=None, n_niches=None, **kw):
        """Which genes mark each niche of this tissue (additive, not in the reference): per group of spots and gene of ``Y`` the
        Wilcoxon rank-sum test and the Welch t test of the group against all other spots, with effect sizes, q values and the
        ranking - ``utils.group_genes.rank_genes_groups``.  Exactly one of ``groups`` ((n_spots,) integer labels, ``-1`` = left
        out) and ``n_niches`` (the ``labels`` of ``get_spatial_niches(n_niches)``) is given.  ``Y``: ``n_spots_`` rows, dense or
        CSR, ANY gene set, tested as it is passed.  Further keywords (``n_groups``, ``pseudocount``, ``n_top``, ``output``) go to
        ``rank_genes_groups``."""
        if (groups is None) == (n_niches is None):
            raise ValueError("exactly one of groups and n_niches must be given")
        self._weights_for(Y, "proportions", None)              # fitted, and Y has the fit's spots as rows
        from ..utils.group_genes import MAX_GROUPS, check_request, rank_genes_groups
        if n_niches is not None:
            if isinstance(n_niches, (int, np.integer)) and n_niches > MAX_GROUPS:
                raise ValueError(f"marker genes are built for at most {MAX_GROUPS} niches, got {n_niches}")
            check_request(tuple(Y.shape), None, None, kw.get("pseudocount", 1e-9), kw.get("n_top"))      # before the k-means
            kw.setdefault("n_groups", n_niches)
            groups = self.get_spatial_niches(n_niches)["labels"]
        return rank_genes_groups(Y, groups, **kw)

    def get_neighborhood_enrichment(self, labels=None, n_niches=None, n_permutations=999, random_state=None, **kw):
        """Which niches or cell types border each other more often than chance over the graph the fit used, and which avoid each
        other (additive, not in the reference): the join counts of spot labels with their exact moments, the analytic z score,
        the interaction matrix and a permutation test on the GPU - ``utils.neighborhoods.neighborhood_enrichment``.  One source
        of labels: ``labels`` ((n_spots,) integers in ``[-1, C)``, ``-1`` = not counted; ``n_labels`` may be passed beside them),
        ``n_niches`` (the ``labels`` of ``get_spatial_niches(n_niches)``, which takes the further keywords) or neither - each
        spot's dominant cell type, with ``C = n_cell_types_``; giving both is a ``ValueError``.  ``random_state``: None is the
        model's.  ``return_null=True`` also returns ``null``.  Works for both ``output`` kinds of ``fit``: labels stay on the
        device where they are."""
        self._require_fitted()
        if labels is not None and n_niches is not None:
            raise ValueError("at most one of labels and n_niches may be given")
        from ..utils._device import check_count
        from ..utils.neighborhoods import _check_flag, neighborhood_enrichment
        check_count("n_permutations", n_permutations)
        return_null = _check_flag("return_null", kw.pop("return_null", False))
        n_labels = kw.pop("n_labels", None)
        labels, n_labels = self._spot_labels(labels, n_niches, n_labels, kw, "neighbourhood enrichment")
        return neighborhood_enrichment(labels, self, n_labels=n_labels, n_permutations=n_permutations,
                                       random_state=self.random_state if random_state is None else random_state,
                                       return_null=return_null)

    def get_co_occurrence(self, coords, labels=None, n_niches=None, radii=None, n_bands=10, n_permutations=999, random_state=None,
                          **kw):
        """At which distances niches or cell types occur together more often than chance, and where the association stops
        (additive, not in the reference): the join counts of spot labels in every distance band of ``radii`` (None: ``n_bands``
        multiples of the grid radius) with their exact moments, the analytic z score, the co-occurrence ratio and a permutation
        test on the GPU - ``utils.cooccurrence.label_cooccurrence``.  The label sources are those of
        ``get_neighborhood_enrichment``: ``labels`` (``n_labels`` may be passed beside them), ``n_niches`` (which takes the further
        keywords of ``get_spatial_niches``) or neither - each spot's dominant cell type; giving both is a ``ValueError``.  The
        model does not keep the coordinates: pass the ones the fit was given (``n_spots_`` rows).  ``random_state``: None is the
        model's.  ``mode`` (``"band"`` or ``"cumulative"``), ``max_candidates`` and ``return_null`` go to ``label_cooccurrence``.
        Works for both ``output`` kinds of ``fit``: labels stay on the device where they are."""
        self._require_fitted()
        if labels is not None and n_niches is not None:
            raise ValueError("at most one of labels and n_niches may be given")
        from ..utils._device import check_count
        from ..utils.cooccurrence import _check_mode, label_cooccurrence
        from ..utils.correlogram import _check_coords, _check_n_bands, _check_radii
        from ..utils.neighborhoods import _check_flag
        check_count("n_permutations", n_permutations)
        return_null = _check_flag("return_null", kw.pop("return_null", False))
        mode, max_candidates = _check_mode(kw.pop("mode", "band")), kw.pop("max_candidates", None)
        n_labels = kw.pop("n_labels", None)
        # the coordinates and the bands fail here, before the k-means (the labels proper are checked with their source)
        shape = tuple(coords.shape) if hasattr(coords, "shape") else np.shape(coords)
        if len(shape) == 2 and shape[0] != self.n_spots_:
            raise ValueError(f"coords must have the {self.n_spots_} spots of the fit as rows, got shape {shape}")
        _check_coords(coords, self.n_spots_)
        if radii is None:
            _check_n_bands(n_bands)
        else:
            _check_radii(radii)
        labels, n_labels = self._spot_labels(labels, n_niches, n_labels, kw, "the co-occurrence")
        return label_cooccurrence(labels, coords, radii=radii, n_bands=n_bands, n_labels=n_labels, n_permutations=n_permutations,
                                  random_state=self.random_state if random_state is None else random_state, mode=mode,
                                  max_candidates=max_candidates, return_null=return_null)

    def _spot_labels(self, labels, n_niches, n_labels, niche_kw, what):
        """``(labels, n_labels)`` of the one label source of a fitted model that the entries on spot labels share (``what`` names
        the entry in the messages): ``labels`` as given (checked, with the fit's spots), the ``labels`` of
        ``get_spatial_niches(n_niches, **niche_kw)``, or - neither given - each spot's dominant cell type."""
        if n_niches is None and niche_kw:
            raise TypeError(f"unexpected keyword arguments without n_niches: {sorted(niche_kw)}")
        if labels is not None:
            from ..utils.neighborhoods import check_labels
            if check_labels(labels, n_labels)[0] != self.n_spots_:
                raise ValueError(f"labels must have the {self.n_spots_} spots of the fit, got {tuple(labels.shape)}")
        elif n_niches is not None:
            if n_labels is not None:
                raise ValueError("n_labels goes with labels: with n_niches the number of labels is n_niches")
            from ..utils.niches import _check_n_niches
            n_labels = _check_n_niches(n_niches, self.n_spots_)              # at most 64 niches: the labels these entries take
            labels = self.get_spatial_niches(n_niches, **niche_kw)["labels"]
        else:
            if n_labels is not None:
                raise ValueError("n_labels goes with labels: the dominant cell types are n_cell_types_ labels")
            if self.n_cell_types_ > 64:
                raise ValueError(f"{what} is built for at most 64 labels, got {self.n_cell_types_} cell types")
            n_labels = int(self.n_cell_types_)
            labels = self.get_dominant_cell_type()
        return labels, n_labels

    def get_ligand_receptor(self, Y, pairs, labels=None, n_niches=None, n_permutations=999, random_state=None, **kw):
        """Between which niches or cell types of this tissue a ligand-receptor pair acts (additive, not in the reference): for every
        pair of ``pairs`` ((P, 2) column indices of ``Y``, ligand then receptor) and every ordered pair of labels (a, b) the mean of
        the ligand in a and of the receptor in b, ranked against random reassignments of the labels to the spots on the GPU -
        ``utils.ligrec.ligand_receptor_test``.  The label sources are those of ``get_neighborhood_enrichment``: ``labels``
        (``n_labels`` may be passed beside them), ``n_niches`` (which takes the further keywords of ``get_spatial_niches``) or
        neither - each spot's dominant cell type; giving both is a ``ValueError``.  ``Y``: ``n_spots_`` rows, dense or CSR, ANY gene
        set, tested as it is passed.  ``random_state``: None is the model's.  ``threshold``, ``n_top`` and ``return_null`` go to
        ``ligand_receptor_test``.  Works for both ``output`` kinds of ``fit``: labels stay on the device where they are."""
        self._weights_for(Y, "proportions", None)              # fitted, and Y has the fit's spots as rows
        if labels is not None and n_niches is not None:
            raise ValueError("at most one of labels and n_niches may be given")
        from ..utils._device import check_count
        from ..utils.ligrec import check_request, ligand_receptor_test
        from ..utils.neighborhoods import _check_flag
        from ..utils.spatial_genes import _check_n_top
        check_count("n_permutations", n_permutations)
        return_null = _check_flag("return_null", kw.pop("return_null", False))
        threshold, n_top = kw.pop("threshold", 0.01), _check_n_top(kw.pop("n_top", None))
        n_labels = kw.pop("n_labels", None)
        # the pairs and the threshold fail here, before the k-means (the labels proper are checked with their source)
        check_request(tuple(Y.shape), pairs, np.zeros(int(Y.shape[0]), dtype=np.int32), None, n_permutations, 0, 0, threshold)
        labels, n_labels = self._spot_labels(labels, n_niches, n_labels, kw, "the ligand-receptor test")
        return ligand_receptor_test(Y, labels, pairs, n_labels=n_labels, n_permutations=n_permutations,
                                    random_state=self.random_state if random_state is None else random_state, threshold=threshold,
                                    n_top=n_top, return_null=return_null)

    def get_dominant_cell_type(self):
        self._require_fitted()
        if hasattr(self.proportions_, "argmax") and not isinstance(self.proportions_, np.ndarray):
            return self.proportions_.argmax(dim=1)
        return np.argmax(self.proportions_, axis=1)

    def summary(self):
        if not self._fitted:
            return {"fitted": False}
        return {
            "fitted": True,
            "n_spots": self.n_spots_,
            "n_cell_types": self.n_cell_types_,
            "n_genes_used": len(self.gene_idx_),
            "sketch_dim": self.sketch_dim,
            "lambda_spatial": self.lambda_used_,
            "rho_sparsity": self.rho_sparsity,
            "preprocess_method": self.preprocess,
            "converged": self.info_["converged"],
            "n_iterations": self.info_["n_iterations"],
            "final_objective": self.info_["final_objective"],
        }

    def __repr__(self):
        status = "fitted" if self._fitted else "not fitted"
        return f"FlashDeconv(sketch_dim={self.sketch_dim}, lambda_spatial={self.lambda_spatial}, status={status})"
