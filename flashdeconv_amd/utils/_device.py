"""What the analysis entries under ``utils/`` share on their way to the device (private): the checks of ``values``, of a spot-by-gene
matrix and of the graph argument, the device a call runs on, the upload of a matrix and the routes of a spot-by-gene matrix to the
kernels that stream it.  Everything that can fail on the host fails here, before the GPU is touched."""
import contextlib
import ctypes

import numpy as np

from .. import _lib


def check_values(values, name="values"):
    """(n, K) of a 2-D, non-empty numpy array or torch tensor of floats, called ``name`` in the messages; ``ValueError`` otherwise."""
    shape = tuple(values.shape) if _lib.is_torch(values) else np.shape(values)
    if len(shape) != 2:
        raise ValueError(f"{name} must be a 2-D (n_spots, n_columns) array, got shape {shape}")
    if shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"{name} must not be empty, got shape {shape}")
    dtype = str(values.dtype).replace("torch.", "") if hasattr(values, "dtype") else "float64"
    if _lib.is_cuda_tensor(values) and dtype not in ("float32", "float64"):
        raise ValueError(f"{name} must be float32 or float64, got {dtype}")
    return shape


def check_count(name, v, lo=0):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < lo:
        raise ValueError(f"{name} must be an int >= {lo}, got {v!r}")
    return int(v)


def device_of(*xs):
    """The device of the first CUDA tensor among ``xs``, else torch's current device."""
    import torch
    for x in xs:
        if _lib.is_cuda_tensor(x):
            return x.device
    return torch.device("cuda", torch.cuda.current_device())


def values_on_device(values, device, stream, dtype=None):
    """(device tensor of ``dtype`` - a torch dtype, float64 when None - with unit column stride, row stride)."""
    import torch
    dtype = dtype or torch.float64
    if _lib.is_cuda_tensor(values):
        v = values.detach()
        if v.dtype != dtype:
            v = v.to(dtype)
        if v.stride(1) != 1 or v.stride(0) < v.shape[1]:
            v = v.contiguous()
        return v, v.stride(0)
    if _lib.is_torch(values):
        values = values.detach().numpy()
    a = np.asarray(values)                            # float32 stays float32 on its way up: the upload converts
    a = np.ascontiguousarray(a, dtype=np.float32 if dtype == torch.float32 or a.dtype == np.float32 else np.float64)
    d = torch.empty(a.shape, dtype=dtype, device=device)
    _lib.check(_lib.load().fdx_upload_convert_dev(ctypes.c_void_p(d.data_ptr()), _lib.dtype_code(dtype),
                                                  a.ctypes.data_as(ctypes.c_void_p), _lib.SRC_CODES[a.dtype.name], a.size, None, stream))
    return d, a.shape[1]


def is_scipy_sparse(Y):
    try:
        from scipy import sparse
    except ImportError:                                   # pragma: no cover
        return False
    return sparse.issparse(Y)


def check_matrix(Y):
    """(n, G) of a 2-D spot-by-gene matrix with at least one gene."""
    if not hasattr(Y, "shape"):
        Y = np.asarray(Y)
    shape = tuple(Y.shape)
    if len(shape) != 2:
        raise ValueError(f"Y must be a 2-D (n_spots, n_genes) matrix, got shape {shape}")
    if shape[1] < 1:
        raise ValueError(f"Y must have at least one gene, got shape {shape}")
    if _lib.is_cuda_tensor(Y) and not _lib.is_torch_sparse_csr(Y) and str(Y.layout) != "torch.strided":
        raise ValueError(f"a sparse CUDA Y must be torch.sparse_csr, got {Y.layout}")
    return int(shape[0]), int(shape[1])


@contextlib.contextmanager
def matrix_on_device(Y, device):
    """The spot-by-gene matrix ``Y`` as the kernels stream it, for the length of a ``with`` block: ``("csr", CsrOnDevice)`` for a
    scipy sparse matrix or a CUDA ``torch.sparse_csr`` tensor (rows as they are: not sorted), else ``("dense", pointer, dtype code,
    row stride)`` - a dense CUDA tensor where it lies (integer counts converted, a column stride removed), a host matrix through
    ``_lib.upload_matrix``.  What was uploaded for the call is freed at the end of the block, after torch's current stream has
    finished with it."""
    import torch
    if is_scipy_sparse(Y) or _lib.is_torch_sparse_csr(Y):
        csr = _lib.CsrOnDevice.from_scipy(Y, sort=False) if is_scipy_sparse(Y) else _lib.CsrOnDevice.from_torch(Y)
        try:
            yield ("csr", csr)
            torch.cuda.current_stream(device).synchronize()       # the arrays go back to the allocator below
        finally:
            csr.free()
    elif _lib.is_cuda_tensor(Y):
        Yd = Y.detach()
        if Yd.dtype not in (torch.float32, torch.float64):
            from ..core.deconv import device_counts_as_float
            Yd, _ = device_counts_as_float(Yd)
        if Yd.stride(1) != 1 or Yd.stride(0) < Yd.shape[1]:
            Yd = Yd.contiguous()
        yield ("dense", ctypes.c_void_p(Yd.data_ptr()), _lib.dtype_code(Yd), int(Yd.stride(0)))
    else:
        Yh = Y.detach().numpy() if _lib.is_torch(Y) else np.asarray(Y)
        ptr, code = _lib.upload_matrix(Yh)
        try:
            yield ("dense", ptr, code, int(Yh.shape[1]))
            torch.cuda.current_stream(device).synchronize()
        finally:
            _lib.load().fdx_free(ptr)


def _check_adjacency(A, n_rows):
    """A scipy sparse adjacency as canonical CSR; shape, symmetry and the empty diagonal are checked on the host."""
    if A.ndim != 2 or A.shape[0] != A.shape[1]:
        raise ValueError(f"graph must be a square adjacency matrix, got shape {A.shape}")
    if A.shape[0] != n_rows:
        raise ValueError(f"values has {n_rows} rows but the graph has {A.shape[0]} spots")
    A = A.tocsr().astype(bool).astype(np.int8)        # binary weights: stored values only mark the edges
    A.eliminate_zeros()
    A.sum_duplicates()
    A.sort_indices()
    if A.diagonal().any():
        raise ValueError("graph must have no self loops (a non-zero diagonal entry was found)")
    if (A != A.T).nnz != 0:
        raise ValueError("graph must be symmetric")
    return A


def resolve_graph(graph, n_rows):
    """(_lib.Graph, owned): the device graph behind `graph`; owned graphs are closed by the caller."""
    if isinstance(graph, _lib.Graph):
        g, owned = graph, False
    elif hasattr(graph, "_graph") and hasattr(graph, "_require_fitted"):      # a FlashDeconv
        graph._require_fitted()
        if graph._graph is None:
            raise RuntimeError("Model has not been fitted. Call fit() first.")
        g, owned = graph._graph, False
    elif hasattr(graph, "tocsr"):
        A = _check_adjacency(graph, n_rows)
        _lib.require_gpu()
        return _lib.Graph.from_csr(A.indptr, A.indices, A.shape[0]), True
    else:
        raise TypeError("graph must be a fitted FlashDeconv, a flashdeconv_amd._lib.Graph or a scipy sparse adjacency matrix, "
                        f"got {type(graph).__name__}")
    n = g.info()[0]
    if n != n_rows:
        raise ValueError(f"values has {n_rows} rows but the graph has {n} spots")
    return g, owned


@contextlib.contextmanager
def resolved_graph(graph, n_rows):
    """The device graph behind `graph` for the length of a ``with`` block; a graph uploaded for the call is closed at its end."""
    g, owned = resolve_graph(graph, n_rows)
    try:
        yield g
    finally:
        if owned:
            g.close()
