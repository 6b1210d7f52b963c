// The restated cKDTree on the device: the layout the query kernel reads (kdtree_query_dev.cpp), filled by the device build
// (kdtree_build_dev.cpp) or by the upload of a host-built tree (kdtree_order.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include "fdx_internal.h"   // DevBuf; PinnedScope below needs pinned_buffer_get / pinned_buffer_put and fail()

namespace fdx {

struct KdDeviceTree {
    DevBuf meta;        // int4 per node: x = split dimension (-1: leaf), y / z = less / greater node, or first / past-last position of a leaf
    DevBuf split;       // double per node
    DevBuf idx;         // int per point: scipy's index array
    int n_nodes = 0;
    int levels = 0;     // (device build only)
    bool overflow = false;   // a selection would have left introselect's partition loop (heap select), or the tree is deeper than the level cap: build on the host
    double mins[3] = {0, 0, 0}, maxes[3] = {0, 0, 0};   // of the whole set
};

// a recycled pinned buffer for the lifetime of one call (uploads / downloads from pageable memory make the driver pin the caller's
// pages, and unmapping such pages later - a freed vector, a collected numpy array - evicts the process's GPU queues for 10-25 ms)
struct PinnedScope {
    void* p = nullptr;
    size_t cap = 0;
    int get(size_t bytes) { p = pinned_buffer_get(bytes, &cap); return p ? 0 : fail(FDX_ERR_HIP, "ckdtree: pinned host buffer"); }
    ~PinnedScope() { if (p) pinned_buffer_put(p, cap); }
};

// coords_dev: n x dim doubles (dim 1-3).  Queued on `st`; returns after the stream has drained (the node count and the flags are read).
int kd_build_device(const double* coords_dev, long long n, int dim, KdDeviceTree* out, hipStream_t st);

// The k-nearest queries of `rows_host` (NULL: every point in order) on a tree that lies on the device, coords_dev being the (n, dim)
// float64 points it was built from: ids_dev (nq, kk) int64 gets the answers, nearest first, self included, -1 padded.  Returns
// after the stream has drained; *over = 1 when a lane's far-node heap was too deep (the caller repeats the queries on the host).
int kd_queries_device(const double* coords_dev, int dim, int kk, const KdDeviceTree& tree, const long long* rows_host, long long nq,
                      long long* ids_dev, int* over, hipStream_t st);

}  // namespace fdx
