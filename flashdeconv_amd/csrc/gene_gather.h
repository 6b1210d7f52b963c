// The column gather of the per-gene permutation entries (gene_perm_kernels.cpp, label_gene_kernels.cpp): the wanted columns of a
// spot-by-gene matrix in the storage type, in tiles of TG genes, position-major inside a tile:
//   Yt[tile][p][g] = Y[perm[p], genes[tile * TG + g]]     (perm null: position p is the caller's spot p), 0 past S
// so one position's TG values are one contiguous read and a tile is one contiguous block.  CSR: the copy zeroed, then the stored
// entries scattered through a column-to-slot map (a wave per position, a lane per stored entry).
#pragma once
#include <algorithm>

#include "fdx_internal.h"
#include "gene_pass.h"

namespace fdx {

// Yt[tile][p][g] (the tiles of a stripe that begins at gene slot s0, width = tiles * TG slots); a thread per element
template <typename T, int TG>
__global__ __launch_bounds__(256) void gp_gather_dense_kernel(const T* __restrict__ Y, long long ldy, const int* __restrict__ perm,
                                                              long long n, const int* __restrict__ genes, int S, int s0, int width,
                                                              T* __restrict__ Yt) {
    const long long total = n * width;                          // width = nt * TG slots
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long p = e / width;
        const int k = (int)(e - p * width), s = s0 + k;
        const long long row = perm ? perm[p] : p;
        Yt[((size_t)(k / TG) * n + p) * TG + (k % TG)] = s < S ? Y[row * ldy + genes[s]] : (T)0;
    }
}

// Yt (zeroed) takes the stored entries of the stripe's columns: a wave per position, a lane per stored entry of its row
template <typename T, int TG>
__global__ __launch_bounds__(256) void gp_gather_csr_kernel(const long long* __restrict__ indptr, const int* __restrict__ indices,
                                                            const T* __restrict__ values, const int* __restrict__ perm, long long n,
                                                            int G, const int* __restrict__ slot_of, int s0, int width,
                                                            T* __restrict__ Yt) {
    const int lane = threadIdx.x & 63;
    for (long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); p < n; p += (long long)gridDim.x * 4) {
        const long long row = perm ? perm[p] : p;
        const long long e1 = indptr[row + 1];
        for (long long e = indptr[row] + lane; e < e1; e += 64) {
            const int c = indices[e];
            const int k = ((unsigned)c < (unsigned)G ? slot_of[c] : -1) - s0;
            if (k >= 0 && k < width) Yt[((size_t)(k / TG) * n + p) * TG + (k % TG)] = values[e];
        }
    }
}

// One stripe of `tiles` tiles from gene slot s0 on: genes_dev (dense: the S columns) or slot_dev (CSR: the column-to-slot map, -1
// for a column that is not wanted), `data` the dense matrix or the CSR values.
template <typename T, int TG>
int gather_gene_tiles(const int* perm, long long n, const GeneMatrix& y, const T* data, const int* genes_dev, const int* slot_dev, int S,
                      int s0, int tiles, T* Yt, hipStream_t st) {
    const int width = tiles * TG;
    if (y.sparse) {
        FDX_HIP(hipMemsetAsync(Yt, 0, (size_t)n * width * sizeof(T), st));
        hipLaunchKernelGGL((gp_gather_csr_kernel<T, TG>), dim3((unsigned)std::min<long long>(ceil_div(n, 4), 1 << 16)), dim3(256), 0, st,
                           (const long long*)y.csr->indptr, y.csr->indices, data, perm, n, y.G, slot_dev, s0, width, Yt);
    } else {
        const long long blocks = std::min<long long>((n * width + 255) / 256, 1 << 20);
        hipLaunchKernelGGL((gp_gather_dense_kernel<T, TG>), dim3((unsigned)blocks), dim3(256), 0, st, data, y.ldy, perm, n, genes_dev, S,
                           s0, width, Yt);
    }
    FDX_CHECK_LAUNCH();
    return 0;
}

}  // namespace fdx
