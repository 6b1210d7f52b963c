// Graph build, steps 4-5 (graph_internal.h): radius lists, union symmetrisation, sliced ELL, the sweep's tile tables, export.
// The stages a shard's build shares with the whole-graph builds are the host functions declared in graph_internal.h.
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "graph_internal.h"

namespace fdx {

// ------------------------------------------------------------------------------------------------ radius graph
// PASS 0 counts, PASS 1 fills nbr[off[p] + m] (sorted-space indices, unsorted order)
template <int PASS>
__global__ __launch_bounds__(128) void radius_kernel(const double* __restrict__ sc, const int* __restrict__ cstart,
                                                     const int* __restrict__ cend, long long n, GridParams gp,
                                                     double radius, int R, int* __restrict__ cnt,
                                                     const int* __restrict__ off, int* __restrict__ nbr, long long lo,
                                                     long long hi) {
    const long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (p >= n) return;
    if (p < lo || p >= hi) {                                               // a shard builds its own rows; the others stay empty
        if (!PASS) cnt[p] = 0;
        return;
    }
    const double px = sc[p], py = sc[(size_t)n + p], pz = sc[2 * (size_t)n + p];
    const double pc[3] = {px, py, pz};
    int c[3];
    for (int a = 0; a < 3; ++a) c[a] = (a < gp.dim) ? cell_coord(pc[a], gp.mn[a], gp.inv_h[a], gp.nc[a]) : 0;
    int m = 0;
    const int base = PASS ? off[p] : 0;
    for (int z = max(0, c[2] - R); z <= min(gp.nc[2] - 1, c[2] + R); ++z)
        for (int y = max(0, c[1] - R); y <= min(gp.nc[1] - 1, c[1] + R); ++y)
            for (int x = max(0, c[0] - R); x <= min(gp.nc[0] - 1, c[0] + R); ++x) {
                const int cell = x * gp.stride[0] + y * gp.stride[1] + z * gp.stride[2];
                for (int q = cstart[cell]; q < cend[cell]; ++q) {
                    if (q == (int)p) continue;
                    const double d2 = dist2_exact(sc[q] - px, sc[(size_t)n + q] - py, sc[2 * (size_t)n + q] - pz);
                    if (sqrt(d2) <= radius) {   // query_pairs(r): distance <= r   (graph.py:115)
                        if (PASS) nbr[base + m] = q;
                        ++m;
                    }
                }
            }
    if (!PASS) cnt[p] = m;
}

// ------------------------------------------------------------------------------------------------ symmetrise
// in-degrees / reverse lists over the rows that HAVE lists (every other row is skipped without a look at its count); only edges
// INTO rows [lo, hi) count (a shard builds its own rows)
__global__ __launch_bounds__(256) void indegree_kernel(const int* __restrict__ nbr, const int* __restrict__ nbr_cnt, int kk,
                                                       const RowSet rs, int* __restrict__ indeg, int lo, int hi) {
    const long long p = row_of_set(rs, blockIdx.x * 256LL + threadIdx.x);
    if (p < 0) return;
    for (int m = 0; m < nbr_cnt[p]; ++m) {
        const int q = nbr[(size_t)p * kk + m];
        if (q >= lo && q < hi) atomicAdd(&indeg[q], 1);
    }
}

__global__ __launch_bounds__(256) void fill_reverse_kernel(const int* __restrict__ nbr, const int* __restrict__ nbr_cnt, int kk,
                                                           const RowSet rs, const int* __restrict__ rev_off,
                                                           int* __restrict__ cursor, int* __restrict__ rev, int lo, int hi) {
    const long long p = row_of_set(rs, blockIdx.x * 256LL + threadIdx.x);
    if (p < 0) return;
    for (int m = 0; m < nbr_cnt[p]; ++m) {
        const int q = nbr[(size_t)p * kk + m];
        if (q >= lo && q < hi) rev[rev_off[q] + atomicAdd(&cursor[q], 1)] = (int)p;
    }
}

// the same with the places drawn by the k-NN kernel: plain stores
__global__ __launch_bounds__(256) void fill_reverse_placed_kernel(const int* __restrict__ nbr, const int* __restrict__ nbr_cnt,
                                                                  const int* __restrict__ arrival, long long n, int kk,
                                                                  const int* __restrict__ rev_off, int* __restrict__ rev) {
    const long long p = blockIdx.x * 256LL + threadIdx.x;
    if (p >= n) return;
    for (int m = 0; m < nbr_cnt[p]; ++m) rev[rev_off[nbr[(size_t)p * kk + m]] + arrival[(size_t)p * kk + m]] = (int)p;
}

// Row p: candidates = out(p) U in(p) -> sorted by ORIGINAL index, duplicates removed, stored at ws[seg_off(p) ...].
// seg_off(p) = p*kk + rev_off[p] (capacity kk + indeg[p]).  The arrival order of the reverse list is arbitrary (atomics);
// sorting makes the result deterministic.
__global__ __launch_bounds__(128) void merge_rows_kernel(const int* __restrict__ nbr, const int* __restrict__ nbr_cnt,
                                                         const int* __restrict__ rev, const int* __restrict__ rev_off,
                                                         const int* __restrict__ perm, const int* __restrict__ rank,
                                                         long long lo, long long hi, int kk,
                                                         int* __restrict__ ws, int* __restrict__ deg) {
    const long long p = lo + blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (p >= hi) return;
    int* seg = ws + (size_t)p * kk + rev_off[p];
    const int n_out = nbr_cnt[p], n_in = rev_off[p + 1] - rev_off[p];
    const int m = n_out + n_in;
    constexpr int CAP = 32;
    __shared__ int keys[CAP * 128];                  // keys[a * 128 + tid]: a thread's slots are 128 apart -> conflict-free
    if (m <= CAP) {
        // common case: sort the ORIGINAL indices (a bijection of the positions: rank[] leads back) in LDS and write the row
        // ONCE.  (An in-place insertion sort in global memory costs a 64-byte write per 4-byte move - measured 2 GB written
        // for 100 MB - and a private key[] array is dynamically indexed, i.e. scratch memory: 3.5 ms at 8M spots.  32-bit
        // keys: 16 KB per workgroup, twice the resident workgroups of the (original index, position) pairs used before.)
        int* key = keys + threadIdx.x;
        for (int t = 0; t < n_out; ++t) key[t * 128] = perm[nbr[(size_t)p * kk + t]];
        for (int t = 0; t < n_in; ++t) key[(n_out + t) * 128] = perm[rev[rev_off[p] + t]];
        for (int a = 1; a < m; ++a) {
            const int kv = key[a * 128];
            int b = a - 1;
            while (b >= 0 && key[b * 128] > kv) { key[(b + 1) * 128] = key[b * 128]; --b; }
            key[(b + 1) * 128] = kv;
        }
        int u = 0;
        int prev = -1;
        for (int a = 0; a < m; ++a) {
            const int kv = key[a * 128];
            if (a == 0 || kv != prev) seg[u++] = rank[kv];
            prev = kv;
        }
        deg[p] = u;
        return;
    }
    int mm = 0;
    for (int t = 0; t < n_out; ++t) seg[mm++] = nbr[(size_t)p * kk + t];
    for (int t = rev_off[p]; t < rev_off[p + 1]; ++t) seg[mm++] = rev[t];
    for (int a = 1; a < mm; ++a) {   // insertion sort by original index
        const int v = seg[a];
        const int kv = perm[v];
        int b = a - 1;
        while (b >= 0 && perm[seg[b]] > kv) { seg[b + 1] = seg[b]; --b; }
        seg[b + 1] = v;
    }
    int u = 0;
    for (int a = 0; a < mm; ++a)
        if (a == 0 || seg[a] != seg[a - 1]) seg[u++] = seg[a];
    deg[p] = u;
}

// Variant for already-symmetric neighbour lists with explicit offsets (radius graph): sort only.
__global__ __launch_bounds__(128) void sort_rows_kernel(int* __restrict__ nbr, const int* __restrict__ off,
                                                        const int* __restrict__ perm, long long n) {
    const long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (p >= n) return;
    int* seg = nbr + off[p];
    const int m = off[p + 1] - off[p];
    for (int a = 1; a < m; ++a) {
        const int v = seg[a];
        const int kv = perm[v];
        int b = a - 1;
        while (b >= 0 && perm[seg[b]] > kv) { seg[b + 1] = seg[b]; --b; }
        seg[b + 1] = v;
    }
}

// ------------------------------------------------------------------------------------------------ ELL
// width[s] = widest row of slice s; per block the sum of its degrees and its widest slice (part[2b], part[2b + 1]).
// (One atomic per slice on a single pair of counters was 370 us at 1M spots: 31k same-address atomics, ~12 ns each.)
// zero_tail: the closing entry of the scan's input (width[n_slices]) and the two summary words the tile kernel raises are cleared
// here instead of by a fill of their own in front of this launch
__global__ __launch_bounds__(256) void slice_width_kernel(const int* __restrict__ deg, long long n, int n_slices,
                                                          int* __restrict__ width, long long* __restrict__ part,
                                                          int* __restrict__ summary_zero = nullptr) {
    __shared__ long long s_sum[4];
    __shared__ int s_max[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (summary_zero && blockIdx.x == 0 && threadIdx.x == 0) { width[n_slices] = 0; summary_zero[0] = 0; summary_zero[1] = 0; }
    long long tot = 0;
    int wmax = 0;
    for (int s = blockIdx.x * 4 + wv; s < n_slices; s += gridDim.x * 4) {
        const long long i = (long long)s * 64 + lane;
        const int d = (i < n) ? deg[i] : 0;
        int w = d, sum = d;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            w = max(w, __shfl_xor(w, off, 64));
            sum += __shfl_xor(sum, off, 64);
        }
        if (lane == 0) width[s] = w;
        tot += sum;
        wmax = max(wmax, w);
    }
    if (lane == 0) { s_sum[wv] = tot; s_max[wv] = wmax; }
    __syncthreads();
    if (threadIdx.x == 0 && part) {
        part[2 * blockIdx.x] = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
        part[2 * blockIdx.x + 1] = (long long)max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
    }
}

// red[0] = nnz, red[1] = widest slice, from the blocks' partials; with `meta` (a queued build): the numbers the host will ask
// for, written straight into its pinned block (one launch instead of a copy each)
__global__ __launch_bounds__(256) void graph_meta_kernel(const long long* __restrict__ part, int n_part, long long* __restrict__ red,
                                                         const int* __restrict__ slice_off, int n_slices,
                                                         const int* __restrict__ summary, const int* __restrict__ ties,
                                                         long long* __restrict__ meta) {
    long long nnz;
    int widest;
    reduce_width_partials(part, n_part, &nnz, &widest);
    if (threadIdx.x != 0) return;
    red[0] = nnz;
    red[1] = (long long)widest;
    if (meta) write_meta_head(meta, slice_off, n_slices, nnz, widest, summary, ties);
}

// seg_off(p) = p*seg_stride + seg_extra[p]   (k-NN: seg_stride = kk, seg_extra = rev_off; radius: stride 0, extra = off)
// LOCAL (a shard's local graph straight from its n own rows' segments): own neighbour -> q - lo, outside -> n + its halo slot
// hscan[q], pad -> n + the number of halo slots hscan[n_all]
template <bool LOCAL>
__global__ __launch_bounds__(256) void fill_ell_kernel(const int* __restrict__ ws, int seg_stride,
                                                       const int* __restrict__ seg_extra, const int* __restrict__ deg,
                                                       const int* __restrict__ slice_off, long long n, int n_slices,
                                                       int pad, int* __restrict__ ell, long long cap_rows, long long lo,
                                                       const int* __restrict__ hscan, long long n_all) {
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= n_slices) return;
    if ((long long)slice_off[n_slices] > cap_rows) return;      // queued build with too small a bound: rebuilt later
    const long long i = (long long)s * 64 + lane;
    const int w0 = slice_off[s], w = slice_off[s + 1] - w0;
    const int dg = (i < n) ? deg[i] : 0;
    const int* seg = (i < n) ? ws + (size_t)i * seg_stride + seg_extra[i] : ws;
    if (LOCAL) pad = (int)n + hscan[n_all];
    for (int m = 0; m < w; ++m) {
        int v = pad;
        if (m < dg) {
            v = seg[m];
            if (LOCAL) v = (v >= lo && v < lo + n) ? (int)(v - lo) : (int)n + hscan[v];
        }
        ell[((size_t)w0 + m) * 64 + lane] = v;
    }
}

// export: CSR in the caller's labels.  deg_orig[perm[p]] = deg[p]; then indices[indptr[o] + m] = perm[seg_p[m]].
__global__ __launch_bounds__(256) void deg_to_orig_kernel(const int* __restrict__ deg, const int* __restrict__ perm,
                                                          long long n, int* __restrict__ deg_orig) {
    const long long p = blockIdx.x * 256LL + threadIdx.x;
    // rows without entries are skipped, not copied (deg_orig arrives zeroed): the full-size graph of a spot shard has its
    // permutation laid out only where the shard looks (bin_points, shard mode) - an empty row's perm[p] is not data there
    if (p < n && deg[p] > 0) deg_orig[perm[p]] = deg[p];
}

__global__ __launch_bounds__(256) void export_rows_kernel(const int* __restrict__ ws, int seg_stride,
                                                          const int* __restrict__ seg_extra, const int* __restrict__ deg,
                                                          const int* __restrict__ perm, const long long* __restrict__ indptr,
                                                          long long n, int* __restrict__ indices) {
    const long long p = blockIdx.x * 256LL + threadIdx.x;
    if (p >= n || deg[p] <= 0) return;              // empty rows: nothing to write, and (spot shards) no valid perm[p] to look up
    const int* seg = ws + (size_t)p * seg_stride + seg_extra[p];
    const long long base = indptr[perm[p]];
    for (int m = 0; m < deg[p]; ++m) indices[base + m] = perm[seg[m]];
}

__global__ __launch_bounds__(256) void iota_kernel(int* __restrict__ v, long long n) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i < n) v[i] = (int)i;
}

// ------------------------------------------------------------------------------------------------ sweep tiles
// A tile = 256 consecutive sorted spots = one workgroup of the tiled BCD sweep.  For every tile: the sorted, duplicate-
// free list of neighbour positions OUTSIDE the tile (its halo), and every ELL entry of its rows translated to a
// tile-local slot: 0..255 own spot, 256+h the h-th halo entry, 256+H the all-zero pad slot.
constexpr int TILE_HASH = 2048;
// SEG: a row is read from its segment (src, seg_stride, seg_extra) and goes to the global-index ELL too - fill_ell_kernel and the
// tile tables in one pass over the rows; else src is the ELL and the row is read from there
template <bool SEG>
__device__ __forceinline__ void tile_tables(const int* __restrict__ src, int seg_stride, const int* __restrict__ seg_extra, int pad,
                                            int* __restrict__ ell, const int* __restrict__ deg, const int* __restrict__ slice_off,
                                            long long n, int* __restrict__ tile_halo, int* __restrict__ tile_hcnt,
                                            unsigned short* __restrict__ ell_local, long long cap_rows,
                                            int* __restrict__ summary /* [0] largest halo, [1] some tile failed */) {
    if ((long long)slice_off[(n + 63) >> 6] > cap_rows) return;
    __shared__ int tab[TILE_HASH];
    __shared__ int list[FDX_TILE_HALO_CAP];
    __shared__ int s_cnt, s_over;
    const int tid = threadIdx.x, tile = blockIdx.x;
    for (int s = tid; s < TILE_HASH; s += 256) tab[s] = -1;
    if (tid == 0) { s_cnt = 0; s_over = 0; }
    __syncthreads();
    const long long p = (long long)tile * 256 + tid;
    const int dg = (p < n) ? deg[p] : 0;
    // row p: entry m at seg[m * step] - in its segment, or in the sliced ELL at src[(slice_off[p/64] + m)*64 + p%64]
    constexpr size_t step = SEG ? 1 : 64;
    const int* seg = SEG ? ((p < n) ? src + (size_t)p * seg_stride + seg_extra[p] : src)
                         : ((p < n) ? src + (size_t)slice_off[p >> 6] * 64 + (p & 63) : src);
    // SEG: every lane of the last slice writes - lanes past n carry the pad index / the zero slot
    const bool writes = SEG ? (p >> 6) < ((n + 63) >> 6) : p < n;
    const int sl = (int)(p >> 6), lane = (int)(p & 63);
    for (int m = 0; m < dg; ++m) {
        const int q = seg[m * step];
        if ((q >> 8) == tile && q < n) continue;          // a LOCAL graph's halo slots n..n_total-1 can carry the last tile's number: they are halo
        unsigned h = ((unsigned)q * 2654435761u) >> 21;   // 11 bits
        int probes = 0;
        while (true) {
            const int old = atomicCAS(&tab[h], -1, q);
            if (old == -1 || old == q) break;
            h = (h + 1) & (TILE_HASH - 1);
            if (++probes > TILE_HASH) { s_over = 1; break; }
        }
    }
    __syncthreads();
    for (int s = tid; s < TILE_HASH; s += 256)
        if (tab[s] != -1) {
            const int pos = atomicAdd(&s_cnt, 1);
            if (pos < FDX_TILE_HALO_CAP) list[pos] = tab[s];
        }
    __syncthreads();
    const int H = s_cnt;
    if (H > FDX_TILE_HALO_CAP || s_over) {      // irregular graph: this tile cannot use the LDS path - the global-index ELL is still written
        if (tid == 0) { tile_hcnt[tile] = -1; if (summary) atomicOr(summary + 1, 1); }
        if (SEG && writes) {
            const int w0 = slice_off[sl], w = slice_off[sl + 1] - w0;
            for (int m = 0; m < w; ++m) ell[((size_t)w0 + m) * 64 + lane] = (m < dg) ? seg[m] : pad;
        }
        return;
    }
    if (tid == 0 && summary && H > __builtin_nontemporal_load(summary)) atomicMax(summary, H);   // a glance first: one address for 4000 tiles
    int P = 1;
    while (P < H) P <<= 1;
    for (int s = H + tid; s < P; s += 256) list[s] = 0x7fffffff;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int idx = tid; idx < P; idx += 256) {
                const int ixj = idx ^ j;
                if (ixj > idx) {
                    const int a = list[idx], b = list[ixj];
                    const bool up = ((idx & k) == 0);
                    if ((a > b) == up) { list[idx] = b; list[ixj] = a; }
                }
            }
            __syncthreads();
        }
    for (int h = tid; h < H; h += 256) tile_halo[(size_t)tile * FDX_TILE_HALO_CAP + h] = list[h];
    if (tid == 0) tile_hcnt[tile] = H;
    if (writes) {
        const int w0 = slice_off[sl], w = slice_off[sl + 1] - w0;
        for (int m = 0; m < w; ++m) {
            int slot = 256 + H;   // pad -> zero slot
            if (SEG && m >= dg) ell[((size_t)w0 + m) * 64 + lane] = pad;
            if (m < dg) {
                const int q = seg[m * step];
                if (SEG) ell[((size_t)w0 + m) * 64 + lane] = q;
                if ((q >> 8) == tile && q < n) slot = q & 255;
                else {
                    int lo = 0, hi = H;   // lower_bound in the sorted halo list
                    while (lo < hi) { const int mid = (lo + hi) >> 1; if (list[mid] < q) lo = mid + 1; else hi = mid; }
                    slot = 256 + lo;
                }
            }
            ell_local[((size_t)w0 + m) * 64 + lane] = (unsigned short)slot;
        }
    }
}

__global__ __launch_bounds__(256) void tile_halo_kernel(const int* __restrict__ ell, const int* __restrict__ deg,
                                                        const int* __restrict__ slice_off, long long n,
                                                        int* __restrict__ tile_halo, int* __restrict__ tile_hcnt,
                                                        unsigned short* __restrict__ ell_local, long long cap_rows,
                                                        int* __restrict__ summary) {
    tile_tables<false>(ell, 0, nullptr, 0, nullptr, deg, slice_off, n, tile_halo, tile_hcnt, ell_local, cap_rows, summary);
}

// the one-pass form (queued whole-graph build)
__global__ __launch_bounds__(256) void tile_ell_kernel(const int* __restrict__ ws, int seg_stride, const int* __restrict__ seg_extra,
                                                       int pad, int* __restrict__ ell, const int* __restrict__ deg,
                                                       const int* __restrict__ slice_off, long long n,
                                                       int* __restrict__ tile_halo, int* __restrict__ tile_hcnt,
                                                       unsigned short* __restrict__ ell_local, long long cap_rows,
                                                       int* __restrict__ summary) {
    tile_tables<true>(ws, seg_stride, seg_extra, pad, ell, deg, slice_off, n, tile_halo, tile_hcnt, ell_local, cap_rows, summary);
}

// ------------------------------------------------------------------------------------------------ host side
int exclusive_scan_int(const int* in, int* out, long long count, hipStream_t st, DevBuf& tmp) {
    return with_temp(tmp, [&](void* t, size_t& bytes) {
        return rocprim::exclusive_scan(t, bytes, in, out, 0, (size_t)count, rocprim::plus<int>(), st);
    });
}

static int exclusive_scan_i64(const int* in, long long* out, long long count, hipStream_t st, DevBuf& tmp) {
    auto in64 = rocprim::make_transform_iterator(in, [] __device__(int v) { return (long long)v; });
    return with_temp(tmp, [&](void* t, size_t& bytes) {
        return rocprim::exclusive_scan(t, bytes, in64, out, 0LL, (size_t)count, rocprim::plus<long long>(), st);
    });
}

int queue_slice_offsets(const int* deg, long long n, int n_slices, int wblocks, int* width, long long* part, int* summary_zero,
                        int* slice_off, hipStream_t st, DevBuf& scan_tmp) {
    hipLaunchKernelGGL(slice_width_kernel, dim3(wblocks), dim3(256), 0, st, deg, n, n_slices, width, part, summary_zero);
    FDX_CHECK_LAUNCH();
    return exclusive_scan_int(width, slice_off, n_slices + 1, st, scan_tmp);
}

int ell_w_cap(int list_len, bool forced) {
    return forced ? std::max(1, atoi(fdx::env("FDX_GRAPH_WCAP"))) : std::min(96, std::max(24, 3 * std::max(list_len, 1) + 3));
}

int queue_fill_ell(const int* ws, int seg_stride, const int* seg_extra, const int* deg, const int* slice_off, long long n, int n_slices,
                   int pad, int* ell, long long cap_rows, hipStream_t st, long long lo, const int* hscan, long long n_all) {
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(ceil_div(n_slices, 4)), dim3(256), 0, st, ws, seg_stride, seg_extra, deg, slice_off, n, n_slices, pad,
                           ell, cap_rows, lo, hscan, n_all);
    };
    if (hscan) go(fill_ell_kernel<true>);
    else go(fill_ell_kernel<false>);
    FDX_CHECK_LAUNCH();
    return 0;
}

int queue_tile_tables(fdx_graph* g, long long cap_rows, int* summary, hipStream_t st, const int* ws, int seg_stride, const int* seg_extra) {
    FDX_TRY(g->tile_halo.alloc((size_t)g->n_tiles * FDX_TILE_HALO_CAP * 4));
    FDX_TRY(g->tile_hcnt.alloc((size_t)g->n_tiles * 4));
    FDX_TRY(g->ell_local.alloc(((size_t)cap_rows + 16) * 64 * 2));   // + 16 rows: the tiled sweep loads 16 rows per slice unconditionally
    if (g->n_tiles <= 0) return 0;
    if (ws)
        hipLaunchKernelGGL(tile_ell_kernel, dim3(g->n_tiles), dim3(256), 0, st, ws, seg_stride, seg_extra, (int)g->n_total, g->ell.as<int>(),
                           g->deg.as<int>(), g->slice_off.as<int>(), g->n, g->tile_halo.as<int>(), g->tile_hcnt.as<int>(),
                           g->ell_local.as<unsigned short>(), cap_rows, summary);
    else
        hipLaunchKernelGGL(tile_halo_kernel, dim3(g->n_tiles), dim3(256), 0, st, g->ell.as<int>(), g->deg.as<int>(), g->slice_off.as<int>(),
                           g->n, g->tile_halo.as<int>(), g->tile_hcnt.as<int>(), g->ell_local.as<unsigned short>(), cap_rows, summary);
    FDX_CHECK_LAUNCH();
    return 0;
}

// workgroup tiles of the LDS-tiled sweep (needs g->ell / deg / slice_off / ell_rows / n)
static int build_tiles(fdx_graph* g, hipStream_t st) {
    g->n_tiles = (int)((g->n + 255) / 256);
    g->tiled = false;
    g->halo_max = 0;
    if (g->n_tiles > 0 && g->ell_rows > 0) {
        FDX_TRY(queue_tile_tables(g, g->ell_rows, nullptr, st));
        trace_host("tiles: allocs + kernel");
        std::vector<int> hc((size_t)g->n_tiles);
        FDX_HIP(hipMemcpyAsync(hc.data(), g->tile_hcnt.p, hc.size() * 4, hipMemcpyDeviceToHost, st));
        FDX_HIP(hipStreamSynchronize(st));
        trace_host("tiles: read-back + sync");
        bool ok = true;
        int mx = 0;
        for (int v : hc) { if (v < 0) ok = false; mx = std::max(mx, v); }
        g->tiled = ok;
        g->halo_max = mx;
        if (fdx::env("FDX_TRACE_HOST")) std::fprintf(stderr, "[fdx-host] tiles: %d tiles, largest halo %d, tiled %d\n", g->n_tiles, mx, (int)ok);
    }
    return 0;
}

// deg + row segments -> sliced ELL inside g (pad index = n_total)
// defer: nothing is read back here - the ELL gets room for ell_w_cap entries per row on average (the kernels stop at that bound),
// the tile tables are built behind it and the counts travel to pinned memory behind g->meta_event (graph_meta_sync).
// no_tiles (the full-size graph of a spot shard: only rows [lo, hi) are filled): no tile tables - graph_localize builds the local
// graph's own, and a pass over all n / 256 tiles here would be the shard's only work proportional to the whole graph
static int finish_ell(fdx_graph* g, const int* ws, int seg_stride, const int* seg_extra, hipStream_t st, bool defer = false,
                      bool no_tiles = false) {
    const long long n = g->n;
    g->n_slices = (int)((n + 63) / 64);
    DevBuf width, tmp;
    // width (n_slices + 1 ints), then - 16-byte aligned - red: [0] nnz, [1] widest slice; summary (2 ints, zeroed); the blocks'
    // partials.  One block, one fill.
    const int wblocks = std::min(SLICE_WIDTH_BLOCKS, std::max(1, ceil_div(g->n_slices, 4)));
    const size_t red_at = ((size_t)(g->n_slices + 1) * 4 + 15) / 16 * 16;
    FDX_TRY(width.alloc(red_at + 32 + (size_t)wblocks * 16));
    FDX_TRY(g->slice_off.alloc((size_t)(g->n_slices + 1) * 4));
    long long* red = reinterpret_cast<long long*>(static_cast<char*>(width.p) + red_at);
    int* summary = reinterpret_cast<int*>(red + 2);
    long long* part = red + 4;
    FDX_TRY(queue_slice_offsets(g->deg.as<int>(), n, g->n_slices, wblocks, width.as<int>(), part, summary, g->slice_off.as<int>(), st, tmp));
    trace_host("ell: width + sums + scan");
    if (defer) {
        // a graph that needs more room than the bound (hubs) is rebuilt with its exact size by graph_meta_sync
        const long long cap = (long long)g->n_slices * ell_w_cap(seg_stride, fdx::env("FDX_GRAPH_WCAP") != nullptr);   // tests: force the rebuild
        g->ell_cap_rows = cap;
        g->n_tiles = (int)((n + 255) / 256);
        FDX_TRY(g->ell.alloc((size_t)std::max<long long>(cap, 1) * 64 * 4));
        const bool one_pass = !fdx::env("FDX_GRAPH_TWO_ELL_KERNELS");
        if (!one_pass)
            FDX_TRY(queue_fill_ell(ws, seg_stride, seg_extra, g->deg.as<int>(), g->slice_off.as<int>(), n, g->n_slices, (int)g->n_total,
                                   g->ell.as<int>(), cap, st));
        FDX_TRY(queue_tile_tables(g, cap, summary, st, one_pass ? ws : nullptr, seg_stride, seg_extra));
        if (!g->meta_host) g->meta_host = (long long*)pinned_block_get();
        FDX_REQUIRE(g->meta_host != nullptr, "graph: pinned host block");
        if (!g->meta_event) FDX_HIP(hipEventCreateWithFlags(&g->meta_event, hipEventDisableTiming));
        for (int j = 0; j < 8; ++j) g->meta_host[j] = 0;
        void* meta_dev = nullptr;                    // the block's words: write_meta_head
        FDX_HIP(hipHostGetDevicePointer(&meta_dev, g->meta_host, 0));
        hipLaunchKernelGGL(graph_meta_kernel, dim3(1), dim3(256), 0, st, part, wblocks, red, g->slice_off.as<int>(), g->n_slices, summary,
                           g->ties_dev.as<int>(), (long long*)meta_dev);
        FDX_CHECK_LAUNCH();
        FDX_HIP(hipEventRecord(g->meta_event, st));
        g->meta_stream = st;
        g->meta_pending = true;
        g->ell_rows = 0; g->nnz = 0; g->max_deg = 0; g->tiled = false; g->halo_max = 0;   // until graph_meta_sync
        trace_host("ell: deferred build queued");
        return 0;
    }
    hipLaunchKernelGGL(graph_meta_kernel, dim3(1), dim3(256), 0, st, part, wblocks, red, nullptr, 0, nullptr, nullptr, nullptr);
    FDX_CHECK_LAUNCH();
    int total = 0;
    FDX_HIP(hipMemcpyAsync(&total, g->slice_off.as<int>() + g->n_slices, 4, hipMemcpyDeviceToHost, st));
    long long h_red[2] = {0, 0};
    int h_ties[2] = {0, 0};
    FDX_HIP(hipMemcpyAsync(h_red, red, 16, hipMemcpyDeviceToHost, st));
    if (g->ties_dev.p) FDX_HIP(hipMemcpyAsync(h_ties, g->ties_dev.p, std::min<size_t>(8, g->ties_dev.bytes), hipMemcpyDeviceToHost, st));
    FDX_HIP(hipStreamSynchronize(st));
    g->knn_ties = h_ties[0];
    g->knn_far = h_ties[1];
    trace_host("ell: read-back + sync");
    g->ell_rows = total;
    g->nnz = h_red[0];
    g->max_deg = (int)(h_red[1] & 0xffffffffLL);
    FDX_TRY(g->ell.alloc((size_t)std::max<long long>(g->ell_rows, 1) * 64 * 4));
    FDX_TRY(queue_fill_ell(ws, seg_stride, seg_extra, g->deg.as<int>(), g->slice_off.as<int>(), n, g->n_slices, (int)g->n_total,
                           g->ell.as<int>(), (long long)g->ell_rows, st));
    trace_host("ell: alloc + fill_ell");
    if (no_tiles) { g->n_tiles = (int)((n + 255) / 256); g->tiled = false; g->halo_max = 0; return 0; }
    FDX_TRY(build_tiles(g, st));
    return 0;
}

static int empty_graph(long long n, fdx_graph* g, hipStream_t st) {
    g->n = n; g->n_total = n; g->nnz = 0; g->max_deg = 0; g->ell_rows = 0;
    g->n_slices = (int)((n + 63) / 64);
    g->identity_order = true;
    FDX_TRY(g->deg.alloc((size_t)std::max<long long>(n, 1) * 4));
    FDX_TRY(g->slice_off.alloc((size_t)(g->n_slices + 1) * 4));
    FDX_TRY(g->ell.alloc(256));
    FDX_HIP(hipMemsetAsync(g->deg.p, 0, g->deg.bytes, st));
    FDX_HIP(hipMemsetAsync(g->slice_off.p, 0, g->slice_off.bytes, st));
    FDX_HIP(hipStreamSynchronize(st));
    return 0;
}

int symmetrise_rows(const int* nbr, const int* cnt, int kk, const RowSet& rs, long long lo, long long hi, long long base, long long count,
                    int* indeg, int* cursor, int* rev_off, const int* arrival, DevBuf& rev, long long rev_cap, const int* perm,
                    const int* rank, int* ws, int* deg, hipStream_t st, DevBuf& scan_tmp) {
    const dim3 grid(ceil_div(rs.threads(), 256)), blk(256);
    int* rev_off_row = rev_off - base;               // the kernels index by the row itself
    if (!arrival) {
        hipLaunchKernelGGL(indegree_kernel, grid, blk, 0, st, nbr, cnt, kk, rs, indeg - base, (int)lo, (int)hi);
        FDX_CHECK_LAUNCH();
    }
    FDX_TRY(exclusive_scan_int(indeg, rev_off, count + 1, st, scan_tmp));
    trace_host("sym: indegree + scan");
    if (rev_cap < 0) {
        int total_in = 0;                                // edges into [lo, hi): known only now
        FDX_HIP(hipMemcpyAsync(&total_in, rev_off + count, 4, hipMemcpyDeviceToHost, st));
        FDX_HIP(hipStreamSynchronize(st));
        FDX_REQUIRE(total_in >= 0 && (long long)total_in <= count * (long long)kk, "graph: reverse edge count out of range");
        rev_cap = std::max(total_in, 1);
    }
    FDX_TRY(rev.alloc((size_t)rev_cap * 4));
    if (arrival)                                         // the places drawn by the k-NN kernel: whole graph, base 0
        hipLaunchKernelGGL(fill_reverse_placed_kernel, dim3(ceil_div(count, 256)), blk, 0, st, nbr, cnt, arrival, count, kk, rev_off,
                           rev.as<int>());
    else
        hipLaunchKernelGGL(fill_reverse_kernel, grid, blk, 0, st, nbr, cnt, kk, rs, rev_off_row, cursor - base, rev.as<int>(), (int)lo,
                           (int)hi);
    FDX_CHECK_LAUNCH();
    if (hi > lo) {
        hipLaunchKernelGGL(merge_rows_kernel, dim3(ceil_div(hi - lo, 128)), dim3(128), 0, st, nbr, cnt, rev.as<int>(), rev_off_row, perm,
                           rank, lo, hi, kk, ws - (size_t)base * kk, deg - base);
        FDX_CHECK_LAUNCH();
    }
    trace_host("sym: fill_reverse, merge_rows launched");
    return 0;
}

static int graph_from_knn_lists_impl(fdx_graph_plan* plan, const int* nbr, const int* cnt, long long lo, long long hi, fdx_graph* g,
                                     hipStream_t st, bool defer) {
    const long long n = plan->n;
    const int kk = plan->kk;
    FDX_REQUIRE(0 <= lo && lo <= hi && hi <= n, "graph: bad row range");
    FDX_REQUIRE(lo % 64 == 0, "graph: a shard must start on a 64-row slice boundary");
    g->n = n; g->n_total = n; g->identity_order = false;
    g->perm.take(plan->b.perm);
    g->rank.take(plan->b.rank);
    g->ties_dev.take(plan->ties);
    DevBuf indeg, rev_off, cursor, rev, tmp;
    // symmetrise: A + A^T, binary   (graph.py:80-81)
    FDX_TRY(rev_off.alloc((size_t)(n + 1) * 4));
    const bool whole = lo == 0 && hi == n;
    const bool placed = whole && plan->indeg.p && plan->arrival.p;   // the k-NN kernel counted and placed already
    const bool band = plan->band_rows.p != nullptr;                  // band recompute: only the own rows and the band have lists
    if (placed) {
        indeg.take(plan->indeg);
    } else {
        FDX_TRY(indeg.alloc((size_t)(n + 1) * 4));
        FDX_TRY(cursor.alloc((size_t)n * 4));
        FDX_HIP(hipMemsetAsync(indeg.p, 0, indeg.bytes, st));
        FDX_HIP(hipMemsetAsync(cursor.p, 0, cursor.bytes, st));
        trace_host("sym: allocs + 2 memsets");
    }
    const RowSet rs = band ? RowSet{lo, hi - lo, plan->band_rows.as<int>(), plan->band_counters.as<int>() + 1, plan->band_cap}
                           : RowSet{0, n, nullptr, nullptr, 0};
    // reverse entries.  Whole graph: every list entry is a reverse edge.  Band recompute: at most (own + band) * kk entries point
    // into [lo, hi) - a bound known on the host: no read-back of the count (a synchronisation per plan).  Else: known behind the scan.
    const long long rev_cap = whole ? n * kk : band ? ((hi - lo) + plan->band_cap) * kk + 1 : -1;
    FDX_TRY(g->rows.alloc((size_t)n * kk * 2 * 4));     // capacity sum_p (kk + indeg[p]) <= 2*n*kk
    FDX_TRY(g->deg.alloc((size_t)n * 4));
    if (!whole) FDX_HIP(hipMemsetAsync(g->deg.p, 0, g->deg.bytes, st));
    FDX_TRY(symmetrise_rows(nbr, cnt, kk, rs, lo, hi, 0, n, indeg.as<int>(), cursor.as<int>(), rev_off.as<int>(),
                            placed ? plan->arrival.as<int>() : nullptr, rev, rev_cap, g->perm.as<int>(), g->rank.as<int>(),
                            g->rows.as<int>(), g->deg.as<int>(), st, tmp));
    g->row_stride = kk;
    g->row_extra.take(rev_off);   // keep: segment offsets
    int band_over = 0;
    if (!whole && plan->band_counters.p) FDX_HIP(hipMemcpyAsync(&band_over, plan->band_counters.as<int>() + 3, 4, hipMemcpyDeviceToHost, st));
    FDX_TRY(finish_ell(g, g->rows.as<int>(), g->row_stride, g->row_extra.as<int>(), st, defer, !whole));
    if (!defer) FDX_HIP(hipStreamSynchronize(st));
    if (band_over) g->knn_far = 1;          // the band list overflowed: same remedy as a far walk (exchange the lists)
    return 0;
}

int graph_from_knn_lists(fdx_graph_plan* plan, const int* nbr, const int* cnt, long long lo, long long hi, fdx_graph* g,
                         hipStream_t st) {
    return graph_from_knn_lists_impl(plan, nbr, cnt, lo, hi, g, st, false);
}

// Waits for a deferred build (finish_ell) and takes over what only the device knew.  Cheap no-op otherwise.
int graph_meta_sync(const fdx_graph* gc) {
    if (gc && gc->shard_pending) return shard_meta_sync(const_cast<fdx_graph*>(gc));
    if (!gc || !gc->meta_pending) return 0;
    fdx_graph* g = const_cast<fdx_graph*>(gc);
    FDX_HIP(hipEventSynchronize(g->meta_event));
    g->meta_pending = false;
    // the queued kernels are done: their inputs can go
    g->keep_nbr.release();
    g->keep_cnt.release();
    if (g->keep_plan) { g->keep_plan->kernels_done = true; graph_plan_destroy(g->keep_plan); g->keep_plan = nullptr; }
    const long long rows = g->meta_host[0] & 0xffffffffLL;
    g->nnz = g->meta_host[1];
    g->max_deg = (int)(g->meta_host[2] & 0xffffffffLL);
    g->knn_ties = g->meta_host[4] & 0xffffffffLL;
    if (rows > g->ell_cap_rows) {                     // the bound was too small (hubs): build the ELL again with its exact size
        trace_host("meta: ELL bound too small, rebuilding");
        FDX_TRY(finish_ell(g, g->rows.as<int>(), g->row_stride, g->row_extra.as<int>(), g->meta_stream, false));
        graph_cache_publish(g);                       // complete (the rebuild ends synchronously)
        return 0;
    }
    g->ell_rows = rows;
    g->halo_max = (int)(g->meta_host[3] & 0xffffffffLL);
    g->tiled = g->n_tiles > 0 && rows > 0 && (g->meta_host[3] >> 32) == 0;
    if (fdx::env("FDX_TRACE_HOST")) std::fprintf(stderr, "[fdx-host] meta: rows %lld of %lld, nnz %lld, largest halo %d, tiled %d\n", rows, g->ell_cap_rows, g->nnz, g->halo_max, (int)g->tiled);
    graph_cache_publish(g);                           // complete: a build that missed the cache becomes an entry (graph_cache.cpp)
    return 0;
}

int whole_graph_tables(const fdx_graph* g, const char* who, GraphTables* out) {
    const std::string w(who);
    FDX_REQUIRE(g != nullptr, w + ": null argument");
    FDX_TRY(graph_meta_sync(g));
    FDX_REQUIRE(!g->shard_pending && g->n_total == g->n && g->world_n == 0,
                w + ": a shard's local graph is refused (whole graphs on one GPU only)");
    FDX_REQUIRE(g->n < (1LL << 31) - 128, w + ": too many spots");
    FDX_REQUIRE(g->n == 0 || (g->ell.p && g->slice_off.p && g->deg.p), w + ": the graph has no device tables");
    *out = GraphTables{g->ell.as<int>(), g->slice_off.as<int>(), g->deg.as<int>(), caller_order_perm(g), (int)g->n};
    return 0;
}

int graph_build_knn(const double* d_coords, long long n, int dim, int k, fdx_graph* g, hipStream_t st, const GraphBuildHooks* hooks) {
    FDX_REQUIRE(dim >= 1 && dim <= FDX_KNN_MAX_DIM, "graph: k-NN graphs take coordinates of 1 to 8 dimensions");
    FDX_REQUIRE(n >= 0 && n < 0x7fffff00LL, "graph: n out of range");
    FDX_REQUIRE(k >= 0, "graph: k must be non-negative");
    const int k_act = (int)std::min<long long>(k, n - 1);           // graph.py:51
    if (k_act <= 0) {                                               // graph.py:53-57
        FDX_TRY(graph_hook_under_wait(hooks));
        return empty_graph(n, g, st);
    }
    const int kk = k_act + 1;
    FDX_REQUIRE(kk <= 64, "graph: k_neighbors above 63 is not supported");
    FDX_REQUIRE((long long)n * kk < 0x7fffff00LL, "graph: n*k too large");
    DevBuf nbr, cnt;
    FDX_TRY(nbr.alloc((size_t)n * kk * 4));
    FDX_TRY(cnt.alloc((size_t)n * 4));
    fdx_graph_plan* plan = nullptr;
    FDX_TRY(graph_knn_lists(d_coords, n, dim, k, 0, n, nbr.as<int>(), cnt.as<int>(), &plan, st, false, hooks));
    // Whole graph in one piece: the rest is queued without a host round trip (FDX_GRAPH_SYNC=1: built to the end here); the
    // lists and the binned points stay with the graph until graph_meta_sync has seen the kernels finish.
    const bool defer = !fdx::env("FDX_GRAPH_SYNC");
    const int rc = graph_from_knn_lists_impl(plan, nbr.as<int>(), cnt.as<int>(), 0, n, g, st, defer);
    if (rc == 0 && defer && g->meta_pending) {
        g->keep_nbr.take(nbr);
        g->keep_cnt.take(cnt);
        g->keep_plan = plan;
        return 0;
    }
    delete plan;
    return rc;
}

// Rows [lo, hi) (solver positions) of the radius graph; the other rows are left empty.  A radius graph is symmetric by
// construction (graph.py:115-121), so a shard's own rows need nothing from the other shards.
int graph_build_radius(const double* d_coords, long long n, int dim, double radius, long long lo, long long hi, fdx_graph* g,
                       hipStream_t st, const GraphBuildHooks* hooks) {
    FDX_REQUIRE(dim >= 1 && dim <= 3, "graph: coordinate dimension must be 1, 2 or 3");
    FDX_REQUIRE(n >= 0 && n < 0x7fffff00LL, "graph: n out of range");
    FDX_REQUIRE(radius > 0.0 && std::isfinite(radius), "graph: radius must be positive");
    FDX_REQUIRE(0 <= lo && lo <= hi && hi <= n, "graph: bad row range");
    FDX_REQUIRE(lo % 64 == 0, "graph: a shard must start on a 64-row slice boundary");
    if (n <= 1) {
        FDX_TRY(graph_hook_under_wait(hooks));
        return empty_graph(n, g, st);
    }
    BinnedPoints b;
    FDX_TRY(bin_points(d_coords, n, dim, 1.0, radius, &b, st, 0, 0, 0, hooks ? hooks->under_wait : nullptr));   // cell edge >= radius: one shell suffices
    const int R = (int)std::ceil(radius / b.gp.h[0] * (1.0 + 1e-12));
    g->n = n; g->n_total = n; g->identity_order = false;
    g->perm.take(b.perm);
    g->rank.take(b.rank);
    DevBuf cnt, tmp;
    FDX_TRY(cnt.alloc((size_t)(n + 1) * 4));
    FDX_TRY(g->row_extra.alloc((size_t)(n + 1) * 4));
    FDX_HIP(hipMemsetAsync(cnt.p, 0, cnt.bytes, st));
    const int nb = ceil_div(n, 128);
    hipLaunchKernelGGL(radius_kernel<0>, dim3(nb), dim3(128), 0, st, b.sc.as<double>(), b.cstart.as<int>(), b.cend_p, n,
                       b.gp, radius, R, cnt.as<int>(), (const int*)nullptr, (int*)nullptr, lo, hi);
    FDX_CHECK_LAUNCH();
    FDX_TRY(exclusive_scan_int(cnt.as<int>(), g->row_extra.as<int>(), n + 1, st, tmp));
    int total = 0;
    FDX_HIP(hipMemcpyAsync(&total, g->row_extra.as<int>() + n, 4, hipMemcpyDeviceToHost, st));
    FDX_HIP(hipStreamSynchronize(st));
    FDX_REQUIRE(total >= 0, "graph: radius graph has too many edges");
    FDX_TRY(g->rows.alloc((size_t)std::max(total, 1) * 4));
    hipLaunchKernelGGL(radius_kernel<1>, dim3(nb), dim3(128), 0, st, b.sc.as<double>(), b.cstart.as<int>(), b.cend_p, n,
                       b.gp, radius, R, (int*)nullptr, g->row_extra.as<int>(), g->rows.as<int>(), lo, hi);
    FDX_CHECK_LAUNCH();
    hipLaunchKernelGGL(sort_rows_kernel, dim3(nb), dim3(128), 0, st, g->rows.as<int>(), g->row_extra.as<int>(), g->perm.as<int>(), n);
    FDX_CHECK_LAUNCH();
    g->deg.take(cnt);
    g->row_stride = 0;
    FDX_TRY(finish_ell(g, g->rows.as<int>(), 0, g->row_extra.as<int>(), st, false, lo > 0 || hi < n));
    FDX_HIP(hipStreamSynchronize(st));
    return 0;
}

// CSR in the caller's labels: indptr (n+1) int64, indices (nnz) int32 ascending per row.  Device outputs.
int graph_export_csr(const fdx_graph* g, long long* d_indptr, int* d_indices, hipStream_t st) {
    const long long n = g->n;
    if (n == 0) return 0;
    if (g->nnz == 0) {
        FDX_HIP(hipMemsetAsync(d_indptr, 0, (size_t)(n + 1) * 8, st));
        return 0;
    }
    FDX_REQUIRE(!g->identity_order && g->rows.p, "graph export: graph was not built from coordinates");
    DevBuf deg_o, tmp;
    FDX_TRY(deg_o.alloc((size_t)(n + 1) * 4));
    FDX_HIP(hipMemsetAsync(deg_o.p, 0, deg_o.bytes, st));
    const int nb = ceil_div(n, 256);
    hipLaunchKernelGGL(deg_to_orig_kernel, dim3(nb), dim3(256), 0, st, g->deg.as<int>(), g->perm.as<int>(), n, deg_o.as<int>());
    FDX_CHECK_LAUNCH();
    FDX_TRY(exclusive_scan_i64(deg_o.as<int>(), d_indptr, n + 1, st, tmp));
    hipLaunchKernelGGL(export_rows_kernel, dim3(nb), dim3(256), 0, st, g->rows.as<int>(), g->row_stride, g->row_extra.as<int>(),
                       g->deg.as<int>(), g->perm.as<int>(), d_indptr, n, d_indices);
    FDX_CHECK_LAUNCH();
    FDX_HIP(hipStreamSynchronize(st));
    return 0;
}

int graph_copy_perm(const fdx_graph* g, int* d_out, hipStream_t st) {
    if (g->n == 0) return 0;
    if (!caller_order_perm(g)) {
        hipLaunchKernelGGL(iota_kernel, dim3(ceil_div(g->n, 256)), dim3(256), 0, st, d_out, g->n);
        FDX_CHECK_LAUNCH();
    } else {
        // a shard build still pending: its first phase wrote the ids on the stream it was given
        if (g->shard_pending && g->keep_shard && g->keep_shard->ev_first && st != g->keep_shard->st_first)
            FDX_HIP(hipStreamWaitEvent(st, g->keep_shard->ev_first, 0));
        FDX_HIP(hipMemcpyAsync(d_out, g->perm.p, (size_t)g->n * 4, hipMemcpyDeviceToDevice, st));
    }
    return 0;
}

}  // namespace fdx
