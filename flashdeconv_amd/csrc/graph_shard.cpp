// A rank's local graph (graph_internal.h): cut from a full-size graph (graph_localize) or built in one queued pipeline.
#include <mutex>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "graph_internal.h"

namespace fdx {

// ------------------------------------------------------------------------------------------------ sharding
// A rank owns the contiguous range [lo, hi) of the sorted order (lo a multiple of 256).  Its local graph indexes own
// spots 0..n_own-1, then the halo (neighbour positions outside the range, ascending global position), then the zero row.
// External neighbours of the own rows, with repetitions: PASS 0 counts them, PASS 1 appends them to `list` (order
// irrelevant: the list is sorted and made unique afterwards).  The halo is found from what the own rows reference, so the
// cost is proportional to the shard, not to the whole graph.
// PASS 1 also emits, for every such reference, the key (owner rank of q) << 32 | (own row - lo): by symmetry of the graph
// the owner of q needs this row in ITS halo, so the sorted unique keys are the send lists of all peers at once.
template <int PASS>
__global__ __launch_bounds__(256) void collect_halo_kernel(const int* __restrict__ ell, const int* __restrict__ slice_off,
                                                           const int* __restrict__ deg, long long lo, long long hi,
                                                           const long long* __restrict__ bounds, int n_ranks,
                                                           int* __restrict__ counter, int* __restrict__ list,
                                                           unsigned long long* __restrict__ send_keys) {
    const long long p = lo + blockIdx.x * 256LL + threadIdx.x;
    if (p >= hi) return;
    const int* seg = ell + (size_t)slice_off[p >> 6] * 64 + (p & 63);
    int local = 0;
    for (int m = 0; m < deg[p]; ++m) {
        const int q = seg[(size_t)m * 64];
        if (q < lo || q >= hi) {
            if (PASS) {
                const int at = atomicAdd(counter, 1);
                list[at] = q;
                int r = 0;
                while (r + 1 < n_ranks && (long long)q >= bounds[r + 1]) ++r;          // owner of q (a handful of ranks)
                send_keys[at] = ((unsigned long long)r << 32) | (unsigned long long)(p - lo);
            } else {
                ++local;
            }
        }
    }
    if (!PASS && local) atomicAdd(counter, local);
}

__global__ __launch_bounds__(256) void localize_ell_kernel(const int* __restrict__ ell_g, const int* __restrict__ slice_off_g,
                                                           const int* __restrict__ deg_g, const int* __restrict__ perm_g,
                                                           const int* __restrict__ halo, int n_halo, long long lo, long long hi,
                                                           int n_total_g, int* __restrict__ ell_l,
                                                           int* __restrict__ slice_off_l, int* __restrict__ deg_l,
                                                           int* __restrict__ perm_l) {
    const long long n_own = hi - lo;
    const int n_slices_l = (int)((n_own + 63) / 64);
    const int s0 = (int)(lo >> 6);
    const int base_rows = slice_off_g[s0];
    const long long t = blockIdx.x * 256LL + threadIdx.x;
    if (t <= n_slices_l) slice_off_l[t] = slice_off_g[s0 + t] - base_rows;
    if (t < n_own) {
        deg_l[t] = deg_g[lo + t];
        perm_l[t] = perm_g ? perm_g[lo + t] : (int)(lo + t);
    }
    const int s = (int)(t >> 6), lane = (int)(t & 63);
    if (s < n_slices_l) {
        const int w0 = slice_off_g[s0 + s], w = slice_off_g[s0 + s + 1] - w0;
        const int n_total_l = (int)n_own + n_halo;
        for (int m = 0; m < w; ++m) {
            const int q = ell_g[((size_t)w0 + m) * 64 + lane];
            int v;
            if (q == n_total_g) v = n_total_l;                 // pad -> local zero row
            else if (q >= lo && q < hi) v = (int)(q - lo);
            else {                                             // halo slot = rank of q in the sorted, unique halo list
                int a = 0, b = n_halo;
                while (a < b) { const int mid = (a + b) >> 1; if (halo[mid] < q) a = mid + 1; else b = mid; }
                v = (int)n_own + a;
            }
            ell_l[((size_t)(w0 - base_rows) + m) * 64 + lane] = v;
        }
    }
}

// the sorted unique keys of `in` (their number: *n_out, on the device)
template <class K>
static int sorted_unique(const K* in, K* sorted, K* out, int* n_out, size_t count, unsigned bits, DevBuf& tmp, hipStream_t st) {
    FDX_TRY(with_temp(tmp, [&](void* t, size_t& bytes) { return rocprim::radix_sort_keys(t, bytes, in, sorted, count, 0, bits, st); }));
    return with_temp(tmp, [&](void* t, size_t& bytes) {
        return rocprim::unique(t, bytes, sorted, out, n_out, count, rocprim::equal_to<K>(), st);
    });
}

int graph_localize(const fdx_graph* full, long long lo, long long hi, int n_ranks, const long long* bounds, int my_rank,
                   fdx_graph* loc, hipStream_t st) {
    FDX_REQUIRE(full && loc && bounds, "graph_localize: null argument");
    FDX_REQUIRE(lo >= 0 && hi >= lo && hi <= full->n, "graph_localize: bad range");
    FDX_REQUIRE(lo % 256 == 0, "graph_localize: range start must be a multiple of 256");
    FDX_REQUIRE(full->n_total == full->n, "graph_localize: input must be a full (unsharded) graph");
    loc->knn_ties = full->knn_ties;   // a shard's full-size graph counted the ties of the rows it was built for
    const long long ng = full->n, n_own = hi - lo;
    loc->n = n_own;
    loc->identity_order = false;
    loc->global_lo = lo;
    loc->world_n = bounds[n_ranks];
    loc->n_slices = (int)((n_own + 63) / 64);
    // halo = sorted unique set of the neighbour positions outside [lo, hi) that the own rows reference
    DevBuf tmp, counter, ext, ext_sorted, n_uniq, d_bounds, skeys, skeys_sorted, skeys_uniq;
    int n_halo = 0, n_send = 0;
    const int s0 = (int)(lo >> 6);
    int so2[2] = {0, 0};
    bool have_so2 = false;
    FDX_TRY(counter.alloc(8));
    FDX_TRY(d_bounds.alloc((size_t)(n_ranks + 1) * 8));
    FDX_HIP(hipMemcpyAsync(d_bounds.p, bounds, (size_t)(n_ranks + 1) * 8, hipMemcpyHostToDevice, st));
    if (n_own > 0 && full->ell_rows > 0) {
        FDX_HIP(hipMemsetAsync(counter.p, 0, 8, st));
        hipLaunchKernelGGL(collect_halo_kernel<0>, dim3(ceil_div(n_own, 256)), dim3(256), 0, st, full->ell.as<int>(),
                           full->slice_off.as<int>(), full->deg.as<int>(), lo, hi, d_bounds.as<long long>(), n_ranks,
                           counter.as<int>(), (int*)nullptr, (unsigned long long*)nullptr);
        FDX_CHECK_LAUNCH();
        int n_ext = 0;
        FDX_HIP(hipMemcpyAsync(&n_ext, counter.p, 4, hipMemcpyDeviceToHost, st));
        if (loc->n_slices > 0) {                         // the two slice offsets that bound the own rows ride in the same round trip
            FDX_HIP(hipMemcpyAsync(&so2[0], full->slice_off.as<int>() + s0, 4, hipMemcpyDeviceToHost, st));
            FDX_HIP(hipMemcpyAsync(&so2[1], full->slice_off.as<int>() + s0 + loc->n_slices, 4, hipMemcpyDeviceToHost, st));
            have_so2 = true;
        }
        FDX_HIP(hipStreamSynchronize(st));
        if (n_ext > 0) {
            FDX_TRY(ext.alloc((size_t)n_ext * 4));
            FDX_TRY(ext_sorted.alloc((size_t)n_ext * 4));
            FDX_TRY(loc->halo_global.alloc((size_t)n_ext * 4));
            FDX_TRY(n_uniq.alloc(8));
            FDX_TRY(skeys.alloc((size_t)n_ext * 8));
            FDX_TRY(skeys_sorted.alloc((size_t)n_ext * 8));
            FDX_TRY(skeys_uniq.alloc((size_t)n_ext * 8));
            FDX_HIP(hipMemsetAsync(counter.p, 0, 8, st));
            hipLaunchKernelGGL(collect_halo_kernel<1>, dim3(ceil_div(n_own, 256)), dim3(256), 0, st, full->ell.as<int>(),
                               full->slice_off.as<int>(), full->deg.as<int>(), lo, hi, d_bounds.as<long long>(), n_ranks,
                               counter.as<int>(), ext.as<int>(), skeys.as<unsigned long long>());
            FDX_CHECK_LAUNCH();
            // send lists of all peers: sort + unique of the (peer, row) keys; then the halo: sort + unique of the positions
            FDX_TRY(sorted_unique(skeys.as<unsigned long long>(), skeys_sorted.as<unsigned long long>(), skeys_uniq.as<unsigned long long>(),
                                  n_uniq.as<int>() + 1, (size_t)n_ext, 64, tmp, st));
            FDX_HIP(hipMemcpyAsync(&n_send, n_uniq.as<int>() + 1, 4, hipMemcpyDeviceToHost, st));
            FDX_TRY(sorted_unique(ext.as<int>(), ext_sorted.as<int>(), loc->halo_global.as<int>(), n_uniq.as<int>(), (size_t)n_ext, 32, tmp, st));
            FDX_HIP(hipMemcpyAsync(&n_halo, n_uniq.p, 4, hipMemcpyDeviceToHost, st));
            FDX_HIP(hipStreamSynchronize(st));
        }
    }
    if (!loc->halo_global.p) FDX_TRY(loc->halo_global.alloc(4));
    loc->n_total = n_own + n_halo;
    // local ELL / deg / perm
    if (loc->n_slices > 0 && !have_so2) {
        FDX_HIP(hipMemcpyAsync(&so2[0], full->slice_off.as<int>() + s0, 4, hipMemcpyDeviceToHost, st));
        FDX_HIP(hipMemcpyAsync(&so2[1], full->slice_off.as<int>() + s0 + loc->n_slices, 4, hipMemcpyDeviceToHost, st));
        FDX_HIP(hipStreamSynchronize(st));
    }
    loc->ell_rows = so2[1] - so2[0];
    FDX_TRY(loc->ell.alloc((size_t)std::max<long long>(loc->ell_rows, 1) * 64 * 4));
    FDX_TRY(loc->slice_off.alloc((size_t)(loc->n_slices + 1) * 4));
    FDX_TRY(loc->deg.alloc((size_t)std::max<long long>(n_own, 1) * 4));
    FDX_TRY(loc->perm.alloc((size_t)std::max<long long>(n_own, 1) * 4));
    if (n_own > 0) {
        hipLaunchKernelGGL(localize_ell_kernel, dim3(ceil_div(loc->n_slices * 64LL + 1, 256)), dim3(256), 0, st,
                           full->ell.as<int>(), full->slice_off.as<int>(), full->deg.as<int>(),
                           full->identity_order ? (const int*)nullptr : full->perm.as<int>(), loc->halo_global.as<int>(), n_halo,
                           lo, hi, (int)ng,
                           loc->ell.as<int>(), loc->slice_off.as<int>(), loc->deg.as<int>(), loc->perm.as<int>());
        FDX_CHECK_LAUNCH();
    } else {
        FDX_HIP(hipMemsetAsync(loc->slice_off.p, 0, loc->slice_off.bytes, st));
    }
    // Everything else the host needs arrives in ONE round trip (each used to have its own - seven synchronisations, ~0.2 ms for
    // a strong-scaled rank whose whole sketch is 0.25 ms): nnz / widest row of the own rows, the tile tables' summary, the halo
    // positions (recv lists) and the (peer, row) send keys, all into pinned memory.
    loc->nnz = 0;
    loc->max_deg = 0;
    loc->n_tiles = (int)((n_own + 255) / 256);
    loc->tiled = false;
    loc->halo_max = 0;
    const bool tiles = loc->n_tiles > 0 && loc->ell_rows > 0;
    DevBuf red, rtmp;
    FDX_TRY(red.alloc(32));                               // [0] nnz, [1] low word: max degree; summary: 2 ints at byte 16
    FDX_HIP(hipMemsetAsync(red.p, 0, 32, st));
    int* summary = red.as<int>() + 4;
    if (n_own > 0) {
        auto deg64 = rocprim::make_transform_iterator(loc->deg.as<int>(), [] __device__(int v) { return (long long)v; });
        FDX_TRY(with_temp(rtmp, [&](void* t, size_t& bytes) {
            return rocprim::reduce(t, bytes, deg64, red.as<long long>(), 0LL, (size_t)n_own, rocprim::plus<long long>(), st);
        }));
        FDX_TRY(with_temp(rtmp, [&](void* t, size_t& bytes) {
            return rocprim::reduce(t, bytes, loc->deg.as<int>(), red.as<int>() + 2, 0, (size_t)n_own, rocprim::maximum<int>(), st);
        }));
    }
    if (tiles) FDX_TRY(queue_tile_tables(loc, loc->ell_rows, summary, st));
    const size_t hg_at = 64, hk_at = hg_at + ((size_t)n_halo * 4 + 63) / 64 * 64;
    unsigned char* pin = (unsigned char*)pinned_scratch(3, hk_at + (size_t)n_send * 8 + 64);
    FDX_REQUIRE(pin != nullptr, "graph_localize: pinned host buffer");
    FDX_HIP(hipMemcpyAsync(pin, red.p, 32, hipMemcpyDeviceToHost, st));
    if (n_halo) FDX_HIP(hipMemcpyAsync(pin + hg_at, loc->halo_global.p, (size_t)n_halo * 4, hipMemcpyDeviceToHost, st));
    if (n_send) FDX_HIP(hipMemcpyAsync(pin + hk_at, skeys_uniq.p, (size_t)n_send * 8, hipMemcpyDeviceToHost, st));
    FDX_HIP(hipStreamSynchronize(st));
    {
        const long long* h_red = (const long long*)pin;
        const int* h_sum = (const int*)(pin + 16);
        loc->nnz = h_red[0];
        loc->max_deg = (int)(h_red[1] & 0xffffffffLL);
        if (tiles) {
            loc->tiled = h_sum[1] == 0;
            loc->halo_max = h_sum[0];
        }
    }
    // halo ownership (recv) and send lists per peer
    loc->recv_off.assign((size_t)n_ranks + 1, 0);
    loc->send_off.assign((size_t)n_ranks + 1, 0);
    const int* hg_p = (const int*)(pin + hg_at);
    const unsigned long long* hk = (const unsigned long long*)(pin + hk_at);
    struct { const int* p; const int* begin() const { return p; } } hg{hg_p};
    for (int r = 0; r < n_ranks; ++r) {
        const long long e = bounds[r + 1];
        loc->recv_off[(size_t)r + 1] = (int)(std::lower_bound(hg.begin(), hg.begin() + n_halo, (int)std::min<long long>(e, 0x7fffffff)) - hg.begin());
    }
    // send lists: the unique (peer, row) keys are already grouped by peer and ascending in the row
    std::vector<int> all_send((size_t)n_send);
    {
        int at = 0;
        for (int r = 0; r < n_ranks; ++r) {
            while (at < n_send && (int)(hk[(size_t)at] >> 32) == r) { all_send[(size_t)at] = (int)(hk[(size_t)at] & 0xffffffffULL); ++at; }
            loc->send_off[(size_t)r + 1] = at;
        }
    }
    FDX_TRY(loc->send_idx.alloc(std::max<size_t>(all_send.size(), 1) * 4));
    if (!all_send.empty())
        FDX_HIP(hipMemcpyAsync(loc->send_idx.p, all_send.data(), all_send.size() * 4, hipMemcpyHostToDevice, st));
    FDX_HIP(hipStreamSynchronize(st));
    return 0;
}

// ------------------------------------------------------------------------------------------------ deferred shard build
// One rank's LOCAL graph of a k-NN job in one queued pipeline (graph_shard_knn): after the bounding box nothing returns to the
// host.  Replaces, for the common case, the sequence knn_lists(band) -> from_knn_lists -> localize with its seven round trips
// (a strong-scaled rank of 125k spots spent 0.9 ms there for ~0.1 ms of kernels).  Every quantity the stepwise path read back
// to size an allocation is replaced by a bound the host knows (ELL rows: w_cap per slice as in the deferred whole-graph build;
// halo: the band capacity; send lists: 3 x own rows); a bound that turns out too small is reported (shard_overflow) and the
// caller rebuilds by the stepwise path.  Rows, order of the entries and tile tables are those of the stepwise path bit for bit.

// own row p: every neighbour position outside [lo, hi) is flagged (the halo is the set of flagged positions) and the owner
// ranks of those neighbours are collected in a bit mask (by symmetry the owner of q needs row p in ITS halo: the masks are the
// send lists); per 256-row tile and peer the number of rows to send, and whether the tile holds any such row
__global__ __launch_bounds__(256) void shard_mark_kernel(const int* __restrict__ ws, int kk, const int* __restrict__ seg_extra,
                                                         const int* __restrict__ deg, long long lo, long long hi,
                                                         const ShardBounds bounds_v, int n_ranks,
                                                         int* __restrict__ flag, unsigned* __restrict__ mask,
                                                         int* __restrict__ cnt_rb, int nblk, int* __restrict__ tileflag) {
    __shared__ int s_cnt[32];
    const int tid = threadIdx.x;
    if (tid < 32) s_cnt[tid] = 0;
    __syncthreads();
    const long long t = blockIdx.x * 256LL + tid;
    const long long p = lo + t;
    unsigned m = 0;
    if (p < hi) {
        const int* seg = ws + (size_t)t * kk + seg_extra[t];
        const int dg = deg[t];
        for (int e = 0; e < dg; ++e) {
            const int q = seg[e];
            if (q < lo || q >= hi) {
                flag[q] = 1;
                int r = 0;
#pragma unroll
                for (int j = 1; j < SHARD_MAX_RANKS; ++j) r += (j < n_ranks && (long long)q >= bounds_v.b[j]) ? 1 : 0;   // no dynamic index into the by-value array
                m |= 1u << r;
            }
        }
        mask[t] = m;
    }
    unsigned any = m;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) any |= __shfl_xor(any, off, 64);
    if (any) {
        for (int r = 0; r < n_ranks; ++r)
            if ((any >> r) & 1u) {
                const int c = __popcll(__ballot((m >> r) & 1u));
                if ((tid & 63) == 0) atomicAdd(&s_cnt[r], c);
            }
    }
    __syncthreads();
    if (tid < n_ranks) cnt_rb[(size_t)tid * nblk + blockIdx.x] = s_cnt[tid];
    if (tid == 0) {
        int a = 0;
        for (int r = 0; r < n_ranks; ++r) a |= s_cnt[r];
        tileflag[blockIdx.x] = a ? 1 : 0;
    }
}

// halo_global[slot] = q for every flagged position (ascending: slot = number of flagged positions before q)
__global__ __launch_bounds__(256) void shard_halo_scatter_kernel(const int* __restrict__ flag, const int* __restrict__ hscan,
                                                                 long long n, int* __restrict__ halo_global, long long cap) {
    const long long q = blockIdx.x * 256LL + threadIdx.x;
    if (q >= n || !flag[q]) return;
    const int s = hscan[q];
    if (s < cap) halo_global[s] = (int)q;
}


// send_idx, grouped by peer, ascending row inside a peer: off_rb (exclusive scan of cnt_rb, peer-major) places every tile's rows
__global__ __launch_bounds__(256) void shard_send_fill_kernel(const unsigned* __restrict__ mask, const int* __restrict__ off_rb,
                                                              const int* __restrict__ tileflag, int nblk, long long n_own,
                                                              int n_ranks, int* __restrict__ send_idx, long long cap) {
    if (!tileflag[blockIdx.x]) return;
    __shared__ int s_w[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long t = blockIdx.x * 256LL + tid;
    const unsigned m = (t < n_own) ? mask[t] : 0u;
    for (int r = 0; r < n_ranks; ++r) {
        const int base = off_rb[(size_t)r * nblk + blockIdx.x];
        const int cnt = off_rb[(size_t)r * nblk + blockIdx.x + 1] - base;       // peer-major: the next entry is the next tile (or the next peer's first)
        if (cnt == 0) continue;                                                // block-uniform
        const unsigned long long b = __ballot((m >> r) & 1u);
        if (lane == 0) s_w[wv] = __popcll(b);
        __syncthreads();
        int before = 0;
        for (int w2 = 0; w2 < wv; ++w2) before += s_w[w2];
        if ((m >> r) & 1u) {
            const long long at = (long long)base + before + __popcll(b & ((1ULL << lane) - 1ULL));
            if (at < cap) send_idx[at] = (int)t;
        }
        __syncthreads();
    }
}

// boundary tiles (hold a row some peer needs) and interior tiles, each ascending; one workgroup
__global__ __launch_bounds__(256) void shard_tile_lists_kernel(const int* __restrict__ tileflag, int n_tiles,
                                                               int* __restrict__ tiles_b, int* __restrict__ tiles_i,
                                                               int* __restrict__ counts) {
    __shared__ int s_w[4];
    __shared__ int s_base_b, s_base_i;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) { s_base_b = 0; s_base_i = 0; }
    __syncthreads();
    for (int t0 = 0; t0 < n_tiles; t0 += 256) {
        const int t = t0 + tid;
        const bool in = t < n_tiles;
        const bool isb = in && tileflag[t] != 0;
        const unsigned long long b = __ballot(isb);
        if (lane == 0) s_w[wv] = __popcll(b);
        __syncthreads();
        int before = 0, total = 0;
        for (int w2 = 0; w2 < 4; ++w2) { if (w2 < wv) before += s_w[w2]; total += s_w[w2]; }
        const int rb = before + __popcll(b & ((1ULL << lane) - 1ULL));      // boundary tiles before t in this round
        const int bb = s_base_b, bi = s_base_i;
        if (in) {
            if (isb) tiles_b[bb + rb] = t;
            else tiles_i[bi + (tid - rb)] = t;
        }
        __syncthreads();
        if (tid == 0) { s_base_b = bb + total; s_base_i = bi + (min(256, n_tiles - t0) - total); }
        __syncthreads();
    }
    if (tid == 0) { counts[0] = s_base_b; counts[1] = s_base_i; }
}

// everything the host will ask for, in one pinned block (FDX_PINNED_BLOCK_BYTES): [0] ELL rows, [1] nnz of the own rows,
// [2] widest slice, [3] largest tile halo | failed-tile flag << 32, [4] tied rows, [5] far | band overflow << 1, [6] halo spots,
// [7] rows to send (all peers), [8] boundary tiles, [9] interior tiles; [16 + r] send_off[r], [56 + r] recv_off[r] (r = 0..n_ranks)
constexpr int SHARD_META_SEND = 16, SHARD_META_RECV = 56;
__global__ __launch_bounds__(256) void shard_meta_kernel(const long long* __restrict__ part, int n_part, const int* __restrict__ slice_off,
                                                         int n_slices, const int* __restrict__ summary, const int* __restrict__ ties,
                                                         const int* __restrict__ band_ctr, const int* __restrict__ hscan, long long n_all,
                                                         const int* __restrict__ off_rb, int nblk, const ShardBounds bounds_v, int n_ranks,
                                                         const int* __restrict__ tile_counts, int* __restrict__ send_off_dev,
                                                         int* __restrict__ recv_off_dev, long long* __restrict__ meta,
                                                         double* __restrict__ counts_dev, long long ell_cap, long long halo_cap,
                                                         long long send_cap) {
    __shared__ long long s_b[SHARD_MAX_RANKS + 1];
    const int r = threadIdx.x;
    if (r <= SHARD_MAX_RANKS) s_b[r] = bounds_v.b[r];
    long long nnz;
    int widest;
    reduce_width_partials(part, n_part, &nnz, &widest);
    if (r <= n_ranks) {
        const int so = off_rb[(size_t)r * nblk];                      // r == n_ranks: the total (last entry of the scan)
        const int ro = hscan[s_b[r]];
        send_off_dev[r] = so;
        recv_off_dev[r] = ro;
        meta[SHARD_META_SEND + r] = so;
        meta[SHARD_META_RECV + r] = ro;
    }
    if (r != 0) return;
    write_meta_head(meta, slice_off, n_slices, nnz, widest, summary, ties);
    meta[5] = (long long)(ties[1] != 0) | ((long long)(band_ctr[3] != 0) << 1);
    meta[6] = (long long)hscan[n_all];
    meta[7] = (long long)off_rb[(size_t)n_ranks * nblk];
    meta[8] = (long long)tile_counts[0];
    meta[9] = (long long)tile_counts[1];
    // the same counts where an all-reduce over the ranks can take them without the host: edges of the own rows, tied own rows,
    // "a walk left its block / the band list overflowed", "a bound of this pipeline was too small"
    counts_dev[0] = (double)nnz;
    counts_dev[1] = (double)ties[0];
    counts_dev[2] = (ties[1] != 0 || band_ctr[3] != 0) ? 1.0 : 0.0;
    counts_dev[3] = ((long long)slice_off[n_slices] > ell_cap || (long long)hscan[n_all] > halo_cap ||
                     (long long)off_rb[(size_t)n_ranks * nblk] > send_cap) ? 1.0 : 0.0;
}

}  // namespace fdx
static void shard_build_join(fdx_shard_build* sb) {
    if (sb->ticket) { (void)fdx::helper_wait(sb->ticket); sb->ticket.reset(); }
}
static void shard_build_drop(fdx_shard_build* sb) {
    if (sb->ticket) { (void)fdx::helper_wait(sb->ticket); sb->ticket.reset(); }
    // second phase queued: the graph's meta event has completed, nothing reads the buffers any more; never queued: the plan's
    // destructor waits for the first phase's stream
    if (sb->plan && sb->queued) sb->plan->kernels_done = true;
    delete sb;
}
fdx_graph::~fdx_graph() {
    if (keep_shard) shard_build_join(keep_shard);             // the helper thread may still be queueing the build's second phase
    if ((meta_pending || shard_pending) && meta_event) (void)hipEventSynchronize(meta_event);   // queued kernels still write into the buffers below
    if (keep_shard) { shard_build_drop(keep_shard); keep_shard = nullptr; }
    if (keep_plan) { delete keep_plan; keep_plan = nullptr; }
    if (meta_event) (void)hipEventDestroy(meta_event);
    if (begin_event) (void)hipEventDestroy(begin_event);
    if (meta_host) fdx::pinned_block_put(meta_host);
}
namespace fdx {

// the library's per-device stream for the second phase of a shard build (beside the sketch of the own rows on the caller's stream)
static hipStream_t library_plan_stream() {
    static hipStream_t streams[64] = {};
    static std::mutex mu;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    if (!streams[dev]) {
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        if (hipStreamCreateWithPriority(&streams[dev], hipStreamNonBlocking, hi) != hipSuccess &&
            hipStreamCreateWithFlags(&streams[dev], hipStreamNonBlocking) != hipSuccess)
            streams[dev] = nullptr;
    }
    return streams[dev];
}


int graph_shard_knn(const double* d_coords, long long n, int dim, int k, int n_ranks, const long long* bounds, int my_rank,
                    fdx_graph* loc, hipStream_t st) {
    FDX_REQUIRE(dim >= 1 && dim <= 3, "graph_shard_knn: the deferred shard build takes 1 to 3 coordinates");
    FDX_REQUIRE(n_ranks >= 2 && n_ranks <= SHARD_MAX_RANKS && my_rank >= 0 && my_rank < n_ranks, "graph_shard_knn: 2 to 32 ranks");
    static_assert(SHARD_META_RECV + SHARD_MAX_RANKS + 1 <= (int)(FDX_PINNED_BLOCK_BYTES / 8), "shard meta block");
    FDX_REQUIRE(n >= 2 && k >= 1, "graph_shard_knn: needs at least two spots and k >= 1");
    const long long lo = bounds[my_rank], hi = bounds[my_rank + 1];
    FDX_REQUIRE(bounds[0] == 0 && bounds[n_ranks] == n, "graph_shard_knn: bounds must cover [0, n]");
    for (int r = 0; r < n_ranks; ++r)
        FDX_REQUIRE(bounds[r + 1] >= bounds[r] && bounds[r] % 256 == 0, "graph_shard_knn: range starts must be non-decreasing multiples of 256");
    FDX_REQUIRE(hi > lo, "graph_shard_knn: this rank owns no row (use the stepwise path)");
    const long long n_own = hi - lo;
    auto sb = std::make_unique<fdx_shard_build>();
    const int kk = (int)std::min<long long>(k, n - 1) + 1;
    FDX_REQUIRE(kk <= 64, "graph: k_neighbors above 63 is not supported");
    FDX_REQUIRE((long long)n * kk < 0x7fffff00LL, "graph: n*k too large");
    FDX_TRY(sb->nbr.alloc((size_t)n * kk * 4));
    FDX_TRY(sb->cnt.alloc((size_t)n * 4));
    // lists of the own rows and of the band (bin_points reads the bounding box back: the one round trip of the build)
    FDX_TRY(graph_knn_lists(d_coords, n, dim, k, lo, hi, sb->nbr.as<int>(), sb->cnt.as<int>(), &sb->plan, st, true));
    fdx_graph_plan* plan = sb->plan;
    FDX_REQUIRE(plan->band_rows.p != nullptr, "graph_shard_knn: no band (one rank owns everything)");
    // the caller's ids of the own rows are final with the binning: copied now, so that the caller can lay its rows out while the
    // rest of the build is still to be queued
    FDX_TRY(loc->perm.alloc((size_t)n_own * 4));
    FDX_HIP(hipMemcpyAsync(loc->perm.p, plan->b.perm.as<int>() + lo, (size_t)n_own * 4, hipMemcpyDeviceToDevice, st));
    loc->n = n_own;
    loc->n_total = n_own;                        // until graph_meta_sync
    loc->identity_order = false;
    loc->global_lo = lo;
    loc->world_n = n;
    loc->n_tiles = ceil_div(n_own, 256);
    loc->n_slices = (int)((n_own + 63) / 64);
    loc->shard_world = n_ranks;
    sb->n = n; sb->lo = lo; sb->hi = hi; sb->kk = kk; sb->n_ranks = n_ranks;
    for (int r = 0; r <= SHARD_MAX_RANKS; ++r) sb->bounds[r] = r <= n_ranks ? bounds[r] : n;
    sb->st_first = st;
    FDX_HIP(hipEventCreateWithFlags(&sb->ev_first, hipEventDisableTiming));
    FDX_HIP(hipEventRecord(sb->ev_first, st));
    if (!loc->meta_event) FDX_HIP(hipEventCreateWithFlags(&loc->meta_event, hipEventDisableTiming));
    loc->shard_pending = true;
    loc->keep_shard = sb.release();
    // The second phase (~35 dependent launches, 0.12 ms of host time) is queued by the library's helper thread on the plan stream
    // while this thread returns to the caller: a rank's critical path is the host's way to the sketch of its own rows, which does
    // not need the graph.  Consumers join (graph_shard_join).
    loc->keep_shard->ticket = helper_submit([loc] { return shard_queue_rest(loc, nullptr); });
    return 0;
}

// the second phase of a pending shard build is queued when this returns (by the helper thread, or here)
int graph_shard_join(const fdx_graph* gc) {
    fdx_graph* g = const_cast<fdx_graph*>(gc);
    if (!g || !g->shard_pending || !g->keep_shard) return 0;
    fdx_shard_build* sb = g->keep_shard;
    if (sb->ticket) {
        const std::shared_ptr<HelperTicket> t = sb->ticket;
        sb->ticket.reset();
        FDX_TRY(helper_wait(t));
    }
    return shard_queue_rest(g, nullptr);         // no-op when queued
}

// Second phase of graph_shard_knn: symmetrisation of the own rows, halo, local ELL, tile tables, send lists, meta block - on `st`
// (the library's plan stream when NULL), behind the first phase.
int shard_queue_rest(fdx_graph* loc, hipStream_t st) {
    fdx_shard_build* sb = loc->keep_shard;
    if (!sb || sb->queued) return 0;
    if (!st) st = library_plan_stream();
    if (!st) st = sb->st_first;
    PoolStream pool_stream(st);
    if (st != sb->st_first) FDX_HIP(hipStreamWaitEvent(st, sb->ev_first, 0));
    sb->queued = true;                           // whatever happens below, kernels of this phase may be in flight on `st`
    fdx_graph_plan* plan = sb->plan;
    plan->st = st;
    const long long n = sb->n, lo = sb->lo, hi = sb->hi, n_own = hi - lo;
    const int kk = sb->kk, n_ranks = sb->n_ranks;

    // ---- everything that must start as zero, in one block with one fill: in-degrees and cursors of the own rows, the halo flags
    // (one per position of the whole order), per-tile / per-peer send counts (+ the closing entry of their scan), slice widths and
    // the reduction cells behind them
    const int nblk = ceil_div(n_own, 256);
    const int wblocks = std::min(SLICE_WIDTH_BLOCKS, std::max(1, ceil_div(loc->n_slices, 4)));
    auto up16 = [](size_t v) { return (v + 15) / 16 * 16; };
    const size_t z_indeg = 0, z_cursor = up16(z_indeg + (size_t)(n_own + 1) * 4), z_flag = up16(z_cursor + (size_t)n_own * 4),
                 z_cntrb = up16(z_flag + (size_t)(n + 1) * 4), z_width = up16(z_cntrb + ((size_t)n_ranks * nblk + 1) * 4),
                 z_red = up16(z_width + (size_t)(loc->n_slices + 1) * 4), z_end = z_red + 32 + (size_t)wblocks * 16;
    FDX_TRY(sb->zeros.alloc(z_end));
    FDX_HIP(hipMemsetAsync(sb->zeros.p, 0, z_red + 32, st));
    char* zb = static_cast<char*>(sb->zeros.p);
    int* indeg_l = reinterpret_cast<int*>(zb + z_indeg);
    int* cursor_l = reinterpret_cast<int*>(zb + z_cursor);
    int* flag = reinterpret_cast<int*>(zb + z_flag);
    int* cnt_rb = reinterpret_cast<int*>(zb + z_cntrb);
    int* width = reinterpret_cast<int*>(zb + z_width);
    long long* red = reinterpret_cast<long long*>(zb + z_red);
    int* summary = reinterpret_cast<int*>(red + 2);
    long long* part = red + 4;
    ShardBounds bv;
    for (int r = 0; r <= SHARD_MAX_RANKS; ++r) bv.b[r] = sb->bounds[r];

    // ---- symmetrise the own rows: everything indexed by the LOCAL row t = p - lo; the lists are those of the own rows and the band
    const int bcap = plan->band_cap;
    const RowSet rs{lo, n_own, plan->band_rows.as<int>(), plan->band_counters.as<int>() + 1, bcap};
    FDX_TRY(sb->rev_off.alloc((size_t)(n_own + 1) * 4));
    FDX_TRY(sb->rows.alloc((size_t)n_own * kk * 2 * 4));
    FDX_TRY(loc->deg.alloc((size_t)n_own * 4));
    FDX_TRY(symmetrise_rows(sb->nbr.as<int>(), sb->cnt.as<int>(), kk, rs, lo, hi, lo, n_own, indeg_l, cursor_l, sb->rev_off.as<int>(), nullptr,
                            sb->rev, (n_own + bcap) * kk + 1, plan->b.perm.as<int>(), plan->b.rank.as<int>(), sb->rows.as<int>(),
                            loc->deg.as<int>(), st, sb->scan_tmp));

    // ---- halo and send masks
    FDX_TRY(sb->hscan.alloc((size_t)(n + 1) * 4));
    FDX_TRY(sb->mask.alloc((size_t)n_own * 4));
    FDX_TRY(sb->off_rb.alloc(((size_t)n_ranks * nblk + 1) * 4));
    FDX_TRY(sb->tileflag.alloc((size_t)nblk * 4));
    FDX_TRY(sb->tile_counts.alloc(8));
    hipLaunchKernelGGL(shard_mark_kernel, dim3(nblk), dim3(256), 0, st, sb->rows.as<int>(), kk, sb->rev_off.as<int>(),
                       loc->deg.as<int>(), lo, hi, bv, n_ranks, flag, sb->mask.as<unsigned>(), cnt_rb, nblk, sb->tileflag.as<int>());
    FDX_CHECK_LAUNCH();
    FDX_TRY(exclusive_scan_int(flag, sb->hscan.as<int>(), n + 1, st, sb->scan_tmp));
    loc->shard_halo_cap = std::max<long long>(plan->band_cap, 1);          // halo rows are band rows
    FDX_TRY(loc->halo_global.alloc((size_t)loc->shard_halo_cap * 4));
    hipLaunchKernelGGL(shard_halo_scatter_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, flag, sb->hscan.as<int>(), n,
                       loc->halo_global.as<int>(), loc->shard_halo_cap);
    FDX_CHECK_LAUNCH();

    // ---- local sliced ELL, tile tables
    FDX_TRY(loc->slice_off.alloc((size_t)(loc->n_slices + 1) * 4));
    FDX_TRY(queue_slice_offsets(loc->deg.as<int>(), n_own, loc->n_slices, wblocks, width, part, nullptr, loc->slice_off.as<int>(), st,
                                sb->scan_tmp));
    // (tests: FDX_GRAPH_WCAP forces the "bound too small" remedy, on every rank or - FDX_GRAPH_WCAP_RANK - on one)
    int rank = 0;
    while (rank + 1 < n_ranks && !(sb->bounds[rank] == lo && sb->bounds[rank + 1] == hi)) ++rank;
    const bool cap_forced = fdx::env("FDX_GRAPH_WCAP") && (!fdx::env("FDX_GRAPH_WCAP_RANK") || atoi(fdx::env("FDX_GRAPH_WCAP_RANK")) == rank);
    const long long cap = (long long)loc->n_slices * ell_w_cap(kk, cap_forced);
    loc->shard_ell_cap = cap;
    FDX_TRY(loc->ell.alloc((size_t)std::max<long long>(cap, 1) * 64 * 4));
    FDX_TRY(queue_fill_ell(sb->rows.as<int>(), kk, sb->rev_off.as<int>(), loc->deg.as<int>(), loc->slice_off.as<int>(), n_own, loc->n_slices, 0,
                           loc->ell.as<int>(), cap, st, lo, sb->hscan.as<int>(), n));
    FDX_TRY(queue_tile_tables(loc, cap, summary, st));

    // ---- send lists, boundary / interior tiles
    FDX_TRY(exclusive_scan_int(cnt_rb, sb->off_rb.as<int>(), (long long)n_ranks * nblk + 1, st, sb->scan_tmp));
    loc->shard_send_cap = n_own * std::min(n_ranks - 1, 3) + 1024;
    FDX_TRY(loc->send_idx.alloc((size_t)loc->shard_send_cap * 4));
    hipLaunchKernelGGL(shard_send_fill_kernel, dim3(nblk), dim3(256), 0, st, sb->mask.as<unsigned>(), sb->off_rb.as<int>(),
                       sb->tileflag.as<int>(), nblk, n_own, n_ranks, loc->send_idx.as<int>(), loc->shard_send_cap);
    FDX_TRY(loc->tiles_boundary.alloc((size_t)nblk * 4));
    FDX_TRY(loc->tiles_interior.alloc((size_t)nblk * 4));
    hipLaunchKernelGGL(shard_tile_lists_kernel, dim3(1), dim3(256), 0, st, sb->tileflag.as<int>(), nblk, loc->tiles_boundary.as<int>(),
                       loc->tiles_interior.as<int>(), sb->tile_counts.as<int>());
    FDX_CHECK_LAUNCH();

    // ---- the numbers the host will ask for
    FDX_TRY(loc->send_off_dev.alloc((size_t)(n_ranks + 1) * 4));
    FDX_TRY(loc->recv_off_dev.alloc((size_t)(n_ranks + 1) * 4));
    FDX_TRY(loc->counts_dev.alloc(4 * sizeof(double)));
    if (!loc->meta_host) loc->meta_host = (long long*)pinned_block_get();
    FDX_REQUIRE(loc->meta_host != nullptr, "graph: pinned host block");
    std::memset(loc->meta_host, 0, FDX_PINNED_BLOCK_BYTES);
    void* meta_dev = nullptr;
    FDX_HIP(hipHostGetDevicePointer(&meta_dev, loc->meta_host, 0));
    hipLaunchKernelGGL(shard_meta_kernel, dim3(1), dim3(256), 0, st, part, wblocks, loc->slice_off.as<int>(), loc->n_slices, summary,
                       plan->ties.as<int>(), plan->band_counters.as<int>(), sb->hscan.as<int>(), n, sb->off_rb.as<int>(), nblk, bv, n_ranks,
                       sb->tile_counts.as<int>(), loc->send_off_dev.as<int>(), loc->recv_off_dev.as<int>(), (long long*)meta_dev,
                       loc->counts_dev.as<double>(), loc->shard_ell_cap, loc->shard_halo_cap, loc->shard_send_cap);
    FDX_CHECK_LAUNCH();
    FDX_HIP(hipEventRecord(loc->meta_event, st));
    loc->meta_stream = st;
    return 0;
}

// takes over what the queued shard build left in the pinned block
int shard_meta_sync(fdx_graph* g) {
    // a failed second phase (helper-thread error, allocation failure in shard_queue_rest) stays failed: the join is a no-op the next
    // time round, the meta event was never recorded and the pinned block is empty or absent - every later call must fail again
    if (g->shard_failed) return fail(g->shard_failed, "graph: the queued shard build failed earlier; the graph is unusable");
    if (const int jrc = graph_shard_join(g)) { g->shard_failed = jrc; return jrc; }
    if (!g->meta_host || !g->meta_event) { g->shard_failed = FDX_ERR_INVALID; return fail(FDX_ERR_INVALID, "graph: the queued shard build left no counts"); }
    FDX_HIP(hipEventSynchronize(g->meta_event));
    g->shard_pending = false;
    if (g->keep_shard) { shard_build_drop(g->keep_shard); g->keep_shard = nullptr; }
    const long long* m = g->meta_host;
    const int W = g->shard_world;
    const long long rows = m[0], n_halo = m[6], n_send = m[7];
    g->nnz = m[1];
    g->max_deg = (int)(m[2] & 0xffffffffLL);
    g->knn_ties = m[4];
    g->knn_far = (int)(m[5] & 3) ? 1 : 0;
    g->shard_overflow = (rows > g->shard_ell_cap || n_halo > g->shard_halo_cap || n_send > g->shard_send_cap) ? 1 : 0;
    g->ell_rows = rows;
    g->n_total = g->n + n_halo;
    g->halo_max = (int)(m[3] & 0xffffffffLL);
    g->tiled = g->n_tiles > 0 && rows > 0 && (m[3] >> 32) == 0 && !g->shard_overflow;
    g->send_off.assign((size_t)W + 1, 0);
    g->recv_off.assign((size_t)W + 1, 0);
    for (int r = 0; r <= W; ++r) {
        g->send_off[(size_t)r] = (int)m[SHARD_META_SEND + r];
        g->recv_off[(size_t)r] = (int)m[SHARD_META_RECV + r];
    }
    g->n_tiles_boundary = (int)m[8];
    g->n_tiles_interior = (int)m[9];
    return 0;
}

}  // namespace fdx
