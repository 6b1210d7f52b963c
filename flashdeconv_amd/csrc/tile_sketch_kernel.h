// Tile kernel: preprocess + CountSketch + H contraction of 16 spots at a time, without atomics and without Y_sketch.
//
// Replaces, for the common shapes, both sketch_contract_kernel (fused_kernels.cpp: LDS atomics, 34 % of the HBM roofline,
// bound by ds_add_f64 bank conflicts) and the pair sketch_rows_scatter_kernel -> xyt_split_kernel
// (flashdeconv/core/deconv.py:177-197 _preprocess_data, core/sketching.py:160-206 project_to_sketch,
// core/solver.py:205-223 precompute_XtY).
//
//   staging     The rows of a tile (16 consecutive spots in solver order) are copied HBM -> LDS by LDS-DMA
//               (global_load_lds_dwordx4: 1 KB per wave instruction, no registers, no ds_write), one column block of GB
//               genes at a time, double buffered: block i+1 is in flight while block i is consumed.
//   gather      lane (r, q) of wave w owns spot r of the tile and the buckets of the slots (w, j, q), j < JW (tile_plan.h).
//               It walks the genes of those buckets through a static table in LDS {weight f64, offset u16} and adds
//               weight * f(y) into a register - no atomics, genes in ascending order inside every bucket (the
//               reference's summation order), bit-reproducible.
//   contraction the bucket sums sit exactly where v_mfma_f64_16x16x4_f64 wants its B operand (B[k = q][n = r]); the
//               wave's slice of X_sketch is register-resident as A operands, so the sums never leave the registers.
//               The NW partial 16 x 16 type tiles are added in wave order through LDS (deterministic) and stored to H.
//   log-CPM     needs the row sum before the first element can be transformed: each wave sums one or two rows of the
//               NEXT tile from registers (plain global loads, which also pull the rows into L2 / Infinity Cache ahead of
//               the DMA) while the current tile is consumed.  log1p is table driven: 1 + x is reduced by a 7-bit
//               reciprocal (v_rcp_f32) to 1 + r with |r| <= 2^-7, log1p(x) = T[reciprocal] + r - r^2/2 + ... + r^7/7
//               (~21 instructions instead of ~45; < 3 ulp; tile_device.h).
#pragma once
#include <type_traits>

#include "device_math.h"
#include "fdx_internal.h"
#include "tile_device.h"
#include "tile_variant.h"

namespace fdx {

template <typename T> struct TileVec;
template <> struct TileVec<float> { typedef float type __attribute__((ext_vector_type(4))); };
template <> struct TileVec<double> { typedef double type __attribute__((ext_vector_type(2))); };

// One 1 KB piece of a staged row: lane l copies 16 bytes from src to lds_base + 16 * l.
__device__ __forceinline__ void dma16(const void* src, unsigned char* lds_base) {
    __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)src,
                                     (void __attribute__((address_space(3)))*)lds_base, 16, 0, 0);
}

// Waves of a workgroup: NWC consumers (they own the bucket slots: gather, MFMA, reduction) and NWL loaders (they only
// stage: a wave that issues vector-memory instructions sits at the issue port while the memory pipeline takes a CU's
// ~50 KB block over thousands of cycles, so staging from the consumers stalls them).  NWL = 0: the consumers stage
// themselves - better for the log modes, where the gather is bound by the vector ALU and every wave is needed for it.
// JW: groups per consumer wave, TT: 16-type tiles.  AVL2 (the wide form: up to 64 cell types, sketch_dim up to 1024): the
// wave's slice of X_sketch does not stay in registers as MFMA A operands (JW x TT of them would not fit beside the bucket
// sums) - each group's TT operands are fetched from a copy of X_sketch laid out in operand order (tile_xa_kernel; it
// stays in L2) when the group's gather starts, and have landed when its sums are final.
// LOGV (float32 input, log modes): 0 = the float64 table chain, 2 = the float32-class log1p (tile_device.h: tile_log1p_f32).
// WG (round 4, the wide raw form): the per-entry weight table (8 bytes per scheduled step and lane class: 55-65 KB at 5000 genes)
// is replaced by the weights BY GENE of the column block in flight - (GB + 1) doubles at the head of every stage buffer, copied
// by the loaders with the block's rows (w_tab then holds NBLK such tables back to back, WB bytes each; entry GB is 0.0 and is
// what the lockstep padding steps point at, together with the zeroed pad behind every staged row).  The 40 KB this frees make
// the column blocks larger: 5 of 1024 genes instead of 7 of 736 at 5000 genes - fewer barriers, fewer (group, block) loop
// entries (they average ~1.1 steps), 12 % less lockstep padding.
// FF: always false.  It was the flat schedule of the wide raw form, measured slower and removed; the
// parameter keeps its place because bench.py looks the kernel up in profiler output by its ten-parameter name.
template <typename T, int MODE, int NWC, int NWL, int JW, int TT, bool AVL2, int LOGV = 0, bool WG = false, bool FF = false>
__global__ __launch_bounds__((NWC + NWL) * 64, (NWC + NWL) / 4) void tile_sketch_kernel(
    const TileArgs a, const T* __restrict__ Yp, const int* __restrict__ row_map, const double* __restrict__ Xs,
    double* __restrict__ H, double* __restrict__ row_sumsq, const double* __restrict__ w_tab,
    const unsigned short* __restrict__ off_tab, const unsigned char* __restrict__ len_tab,
    const int* __restrict__ ent_base, const int* __restrict__ slot_bucket, const double* __restrict__ log_tab,
    const double* __restrict__ XA) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    typedef typename TileVec<T>::type V;
    constexpr int PER = 16 / sizeof(T);
    constexpr int NT = (NWC + NWL) * 64;
    constexpr int NWS = NWL > 0 ? NWL : NWC;                                // waves that stage
    constexpr int RPL = (TILE_ROWS + NWS - 1) / NWS;                        // rows a staging wave handles
    constexpr bool PAIR = tile_red_pair(NWC, AVL2);                        // wave w + NR hands its tile to wave w first
    constexpr int NR = PAIR ? NWC / 2 : NWC;                               // partial tiles that reach the final sum
    static_assert(!PAIR || NWC % 2 == 0, "paired reduction needs an even number of consumer waves");
    static_assert(TT == 1 || TT == 2 || TT == 4, "type tiles: 1, 2 or 4");
    constexpr int TH = tile_red_th(TT);                                     // type tiles per round of the final reduction
    constexpr int ROUNDS = TT / TH;
    constexpr int TS = TH * 4 * 64;
    static_assert(tile_red_bytes(NWC, AVL2, TT) == (size_t)NR * (TS + 64) * 8, "the host sizes the column blocks by the reduction area");
    static_assert(!FF, "the flat schedule is gone: FF only keeps the kernel's ten-parameter name");
    constexpr int NST = 2;                                                  // stage buffers: block i + 1 lands while block i is consumed
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int WB = WG ? a.WB : 0;
    const int stage_bytes = WB + TILE_ROWS * a.RS;
    const int NEp = (a.NE + 7) & ~7;
    double* w_l = reinterpret_cast<double*>(smem + (size_t)NST * stage_bytes);
    unsigned short* off_l = reinterpret_cast<unsigned short*>(w_l + (WG ? 0 : NEp));
    double* scales = reinterpret_cast<double*>(off_l + NEp);               // [2][16] scale of a row (log modes)
    int* rowok = reinterpret_cast<int*>(scales + 2 * TILE_ROWS);           // [2][16] every log argument of the row in the fast range
    double* logt = reinterpret_cast<double*>(smem + LOG_TAB_LDS);          // [LOG_TAB_N] (log modes), fixed place: see LOG_TAB_LDS
    for (int i = tid; i < a.NE; i += NT) {
        if (!WG) w_l[i] = w_tab[i];
        off_l[i] = off_tab[i];
    }
    if (WG) {       // the pad behind every staged row is what a padding step reads (times weight 0.0): finite, i.e. zero
        for (int i = tid; i < NST * TILE_ROWS * 4; i += NT)
            *reinterpret_cast<unsigned*>(smem + (size_t)(i / (TILE_ROWS * 4)) * stage_bytes + WB + ((i >> 2) % TILE_ROWS) * a.RS + a.RS - TILE_ROW_PAD + (i & 3) * 4) = 0u;
    }
    constexpr bool F32LOG = LOGV != 0 && sizeof(T) == 4 && MODE != FDX_PRE_RAW;   // float32-class log1p: no table, no float64 chain
    if (MODE != FDX_PRE_RAW && !F32LOG)
        for (int i = tid; i < LOG_TAB_N; i += NT) logt[i] = log_tab[i];
    const long long n_tiles = (a.n + TILE_ROWS - 1) / TILE_ROWS;
    long long tile = blockIdx.x;
    if (tile >= n_tiles) return;

    // ---- staging (loader waves, or every wave when NWL = 0): wave lw stages rows lw, lw + NWS, ...
    const int lw = NWL > 0 ? wave - NWC : wave;
    auto load_rows = [&](long long t, const T* (&rp)[RPL]) {                // row addresses by scalar loads
#pragma unroll
        for (int k = 0; k < RPL; ++k) {
            const int rr = lw + NWS * k;
            rp[k] = nullptr;
            if (rr >= TILE_ROWS || t >= n_tiles) continue;
            const long long sp = t * TILE_ROWS + rr;
            if (sp < a.n) {
                const long long row = row_map ? (long long)row_map[sp] : sp;
                rp[k] = Yp + (size_t)row * (size_t)a.ldy;
            }
        }
    };
    auto issue_stage = [&](const T* const (&rp)[RPL], int c, int buf) {
        const int gene0 = c * a.GB;
        const int bytes = (min(a.GB, a.G - gene0)) * (int)sizeof(T);
        unsigned char* base = smem + (size_t)buf * stage_bytes + WB;
        if (WG) {                                                           // the block's weights by gene: pieces lw, lw + NWS, ...
            const unsigned char* wsrc = reinterpret_cast<const unsigned char*>(w_tab) + (size_t)c * WB + lane * 16;
            for (int o = lw * 1024; o < WB; o += NWS * 1024)
                if (o + lane * 16 < WB) dma16(wsrc + o, base - WB + o);
        }
#pragma unroll
        for (int k = 0; k < RPL; ++k) {
            if (!rp[k]) continue;                                           // row past the end: stale LDS, never stored
            const unsigned char* src = reinterpret_cast<const unsigned char*>(rp[k] + gene0) + lane * 16;
            unsigned char* dst = base + (lw + NWS * k) * a.RS;
            for (int o = 0; o < bytes; o += 1024)
                if (o + lane * 16 < bytes) dma16(src + o, dst + o);
        }
    };
    // Row sums (log modes) in the scatter kernels' order (per-lane partials over ascending vectors, butterfly over the
    // wave), so every sketch path sees the same bits; with them the row's extremes, which tell whether every log argument
    // of the row lies in the fast range.  Two rows at a time: the loads of both (up to 16 KB) are in flight before the
    // first is summed.
    const int nvec = a.G / PER;                                             // launch requires G % PER == 0
    constexpr bool TWO = RPL > 1;                                           // a wave with one row has no second one to overlap
    auto scale_two = [&](const T* r0, const T* r1_, double* out_scale, int* out_ok, int i0, int i1) {
        const T* r1 = TWO ? r1_ : nullptr;
        const V* src0 = reinterpret_cast<const V*>(r0);
        const V* src1 = reinterpret_cast<const V*>(r1);
        double p0 = 0.0, p1 = 0.0;
        // "some element negative" by OR-ing the raw bits (the sign bit survives); NaN / Inf show up in the sum.  With every
        // element >= 0 the log argument y * 1e4 / sum cannot exceed 1e4, inside the fast range: no maximum is needed.
        unsigned long long sg0 = 0ULL, sg1 = 0ULL;
        auto bits_of = [](T v) -> unsigned long long {
            if constexpr (sizeof(T) == 4) return (unsigned long long)__float_as_uint((float)v) << 32;
            else return (unsigned long long)__double_as_longlong((double)v);
        };
        for (int v0 = 0; v0 < nvec; v0 += 512) {
            V x0[8], x1[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int v = v0 + u * 64 + lane;
                if (v < nvec) {
                    if (r0) x0[u] = src0[v];
                    if (TWO && r1) x1[u] = src1[v];
                }
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int v = v0 + u * 64 + lane;
                if (v < nvec) {
#pragma unroll
                    for (int e = 0; e < PER; ++e) {
                        if (r0) { p0 += (double)x0[u][e]; sg0 |= bits_of(x0[u][e]); }
                        if (TWO && r1) { p1 += (double)x1[u][e]; sg1 |= bits_of(x1[u][e]); }
                    }
                }
            }
        }
        const double sum0 = wave_sum(p0);
        const double s0 = tile_row_scale<MODE>(sum0);
        // false for a NaN / Inf sum; above 1e18 the scale * 2^-65 would leave the float range, below 1e-30 the scale itself
        auto sum_ok = [](double s) { return fabs(s) <= 1e18 && (s == 0.0 || fabs(s) >= 1e-30); };
        const bool ok0 = sum_ok(sum0) && !__any((long long)sg0 < 0);
        // rows past the end of the matrix: a defined scale and a set flag (a stale flag would send the whole tile down the
        // general path - same values in float64, but not in the float32 class)
        if (lane == 0 && i0 < TILE_ROWS) { out_scale[i0] = r0 ? s0 : 0.0; out_ok[i0] = (!r0 || ok0) ? 1 : 0; }
        if (TWO && !r1 && lane == 0 && i1 < TILE_ROWS) { out_scale[i1] = 0.0; out_ok[i1] = 1; }
        if (TWO && r1) {
            const double sum1 = wave_sum(p1);
            const double s1 = tile_row_scale<MODE>(sum1);
            const bool ok1 = sum_ok(sum1) && !__any((long long)sg1 < 0);
            if (lane == 0) { out_scale[i1] = s1; out_ok[i1] = ok1 ? 1 : 0; }
        }
    };
    // rows k = first, first + step, ... < RPL of `rp`, two at a time
    auto scale_rows = [&](const T* const (&rp)[RPL], int first, int step, int par) {
        for (int k = first; k < RPL; k += 2 * step) {
            const T* r0 = nullptr;
            const T* r1 = nullptr;
#pragma unroll
            for (int kk = 0; kk < RPL; ++kk) {                              // static indexing of rp[]
                if (kk == k) r0 = rp[kk];
                if (kk == k + step) r1 = rp[kk];
            }
            scale_two(r0, r1, scales + par * TILE_ROWS, rowok + par * TILE_ROWS, lw + NWS * k, lw + NWS * (k + step));
        }
    };
    const T* rowp[RPL];
    const T* rown[RPL];
    bool has_next = false;
    // one block step of a staging wave: block c of the current tile has landed; stage the next block, sum a share of the
    // next tile's rows
    auto stage_step = [&](int c, int buf, int par) {
        if (c + 1 < a.NBLK) issue_stage(rowp, c + 1, buf ^ 1);
        else if (has_next) issue_stage(rown, 0, buf ^ 1);
    };
    // Row sums of the next tile as LATE as possible (the wave's k-th pair of rows in block NBLK-1-k, counted from the end):
    // the sums read the rows from HBM, the DMA of the next tile re-reads them 0 - 1 tile periods later, and the closer the
    // two reads the more of the second one the XCD's 4 MB L2 still holds (32 CUs x 128 KB of rows per tile period).
    auto sums_step = [&](int c, int par) {
        if (MODE != FDX_PRE_RAW && has_next) scale_rows(rown, a.NBLK - 1 - c, a.NBLK, par ^ 1);
    };
    if (NWL == 0 || wave >= NWC) {
        load_rows(tile, rowp);
        issue_stage(rowp, 0, 0);
        if (MODE != FDX_PRE_RAW) scale_rows(rowp, 0, 1, 0);
    }

    if (NWL > 0 && wave >= NWC) {
        // ================================================================================================ loader wave
        // Two stage buffers: block s is consumed from buffer s % 2.  At the barrier that opens block s (block s has landed,
        // block s - 1 is done with) the loaders request block s + 1 into the buffer block s - 1 has left.
        int buf = 0, par = 0;
        for (; tile < n_tiles; tile += gridDim.x) {
            has_next = tile + gridDim.x < n_tiles;
            load_rows(tile + gridDim.x, rown);
            for (int c = 0; c < a.NBLK; ++c) {
                __builtin_amdgcn_s_waitcnt(0x0f70);                          // vmcnt(0): this wave's pieces of block c have landed
                lds_barrier();                                              // everybody's have; the buffer of block c - 1 is free
                stage_step(c, buf, par);
                sums_step(c, par);
                buf ^= 1;
            }
            par ^= 1;
#pragma unroll
            for (int k = 0; k < RPL; ++k) rowp[k] = rown[k];
            for (int rd = 0; rd < ROUNDS; ++rd) {                            // the consumers' reduction
                lds_barrier();
                if (PAIR) lds_barrier();
                lds_barrier();
            }
            if (WG) lds_barrier();
        }
        return;
    }

    // ==================================================================================================== consumer wave
    // this wave's slice of X_sketch as MFMA A operands: A[m = type r][k = q] = X_sketch[type, bucket of slot (w, j, q)];
    // unconditional loads (index clamped, value selected) and one wait, so nothing of this is pending in the tile loop
    double av[AVL2 ? 1 : JW][TT];
    // AVL2: operand (j, t) of this wave at xu[(j * TT + t) * 64 + lane] - a uniform base per operand plus the lane, so that
    // the loads take scalar bases (128 per-lane 64-bit addresses would be hoisted out of the tile loop and spilled)
    const double* xu = XA + ((size_t)wave * JW * TT) * 64;
    unsigned lane8 = (unsigned)lane * 8u;
#pragma unroll
    for (int j = 0; j < (AVL2 ? 0 : JW); ++j) {
        const int b = slot_bucket[(wave * JW + j) * 4 + q];
#pragma unroll
        for (int t = 0; t < TT; ++t) {
            const int type = t * 16 + r;
            const bool ok = b >= 0 && type < a.K;
            const double v = Xs[(size_t)(ok ? type : 0) * a.d + (ok ? b : 0)];
            av[j][t] = ok ? v : 0.0;
        }
    }
    if (NWL > 0) __builtin_amdgcn_s_waitcnt(0x0f70);
    LogConsts lc{};
    if constexpr (!F32LOG) lc = log_consts();
    int buf = 0, par = 0;
    for (; tile < n_tiles; tile += gridDim.x) {
        if (AVL2) asm volatile("" : "+v"(lane8));                           // the operand addresses are formed where they are used
        if (NWL == 0) {
            has_next = tile + gridDim.x < n_tiles;
            load_rows(tile + gridDim.x, rown);
        }
        double acc[JW];
#pragma unroll
        for (int j = 0; j < JW; ++j) acc[j] = 0.0;
        double4_t accm[TT];
#pragma unroll
        for (int t = 0; t < TT; ++t) accm[t] = double4_t{0.0, 0.0, 0.0, 0.0};
        double sq = 0.0;
        double scale = 1.0;
        double scale_s = FDX_LOG_DOWN;                                      // scale * 2^-65 (tile_device.h)
        float scale_sf = FDX_LOG_DOWN_F;
        float scale_f = 1.0f;
        bool fast = true;
        // One column block: software pipeline over the flat entry stream - weight and value of the current step in
        // registers, the offset of the step after next already fetched, so a step costs one LDS round trip, not two.
        // LAST: the group's sum is final when its loop ends, and its MFMAs go out at once - they run in the matrix pipe
        // beside the gather of the following groups.  (A run-time test per group instead of the template parameter would
        // make the accumulators merge points and serialise the MFMAs behind register copies.)  FAST: every log argument
        // of the tile is known to be in the fast range (rowok), no per-element test.
        auto consume = [&](int c, auto last_tag, auto fast_tag) {
            constexpr bool LAST = decltype(last_tag)::value;
            constexpr bool FAST = decltype(fast_tag)::value;
            const unsigned char* rowb = smem + (size_t)buf * stage_bytes + WB + r * a.RS;
            const double* wgl = reinterpret_cast<const double*>(smem + (size_t)buf * stage_bytes);   // WG: this block's weights by gene
            int p = ent_base[wave * (a.NBLK + 1) + c] + q;
            const unsigned long long* lens = reinterpret_cast<const unsigned long long*>(len_tab + ((size_t)wave * a.NBLK + c) * JW_PAD(JW));
            const unsigned off0 = off_l[p];
            double wv = WG ? wgl[off0] : w_l[p];
            T yv = *reinterpret_cast<const T*>(rowb + (size_t)off0 * sizeof(T));
            unsigned offn = off_l[p + 4];
            auto f = [&](T yy) -> double {
                if (MODE == FDX_PRE_RAW) return (double)yy;
                if constexpr (F32LOG) {
                    if (FAST) return (double)tile_log1p_f32((float)yy, scale_f);
                    return tile_log1p_any((double)yy * scale);
                } else {
                    if (FAST) return tile_log1p_scaled(yy, scale_s, scale_sf, lc);
                    return tile_log1p((double)yy * scale, lc);
                }
            };
#pragma unroll
            for (int j = 0; j < JW; ++j) {
                const int len = (int)((lens[j >> 3] >> ((j & 7) * 8)) & 0xffULL);
                double an[TT];
                if (LAST && AVL2) {
                    __builtin_amdgcn_sched_barrier(0);                       // the operand loads of later groups stay with their groups
#pragma unroll
                    for (int t = 0; t < TT; ++t) an[t] = *reinterpret_cast<const double*>(reinterpret_cast<const char*>(xu + (size_t)(j * TT + t) * 64) + lane8);
                }
                int t = 0;
                for (; t + 2 <= len; t += 2) {                            // two steps per trip: the register sets swap roles
                    const double wb = WG ? wgl[offn] : w_l[p + 4];
                    const T yb = *reinterpret_cast<const T*>(rowb + (size_t)offn * sizeof(T));
                    const unsigned offb = off_l[p + 8];
                    acc[j] = fma(wv, f(yv), acc[j]);
                    p += 8;
                    wv = WG ? wgl[offb] : w_l[p];
                    yv = *reinterpret_cast<const T*>(rowb + (size_t)offb * sizeof(T));
                    offn = off_l[p + 4];
                    acc[j] = fma(wb, f(yb), acc[j]);
                }
                if (t < len) {
                    p += 4;
                    const double wn = WG ? wgl[offn] : w_l[p];
                    const T yn = *reinterpret_cast<const T*>(rowb + (size_t)offn * sizeof(T));
                    offn = off_l[p + 4];
                    acc[j] = fma(wv, f(yv), acc[j]);
                    wv = wn;
                    yv = yn;
                }
                if (LAST) {
#pragma unroll
                    for (int t = 0; t < TT; ++t)
                        accm[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(AVL2 ? an[t] : av[AVL2 ? 0 : j][t], acc[j], accm[t], 0, 0, 0);
                    sq = fma(acc[j], acc[j], sq);
                }
            }
        };
        auto block = [&](int c, auto last_tag) {
            if (NWL == 0) __builtin_amdgcn_s_waitcnt(0x0f70);                // vmcnt(0): this wave's pieces of block c have landed
            lds_barrier();                                                  // everybody's have (the loaders waited for theirs)
            if (NWL == 0) stage_step(c, buf, par);
            if (MODE != FDX_PRE_RAW && c == 0) {
                scale = scales[par * TILE_ROWS + r];
                if constexpr (F32LOG) {
                    scale_f = (float)scale;
                } else {
                    scale_s = scale * FDX_LOG_DOWN;
                    scale_sf = (float)scale_s;
                }
                fast = __all(rowok[par * TILE_ROWS + r] != 0);
            }
            if (MODE == FDX_PRE_RAW || fast) consume(c, last_tag, std::true_type{});
            else consume(c, last_tag, std::false_type{});
            if (NWL == 0) sums_step(c, par);
            buf ^= 1;
        };
        // raw: MFMAs interleaved with the last block's gather.  Log modes: afterwards - the gather is bound by the vector ALU
        // there, and the 16 accumulator registers held through it would spill.
        constexpr bool INTERLEAVE = MODE == FDX_PRE_RAW;
        for (int c = 0; c + 1 < a.NBLK; ++c) block(c, std::false_type{});
        block(a.NBLK - 1, std::integral_constant<bool, INTERLEAVE>{});
        if constexpr (!INTERLEAVE) {
#pragma unroll
            for (int j = 0; j < JW; ++j) {
                double an[TT];
                if (AVL2) {
                    if ((j & 3) == 0) __builtin_amdgcn_sched_barrier(0);    // at most four groups' operands in flight
#pragma unroll
                    for (int t = 0; t < TT; ++t) an[t] = *reinterpret_cast<const double*>(reinterpret_cast<const char*>(xu + (size_t)(j * TT + t) * 64) + lane8);
                }
#pragma unroll
                for (int t = 0; t < TT; ++t)
                    accm[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(AVL2 ? an[t] : av[AVL2 ? 0 : j][t], acc[j], accm[t], 0, 0, 0);
                sq = fma(acc[j], acc[j], sq);
            }
        }
        par ^= 1;
        if (NWL == 0) {
#pragma unroll
            for (int k = 0; k < RPL; ++k) rowp[k] = rown[k];
        }
        // ---- the partial tiles are added in a fixed order through LDS (the buffer of the block just consumed) and stored,
        // TH type tiles per round (the area must fit a stage buffer)
        double* red = reinterpret_cast<double*>(smem + (size_t)(buf ^ 1) * stage_bytes);   // the block just consumed: [NR][TS] + [NR][64]
        double* red_sq = red + (size_t)NR * TS;
        const long long s0 = tile * TILE_ROWS;
#pragma unroll
        for (int rd = 0; rd < ROUNDS; ++rd) {
            lds_barrier();                                                  // the last block's buffer / the previous round's sums are free
            if (PAIR) {
                if (wave >= NR) {
#pragma unroll
                    for (int t = 0; t < TH; ++t)
#pragma unroll
                        for (int rr = 0; rr < 4; ++rr) red[(size_t)(wave - NR) * TS + (t * 4 + rr) * 64 + lane] = accm[rd * TH + t][rr];
                    if (rd == 0) red_sq[(wave - NR) * 64 + lane] = sq;
                }
                lds_barrier();
                if (wave < NR) {
#pragma unroll
                    for (int t = 0; t < TH; ++t)
#pragma unroll
                        for (int rr = 0; rr < 4; ++rr) red[(size_t)wave * TS + (t * 4 + rr) * 64 + lane] += accm[rd * TH + t][rr];
                    if (rd == 0) red_sq[wave * 64 + lane] += sq;
                }
            } else {
#pragma unroll
                for (int t = 0; t < TH; ++t)
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) red[(size_t)wave * TS + (t * 4 + rr) * 64 + lane] = accm[rd * TH + t][rr];
                if (rd == 0) red_sq[wave * 64 + lane] = sq;
            }
            lds_barrier();
            for (int o = tid; o < TS; o += NWC * 64) {
                double sum = 0.0;
#pragma unroll
                for (int v = 0; v < NR; ++v) sum += red[(size_t)v * TS + o];              // fixed order: deterministic
                const int l = o & 63, tr = o >> 6;
                const int type = (rd * TH + (tr >> 2)) * 16 + (l >> 4) + 4 * (tr & 3);
                const long long sp = s0 + (l & 15);
                if (type < a.K && sp < a.n) H[(size_t)type * a.ldh + sp] = sum;
            }
            if (rd == 0 && row_sumsq && tid < TILE_ROWS && s0 + tid < a.n) {
                double sum = 0.0;
                for (int v = 0; v < NR; ++v)
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq) sum += red_sq[v * 64 + qq * 16 + tid];
                row_sumsq[s0 + tid] = sum;
            }
        }
        if (WG) {   // the sums were written over this buffer's row pads: zero them again before the next block lands here
            lds_barrier();
            if (tid < TILE_ROWS * 4)
                *reinterpret_cast<unsigned*>(reinterpret_cast<unsigned char*>(red) + WB + (tid >> 2) * a.RS + a.RS - TILE_ROW_PAD + (tid & 3) * 4) = 0u;
        }
        // the first barrier of the next tile orders these reads before the next DMA into this buffer
    }
}

}  // namespace fdx
