// Host side of the tile kernel (tile_sketch_kernel.h: preprocess + CountSketch + H contraction of 16 spots at a time): which
// variant serves a shape (tile_cfg), the cache of its gather schedules, the launch, and the probes of include/fdx.h.  The kernel
// template itself is instantiated in tile_inst.cpp; this file does not see it.
#include "fdx_env.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <mutex>

#include "fdx_internal.h"
#include "fdx_kernels.h"
#include "sketch_plan.h"
#include "tile_device.h"
#include "tile_plan.h"
#include "tile_variant.h"

namespace fdx {

// The schedule of one cache slot on the device (tile_plan_for)
struct TilePlanDevice {
    TilePlanHost h;
    DevBuf w, off, len, ent_base, slot_bucket;
    int RS = 0;
    int WB = 0;          // WG form: bytes of a block's weights-by-gene table (w holds NBLK of them); 0 = per-entry weights
    size_t lds = 0;
};

const double* log_table_dev(hipStream_t st) {   // -log of every table reciprocal in [2^-15, 1], one copy per device
    static std::mutex mu;
    static double* tabs[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    if (!tabs[dev]) {
        std::vector<double> t((size_t)LOG_TAB_N);
        for (int i = 0; i < LOG_TAB_N; ++i) {
            const unsigned bits = (unsigned)(LOG_TAB_BASE + i) << LOG_TAB_SHIFT;
            float c;                                                        // 2^65 x the reciprocal
            std::memcpy(&c, &bits, 4);
            t[(size_t)i] = (double)(-logl((long double)c) + (long double)LOG_TAB_EXP_SHIFT * 0.693147180559945309417232121458176568L);
        }
        double* p = nullptr;
        if (hipMalloc(&p, t.size() * sizeof(double)) != hipSuccess) return nullptr;
        if (hipMemcpyAsync(p, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess) {
            (void)hipFree(p);
            return nullptr;
        }
        tabs[dev] = p;
    }
    return tabs[dev];
}

static thread_local bool t_f64_math = false;
TileF64Math::TileF64Math(bool on) : prev(t_f64_math) { t_f64_math = on; }
TileF64Math::~TileF64Math() { t_f64_math = prev; }

// the log1p chain of float32 rows in a log mode: 0 = float64 (the table), anything else = the float32 class
static int tile_logv() {
    if (t_f64_math) return 0;
    const char* e = fdx::env("FDX_TILE_LOGV");
    return e ? atoi(e) : 2;
}

// The variant that serves a shape, false for none - the only place that knows the rules.
// Wave split: raw 12 consumer + 4 loader waves x 11 groups, log modes 16 self-staging waves x 8 (dead ends).
// Wide form (33..64 cell types, or more buckets than the narrow split owns): four type tiles, MFMA A operands from the L2-resident
// operand copy of X_sketch (AVL2); raw 12 + 4 x 22 with the weights by gene in the stage buffers (WG: 5 column blocks of 1024
// genes instead of 7 of 736 at 5000 genes; one 1.25M x 5000 x 50 shard: 8.40 -> 8.05 ms), log modes 8 x 32: 256 registers each
// hold 32 bucket sums, four type tiles and the gather's pipeline.
// Narrow log modes: the float64 chain (float64 rows; float32 rows with integer counts or FDX_TILE_LOGV=0) takes its operands from
// the L2 copy too - the 32 registers they would occupy are what the 128-register budget lacks for the log1p chains (22 spills
// with them; 4.23 -> 4.1 ms).  The float32-class chain (float32 rows, LOGV 2) has no table and no polynomial constants: the
// operands fit back into registers (127 VGPRs, no spills: 3.08 -> 2.87 ms).  Raw keeps them there: 2.34 ms with the fetches
// against 1.98 ms.
static bool tile_cfg(int dtype, int mode, int K, int d, int logv, TileVariant* out) {
    if ((dtype != FDX_F32 && dtype != FDX_F64) || K < 1 || K > 64 || d < 1) return false;
    if (mode != FDX_PRE_RAW && mode != FDX_PRE_LOG_CPM && mode != FDX_PRE_LOG_CPM_SPARSE) return false;
    const bool raw = mode == FDX_PRE_RAW;
    TileVariant v = raw ? TileVariant{12, 4, 11} : TileVariant{16, 0, 8};
    v.TT = (K + 15) / 16;
    if (K > 32 || d > 4 * v.NWC * v.JW) {
        v = raw ? TileVariant{12, 4, 22, 4, true} : TileVariant{8, 0, 32, 4, true};
        if (d > 4 * v.NWC * v.JW) return false;
    }
    v.logv = (dtype == FDX_F32 && !raw && logv != 0) ? 2 : 0;
    v.avl2 = v.wide || (!raw && v.logv == 0);
    v.wg = v.wide && raw;
    *out = v;
    return true;
}

static size_t tile_lds_bytes(int RS, int NE, int mode, int WB = 0) {
    const size_t NEp = ((size_t)NE + 7) & ~(size_t)7;
    // WB > 0 (WG form): weights by gene inside every stage buffer, the entry table holds the 2-byte offsets only
    const size_t below = 2 * ((size_t)WB + (size_t)TILE_ROWS * RS) + NEp * (WB ? 2 : 10) + 2 * TILE_ROWS * (8 + 4);
    if (mode == FDX_PRE_RAW) return below;
    // log modes: the table has a fixed place at the top of the 160 KB (LOG_TAB_LDS); everything else must end below it
    return below <= (size_t)LOG_TAB_LDS ? (size_t)160 * 1024 : (size_t)161 * 1024;
}

// The schedule of variant v (= tile_cfg of the shape) for the largest column block that fits the LDS, built once per SketchPlan,
// input type, raw / log and form (one tile, two tiles, wide).  Log-CPM and sparse log-CPM share a schedule, and so do the two
// log1p chains of float32 rows: nothing below depends on v.logv (the narrow splits have more than 8 consumer waves, so the
// reduction area is the same with and without AVL2).
static const TilePlanDevice* tile_plan_for(const SketchPlan& sp, int dtype, int mode, const TileVariant& v, hipStream_t st) {
    const int sz = dtype == FDX_F32 ? 4 : 8;
    const int key = ((dtype == FDX_F32 ? 0 : 1) * 2 + (mode != FDX_PRE_RAW ? 1 : 0)) * 3 + (v.wide ? 2 : v.TT - 1);
    static_assert(SketchPlan::kTileKeys == 12, "key space of the schedules: input type x raw / log x {one tile, two tiles, wide}");
    std::lock_guard<std::mutex> lock(sp.tile_mu);
    if (sp.tile_tried[key]) return sp.tile[key].get();
    sp.tile_tried[key] = true;
    const bool dbg = fdx::env("FDX_DEBUG") != nullptr;
    if (!sp.scatter_ok || sp.host_bucket.empty()) return nullptr;
    const size_t red_bytes = tile_red_bytes(v.NWC, v.avl2, v.TT);   // the kernel's reduction area
    // block sizes tried: whole 1 KB pieces; the wide form's tables leave less room, and an eighth of a piece more or less decides
    // whether 5000 genes take 7 blocks or 10 (21 % more lockstep padding)
    const int unit = (v.wide ? 128 : 1024) / sz;
    std::unique_ptr<TilePlanDevice> best;
    // The reduction area overlays a stage buffer.  Rows shorter than it (up to 256 float32 genes in the log modes, 512 with two
    // type tiles; 128 float64 genes in the wide raw form) used to find no block size at all and went to the two-kernel path
    // unseen: they take one column block long enough to hold the area - only the row's own bytes are staged into it.
    int GB0 = (int)round_up(sp.G, unit);
    while ((size_t)(v.wg ? round_up((GB0 + 1) * 8, 16) : 0) + (size_t)TILE_ROWS * (GB0 * sz + TILE_ROW_PAD) < red_bytes) GB0 += unit;
    for (int GB = GB0; GB >= unit; GB -= unit) {
        const int RS = GB * sz + TILE_ROW_PAD;
        const int WB = v.wg ? (int)round_up((GB + 1) * 8, 16) : 0;
        if ((size_t)WB + (size_t)TILE_ROWS * RS < red_bytes) break;
        // cheap bound before building: the tables hold at least G entries
        if (tile_lds_bytes(RS, sp.G, mode, WB) > 160 * 1024) continue;
        auto cand = std::make_unique<TilePlanDevice>();
        if (!build_tile_plan(sp.host_bucket.data(), sp.host_w.data(), sp.G, sp.d, v.NWC, v.JW, GB, &cand->h)) return nullptr;
        cand->RS = RS;
        cand->WB = WB;
        cand->lds = tile_lds_bytes(RS, cand->h.NE, mode, WB);
        if (dbg) std::fprintf(stderr, "[fdx] tile plan: G=%d d=%d waves=%d+%d GB=%d blocks=%d NE=%d steps=%d lds=%zu\n", sp.G, sp.d, v.NWC,
                              v.NWL, GB, cand->h.NBLK, cand->h.NE, cand->h.steps, cand->lds);
        if (cand->lds > 160 * 1024) continue;
        best = std::move(cand);
        break;
    }
    if (!best) return nullptr;
    TilePlanDevice& t = *best;
    auto up = [&](DevBuf& b, const void* src, size_t bytes) -> int {
        FDX_TRY(b.alloc(bytes));
        FDX_TRY(copy_h2d(b.p, src, bytes, st));
        return 0;
    };
    // group lengths, 8 to a 64-bit word: rows of JW_PAD(JW) bytes
    const int jp = JW_PAD(v.JW);
    std::vector<unsigned char> len_pad((size_t)v.NWC * t.h.NBLK * jp + 16, 0);
    for (int wv = 0; wv < v.NWC; ++wv)
        for (int c = 0; c < t.h.NBLK; ++c)
            for (int j = 0; j < v.JW; ++j)
                len_pad[((size_t)wv * t.h.NBLK + c) * jp + j] = t.h.len[((size_t)wv * t.h.NBLK + c) * v.JW + j];
    std::vector<double> wg_tab;
    if (t.WB) {
        // weights by gene, one table of WB bytes per column block ((GB + 1) doubles: entry GB stays 0.0); the padding steps of the
        // schedule (no gene) point at entry GB - weight 0.0 times the zeroed pad behind the staged row
        const int per = t.WB / 8;
        wg_tab.assign((size_t)t.h.NBLK * per, 0.0);
        for (int g = 0; g < sp.G; ++g)
            if (sp.host_bucket[(size_t)g] >= 0) wg_tab[(size_t)(g / t.h.GB) * per + g % t.h.GB] = sp.host_w[(size_t)g];
        for (size_t i = 0; i < t.h.off.size(); ++i)
            if (t.h.gene[i] < 0) t.h.off[i] = (unsigned short)t.h.GB;
    }
    if ((t.WB ? up(t.w, wg_tab.data(), wg_tab.size() * 8) : up(t.w, t.h.w.data(), t.h.w.size() * 8)) ||
        up(t.off, t.h.off.data(), t.h.off.size() * 2) || up(t.len, len_pad.data(), len_pad.size()) || up(t.ent_base, t.h.ent_base.data(), t.h.ent_base.size() * 4) ||
        up(t.slot_bucket, t.h.slot_bucket.data(), t.h.slot_bucket.size() * 4))
        return nullptr;
    if (hipStreamSynchronize(st) != hipSuccess) return nullptr;            // the host vectors may die with the plan
    sp.tile[key] = std::move(best);
    return sp.tile[key].get();
}

// X_sketch rearranged into MFMA A operands for the wide form: XA[((w * JW + j) * TT + t) * 64 + lane] =
// X_sketch[type = 16 t + (lane & 15), bucket of slot (w, j, lane >> 4)], 0 where there is no such type or bucket.
__global__ void tile_xa_kernel(const double* __restrict__ Xs, const int* __restrict__ slot_bucket, int K, int d, int n_groups,
                               int TT, double* __restrict__ XA) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_groups * TT * 64) return;
    const int lane = i & 63, t = (i >> 6) % TT, wj = (i >> 6) / TT;
    const int b = slot_bucket[wj * 4 + (lane >> 4)];
    const int type = t * 16 + (lane & 15);
    XA[i] = (b >= 0 && type < K) ? Xs[(size_t)type * d + b] : 0.0;
}

bool tile_sketch_ok(int dtype, long long ldy, const void* Y, int G, int d, int K, int mode, const SketchPlanDev& plan,
                    hipStream_t st) {
    if (!plan.owner) return false;
    TileVariant v;
    if (G <= 0 || !tile_cfg(dtype, mode, K, d, tile_logv(), &v)) return false;
    const int sz = dtype == FDX_F32 ? 4 : 8;
    if ((K > 32 || d > 512) && fdx::env("FDX_NO_TILE_WIDE")) return false;
    // whole 16-byte vectors only: row starts and row lengths multiples of 16 bytes
    if (((size_t)G * sz) % 16 != 0 || ((size_t)ldy * sz) % 16 != 0 || (reinterpret_cast<uintptr_t>(Y) & 15) != 0) return false;
    return tile_plan_for(*plan.owner, dtype, mode, v, st) != nullptr;
}

// H[:, 0..n) (type-major, row stride ldh) and row_sumsq[0..n) for the n spots listed by row_map (NULL = rows 0..n-1).
// A persistent workgroup fills its compute unit (16 waves x 127 registers): one per unit, at most 256.
// Call only when tile_sketch_ok(...) holds.
int launch_tile_sketch(const void* Y, int dtype, long long ldy, const int* row_map, long long n, int G, int d, int mode,
                       const SketchPlanDev& plan, const double* Xs, int K, double* H, long long ldh, double* row_sumsq,
                       hipStream_t st) {
    if (n <= 0) return 0;
    TileVariant v;
    const TilePlanDevice* t = plan.owner && tile_cfg(dtype, mode, K, d, tile_logv(), &v) ? tile_plan_for(*plan.owner, dtype, mode, v, st) : nullptr;
    if (!t) return fail(FDX_ERR_INVALID, "tile sketch: no schedule for this shape");
    const void* kern = dtype == FDX_F32 ? tile_kernel<float>(mode, v) : tile_kernel<double>(mode, v);
    if (!kern) {
        char msg[128];
        std::snprintf(msg, sizeof msg, "tile sketch: no kernel for dtype %d mode %d, waves %d + %d x %d, TT %d, AVL2 %d, LOGV %d, WG %d",
                      dtype, mode, v.NWC, v.NWL, v.JW, v.TT, (int)v.avl2, v.logv, (int)v.wg);
        return fail(FDX_ERR_INVALID, msg);
    }
    TileArgs a{};
    a.ldy = ldy; a.n = n; a.ldh = ldh; a.G = G; a.d = d; a.K = K;
    a.NE = t->h.NE; a.GB = t->h.GB; a.NBLK = t->h.NBLK; a.RS = t->RS; a.jw_used = t->h.jw_used; a.WB = t->WB;
    const double* w_tab = t->w.as<double>();
    const unsigned short* off_tab = t->off.as<unsigned short>();
    const unsigned char* len_tab = t->len.as<unsigned char>();
    const int* ent_base = t->ent_base.as<int>();
    const int* slot_bucket = t->slot_bucket.as<int>();
    const double* log_tab = nullptr;
    if (mode != FDX_PRE_RAW) {
        log_tab = log_table_dev(st);
        if (!log_tab) return fail(FDX_ERR_HIP, "tile sketch: log table upload failed");
    }
    const long long n_tiles = (n + TILE_ROWS - 1) / TILE_ROWS;
    const int grid = (int)std::min<long long>(n_tiles, 256);
    DevBuf xa;                                                              // AVL2: X_sketch in operand order
    const double* XA = nullptr;
    if (v.avl2) {
        const int n_groups = v.NWC * v.JW;
        FDX_TRY(xa.alloc((size_t)n_groups * v.TT * 64 * sizeof(double)));
        hipLaunchKernelGGL(tile_xa_kernel, dim3(ceil_div((long long)n_groups * v.TT * 64, 256)), dim3(256), 0, st, Xs, slot_bucket, K, d,
                           n_groups, v.TT, xa.as<double>());
        FDX_CHECK_LAUNCH();
        XA = xa.as<double>();
    }
    if (t->lds > 64 * 1024) FDX_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)t->lds));
    void* args[] = {(void*)&a, (void*)&Y, (void*)&row_map, (void*)&Xs, (void*)&H, (void*)&row_sumsq, (void*)&w_tab, (void*)&off_tab,
                    (void*)&len_tab, (void*)&ent_base, (void*)&slot_bucket, (void*)&log_tab, (void*)&XA};
    FDX_HIP(hipLaunchKernel(kern, dim3(grid), dim3((v.NWC + v.NWL) * 64), args, t->lds, st));
    return 0;
}

// The one-kernel sketch -> H stage: the tile kernel for every shape it takes (a CountSketch with d <= 1056, K <= 64, rows whole
// 16-byte vectors); everything else runs the two-kernel path (sketch_rows_* + xyt_split), also selected by FDX_NO_FUSED=1.
// (The round-1 atomic fused kernel that used to serve odd row lengths behind this pair was slower than the two-kernel path it
// replaced there and is gone.)
bool fused_sketch_contract_ok(int dtype, long long ldy, const void* Y, int G, int d, int K, int mode, const SketchPlanDev& plan,
                              hipStream_t st) {
    if (fdx::env("FDX_NO_FUSED")) return false;
    return tile_sketch_ok(dtype, ldy, Y, G, d, K, mode, plan, st);
}

int launch_sketch_contract(const void* Y, int dtype, long long ldy, const int* row_map, long long n, int G, int d, int mode,
                           const SketchPlanDev& plan, const double* Xs, int K, double* H, long long ldh, double* row_sumsq,
                           hipStream_t st) {
    if (n <= 0) return 0;
    if (!tile_sketch_ok(dtype, ldy, Y, G, d, K, mode, plan, st)) return fail(FDX_ERR_INVALID, "sketch -> H: no one-kernel form for this shape");
    return launch_tile_sketch(Y, dtype, ldy, row_map, n, G, d, mode, plan, Xs, K, H, ldh, row_sumsq, st);
}

}  // namespace fdx

// include/fdx.h: the float32-class log1p of the tile kernel on a host array (accuracy tests)
namespace fdx {
__global__ void log1p_f32_probe_kernel(const float* __restrict__ y, float scale, long long n, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = tile_log1p_f32(y[i], scale);
}
}  // namespace fdx

extern "C" int fdx_log1p_f32(const float* y, float scale, int64_t n, float* out) {
    using namespace fdx;
    FDX_REQUIRE(n >= 0 && (n == 0 || (y && out)), "fdx_log1p_f32: null argument");
    if (n == 0) return 0;
    DevBuf in, res;
    FDX_TRY(in.alloc((size_t)n * 4));
    FDX_TRY(res.alloc((size_t)n * 4));
    FDX_HIP(hipMemcpy(in.p, y, (size_t)n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(log1p_f32_probe_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, nullptr, in.as<float>(), scale,
                       (long long)n, res.as<float>());
    FDX_CHECK_LAUNCH();
    FDX_HIP(hipMemcpy(out, res.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return 0;
}

// include/fdx.h: the schedule the tile kernel would use, so tests can replay it on the host (no device call).
extern "C" int fdx_tile_schedule(const int32_t* gene_bucket, const double* gene_w, int32_t G, int32_t d, int32_t NW,
                                   int32_t JW, int32_t GB, int32_t* dims_out /* NBLK, NE, steps, max_wave_steps */,
                                   int32_t* slot_bucket_out, uint8_t* len_out, int32_t* ent_base_out, double* w_out,
                                   uint16_t* off_out, int64_t cap_entries) {
    using namespace fdx;
    FDX_REQUIRE(gene_bucket && gene_w && dims_out, "fdx_tile_schedule: null argument");
    TilePlanHost h;
    FDX_REQUIRE(build_tile_plan(gene_bucket, gene_w, G, d, NW, JW, GB, &h), "fdx_tile_schedule: shape cannot be scheduled");
    dims_out[0] = h.NBLK; dims_out[1] = h.NE; dims_out[2] = h.steps; dims_out[3] = h.max_wave_steps;
    if (!slot_bucket_out) return 0;
    FDX_REQUIRE(len_out && ent_base_out && w_out && off_out && cap_entries >= h.NE, "fdx_tile_schedule: output too small");
    std::copy(h.slot_bucket.begin(), h.slot_bucket.end(), slot_bucket_out);
    std::copy(h.len.begin(), h.len.end(), len_out);
    std::copy(h.ent_base.begin(), h.ent_base.end(), ent_base_out);
    std::copy(h.w.begin(), h.w.end(), w_out);
    std::copy(h.off.begin(), h.off.end(), off_out);
    return 0;
}

// include/fdx.h: what queue_rows_to_h (prepare.cpp) chooses for a dense matrix, through the functions it calls itself - the
// cached plan of (bucket, weight_y), then fused_sketch_contract_ok, then the schedule launch_tile_sketch would fetch.
extern "C" int fdx_sketch_path(int32_t y_dtype, const void* Y_dev, int64_t ldy, int32_t G, int32_t d, int32_t K, int32_t mode_y_in,
                               const int32_t* bucket, const double* weight_y, int32_t* path_out,
                               int32_t* dims_out /* NWC, NWL, JW, TT, GB, NBLK */) {
    using namespace fdx;
    FDX_REQUIRE(bucket && weight_y && path_out, "fdx_sketch_path: null argument");
    FDX_REQUIRE(G > 0 && K > 0 && d > 0 && ldy >= G, "fdx_sketch_path: bad shape");
    const int32_t mode_y = mode_y_in & 0xff;
    if (dims_out) std::fill(dims_out, dims_out + 6, 0);
    hipStream_t st = nullptr;
    PoolStream pool_stream(st);
    std::shared_ptr<SketchPlan> plan;
    FDX_TRY(sketch_plan_cached(bucket, weight_y, G, d, st, &plan));
    *path_out = 0;
    if (!fused_sketch_contract_ok(y_dtype, ldy, Y_dev, G, d, K, mode_y, plan->dev(), st)) return 0;
    TileVariant v;
    const TilePlanDevice* t = tile_cfg(y_dtype, mode_y, K, d, tile_logv(), &v) ? tile_plan_for(*plan, y_dtype, mode_y, v, st) : nullptr;
    FDX_REQUIRE(t != nullptr, "fdx_sketch_path: the one-kernel form was accepted without a schedule");
    *path_out = v.wide ? 2 : 1;
    if (dims_out) {
        dims_out[0] = v.NWC; dims_out[1] = v.NWL; dims_out[2] = v.JW; dims_out[3] = v.TT;
        dims_out[4] = t->h.GB; dims_out[5] = t->h.NBLK;
    }
    return 0;
}
