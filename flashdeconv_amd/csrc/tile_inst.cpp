// The instantiations of tile_sketch_kernel, one row per kernel.  Compiled once per input type (csrc/Makefile: -DFDX_TILE_F64=0
// for float32 rows, 1 for float64 rows): the two halves build in parallel, and nothing on the host side recompiles them.  Which
// variant serves a shape is decided by tile_cfg (tile_kernels.cpp) alone; this file only holds what exists.
#include "tile_sketch_kernel.h"

#ifndef FDX_TILE_F64
#error "compile with -DFDX_TILE_F64=<0|1>"
#endif

namespace fdx {

using TileT = std::conditional<FDX_TILE_F64, double, float>::type;

template <> const void* tile_kernel<TileT>(int mode, const TileVariant& v) {
    struct Row { int mode; TileVariant v; const void* kernel; };
#define ROW(MODE, NWC, NWL, JW, TT, AVL2, LOGV, WG) \
    {MODE, {NWC, NWL, JW, TT, TT == 4, AVL2, LOGV, WG}, (const void*)tile_sketch_kernel<TileT, MODE, NWC, NWL, JW, TT, AVL2, LOGV, WG>}
    static const Row rows[] = {
        ROW(FDX_PRE_RAW, 12, 4, 11, 1, false, 0, false),
        ROW(FDX_PRE_RAW, 12, 4, 11, 2, false, 0, false),
        ROW(FDX_PRE_RAW, 12, 4, 22, 4, true, 0, true),
        ROW(FDX_PRE_LOG_CPM, 16, 0, 8, 1, true, 0, false),
        ROW(FDX_PRE_LOG_CPM, 16, 0, 8, 2, true, 0, false),
        ROW(FDX_PRE_LOG_CPM, 8, 0, 32, 4, true, 0, false),
        ROW(FDX_PRE_LOG_CPM_SPARSE, 16, 0, 8, 1, true, 0, false),
        ROW(FDX_PRE_LOG_CPM_SPARSE, 16, 0, 8, 2, true, 0, false),
        ROW(FDX_PRE_LOG_CPM_SPARSE, 8, 0, 32, 4, true, 0, false),
#if !FDX_TILE_F64   // the float32-class log1p
        ROW(FDX_PRE_LOG_CPM, 16, 0, 8, 1, false, 2, false),
        ROW(FDX_PRE_LOG_CPM, 16, 0, 8, 2, false, 2, false),
        ROW(FDX_PRE_LOG_CPM, 8, 0, 32, 4, true, 2, false),
        ROW(FDX_PRE_LOG_CPM_SPARSE, 16, 0, 8, 1, false, 2, false),
        ROW(FDX_PRE_LOG_CPM_SPARSE, 16, 0, 8, 2, false, 2, false),
        ROW(FDX_PRE_LOG_CPM_SPARSE, 8, 0, 32, 4, true, 2, false),
#endif
    };
#undef ROW
    for (const Row& r : rows)
        if (r.mode == mode && r.v.NWC == v.NWC && r.v.NWL == v.NWL && r.v.JW == v.JW && r.v.TT == v.TT && r.v.avl2 == v.avl2 &&
            r.v.logv == v.logv && r.v.wg == v.wg)
            return r.kernel;
    return nullptr;
}

}  // namespace fdx
