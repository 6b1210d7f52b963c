// What the host (tile_kernels.cpp) and the tile kernel (tile_sketch_kernel.h) share: the launch scalars, the variant that names
// one instantiation, and the constants of the LDS layout both sides compute with.  No device code.
#pragma once
#include <cstddef>

namespace fdx {

constexpr int TILE_ROW_PAD = 16;          // bytes between staged rows: a 16-byte shift keeps the DMA destination aligned

// Scalars of a launch.  The arrays are separate __restrict__ kernel parameters: only then may the compiler fetch the
// wave-uniform ones (row_map, ent_base, len_tab) with scalar loads.  As vector loads they would sit in vmcnt behind the
// LDS-DMA pieces in flight, and every use would wait for the next block to land - no overlap left.
struct TileArgs {
    long long ldy, n, ldh;
    int G, d, K;
    int NE, GB, NBLK, RS, jw_used;
    int WB;    // WG form: bytes of a block's weight table at the head of every stage buffer ((GB + 1) doubles, 16-byte rounded)
};

// group lengths are stored 8 to a 64-bit word: JW rounded up
constexpr int JW_PAD(int jw) { return (jw + 7) & ~7; }

// The end-of-tile reduction (tile_sketch_kernel.h): with more than 8 consumer waves, or in the AVL2 form, wave w + NWC / 2 hands
// its partial tile to wave w first; at most two type tiles are summed per round.  The area overlays a stage buffer, so the host
// sizes the column blocks by it: [partial tiles][type tiles of a round x 4 x 64] sums + [partial tiles][64] squares, doubles.
constexpr bool tile_red_pair(int NWC, bool AVL2) { return NWC > 8 || AVL2; }
constexpr int tile_red_th(int TT) { return TT > 2 ? 2 : TT; }
constexpr size_t tile_red_bytes(int NWC, bool AVL2, int TT) {
    return (size_t)(tile_red_pair(NWC, AVL2) ? NWC / 2 : NWC) * (tile_red_th(TT) * 4 * 64 + 64) * 8;
}

// One instantiation of tile_sketch_kernel for an input type and a preprocess mode - what tile_cfg (tile_kernels.cpp) decides
// for a shape.  NWC consumer + NWL loader waves, JW groups per consumer wave, TT 16-type tiles (4 = the wide form); avl2, logv
// and wg are the kernel's AVL2, LOGV and WG.
struct TileVariant {
    int NWC, NWL, JW, TT;
    bool wide, avl2;
    int logv;
    bool wg;
};

// tile_inst.cpp, compiled once per input type T: the kernel of a variant, nullptr for one that is not instantiated
template <typename T> const void* tile_kernel(int mode, const TileVariant& v);

}  // namespace fdx
