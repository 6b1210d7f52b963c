// What the two walks over the pairs within a largest radius share (correlogram_kernels.cpp: the band sums of value columns;
// label_band_kernels.cpp: the band join counts of spot labels): the cell edge, the radii of a chunk of bands as a kernel takes them,
// the wave-private hand-off of a staged tile, and the guard - the candidate pairs a walk would examine, counted from the cell table
// and held against a limit before any pair is walked.
#pragma once
#include "graph_internal.h"

namespace fdx {

constexpr int CG_MAX_BANDS = 32;
constexpr int CG_COUNT_BLOCKS = 1024;               // blocks of the candidate count at the most
constexpr int CG_SHELLS = 1;                        // shells of cells around a point's own that hold its pairs (CG_CELL_MARGIN)
constexpr double CG_CELL_MARGIN = 1.0 + 1.0 / 65536.0;   // cell edge = r_B times this: two points within r_B are never two cells apart,
                                                         // whatever the rounding of cell_coord does at a cell border

struct CgRadii {
    double r[CG_MAX_BANDS];      // the chunk's upper radii, ascending
    double lo;                   // the radius below the chunk's first band; < 0: none (d = 0 belongs to band 1)
    double d2_lo, d2_hi;         // squared distances surely outside the chunk: d2 < d2_lo or d2 > d2_hi (a sqrt saved, no decision made)
    int nb;
};

// the chunk of bands [b0, b0 + nb) of the B ascending radii
inline CgRadii cg_chunk_radii(const double* radii, int b0, int nb) {
    CgRadii rc;
    rc.nb = nb;
    for (int i = 0; i < CG_MAX_BANDS; ++i) rc.r[i] = i < nb ? radii[b0 + i] : 0.0;
    rc.lo = b0 > 0 ? radii[b0 - 1] : -1.0;
    rc.d2_lo = b0 > 0 ? rc.lo * rc.lo * (1.0 - 1e-9) : -1.0;
    rc.d2_hi = rc.r[nb - 1] * rc.r[nb - 1] * (1.0 + 1e-9);                  // (an overflow to infinity filters nothing)
    return rc;
}

__device__ __forceinline__ void cg_handoff() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// correlogram_kernels.cpp (cg_candidates_kernel).  The guard of a walk over `bins` (cell edge r_B * CG_CELL_MARGIN): *candidates = sum
// over the occupied cells of count(cell) * count(the 3^dim block of cells around it), the pairs the walk examines; *max_around (may be
// null) = the largest block count of an occupied cell, a bound on the candidates of one point.  Both are read back (one host
// synchronisation) and a call with more than max_candidates fails with FDX_ERR_INVALID in the name of `who`, nothing walked.
int cg_guard(const char* who, const BinnedPoints& bins, long long max_candidates, long long* candidates, long long* max_around,
             hipStream_t st);

}  // namespace fdx
