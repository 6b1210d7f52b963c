// The walk over the graph's positions that the gene spatial sums (gene_spatial_kernels.cpp) and the gene-pair sums
// (gene_pair_kernels.cpp) share: a segment of FDX_GENE_SPATIAL_SEGMENT_POSITIONS positions staged in LDS by one workgroup, and a
// thread's walk over the segment for TWO columns of a dense Y - the row's value and its neighbour sum (the "lag") per column,
// added in the graph's stored neighbour order.  Device code: include it from a translation unit hipcc compiles.
#pragma once
#include "fdx_graph.h"
#include "fdx_internal.h"

namespace fdx {

constexpr int GS_SEG = FDX_GENE_SPATIAL_SEGMENT_POSITIONS;   // = the workgroup: one thread stages one position
constexpr int GS_NB = 8;                                     // neighbours of a position staged in LDS / loaded ahead
static_assert(GS_SEG == 256, "a segment is staged by one workgroup of 256 threads");

struct GsSegmentTables {
    int row[GS_SEG];                 // the caller's row of position p0 + r, -1 past the segment's end
    int deg[GS_SEG];
    int nbr[GS_NB * GS_SEG];         // [m][r]: the caller's row of neighbour m, -1 where there is none
};

// The caller's row of entry m of position p's neighbour list (m < deg[p]); -1 for an index outside the graph.
__device__ __forceinline__ int gs_neighbour_row(const GraphTables& g, int w0, int p, int m) {
    const int j = g.ell[((size_t)w0 + m) * 64 + (p & 63)];
    if (j < 0 || j >= g.n) return -1;
    return g.perm ? g.perm[j] : j;
}

// Stages positions [p0, p1) (at most GS_SEG) and, in the workgroups told to (`owner`), writes deg_out in the caller's order and
// the segment's {sum deg, sum deg^2}.  Barriers: one on entry (the previous segment's readers), one on exit.
__device__ __forceinline__ void gs_stage_segment(const GraphTables& g, int p0, int p1, GsSegmentTables& sh, long long (*red)[4],
                                                 bool owner, int* __restrict__ deg_out, long long* __restrict__ deg_part_seg) {
    __syncthreads();
    const int t = threadIdx.x, p = p0 + t;
    int row = -1, dg = 0;
    if (p < p1) {
        row = g.perm ? g.perm[p] : p;
        const int w0 = g.slice_off[p >> 6];
        dg = min(g.deg[p], g.slice_off[(p >> 6) + 1] - w0);      // (never more entries than the slice is wide)
#pragma unroll
        for (int m = 0; m < GS_NB; ++m) sh.nbr[m * GS_SEG + t] = m < dg ? gs_neighbour_row(g, w0, p, m) : -1;
        if (owner && deg_out) deg_out[row] = dg;
    } else {
#pragma unroll
        for (int m = 0; m < GS_NB; ++m) sh.nbr[m * GS_SEG + t] = -1;
    }
    sh.row[t] = row;
    sh.deg[t] = dg;
    if (owner) {
        long long sd = dg, sd2 = (long long)dg * dg;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            sd += __shfl_xor(sd, off, 64);
            sd2 += __shfl_xor(sd2, off, 64);
        }
        if ((t & 63) == 0) {
            red[0][t >> 6] = sd;
            red[1][t >> 6] = sd2;
        }
    }
    __syncthreads();
    if (owner && t < 2) deg_part_seg[t] = red[t][0] + red[t][1] + red[t][2] + red[t][3];
}

// A thread's walk over the staged segment (positions p0 .. p0 + cnt - 1) for the columns y0p and y1p of Y (pointers to the columns'
// elements of row 0; they may be the same column): for r = 0 .. cnt - 1 in order, use(r, dg, y0, y1, lag0, lag1) with the row's two
// values and their neighbour sums as doubles.  Row and neighbour indices are read from LDS by broadcast; the 1 + GS_NB loads of the
// next position are issued before this position's are consumed; neighbours past GS_NB (a hub) are read from the ELL, eight loads
// at a time.
template <typename T, class Use>
__device__ __forceinline__ void gs_walk_segment(const T* y0p, const T* y1p, long long ldy, const GraphTables& g, int p0,
                                                int cnt, const GsSegmentTables& sh, Use&& use) {
    T ca[1 + GS_NB], cb[1 + GS_NB], na[1 + GS_NB], nb[1 + GS_NB];   // [0]: the row itself, [1 + m]: neighbour m (0 where none)
    auto load = [&](int r, T (&a)[1 + GS_NB], T (&b)[1 + GS_NB]) {
        const long long row = sh.row[r];
        a[0] = y0p[row * ldy];
        b[0] = y1p[row * ldy];
#pragma unroll
        for (int m = 0; m < GS_NB; ++m) {
            const long long nr = sh.nbr[m * GS_SEG + r];
            a[1 + m] = nr >= 0 ? y0p[nr * ldy] : (T)0;
            b[1 + m] = nr >= 0 ? y1p[nr * ldy] : (T)0;
        }
    };
    load(0, ca, cb);
    for (int r = 0; r < cnt; ++r) {
        if (r + 1 < cnt) load(r + 1, na, nb);
        const int dg = sh.deg[r];
        double lag0 = 0.0, lag1 = 0.0;
#pragma unroll
        for (int m = 0; m < GS_NB; ++m) {                    // (x + 0 = x: the slots past the degree change nothing)
            lag0 += (double)ca[1 + m];
            lag1 += (double)cb[1 + m];
        }
        if (dg > GS_NB) {                                    // a hub: the rest of its list from the ELL, eight loads at a time
            const int p = p0 + r, w0 = g.slice_off[p >> 6];
            for (int m0 = GS_NB; m0 < dg; m0 += 8) {
                T ea[8], eb[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const long long nr = m0 + i < dg ? gs_neighbour_row(g, w0, p, m0 + i) : -1;
                    ea[i] = nr >= 0 ? y0p[nr * ldy] : (T)0;
                    eb[i] = nr >= 0 ? y1p[nr * ldy] : (T)0;
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    lag0 += (double)ea[i];
                    lag1 += (double)eb[i];
                }
            }
        }
        use(r, dg, (double)ca[0], (double)cb[0], lag0, lag1);
#pragma unroll
        for (int i = 0; i < 1 + GS_NB; ++i) {
            ca[i] = na[i];
            cb[i] = nb[i];
        }
    }
}

// counts[0 .. 1] = {sum deg, sum deg^2} over the n_seg pairs that the owners of gs_stage_segment left in deg_part (device), queued
// on st: one workgroup, integers (any order gives the same sums).  gene_spatial_kernels.cpp.
int launch_segment_degree_counts(const long long* deg_part, int n_seg, long long* counts, hipStream_t st);

}  // namespace fdx
