// What the readers of a map along rays share (raycast_kernels.hip, view_kernels.hip): the ONLY copies of
//   beam_cells   the start and end cell of a beam, formed as the map was built (W12m/slam_ekf.py:88-90, :115-123)
//   trace        the first occupied cell, in PATH order, of bresenham(start, end).path (W12m/bresenham.py:2-58)
// both on the float-error walk of grid_walk.h.
#pragma once

#include "slam_internal.h"
#include "grid_walk.h"

namespace slam {

// Beam of local direction (ct, st) and range rr from the pose (px, py, theta), c = cos(theta), s = sin(theta):
// obs = u2T(pose).dot(pc), one multiply per coordinate, both cells through to_cell, which collects in `bad` the kStatus*
// bits of a start or end cell that the index rule rejects (an infinite or NaN coordinate is flagged there: every way a
// pose or a range can be non-finite).
__device__ __forceinline__ void beam_cells(const GridDev &g, double px, double py, double c, double s, double ct, double st, double rr,
                                           int &pcx, int &pcy, int &pox, int &poy, int &bad)
{
    const double lx = ct * rr, ly = st * rr;                         // slam_ekf.py:122
    const double x = c * lx + (-s) * ly + px * 1.0;                  // u2T(pose).dot(pc), :89
    const double y = s * lx + c * ly + py * 1.0;
    pcx = to_cell(px, g.scale, g.off_x, bad);
    pcy = to_cell(py, g.scale, g.off_y, bad);
    pox = to_cell(x, g.scale, g.off_x, bad);
    poy = to_cell(y, g.scale, g.off_y, bad);
}

// trace(): path index of the first occupied in-bounds cell at path index >= skip, or -1; Lp = path length;
// (fx, fy) the cell found.  `mask` is the map's own [xw][wpr] words, in global memory or in LDS.  A mask word is
// kept while the walk stays inside it (32 cells of a row: a steep line changes word every 32nd step).
// A line with `flag` set is walked end -> start, so the first occupied cell in path order is the LAST one the walk
// meets: such a line is walked whole and the latest find kept; an unflagged one stops at its first.
__device__ __forceinline__ int trace(const uint32_t *mask, int xw, int yw, int wpr, int sx, int sy, int ex, int ey, int skip,
                                     int &Lp, int &fx, int &fy)
{
    Ray r;
    Lp = 0; fx = fy = -1;
    if (!ray_setup(sx, sy, ex, ey, r)) return -1;                   // identical cells: empty path (bresenham.py:10-11)
    Lp = r.dx + 1;
    // walk steps whose cell is tested: path index j = k, or dx - k on a reversed line (bresenham.py:57-58)
    const int k0 = r.flag ? 0 : skip, k1 = r.flag ? r.dx - skip : r.dx;
    if (k0 > k1) return -1;
    CellWalk w(r);
    int found = -1, cur = -1;
    uint32_t word = 0;
    for (int k = 0; k <= k1; ++k) {
        if (k >= k0 && (unsigned)w.lx < (unsigned)xw && (unsigned)w.ly < (unsigned)yw) {
            const int wi = w.lx * wpr + (w.ly >> 5);
            if (wi != cur) { cur = wi; word = mask[wi]; }
            if ((word >> (w.ly & 31)) & 1u) {
                found = k; fx = w.lx; fy = w.ly;
                if (!r.flag) break;
            }
        }
        (void)w.next();
    }
    return found < 0 ? -1 : r.flag ? r.dx - found : found;
}

}  // namespace slam
