// The float-error Bresenham walk of the reference and the occupied rule of the integer counters: the ONLY copies,
// shared by the update engines (grid_kernels.hip) and the read side of the grid (raycast_kernels.hip).
//   bresenham        W12m/bresenham.py:2-58   -> ray_setup + walk_step (+ CellWalk, the cell as map coordinates)
//   index rule       W12m/mapping.py:33-36    -> to_cell
//   pmap threshold   W12m/mapping.py:47-50    -> OccRule
// To change the walk, change walk_step.
#pragma once

#include "slam_internal.h"

namespace slam {

struct Ray {
    int x0, y0, dx, ystep;   // walk origin (after steep / endpoint swaps), run length, y direction
    double derr;
    bool steep, flag;        // flag: the walk runs end -> start, i.e. path order is reversed (:57-58)
    // the ray of a lane that has none: no step to walk (dx = -1), every field defined
    __device__ __forceinline__ static Ray none()
    {
        Ray r;
        r.x0 = r.y0 = 0; r.dx = -1; r.ystep = 1; r.derr = 0.0; r.steep = r.flag = false;
        return r;
    }
};

// bresenham.__init__ up to the loop (bresenham.py:10-43).  Returns false for identical
// endpoints (empty path, :10-11).
__device__ __forceinline__ bool ray_setup(int sx, int sy, int ex, int ey, Ray &r)
{
    if (sx == ex && sy == ey) return false;
    int adx = abs(ex - sx), ady = abs(ey - sy);
    r.steep = ady > adx;                                             // :14
    if (r.steep) { int t = sx; sx = sy; sy = t; t = ex; ex = ey; ey = t; }   // :15-17
    r.flag = sx > ex;                                                // :19
    if (r.flag) { int t = sx; sx = ex; ex = t; t = sy; sy = ey; ey = t; }    // :20-29
    r.x0 = sx; r.y0 = sy;
    r.dx = ex - sx;                                                  // :32
    int dy = abs(ey - sy);                                           // :33
    r.derr = (double)dy / (double)r.dx;                              // :35  (IEEE division)
    r.ystep = sy < ey ? 1 : -1;                                      // :40-43
    return true;
}

// THE walk step (bresenham.py:51-55), the only copy in this file: every engine's loop calls it once per walk
// step and moves its own notion of the cell by what it returns (true: y advances by ystep).  The subtraction is
// branch-free - minus 1.0, or minus 0.0, which is exact - and gives the bits of `if error >= 0.5: error -= 1.0`.
__device__ __forceinline__ bool walk_step(double &error, double derr)
{
    error += derr;                                                   // :51
    const bool stepy = error >= 0.5;                                 // :53
    error -= __hiloint2double(stepy ? 0x3ff00000 : 0, 0);            // :55
    return stepy;
}

// The checked cell walk: the cell as map coordinates (lx, ly), moved by next(); the caller tests each cell
// against whatever bounds it has.  stride_k / stride_y give the same increments for a cell kept as ONE linear
// index over rows of `row` elements (index = lx * row + ly).
struct CellWalk {
    int lx, ly;                  // current cell
    int klast;                   // walk step of the path's LAST cell (bresenham.py:57-58)
    int ax_x, ax_y, ay_x, ay_y;  // cell step per walk step, and per y step
    double error, derr;
    __device__ __forceinline__ explicit CellWalk(const Ray &r)
    {
        klast = r.flag ? 0 : r.dx;
        ax_x = r.steep ? 0 : 1; ax_y = r.steep ? 1 : 0;              // :46-49
        ay_x = r.steep ? r.ystep : 0; ay_y = r.steep ? 0 : r.ystep;
        lx = r.steep ? r.y0 : r.x0; ly = r.steep ? r.x0 : r.y0;
        error = 0.0; derr = r.derr;                                  // :34-35
    }
    __device__ __forceinline__ int stride_k(int row) const { return ax_x * row + ax_y; }
    __device__ __forceinline__ int stride_y(int row) const { return ay_x * row + ay_y; }
    __device__ __forceinline__ bool next()
    {
        const bool stepy = walk_step(error, derr);
        lx += ax_x + (stepy ? ay_x : 0);
        ly += ax_y + (stepy ? ay_y : 0);
        return stepy;
    }
};

// World coordinate -> cell index, int(scale * (v + off)) truncated toward zero
// (mapping.py:33-36).  Flags what Python would raise on (NaN: ValueError, inf: OverflowError).
__device__ __forceinline__ int to_cell(double v, double scale, double off, int &bad)
{
    double c = scale * (v + off);
    if (c != c) { bad |= kStatusNaN; return 0; }
    if (!(fabs(c) < (double)kMaxRayCells)) { bad |= kStatusOverflow; return 0; }
    return (int)c;
}

// mapping.py:47-50 applied to the integer counters (see the header comment).
struct OccRule {
    int hit_levels;
    uint32_t pass_thresh[kMaxHitLevels];
    __host__ __device__ static OccRule of(const GridDev &g)
    {
        OccRule r;
        r.hit_levels = g.hit_levels;
        for (int k = 0; k < kMaxHitLevels; ++k) r.pass_thresh[k] = g.pass_thresh[k];
        return r;
    }
    __device__ __forceinline__ uint32_t value(uint32_t p, uint32_t h) const
    {
        if ((p | h) == 0) return 50u;
        // (as a sum of per-level tests with constant table indices: written as a select chain over the table the
        // compiler turns it into a per-lane indexed load from a private copy, i.e. scratch memory)
        bool occ = h >= (uint32_t)hit_levels;
#pragma unroll
        for (int k = 0; k < kMaxHitLevels; ++k) occ |= (h == (uint32_t)k) & (p >= pass_thresh[k]) & (k < hit_levels);
        return occ ? 100u : 0u;
    }
};

}  // namespace slam
