// The read side of the occupancy grid for gfx950 (MI355X): rays traced THROUGH a map.
//
//   trace(map, start, end, skip)   the first occupied cell, in PATH order, of bresenham(start, end).path
//                                  (W12m/bresenham.py:2-58) from path index `skip` on (ray_trace.h, shared with
//                                  the view gain of view_kernels.hip)
//   slam_grid_raycast              the scan the map would give: every beam cast to max_range from a pose
//   slam_grid_scan_score           a measured scan against the map: every beam traced to its own end cell and
//                                  put into one of seven classes (SLAM_RAY_*), tallied per hypothesis
//
// The beams are formed as the map was built (W12m/slam_ekf.py:88-90, :115-123; ReplaySource::ray of
// grid_kernels.hip: one multiply per coordinate, u2T(pose).dot(pc), both cells through to_cell), and the line is
// the reference's own float-error walk, grid_walk.h: ray_setup + CellWalk, step for step what Mapping.update
// visits.  "Occupied" is pmap == 100 as k_grid_finalize would write it: OccRule on the integer counters, packed
// by k_raycast_pack into one bit per cell before every call, mask[g][lx][ly / 32] bit ly % 32.
//
// A line with `flag` set (bresenham.py:19-29, half of all directions) is walked end -> start, so the first
// occupied cell in path order is the LAST one the walk meets: such a lane walks its whole line and keeps the
// latest find; an unflagged lane stops at its first.
//
// Two engines run the same per-ray code (one_ray) and differ only in where the mask words come from:
//   direct   one lane per ray over the whole batch, mask words from global memory (L2-resident at the project's
//            map sizes), any map size
//   staged   a workgroup takes a run of consecutive hypotheses, copies their map's mask into LDS with coalesced
//            dword loads (again when the map changes inside the run) and walks from LDS; maps whose mask is at
//            most kRaycastLdsBytes
// choose_raycast_path() picks between them.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "slam_internal.h"
#include "grid_walk.h"
#include "ray_trace.h"

namespace slam {

// One bit per cell: a wave takes 64 consecutive cells of a row, one lane each, and the ballot is their two mask
// words.  Block x = (map, row), 256 lanes stride along the row.
__global__ void __launch_bounds__(256) k_raycast_pack(const uint32_t *__restrict__ pass, const uint32_t *__restrict__ hit,
                                                      long rows, int yw, int wpr, OccRule rule, uint32_t *__restrict__ mask)
{
    for (long row = blockIdx.x; row < rows; row += gridDim.x) {
        const uint32_t *p = pass + (size_t)row * yw, *h = hit + (size_t)row * yw;
        uint32_t *m = mask + (size_t)row * wpr;
        for (int base = (threadIdx.x >> 6) * 64; base < yw; base += blockDim.x) {      // (wave-uniform)
            const int ly = base + (threadIdx.x & 63);
            const bool occ = ly < yw && rule.value(p[ly], h[ly]) == 100u;
            const unsigned long long bits = __ballot(occ);
            if ((threadIdx.x & 63) == 0) {
                m[base >> 5] = (uint32_t)bits;
                if ((base >> 5) + 1 < wpr) m[(base >> 5) + 1] = (uint32_t)(bits >> 32);
            }
        }
    }
}

// Per-hypothesis tallies of a wave's classes: for every hypothesis the wave holds, lane c < 7 adds the number of
// its lanes in class c.  Integer adds, so a hypothesis gets the same counts in any batch.  Called by whole waves.
__device__ __forceinline__ void tally(int32_t *__restrict__ counts, bool active, int b, int cls)
{
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(active);
    while (todo) {
        const int lb = __shfl(b, __ffsll((long long)todo) - 1, kWave);
        const bool mine = active && b == lb;
        int cnt = 0;
#pragma unroll
        for (int c = 0; c < SLAM_RAY_CLASSES; ++c) {
            const int k = __popcll(__ballot(mine && cls == c));
            if (lane == c) cnt = k;
        }
        if (lane < SLAM_RAY_CLASSES && cnt) atomicAdd(&counts[(size_t)lb * SLAM_RAY_CLASSES + lane], cnt);
        todo &= ~__ballot(mine);
    }
}

// Beam i of hypothesis b against map gi (-1: grid_of_batch[b] names no map), `mask` that map's words.
template <bool SCORE>
__device__ __forceinline__ int one_ray(const RaycastArgs &a, const uint32_t *mask, int gi, int b, int i)
{
    const GridDev &g = a.g;
    const size_t out = (size_t)b * a.n + i;
    const double *pose = a.poses + 3 * (size_t)b;
    const double px = pose[0], py = pose[1];
    int bad = gi < 0 ? kStatusOverflow : 0, pcx = 0, pcy = 0, pox = 0, poy = 0;
    if (!bad) {
        const double c = cos(pose[2]), s = sin(pose[2]);
        double rr = SCORE ? (double)a.ranges[(size_t)b * a.range_stride + i] : (double)a.max_range;
        if (SCORE && rr == INFINITY) rr = 30.0;                      // slam_ekf.py:119
        beam_cells(g, px, py, c, s, a.cos_t[i], a.sin_t[i], rr, pcx, pcy, pox, poy, bad);
    }
    int Lp = 0, fx = -1, fy = -1, j = -1;
    if (!bad) j = trace(mask, g.xw, g.yw, a.wpr, pcx, pcy, pox, poy, a.skip, Lp, fx, fy);
    if (!SCORE) {
        float range = __builtin_nanf("");
        if (!bad) {
            range = INFINITY;
            if (j >= 0) {
                const double dx = ((double)fx + 0.5) / g.scale - g.off_x - px;
                const double dy = ((double)fy + 0.5) / g.scale - g.off_y - py;
                range = (float)sqrt(dx * dx + dy * dy);
            }
        }
        a.ranges_out[out] = range;
        if (a.cells_out) { a.cells_out[2 * out] = fx; a.cells_out[2 * out + 1] = fy; }
        return 0;
    }
    int cls;
    if (bad) cls = SLAM_RAY_BAD;
    else if (Lp == 0) cls = SLAM_RAY_EMPTY;
    else if (j == Lp - 1) cls = SLAM_RAY_HIT;
    else if (j >= 0) cls = SLAM_RAY_BLOCKED;
    else if ((unsigned)pox < (unsigned)g.xw && (unsigned)poy < (unsigned)g.yw) {
        const size_t cell = ((size_t)gi * g.xw + pox) * g.yw + poy;
        cls = (g.pass[cell] | g.hit[cell]) ? SLAM_RAY_FREE : SLAM_RAY_UNKNOWN;      // pmap == 50: never touched
    } else cls = SLAM_RAY_OUT;
    if (a.class_out) a.class_out[out] = (int8_t)cls;
    return cls;
}

__device__ __forceinline__ int map_of(const RaycastArgs &a, int b) { return a.maps ? a.maps[b] : 0; }

// Direct engine: one lane per ray, grid-stride over all B * n of them.
template <bool SCORE>
__global__ void __launch_bounds__(256) k_raycast_direct(RaycastArgs a)
{
    const long total = (long)a.B * a.n, stride = (long)gridDim.x * blockDim.x;
    const size_t words = (size_t)a.g.xw * a.wpr;
    for (long base = (long)blockIdx.x * blockDim.x; base < total; base += stride) {   // (block-uniform: tally needs whole waves)
        const long r = base + threadIdx.x;
        const bool active = r < total;
        int b = 0, cls = 0;
        if (active) {
            b = (int)(r / a.n);
            int gi = map_of(a, b);
            if ((unsigned)gi >= (unsigned)a.g.G) gi = -1;
            cls = one_ray<SCORE>(a, a.mask + (size_t)std::max(gi, 0) * words, gi, b, (int)(r - (long)b * a.n));
        }
        if (SCORE) tally(a.counts_out, active, b, cls);
    }
}

// Staged engine: block x takes hypotheses [x * hyps_per_block, ...) and works through them in runs of one map.
template <bool SCORE>
__global__ void __launch_bounds__(256) k_raycast_staged(RaycastArgs a)
{
    extern __shared__ uint32_t lds_mask[];
    const int words = a.g.xw * a.wpr;
    char *guard = reinterpret_cast<char *>(lds_mask + words);
    lds_guard_fill(guard);
    const long h0 = (long)blockIdx.x * a.hyps_per_block, h1 = std::min((long)a.B, h0 + a.hyps_per_block);
    int staged = -1;
    for (long b0 = h0; b0 < h1;) {
        const int raw = map_of(a, (int)b0);
        long e = b0 + 1;
        while (e < h1 && map_of(a, (int)e) == raw) ++e;
        const int gi = (unsigned)raw < (unsigned)a.g.G ? raw : -1;
        if (gi >= 0 && gi != staged) {                                // (block-uniform)
            __syncthreads();                                          // every lane is done with the mask staged before
            const uint32_t *src = a.mask + (size_t)gi * words;
            for (int k = threadIdx.x; k < words; k += blockDim.x) lds_mask[k] = src[k];
            __syncthreads();
            staged = gi;
        }
        const long total = (e - b0) * a.n;
        for (long base = 0; base < total; base += blockDim.x) {
            const long r = base + threadIdx.x;
            const bool active = r < total;
            int b = 0, cls = 0;
            if (active) {
                b = (int)(b0 + r / a.n);
                cls = one_ray<SCORE>(a, lds_mask, gi, b, (int)(r % a.n));
            }
            if (SCORE) tally(a.counts_out, active, b, cls);
        }
        b0 = e;
    }
    lds_guard_check(guard, a.g.status);
}

// ---------------------------------------------------------------------------------
// Which engine traces a call ("raycast_lds": -1 automatic, 0 direct, 1 staged wherever the mask fits).
//
// kRaycastLdsBytes = 64 KiB of mask (512 K cells, e.g. 724 x 724): two 256-lane workgroups share a compute unit's
// 160 KiB; the 20.8 KB of a 400 x 400 map let seven be resident (28 waves of the 32 a compute unit holds).
//
// The automatic rule follows tools/bench_raycast.py (profiles/raycast_bench.json): automatic means
// DIRECT.  Course map at 400 x 400, 360 beams, ms per call, direct / staged:
//     B            1         64       1 024     8 192     65 536
//     ray cast   0.123/0.165 0.146/0.195 0.206/0.244 1.017/1.181 7.40/7.95      staged 7 - 34 % slower everywhere
//     score      0.123/0.108 0.132/0.126 0.169/0.144 0.613/0.639 4.08/4.25      staged 4 - 15 % faster to B = 1 024, 4 % slower beyond
// A walk step is bound by its own dependent instructions (the float64 error chain), not by the mask load: with one
// load per 32 cells of a row kept in a register there is little latency for LDS to remove, and a workgroup per
// hypothesis leaves 152 of its second pass's 256 lanes idle at 360 beams.  The staged engine's one gain (short scored
// beams of small batches, 0.02 ms) does not carry a rule of its own.
// ---------------------------------------------------------------------------------
constexpr size_t kRaycastLdsBytes = 64 * 1024;
constexpr long kRaycastMaxBlocks = 1L << 20;
constexpr long kRaycastStagedBlocks = 2048;        // the staged engine's grid: eight workgroups per compute unit

size_t raycast_mask_words(const GridDev &g) { return (size_t)g.G * g.xw * ((g.yw + 31) / 32); }

bool choose_raycast_path(const GridDev &g, int lds_mode, long B, int n)
{
    const bool fits = (size_t)g.xw * ((g.yw + 31) / 32) * 4 <= kRaycastLdsBytes;
    if (!fits || lds_mode == 0) return false;
    if (lds_mode == 1) return true;
    (void)B; (void)n;                       // automatic: direct at every size measured (the table above)
    return false;
}

hipError_t launch_raycast_pack(const GridDev &g, uint32_t *mask, hipStream_t s)
{
    const long rows = (long)g.G * g.xw;
    SLAM_LAUNCH(k_raycast_pack, dim3((unsigned)std::min(rows, kRaycastMaxBlocks)), dim3(256), 0, s, g.pass, g.hit, rows, g.yw,
                (g.yw + 31) / 32, OccRule::of(g), mask);
    return hipGetLastError();
}

hipError_t launch_raycast(RaycastArgs a, bool staged, hipStream_t s)
{
    a.wpr = (a.g.yw + 31) / 32;
    const bool score = a.counts_out != nullptr;
    if (staged) {
        a.hyps_per_block = (int)((a.B + kRaycastStagedBlocks - 1) / kRaycastStagedBlocks);
        const long blocks = (a.B + a.hyps_per_block - 1) / a.hyps_per_block;
        const int lds = a.g.xw * a.wpr * 4 + kLdsGuard;
        const void *fn = score ? (const void *)k_raycast_staged<true> : (const void *)k_raycast_staged<false>;
        hipError_t e = allow_dynamic_lds(fn, lds);
        if (e != hipSuccess) return e;
        if (score) SLAM_LAUNCH(k_raycast_staged<true>, dim3((unsigned)blocks), dim3(256), lds, s, a);
        else SLAM_LAUNCH(k_raycast_staged<false>, dim3((unsigned)blocks), dim3(256), lds, s, a);
        return hipGetLastError();
    }
    const long blocks = std::min(((long)a.B * a.n + 255) / 256, kRaycastMaxBlocks);
    if (score) SLAM_LAUNCH(k_raycast_direct<true>, dim3((unsigned)blocks), dim3(256), 0, s, a);
    else SLAM_LAUNCH(k_raycast_direct<false>, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace slam
