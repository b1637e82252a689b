// View gain for gfx950 (MI355X): the cells a scan from a pose would reveal.
//
//   slam_grid_view_gain   per view (a pose and the beams of one scan, every beam cast to max_range) the SET of map
//                         cells the beams see - path indices skip .. j of bresenham(start, end).path, j the find of
//                         trace() or the path's end - counted against the map's classes: unknown, free, occupied;
//                         and the beams that found nothing (OPEN)
//
// The beams are the ray cast's (beam_cells, trace: ray_trace.h, the only copies) on the float-error walk of grid_walk.h.
// Beams of one view share most of their cells near the origin, so the answer is a union: one bit per cell of the
// view's box (the bounding box of its start and end cells, clipped to the map, whole 32-cell words in y), set along
// the rays and counted against two bit planes of the map, pmap == 100 and pmap == 50 (k_view_pack).
//
// One workgroup owns a view.  Each lane traces its beam, then walks it again and sets the bits of the steps it sees:
// the float error chain cannot run backwards (trace's own rule), so a reversed line needs its find before it knows
// which steps count - and walking every beam twice keeps one marking loop for both directions.  The bits of the
// current window word wait in a register while the walk stays inside that word: one atomic OR per word change.
//
// Two engines run the same code (k_view<LDS>) and differ only in where the window lies:
//   LDS      in dynamic LDS; boxes whose window is at most kViewLdsBytes
//   global   in a slot of the call's workspace, global atomic ORs and device-scope loads; every other box
// choose_view_lds() (launch_shapes.h) decides per view, on the device, for both kernels.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "slam_internal.h"
#include "grid_walk.h"
#include "ray_trace.h"

namespace slam {

// The two class planes, one bit per cell: a wave takes 64 consecutive cells of a row, one lane each, and its ballots
// are two words of each plane (k_raycast_pack with a second plane).
__global__ void __launch_bounds__(256) k_view_pack(const uint32_t *__restrict__ pass, const uint32_t *__restrict__ hit, long rows,
                                                   int yw, int wpr, OccRule rule, uint32_t *__restrict__ occ_plane,
                                                   uint32_t *__restrict__ unk_plane)
{
    for (long row = blockIdx.x; row < rows; row += gridDim.x) {
        const uint32_t *p = pass + (size_t)row * yw, *h = hit + (size_t)row * yw;
        uint32_t *mo = occ_plane + (size_t)row * wpr, *mu = unk_plane + (size_t)row * wpr;
        for (int base = (threadIdx.x >> 6) * 64; base < yw; base += blockDim.x) {      // (wave-uniform)
            const int ly = base + (threadIdx.x & 63);
            const uint32_t v = ly < yw ? rule.value(p[ly], h[ly]) : 0u;
            const unsigned long long occ = __ballot(v == 100u), unk = __ballot(v == 50u);
            if ((threadIdx.x & 63) == 0) {
                mo[base >> 5] = (uint32_t)occ;
                mu[base >> 5] = (uint32_t)unk;
                if ((base >> 5) + 1 < wpr) {
                    mo[(base >> 5) + 1] = (uint32_t)(occ >> 32);
                    mu[(base >> 5) + 1] = (uint32_t)(unk >> 32);
                }
            }
        }
    }
}

// A window word, in LDS or in a global slot.  The global slot is written by atomics at the L2 and read back by other
// waves of the workgroup: its plain accesses are device-scope atomics too, so no stale line of the L1 is ever read.
template <bool LDS> __device__ __forceinline__ void win_store(uint32_t *w, uint32_t v)
{
    if (LDS) *w = v;
    else __hip_atomic_store(w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool LDS> __device__ __forceinline__ uint32_t win_load(const uint32_t *w)
{
    if (LDS) return *w;
    return __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The box of a view in map coordinates and its window: rows x0 .. x0 + bh - 1, words wy0 .. wy0 + bw - 1 of each.
struct ViewBox {
    int x0, wy0, bh, bw, words;
};

// Sets the bits of the path indices skip .. (j >= 0 ? j : Lp - 1) of bresenham(start, end).path that lie in the map.
// Walk steps: k = path index, or dx - k on a reversed line (bresenham.py:57-58).
template <bool LDS>
__device__ __forceinline__ void mark(uint32_t *win, const ViewBox &bx, int xw, int yw, int sx, int sy, int ex, int ey, int skip, int j)
{
    Ray r;
    if (!ray_setup(sx, sy, ex, ey, r)) return;
    const int jmax = j >= 0 ? j : r.dx;
    if (skip > jmax) return;
    const int k0 = r.flag ? r.dx - jmax : skip, k1 = r.flag ? r.dx - skip : jmax;
    CellWalk w(r);
    int cur = -1;
    uint32_t pend = 0;
    for (int k = 0; k <= k1; ++k) {
        if (k >= k0 && (unsigned)w.lx < (unsigned)xw && (unsigned)w.ly < (unsigned)yw) {
            const int wi = (w.lx - bx.x0) * bx.bw + ((w.ly >> 5) - bx.wy0);
            if (wi != cur) {
                if (pend) atomicOr(&win[cur], pend);
                cur = wi; pend = 0;
            }
            if ((unsigned)wi < (unsigned)bx.words) pend |= 1u << (w.ly & 31);     // (always: a path stays inside its box)
        }
        (void)w.next();
    }
    if (pend) atomicOr(&win[cur], pend);
}

__device__ __forceinline__ int wave_min(int v)
{
    for (int o = kWave / 2; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, kWave));
    return v;
}
__device__ __forceinline__ int wave_max(int v)
{
    for (int o = kWave / 2; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, kWave));
    return v;
}
__device__ __forceinline__ int wave_sum(int v)
{
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

// One workgroup per view, grid-stride over the views.  Every branch around a barrier is on values the whole workgroup
// reads from the same addresses (the pose, the map entry, the box in LDS).
template <bool LDS>
__global__ void __launch_bounds__(kViewThreads) k_view(ViewArgs a, int lds_words)
{
    extern __shared__ uint32_t lds_win[];
    __shared__ int s_box[4], s_cnt[SLAM_VIEW_COUNTS];
    char *guard = reinterpret_cast<char *>(lds_win + lds_words);
    if (LDS) lds_guard_fill(guard);
    const GridDev &g = a.g;
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int map_words = g.xw * a.wpr;
    uint32_t *win = LDS ? lds_win : a.slots + (size_t)blockIdx.x * map_words;
    for (long b = blockIdx.x; b < a.B; b += gridDim.x) {
        const double *pose = a.poses + 3 * (size_t)b;
        const int gi = a.maps ? a.maps[b] : 0;
        int bad_start = 0;
        const int sx = to_cell(pose[0], g.scale, g.off_x, bad_start), sy = to_cell(pose[1], g.scale, g.off_y, bad_start);
        const double hc = cos(pose[2]), hs = sin(pose[2]);            // the heading: once per view
        const bool bad = (unsigned)gi >= (unsigned)g.G || bad_start || !(isfinite(pose[0]) && isfinite(pose[1]) && isfinite(pose[2]));

        // ---- the box: start cell and every valid end cell
        __syncthreads();                                              // every lane is done with the view before
        if (tid == 0) {
            s_box[0] = s_box[2] = sx; s_box[1] = s_box[3] = sy;
            for (int c = 0; c < SLAM_VIEW_COUNTS; ++c) s_cnt[c] = 0;
        }
        __syncthreads();
        if (!bad) {
            int lo_x = sx, lo_y = sy, hi_x = sx, hi_y = sy;
            for (int i = tid; i < a.n; i += kViewThreads) {
                int px, py, ex, ey, be = 0;                           // (the start cell is good: be is the end's)
                beam_cells(g, pose[0], pose[1], hc, hs, a.cos_t[i], a.sin_t[i], (double)a.max_range, px, py, ex, ey, be);
                if (!be) { lo_x = min(lo_x, ex); hi_x = max(hi_x, ex); lo_y = min(lo_y, ey); hi_y = max(hi_y, ey); }
            }
            lo_x = wave_min(lo_x); lo_y = wave_min(lo_y); hi_x = wave_max(hi_x); hi_y = wave_max(hi_y);
            if (lane == 0) { atomicMin(&s_box[0], lo_x); atomicMin(&s_box[1], lo_y); atomicMax(&s_box[2], hi_x); atomicMax(&s_box[3], hi_y); }
        }
        __syncthreads();
        const int x0 = max(s_box[0], 0), y0 = max(s_box[1], 0), x1 = min(s_box[2], g.xw - 1), y1 = min(s_box[3], g.yw - 1);
        const bool any = !bad && x0 <= x1 && y0 <= y1;                // some cell of the box is in the map
        ViewBox bx;
        bx.x0 = x0; bx.wy0 = y0 >> 5;
        bx.bh = any ? x1 - x0 + 1 : 0; bx.bw = any ? (y1 >> 5) - bx.wy0 + 1 : 0;
        bx.words = bx.bh * bx.bw;
        const bool to_lds = bad || choose_view_lds(bx.words, a.lds_mode);
        if (LDS ? !to_lds : (a.lds_mode != 0 && to_lds)) continue;   // the other engine's view
        if (bx.words > (LDS ? lds_words : map_words)) continue;      // (never: a box is inside its map, an LDS window inside the bound)

        int32_t *counts = a.counts_out + (size_t)b * SLAM_VIEW_COUNTS;
        uint32_t *seen = a.seen_out ? a.seen_out + (size_t)b * map_words : nullptr;
        if (bad) {
            if (tid < SLAM_VIEW_COUNTS) counts[tid] = -1;
            if (seen) for (int k = tid; k < map_words; k += kViewThreads) seen[k] = 0u;
            continue;
        }

        // ---- trace, then mark
        for (int k = tid; k < bx.words; k += kViewThreads) win_store<LDS>(&win[k], 0u);
        __syncthreads();
        const uint32_t *occ = a.occ + (size_t)gi * map_words, *unk = a.unk + (size_t)gi * map_words;
        int open = 0;
        for (int base = 0; base < a.n; base += kViewThreads) {      // (whole waves: the ballot below)
            const int i = base + tid;
            bool is_open = false;
            if (i < a.n) {
                int px, py, ex, ey, be = 0;
                beam_cells(g, pose[0], pose[1], hc, hs, a.cos_t[i], a.sin_t[i], (double)a.max_range, px, py, ex, ey, be);
                if (!be) {
                    int Lp, fx, fy;
                    const int j = trace(occ, g.xw, g.yw, a.wpr, sx, sy, ex, ey, a.skip, Lp, fx, fy);
                    is_open = j < 0;
                    mark<LDS>(win, bx, g.xw, g.yw, sx, sy, ex, ey, a.skip, j);
                }
            }
            open += __popcll(__ballot(is_open));
        }
        if (lane == 0 && open) atomicAdd(&s_cnt[SLAM_VIEW_OPEN], open);
        __syncthreads();

        // ---- count the window against the class planes
        int c_unk = 0, c_occ = 0, c_all = 0;
        for (int k = tid; k < bx.words; k += kViewThreads) {
            const uint32_t bits = win_load<LDS>(&win[k]);
            const int at = (x0 + k / bx.bw) * a.wpr + bx.wy0 + k % bx.bw;
            c_unk += __popc(bits & unk[at]);
            c_occ += __popc(bits & occ[at]);
            c_all += __popc(bits);
        }
        c_unk = wave_sum(c_unk); c_occ = wave_sum(c_occ); c_all = wave_sum(c_all);
        if (lane == 0) {
            if (c_unk) atomicAdd(&s_cnt[SLAM_VIEW_UNKNOWN], c_unk);
            if (c_occ) atomicAdd(&s_cnt[SLAM_VIEW_OCCUPIED], c_occ);
            if (c_all - c_unk - c_occ) atomicAdd(&s_cnt[SLAM_VIEW_FREE], c_all - c_unk - c_occ);
        }
        __syncthreads();
        if (tid < SLAM_VIEW_COUNTS) counts[tid] = s_cnt[tid];
        if (seen) {
            for (int k = tid; k < map_words; k += kViewThreads) {    // the whole [xw][wpr] of the view: zero outside the box
                const int rx = k / a.wpr - x0, rw = k % a.wpr - bx.wy0;
                const bool inside = (unsigned)rx < (unsigned)bx.bh && (unsigned)rw < (unsigned)bx.bw;
                seen[k] = inside ? win_load<LDS>(&win[rx * bx.bw + rw]) : 0u;
            }
        }
    }
    if (LDS) lds_guard_check(guard, a.g.status);
}

hipError_t launch_view_pack(const GridDev &g, uint32_t *occ, uint32_t *unk, hipStream_t s)
{
    const long rows = (long)g.G * g.xw;
    SLAM_LAUNCH(k_view_pack, dim3((unsigned)std::min(rows, 1L << 20)), dim3(256), 0, s, g.pass, g.hit, rows, g.yw, (g.yw + 31) / 32,
                OccRule::of(g), occ, unk);
    return hipGetLastError();
}

hipError_t launch_view(const ViewArgs &a, const ViewShape &p, hipStream_t s)
{
    if (p.grid_lds > 0) {
        const int lds = (int)p.launch_lds, lds_words = (lds - kLdsGuard) / 4;
        hipError_t e = allow_dynamic_lds((const void *)k_view<true>, lds);
        if (e != hipSuccess) return e;
        SLAM_LAUNCH(k_view<true>, dim3((unsigned)p.grid_lds), dim3(kViewThreads), lds, s, a, lds_words);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (p.grid_global > 0) SLAM_LAUNCH(k_view<false>, dim3((unsigned)p.grid_global), dim3(kViewThreads), 0, s, a, 0);
    return hipGetLastError();
}

}  // namespace slam
