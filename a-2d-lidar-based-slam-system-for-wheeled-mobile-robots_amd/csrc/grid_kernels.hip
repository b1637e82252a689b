// Occupancy-grid kernels for gfx950 (MI355X): the float-error Bresenham ray walk of the
// reference with integer evidence counters, the threshold/finalize pass, and the
// stand-alone line rasteriser.
//
// Functional spec = the reference's Python (W12m = "W12_LiDAR SLAM/w12-mapping/
// course_agv_slam/scripts" under /root/reference):
//   Mapping.update   W12m/mapping.py:22-51    -> cast_ray / k_grid_update*
//   bresenham        W12m/bresenham.py:2-58   -> ray_setup + walk_step (every engine's loop), k_bresenham
//   pmap threshold   W12m/mapping.py:47-50    -> k_grid_finalize
//   publishMap       W12m/slam_ekf.py:270-271 -> k_grid_transpose
//
// Evidence model (DESIGN.md "K4"): the reference adds 0.01 per pass-through cell and 20
// on the last cell of each ray into a float64 map and thresholds at > 10.  Those sums
// commute only as integers, so the device keeps uint32 pass / hit counters per cell
// (atomicAdd, order-free, bit-reproducible) and the finalize kernel applies the rule the
// float sums obey: untouched -> 50; hit >= 1 (20 > 10) or pass >= 1001 (the 1001st
// sequential +0.01 is the first float64 sum above 10) -> 100; else 0.
//
// The ray walk keeps the reference's float64 error accumulation verbatim
// (error += dy/float(dx); if error >= 0.5: y += ystep; error -= 1.0): 15 % of lines
// differ from integer Bresenham, so anything else breaks cell parity.  The rule lives in ONE
// place, walk_step() of grid_walk.h (with ray_setup, CellWalk, to_cell and OccRule: shared with the kernels that
// read a map along rays, raycast_kernels.hip); the engines share two walks built on it - CellWalk (the cell as map
// coordinates, bounds tested by the caller) and lds_walk (unchecked, the cell as one running LDS byte address) - and
// the plain x0 + k, y loops call walk_step directly.  To change the walk, change walk_step.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <utility>
#include <vector>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "slam_internal.h"
#include "slam_stamps.h"
#include "grid_walk.h"
#include "workspace.h"

namespace slam {

// One ray of Mapping.update (mapping.py:38-50): +1 pass on every in-bounds cell of the
// path except the last, +1 hit on the last.  Returns the number of in-bounds cells.
// The first cell of the path (the ray origin, shared by every ray of the scan) is not
// written here when `skip_first` is set: the caller adds it once per wave.
__device__ __forceinline__ unsigned cast_ray(uint32_t *__restrict__ pass, uint32_t *__restrict__ hit, int xw, int yw,
                                             int pcx, int pcy, int pox, int poy, bool &first_pending)
{
    Ray r;
    first_pending = false;
    if (!ray_setup(pcx, pcy, pox, poy, r)) return 0u;
    unsigned nvis = 0;
    double error = 0.0;                                              // :34
    int y = r.y0;
    for (int k = 0; k <= r.dx; ++k) {                                // :45
        int x = r.x0 + k;
        int lx = r.steep ? y : x, ly = r.steep ? x : y;              // :46-49
        bool last = r.flag ? (k == 0) : (k == r.dx);                 // last cell in PATH order
        bool first = r.flag ? (k == r.dx) : (k == 0);
        if ((unsigned)lx < (unsigned)xw && (unsigned)ly < (unsigned)yw) {   // mapping.py:41
            ++nvis;
            if (first && lx == pcx && ly == pcy) {
                first_pending = true;                                // aggregated by the caller
            } else {
                size_t c = (size_t)lx * yw + ly;
                atomicAdd(last ? &hit[c] : &pass[c], 1u);            // :42-45
            }
        }
        if (walk_step(error, r.derr)) y += r.ystep;
    }
    return nvis;
}

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

__device__ __forceinline__ int wave_or_i32(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v |= __shfl_xor(v, off, kWave);
    return v;
}

// Tail of the direct kernel (k_grid_update): per-wave aggregation of the origin cell and of
// the visit counter, and the sticky status word.
__device__ __forceinline__ void finish_wave(const GridDev &g, uint32_t *pass, int pcx, int pcy, bool first_pending,
                                            unsigned nvis, int bad)
{
    unsigned long long m = __ballot(first_pending);
    unsigned tot = wave_sum_u32(nvis);
    const int anybad = wave_or_i32(bad);
    if ((threadIdx.x & 63) == 0) {
        if (m) atomicAdd(&pass[(size_t)pcx * g.yw + pcy], (unsigned)__popcll(m));
        if (tot) atomicAdd(visit_slot(g.visits), (unsigned long long)tot);
        if (anybad) atomicOr(g.status, anybad);
    }
}

// ---------------------------------------------------------------------------------
// LDS-window ray casting (DESIGN.md "K4 v2").
//
// Direct global atomics run at the chip's scattered memory-side atomic rate (~2e10 /s,
// measured: profiles/r01_v1_*), far below what the walks themselves cost.  All rays of a
// scan start in the same cell and consecutive scans of a stream overlap almost entirely,
// so one workgroup takes a GROUP of consecutive scans of one stream, accumulates their
// pass-through evidence in a window of the map held in LDS and flushes the non-zero cells
// once, row by row, so the global atomics that remain are few and address-contiguous.
// Window cells are 16-bit pass counters, two per dword, updated with ds_add_u32 of
// 1 << 16*(cell & 1): a ray visits a cell at most once, so a count never exceeds the
// group's ray count (<= 65,535 by construction) and never carries into its neighbour.
// 36,864 cells = 72 KiB; with the sorted order and the scan constants of 8 to 16 scans a workgroup
// asks for 82 - 89 KB, which is ONE per CU of 160 KiB (the runtime's occupancy answer; two only with
// the smaller window of win_cells_for's two_per_cu).  Hits (one per ray) went
// straight to the global counters, 80 % of a replay launch's memory-side atomics; the shared-map kernel now counts the hits
// of sorted rays per end cell in the window, once the pass counts have left it, and sends ONE add per distinct end cell
// (flush_hits; context option "win_lds_hits", by default in launches of more workgroups than the chip has CUs: plan_win, launch_shapes.h).
// Every other form still adds its hits directly.  The window is the bounding box of the group's ray
// origins and endpoints (clamped to the map) when that fits, else a sub-rectangle of it
// around the first origin; cells of a ray outside the window fall back to direct global
// atomics, so the result is exact for any window.
//
// Which kernel casts a launch (plan_win in launch_shapes.h decides, launch_win launches; first match wins):
//   the map's only writer (live pmap, one group, one stream or a map per stream), one scan, one hit occupies, rows of a
//   multiple of 16 cells of which one fits the window, and
//       at most 384 beams, a re-do list      k_grid_update_owner8, then k_grid_update_owner_redo for what it left
//       at most 1 024 beams                  k_grid_update_owner (one or two rays per lane)
//   the map's only writer otherwise          k_grid_update_own (several scans: "grid_group"; more beams; three hit levels)
//   a map that other workgroups write too    k_grid_update_win (groups of scans of a replay)
// ---------------------------------------------------------------------------------
// Between a workgroup's own global atomics and its plain loads of the same cells: every wave waits
// for its atomics to be acknowledged, then the workgroup barrier.  The map belongs to this
// workgroup for the whole launch and none of its lines has been loaded before (no stale L1 copy
// can exist), so nothing has to be written back or invalidated: a device-wide __threadfence()
// here made every owner write the XCD's whole L2 back.
__device__ __forceinline__ void owner_fence() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// (the window's constants, LDS sizes and launch decision: launch_shapes.h)

struct ScanConst {
    double px, py, c, s;   // ray origin (world) and heading cos / sin (replay source only)
    int pcx, pcy, cbad, pad;
};
static_assert(sizeof(ScanConst) == kScanConstBytes, "win_sc_bytes (launch_shapes.h) sizes the scan constants by kScanConstBytes");

// Source of rays: scans of a replay (ranges + poses) ...
struct ReplaySource {
    const float *ranges;
    const double *cos_t, *sin_t, *poses;
    int n_scan, n;
    long traj_stride;      // floats between trajectories' scan blocks (0: every trajectory reads the same scans)
    int grid_per_traj;     // trajectory l casts into map l (particle hypotheses, BASELINE configs[2])
    const double *centres; // nullable [L][n_scan-1][2]: ray origins that are not the pose (w12-mapping-online,
                           // W12o/slam_ekf.py:71-77,104: the centre comes from /tf, the points from xEst)
    const double *heading_cs = nullptr;   // nullable [L][n_scan-1][2]: cos / sin of the poses' headings, where the pose kernel left them
    __device__ int scans_per_traj() const { return n_scan - 1; }
    __device__ int own_grid(int l) const { return grid_per_traj ? l : 0; }
    bool maps_are_private() const { return grid_per_traj != 0; }
    // the same streams from trajectory l0 on; scans k0 .. k0 + cnt - 1 of trajectory 0 (launches split by launch_in_chunks)
    ReplaySource trajectories_from(int l0) const
    {
        ReplaySource r = *this;
        const size_t k = (size_t)l0 * (n_scan - 1);
        r.ranges += (size_t)l0 * traj_stride; r.poses += 3 * k;
        if (centres) r.centres += 2 * k;
        if (heading_cs) r.heading_cs += 2 * k;
        return r;
    }
    ReplaySource scans_from(int k0, int cnt) const
    {
        ReplaySource r = *this;
        r.ranges += (size_t)k0 * n; r.poses += 3 * (size_t)k0;
        if (centres) r.centres += 2 * (size_t)k0;
        if (heading_cs) r.heading_cs += 2 * (size_t)k0;
        r.n_scan = cnt + 1;
        return r;
    }
    __device__ void scan_const(int l, int k, const GridDev &g, ScanConst &sc) const
    {
        const double *pose = poses + 3 * ((size_t)l * (n_scan - 1) + k);
        sc.px = pose[0]; sc.py = pose[1];
        if (heading_cs) {
            const double *cs = heading_cs + 2 * ((size_t)l * (n_scan - 1) + k);
            sc.c = cs[0]; sc.s = cs[1];
        } else {
            sc.c = cos(pose[2]); sc.s = sin(pose[2]);
        }
        sc.cbad = 0;
        double ox = sc.px, oy = sc.py;
        if (centres) {
            const double *ctr = centres + 2 * ((size_t)l * (n_scan - 1) + k);
            ox = ctr[0]; oy = ctr[1];
        }
        sc.pcx = to_cell(ox, g.scale, g.off_x, sc.cbad);
        sc.pcy = to_cell(oy, g.scale, g.off_y, sc.cbad);
    }
    // a beam's inputs (fetch) and its end cell (ray) are separate so that a kernel can have the loads in
    // flight while it does something else
    struct Beam { float r; double ct, st; };
    __device__ Beam fetch(int l, int k, int i) const
    {
        return Beam{ranges[(size_t)l * traj_stride + (size_t)(k + 1) * n + i], cos_t[i], sin_t[i]};
    }
    // false: beam skipped (mapping.py:30) or flagged in `bad`
    __device__ bool ray(const Beam &b, const ScanConst &sc, const GridDev &g, int &pox, int &poy, int &bad) const
    {
        double rr = (double)b.r;
        if (rr == INFINITY) rr = 30.0;                               // slam_ekf.py:119
        double lx = b.ct * rr, ly = b.st * rr;                       // :122
        double x = sc.c * lx + (-sc.s) * ly + sc.px * 1.0;           // u2T(pose).dot(pc), :89
        double y = sc.s * lx + sc.c * ly + sc.py * 1.0;
        if (fabs(x) == INFINITY) return false;
        pox = to_cell(x, g.scale, g.off_x, bad);
        poy = to_cell(y, g.scale, g.off_y, bad);
        bad |= sc.cbad;
        return !bad;
    }
    __device__ bool ray(int l, int k, int i, const ScanConst &sc, const GridDev &g, int &pox, int &poy, int &bad) const
    {
        return ray(fetch(l, k, i), sc, g, pox, poy, bad);
    }
};

// ... or the particles of grid FastSLAM (slam_grid_update_particles): trajectory l is particle l0 + l of F filters of P; it
// reads ITS FILTER's scan (l0 + l) / P and its own pose l, and casts into map l of its own.  Everything else - the beam's
// arithmetic above all - is the replay source's.  A dead particle (acc == SLAM_MCL_DEAD) gets a harmless origin and
// every beam skipped as mapping.py:30 skips one: nothing is cast and nothing is flagged.
struct ParticleSource : ReplaySource {
    const int32_t *acc;    // nullable [L]
    int P;
    long l0;               // particles before this launch's first (launches split at 65 535 particles)
    ParticleSource(const float *ranges_, const double *cos_t_, const double *sin_t_, const double *poses_, const int32_t *acc_, int n_, int P_)
        : ReplaySource{ranges_, cos_t_, sin_t_, poses_, 2, n_, 0L, 1, nullptr, nullptr}, acc(acc_), P(P_), l0(0) {}
    ParticleSource trajectories_from(long k) const
    {
        ParticleSource r = *this;
        r.poses += 3 * (size_t)k;
        if (acc) r.acc += k;
        r.l0 += k;
        return r;
    }
    ParticleSource scans_from(int, int) const { return *this; }      // (one scan per particle)
    __device__ void scan_const(int l, int k, const GridDev &g, ScanConst &sc) const
    {
        sc.pad = acc && acc[l] == SLAM_MCL_DEAD;
        if (!sc.pad) {
            ReplaySource::scan_const(l, k, g, sc);
            return;
        }
        sc.px = 0.0; sc.py = 0.0; sc.c = 1.0; sc.s = 0.0;            // (a dead particle's pose may hold anything)
        sc.cbad = 0;
        sc.pcx = to_cell(0.0, g.scale, g.off_x, sc.cbad);
        sc.pcy = to_cell(0.0, g.scale, g.off_y, sc.cbad);
    }
    __device__ Beam fetch(int l, int, int i) const { return Beam{ranges[(size_t)((l0 + l) / P) * n + i], cos_t[i], sin_t[i]}; }
    __device__ bool ray(const Beam &b, const ScanConst &sc, const GridDev &g, int &pox, int &poy, int &bad) const
    {
        return !sc.pad && ReplaySource::ray(b, sc, g, pox, poy, bad);
    }
    __device__ bool ray(int l, int k, int i, const ScanConst &sc, const GridDev &g, int &pox, int &poy, int &bad) const
    {
        return ray(fetch(l, k, i), sc, g, pox, poy, bad);
    }
};

// ... or explicit world-frame endpoints (Mapping.update's own arguments).
struct ExplicitSource {
    const double *ox, *oy, *cx, *cy;
    int B, n;
    __device__ int scans_per_traj() const { return B; }
    __device__ int own_grid(int) const { return 0; }
    bool maps_are_private() const { return false; }
    ExplicitSource trajectories_from(int) const { return *this; }          // (one stream)
    ExplicitSource scans_from(int k0, int cnt) const
    {
        ExplicitSource r = *this;
        r.ox += (size_t)k0 * n; r.oy += (size_t)k0 * n; r.cx += k0; r.cy += k0;
        r.B = cnt;
        return r;
    }
    __device__ void scan_const(int, int k, const GridDev &g, ScanConst &sc) const
    {
        sc.px = cx[k]; sc.py = cy[k]; sc.c = 1.0; sc.s = 0.0;
        sc.cbad = 0;
        sc.pcx = to_cell(sc.px, g.scale, g.off_x, sc.cbad);
        sc.pcy = to_cell(sc.py, g.scale, g.off_y, sc.cbad);
    }
    struct Beam { double x, y; };
    __device__ Beam fetch(int, int k, int i) const { return Beam{ox[(size_t)k * n + i], oy[(size_t)k * n + i]}; }
    __device__ bool ray(const Beam &b, const ScanConst &sc, const GridDev &g, int &pox, int &poy, int &bad) const
    {
        if (fabs(b.x) == INFINITY) return false;                     // mapping.py:30
        pox = to_cell(b.x, g.scale, g.off_x, bad);
        poy = to_cell(b.y, g.scale, g.off_y, bad);
        bad |= sc.cbad;
        return !bad;
    }
    __device__ bool ray(int l, int k, int i, const ScanConst &sc, const GridDev &g, int &pox, int &poy, int &bad) const
    {
        return ray(fetch(l, k, i), sc, g, pox, poy, bad);
    }
};

// Direct global atomics (Mapping.update as written): block (k, l) casts scan k of trajectory l, one lane per beam (a
// workgroup never spans two scans, so the origin cell is wave-uniform).  `maps` (nullable) names the map of every scan
// of explicit endpoints, of every trajectory of a replay.
template <class Src>
__global__ void __launch_bounds__(256) k_grid_update(GridDev g, Src src, const int32_t *__restrict__ maps)
{
    __shared__ int first_bad;
    const int k = blockIdx.x, l = blockIdx.y, n = src.n;
    const int gi = maps ? maps[std::is_same<Src, ExplicitSource>::value ? k : l] : 0;
    uint32_t *pass = g.pass + (size_t)gi * g.xw * g.yw, *hit = g.hit + (size_t)gi * g.xw * g.yw;
    ScanConst sc;                                                    // the origin is the same for every beam; a bad
    src.scan_const(l, k, g, sc);                                     // origin only raises if some beam is actually cast
    // the scan stops at its first beam that Python's int() would raise on (mapping.py:29-36: the beams before it have been
    // applied when the exception leaves update(), and the error is that beam's): find it before anything is cast
    if (threadIdx.x == 0) first_bad = INT_MAX;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        int bad = 0, pox, poy;
        (void)src.ray(l, k, i, sc, g, pox, poy, bad);                // (a skipped beam, mapping.py:30, leaves bad at 0)
        if (bad) atomicMin(&first_bad, i);
    }
    __syncthreads();
    const int stop = first_bad;
    for (int base = 0; base < n; base += blockDim.x) {
        int i = base + threadIdx.x;
        int bad = 0, pox, poy;
        bool first_pending = false;
        unsigned nvis = 0;
        if (i < n && i <= stop && src.ray(l, k, i, sc, g, pox, poy, bad))
            nvis = cast_ray(pass, hit, g.xw, g.yw, sc.pcx, sc.pcy, pox, poy, first_pending);
        finish_wave(g, pass, sc.pcx, sc.pcy, first_pending, nvis, bad);
    }
}

// LDS byte address of a pointer into shared memory, and a fire-and-forget 32-bit add at such an address
typedef __attribute__((address_space(3))) unsigned lds_u32_t;
__device__ __forceinline__ unsigned lds_addr(const void *p)
{
    return (unsigned)(uintptr_t)(__attribute__((address_space(3))) const void *)p;
}
__device__ __forceinline__ void lds_add_u32(unsigned addr, unsigned v)
{
    (void)__hip_atomic_fetch_add((lds_u32_t *)(uintptr_t)addr, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ int wave_min_i32(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, kWave));
    return v;
}
__device__ __forceinline__ int wave_max_i32(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, kWave));
    return v;
}

// The unchecked LDS walk, shared by every engine whose rays cannot leave their window (a Bresenham path never
// leaves the box of its ends): no bounds tests, the cell kept as ONE running LDS byte address `a` of its counter
// (dword = address & ~3, the count's position in it from the low address bits - the same expression for 16-bit
// and for 8-bit counters, whose callers scale a, da_k and da_y by 2 or by 1), four steps per wave-wide loop
// test with no lane mask inside, then a tail of up to three.  9 VALU + 1 LDS instructions per step.
// Adds 1 to the counters of `rem` cells from `a` on and leaves `error` where the walk stands.  `lead_in`: the
// first walk step is not counted (a reversed path starts on its hit cell).  A lane with rem == 0 and no
// lead-in does nothing.
__device__ __forceinline__ void lds_walk(unsigned a, int da_k, int da_y, int rem, double derr, double &error, bool lead_in)
{
    auto advance = [&]() {
        const bool stepy = walk_step(error, derr);
        a += (unsigned)(da_k + (stepy ? da_y : 0));
    };
    auto step = [&]() {
        lds_add_u32(a & ~3u, 1u << ((a << 3) & 31u));                // mapping.py:43
        advance();
    };
    if (lead_in) advance();
    for (;;) {
        const bool full = rem >= 4;
        if (!__any(full)) break;
        if (full) { step(); step(); step(); step(); rem -= 4; }
    }
#pragma unroll
    for (int u = 0; u < 3; ++u)
        if (rem > u) step();
}

// Rays are handed to waves 64 at a time from an LDS counter, in `order` when the group was sorted.  False: none
// are left for this wave; else r is the lane's ray, or -1 for a lane beyond the last one.
// slot: the lane's place in the order (dead once r has been read from it: cast_rays parks the ray's hit there).
__device__ __forceinline__ bool next_rays(int *next_ray, int nrays, const unsigned short *order, int &r, int &slot)
{
    const int lane = threadIdx.x & 63;
    int base = 0;
    if (lane == 0) base = atomicAdd(next_ray, kWave);
    base = __builtin_amdgcn_readfirstlane(base);
    if (base >= nrays) return false;
    slot = base + lane;
    r = slot >= nrays ? -1 : order ? (int)order[slot] : slot;        // longest rays first when sorted
    return true;
}
__device__ __forceinline__ bool next_rays(int *next_ray, int nrays, const unsigned short *order, int &r)
{
    int slot;
    return next_rays(next_ray, nrays, order, r, slot);
}

// Pass 2 of the window kernel: walk a workgroup's rays.  Rays are handed to waves 64 at a
// time from an LDS counter, in order of decreasing length when the group was sorted in pass 1
// (a wave runs as long as its longest ray: unsorted, 54 % of the lane-steps were idle).  The walk
// itself is VALU-issue bound (measured: ~4 cycles per instruction per wave, insensitive to
// occupancy, memory traffic and padding), so the body is kept short: the cell is kept as
// (lx, ly) and advanced incrementally, and the path's last cell (the hit, mapping.py:45) is
// remembered and written once after the loop.  It is the reference's loop
// (bresenham.py:45-55) step for step.
// park (nullable; the sorted order itself, writable): a ray of the unchecked walk sends no hit; it leaves the window index of
// its end cell (< 0xffff) in the slot of the order it was fetched from, and every other fetched slot is set to kNoHit, for
// flush_hits behind the pass flush.  Rays of a wave that walks the checked way add their hits directly, as without park.
template <bool COVERS, class Src>
__device__ __forceinline__ unsigned cast_rays(const GridDev &g, const Src &src, const ScanConst *sc, int l, int s0, int n,
                                              int nrays, int *next_ray, const unsigned short *order, unsigned *win, int wx0,
                                              int wy0, int W, int H, int Hp2, uint32_t *__restrict__ pass,
                                              uint32_t *__restrict__ hit, const int *first_bad, unsigned short *park = nullptr)
{
    unsigned nvis = 0;
    for (int r, slot; next_rays(next_ray, nrays, order, r, slot);) {
        if (r < 0) continue;
        if (park) park[slot] = (unsigned short)kNoHit;
        int s = r / n, i = r - s * n, pox, poy, b2 = 0;
        Ray ry;
        if (i >= first_bad[s]) continue;                             // beams from the scan's first bad one on are not cast
        if (!src.ray(l, s0 + s, i, sc[s], g, pox, poy, b2)) continue;
        if (!ray_setup(sc[s].pcx, sc[s].pcy, pox, poy, ry)) continue;
        CellWalk w(ry);
        int hx = -1, hy = -1;
        // A ray whose two end cells lie in the window stays in it: the unchecked walk (lds_walk).  The path's
        // last cell is the endpoint's cell (mapping.py:44-45); it takes the hit and no pass count, so the walk
        // leaves it out: a reversed path (flag) starts one step in.
        const int Hs = 2 * Hp2;
        const bool safe = (unsigned)(sc[s].pcx - wx0) < (unsigned)W && (unsigned)(sc[s].pcy - wy0) < (unsigned)H &&
                    (unsigned)(pox - wx0) < (unsigned)W && (unsigned)(poy - wy0) < (unsigned)H;
        // (a wave that also holds rays which leave the window walks all its rays the checked way: two loops
        // one after the other made the slowest workgroups - those whose half does not fit - slower)
        if (!__any(!safe)) {
            const unsigned a2 = lds_addr(win) + 2u * (unsigned)((w.lx - wx0) * Hs + (w.ly - wy0));   // 16-bit counters
            nvis += (unsigned)ry.dx + 1u;                             // every cell of the path is in the map
            // pass cells: all but the path's last
            lds_walk(a2, 2 * w.stride_k(Hs), 2 * w.stride_y(Hs), ry.dx, w.derr, w.error, ry.flag);
            if (park) park[slot] = (unsigned short)((pox - wx0) * Hs + (poy - wy0));
            else atomicAdd(&hit[(size_t)pox * g.yw + poy], 1u);       // mapping.py:45
            continue;
        }
        for (int k = 0; k <= ry.dx; ++k, w.next()) {                  // bresenham.py:45
            const int lx = w.lx, ly = w.ly;
            bool last = k == w.klast;
            unsigned wx = (unsigned)(lx - wx0), wy = (unsigned)(ly - wy0);
            bool inwin = wx < (unsigned)W && wy < (unsigned)H;
            bool inmap = COVERS ? inwin : ((unsigned)lx < (unsigned)g.xw && (unsigned)ly < (unsigned)g.yw);   // mapping.py:41
            nvis += inmap ? 1u : 0u;
            hx = last ? lx : hx; hy = last ? ly : hy;
            if (inwin && !last) atomicAdd(&win[wx * Hp2 + (wy >> 1)], 1u << ((wy & 1u) * 16u));          // mapping.py:43
            if (!COVERS) { if (inmap && !inwin && !last) atomicAdd(&pass[(size_t)lx * g.yw + ly], 1u); }
        }
        if ((unsigned)hx < (unsigned)g.xw && (unsigned)hy < (unsigned)g.yw) atomicAdd(&hit[(size_t)hx * g.yw + hy], 1u);   // mapping.py:45
    }
    return nvis;
}

// Single-scan owner form: the rays' bounding box is cut into strips of rows (x ranges) that each fit
// the window, and the scan is walked once per strip, counting only the strip's cells.  A ray whose
// x range misses the strip is skipped; a walk cannot be entered midway (its state is a rounded
// running sum), so a ray that reaches a later strip is walked again from its start.  The path's
// last cell gets its hit in the strip it lies in: the global counter by a fire-and-forget atomic
// and bit 15 of its window cell, so that the sweep knows where this scan's hits fell.
template <class Src>
__device__ __forceinline__ unsigned cast_rays_strip(const GridDev &g, const Src &src, const ScanConst &sc, int l, int s0,
                                                    int nrays, int *next_ray, const unsigned short *order, unsigned *win,
                                                    int wx0, int wy0, int W, int H, int Hp2, uint32_t *__restrict__ hit,
                                                    int first_bad)
{
    unsigned nvis = 0;
    for (int i; next_rays(next_ray, nrays, order, i);) {
        if (i < 0) continue;
        int pox, poy, b2 = 0;
        Ray ry;
        if (i >= first_bad) continue;                                // beams from the first bad one on are not cast
        if (!src.ray(l, s0, i, sc, g, pox, poy, b2)) continue;
        if (max(sc.pcx, pox) < wx0 || min(sc.pcx, pox) >= wx0 + W) continue;   // never enters this strip
        if (!ray_setup(sc.pcx, sc.pcy, pox, poy, ry)) continue;
        CellWalk w(ry);
        for (int k = 0; k <= ry.dx; ++k, w.next()) {                  // bresenham.py:45
            const unsigned wx = (unsigned)(w.lx - wx0), wy = (unsigned)(w.ly - wy0);
            if (wx < (unsigned)W && wy < (unsigned)H) {               // in this strip (every in-map cell of the ray is in some strip)
                ++nvis;                                               // mapping.py:41
                unsigned *cell = &win[wx * Hp2 + (wy >> 1)];
                const unsigned sh = (wy & 1u) * 16u;
                if (k != w.klast) atomicAdd(cell, 1u << sh);          // mapping.py:43
                else { atomicOr(cell, 0x8000u << sh); atomicAdd(&hit[(size_t)w.lx * g.yw + w.ly], 1u); }   // :45
            }
        }
    }
    return nvis;
}

// Control block of a window workgroup, in LDS behind the scan constants.  k_grid_update_win uses all of it, k_grid_update_own
// what is not about quadrants and phases.
struct WinCtl {
    int bbox[4];                     // x0, y0, x1, y1 of everything the group's rays can touch
    int qbox[4][4];                  // the same for the rays of each direction quadrant
    int next_ray;                    // rays handed out so far (next_rays)
    int strips, strip_w;             // single-scan owner form: number of strips of the box and their rows (0: not that form)
    int phases, parity;              // windows this workgroup fills one after the other; rays shared by beam parity
    alignas(8) unsigned long long visits;   // of the whole workgroup: ONE global add, at the very end
    int first_bad[kWinMaxGroup];     // every scan's first beam that Python's int() would raise on
    int phw[4][8];                   // window of a phase: x0, y0, W, H, covers
    int phq[4];                      // phase of a quadrant's rays (-1: not this workgroup's)
    int seg[5];                      // boundaries of the phases in the sorted order
};
static_assert(sizeof(WinCtl) <= kWinBoxInts * 4 && alignof(WinCtl) <= 16, "the control block outgrew its LDS region");

// The LDS regions of a window workgroup, carved for the launch's group size (win_lds_bytes): a small group leaves room
// for a second workgroup on the CU.
struct WinLds {
    ScanConst *sc; WinCtl *ctl; int *hist; unsigned short *order; unsigned *win; char *guard;
    __device__ __forceinline__ WinLds(char *smem, int group_size, int sort_cap, int win_cells)
        : sc(reinterpret_cast<ScanConst *>(smem)),                                       // [group_size]
          ctl(reinterpret_cast<WinCtl *>(smem + win_sc_bytes(group_size))),
          hist(reinterpret_cast<int *>(ctl) + kWinBoxInts),                              // [4][kSortBins]: (phase, length bin)
          order(reinterpret_cast<unsigned short *>(hist + 4 * kSortBins)),               // [sort_cap]
          win(reinterpret_cast<unsigned *>(order + sort_cap)),                           // [W][Hp2] dwords of two 16-bit cells
          guard(reinterpret_cast<char *>(win) + (size_t)win_cells * 2) {}
};

// Pass 1 of a window workgroup: the bounding box of everything the group's rays can touch (into bbox, which the caller
// has set to the empty box), every scan's first bad beam, whose own error is raised, and - when the rays are going to
// be sorted - park(r, i, casts, quad, lbin) for every ray r (beam i of its scan): whether it has anything to cast, its
// direction quadrant (bit 0: end cell right of the origin or in its column, bit 1: above it or in its row) and its
// length bin, longest first.  One barrier, before the errors are raised.
template <class Src, class Park>
__device__ __forceinline__ void win_pass1(const GridDev &g, const Src &src, const ScanConst *sc, int l, int s0, int cnt, int n,
                                          bool sorted, int *bbox, int *first_bad, Park &&park)
{
    const int tid = threadIdx.x;
    int bx0 = INT_MAX, by0 = INT_MAX, bx1 = INT_MIN, by1 = INT_MIN;
    for (int r = tid; r < cnt * n; r += blockDim.x) {
        int s = r / n, i = r - s * n, pox, poy, len = 0, b2 = 0, quad = 0;
        const bool valid = src.ray(l, s0 + s, i, sc[s], g, pox, poy, b2);
        if (valid) {
            quad = (pox >= sc[s].pcx ? 1 : 0) | (poy >= sc[s].pcy ? 2 : 0);
            const int rx0 = min(pox, sc[s].pcx), rx1 = max(pox, sc[s].pcx), ry0 = min(poy, sc[s].pcy), ry1 = max(poy, sc[s].pcy);
            bx0 = min(bx0, rx0); bx1 = max(bx1, rx1);
            by0 = min(by0, ry0); by1 = max(by1, ry1);
            len = max(abs(pox - sc[s].pcx), abs(poy - sc[s].pcy));
        }
        // a scan stops at its first beam that Python's int() would raise on (mapping.py:29-36: the beams before
        // it have been applied when the exception leaves update(), and the error is that beam's)
        if (b2) atomicMin(&first_bad[s], i);
        if (sorted) park(r, i, valid && len > 0, quad, kSortBins - 1 - min(len >> 2, kSortBins - 1));
    }
    bx0 = wave_min_i32(bx0); by0 = wave_min_i32(by0); bx1 = wave_max_i32(bx1); by1 = wave_max_i32(by1);
    if ((tid & 63) == 0 && bx0 <= bx1) {
        atomicMin(&bbox[0], bx0); atomicMin(&bbox[1], by0); atomicMax(&bbox[2], bx1); atomicMax(&bbox[3], by1);
    }
    __syncthreads();
    if (tid < cnt && first_bad[tid] != INT_MAX) {                    // the first bad beam's own error (NaN or overflow)
        int pox, poy, b2 = 0;
        (void)src.ray(l, s0 + tid, first_bad[tid], sc[tid], g, pox, poy, b2);
        atomicOr(g.status, b2);
    }
}

// Counting sort of ray ids by bin (bins[r]; 0xffff: not sorted in), two barriers: exclusive scan of the 64 * kBinsPerLane
// bins' histogram in wave 0, then every ray claims a slot in its bin.  Order inside a bin is arbitrary; the map update does not
// depend on ray order.  seg (nullable): where every block of kSortBins bins starts in the order, and where the last one ends.
template <int kBinsPerLane>
__device__ __forceinline__ void counting_sort(int *hist, const unsigned short *bins, unsigned short *order, int nrays, int *seg)
{
    constexpr int kLanesPerSeg = kSortBins / kBinsPerLane;
    const int lane = threadIdx.x & 63;
    if (threadIdx.x < kWave) {
        int h[kBinsPerLane], tot = 0;
#pragma unroll
        for (int u = 0; u < kBinsPerLane; ++u) { h[u] = hist[kBinsPerLane * lane + u]; tot += h[u]; }
        int inc = tot;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) { int v = __shfl_up(inc, off, kWave); if (lane >= off) inc += v; }
        int run = inc - tot;
        if (seg && lane % kLanesPerSeg == 0) seg[lane / kLanesPerSeg] = run;
        if (seg && lane == kWave - 1) seg[kWave / kLanesPerSeg] = inc;
#pragma unroll
        for (int u = 0; u < kBinsPerLane; ++u) { hist[kBinsPerLane * lane + u] = run; run += h[u]; }
    }
    __syncthreads();
    for (int r = threadIdx.x; r < nrays; r += blockDim.x)
        if (bins[r] != 0xffffu) order[atomicAdd(&hist[bins[r]], 1)] = (unsigned short)r;
    __syncthreads();
}

// (clamp_box, box_fits and the phase rule of k_grid_update_win: launch_shapes.h)
// The window for the rays of a clamped box o (clamp_box, same ymask; any: its result), into w[5] (x0, y0, W, H, covers):
// the box itself when it fits win_cells, else a sub-rectangle of it next to the first origin (the rays start there; clamped
// into the box, i.e. in its corner for a quadrant) - the rest goes by direct atomics.  Nothing in the map: no window.
__device__ __forceinline__ void fit_window(const GridDev &g, bool any, const int *o, int ymask, const ScanConst &first, int win_cells, int *w)
{
    int x0 = any ? o[0] : 0, y0 = any ? o[1] : 0, W = any ? o[2] - o[0] + 1 : 0, H = any ? o[3] - o[1] + 1 : 0, cov = 1;
    if (any && !box_fits(o, win_cells)) {
        const int Hd = min(H, 192), Wd = min(W, win_cells / ((Hd + 1) & ~1));   // rows are stored padded to an even height
        x0 = min(max(first.pcx - Wd / 2, o[0]), o[2] - Wd + 1);
        y0 = min(max(first.pcy - Hd / 2, o[1]), o[3] - Hd + 1) & ~ymask;
        W = Wd; H = Hd; cov = 0;
    }
    // W rows of (H + 1) / 2 dwords must fit the win_cells 16-bit cells carved for them.  Should the sizing above ever be wrong (it
    // once used the unpadded height: a 193 x 191 box wrote 96 dwords past the window): no window at all - every cell then takes
    // the direct-atomic path, still exact - and the internal-error status bit.
    if ((long)W * ((H + 1) >> 1) > win_cells / 2) { atomicOr(g.status, kStatusGuard); W = 0; H = 0; cov = 0; }
    w[0] = x0; w[1] = y0; w[2] = W; w[3] = H; w[4] = cov;
}

// Flush of a window: one wave per window row, lanes along y (contiguous in the [x][y] map), two cells per lane.  Every workgroup
// flushes the same part of the map: each one starts at a different row so that concurrent flushes do not queue on the same addresses.
// zero: every dword is cleared once it has been read (flush_hits counts in the window next).
__device__ __forceinline__ void flush_window(unsigned *win, uint32_t *pass, int yw, int wx0, int wy0, int W, int Hp2, bool pair64,
                                             bool zero = false)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const int rot = W > 0 ? (int)((blockIdx.x * 37u + blockIdx.y * 11u) % (unsigned)W) : 0;
    for (int rr = wave; rr < W; rr += nwaves) {
        const int row = rr + rot < W ? rr + rot : rr + rot - W;
        size_t gbase = (size_t)(wx0 + row) * yw + wy0;
        // The flush is bound by the chip's rate of global atomics (every workgroup of a replay adds its ~25 k touched cells to the
        // same map): a dword of the window - two cells that are neighbours in the map row - goes out as ONE 64-bit add of
        // (count0, count1 << 32).  A carry out of the low counter would need 2^32 passes.
        if (pair64 && (wy0 & 1) == 0) {
            for (int d = lane; d < Hp2; d += kWave) {
                unsigned v = win[row * Hp2 + d];
                if (zero) win[row * Hp2 + d] = 0u;
                if (v) atomicAdd(reinterpret_cast<unsigned long long *>(&pass[gbase + 2 * d]),
                                 (unsigned long long)(v & 0xffffu) | ((unsigned long long)(v >> 16) << 32));
            }
            continue;
        }
        for (int d = lane; d < Hp2; d += kWave) {
            unsigned v = win[row * Hp2 + d];
            if (zero) win[row * Hp2 + d] = 0u;
            unsigned p0 = v & 0xffffu, p1 = v >> 16;
            if (p0) atomicAdd(&pass[gbase + 2 * d], p0);
            if (p1) atomicAdd(&pass[gbase + 2 * d + 1], p1);          // p1 != 0 implies 2d+1 < H
        }
    }
}

// The hits of a phase whose rays parked them (cast_rays), behind a flush_window that has cleared the window (rows of Hs = 2 Hp2
// cells): every parked ray adds 1 to its end cell's 16-bit counter - a phase holds at most kMaxSortRays rays, so a count neither
// overflows nor carries into its neighbour -, the ONE lane that found the cell at zero then reads the cell's total and sends it
// to the global counter: one memory-side atomic per distinct end cell instead of one per ray.  Two barriers; the window is
// left dirty, as the flush of the pass counts leaves it.
__device__ __forceinline__ void flush_hits(unsigned *win, unsigned short *park, int nrays, uint32_t *hit, int yw, int wx0, int wy0,
                                           int Hs)
{
    __syncthreads();                                                 // the flush has read and cleared every dword
    for (int k = threadIdx.x; k < nrays; k += blockDim.x) {
        const unsigned c = park[k];
        if (c == kNoHit) continue;
        const unsigned sh = (c & 1u) * 16u;
        const unsigned old = atomicAdd(&win[c >> 1], 1u << sh);
        if ((old >> sh) & 0xffffu) park[k] = (unsigned short)kNoHit;   // an earlier lane carries this cell
    }
    __syncthreads();
    for (int k = threadIdx.x; k < nrays; k += blockDim.x) {
        const unsigned c = park[k];
        if (c == kNoHit) continue;
        const unsigned tot = (win[c >> 1] >> ((c & 1u) * 16u)) & 0xffffu;
        const unsigned wx = c / (unsigned)Hs, wy = c - wx * (unsigned)Hs;
        atomicAdd(&hit[(size_t)(wx0 + (int)wx) * yw + (wy0 + (int)wy)], tot);   // mapping.py:45, for every ray that ends here
    }
}

// Sweep of a strip of the single-scan owner forms (owner_cast, k_grid_update_own; the rule is spelt out above owner_cast): SW
// window rows of H cells (a multiple of 16: qrow = H / 4 quads, qinv its reciprocal for umulhi) that stand for the map rows from
// sx0 and the cells from wy0 on; a window cell is a 15-bit pass count and, in bit 15, "a hit of this scan fell here".  4 lanes
// per 64-byte piece of a counter row: only pieces the scan touched are read and written back; pmap only where it changes.
__device__ __forceinline__ void sweep_strip(const unsigned *win, uint32_t *pass, int8_t *pm, int yw, int sx0, int wy0, int SW, int H,
                                            int qrow, unsigned qinv, uint32_t pthr)
{
    const int tid = threadIdx.x, lane = tid & 63, Hp2 = H >> 1, total = SW * qrow;
    constexpr int kBatch = 4;                                     // 16-byte read-modify-writes a lane keeps in flight
    for (int q0 = tid; q0 < total; q0 += kBatch * blockDim.x) {
        uint4 p[kBatch];
        uint32_t om[kBatch], d0[kBatch], d1[kBatch];
        size_t at[kBatch];
        bool live[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const int q = q0 + u * (int)blockDim.x;
            d0[u] = d1[u] = 0u;
            if (q < total) {
                const int r = (int)__umulhi((unsigned)q, qinv), c = q - r * qrow;
                const uint2 d = *reinterpret_cast<const uint2 *>(win + (r * Hp2 + 2 * c));
                d0[u] = d.x; d1[u] = d.y;
                at[u] = (size_t)(sx0 + r) * yw + (wy0 + 4 * c);
            }
            // the four lanes of a piece decide together (total and blockDim are multiples of 4)
            const unsigned long long m = __ballot((d0[u] | d1[u]) != 0u);
            live[u] = ((m >> (lane & 60)) & 0xFull) != 0ull;
            if (live[u]) {
                p[u] = *reinterpret_cast<const uint4 *>(pass + at[u]);
                om[u] = *reinterpret_cast<const uint32_t *>(pm + at[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            if (!live[u]) continue;
            const uint32_t d0v = d0[u], d1v = d1[u];
            p[u].x += d0v & 0x7fffu; p[u].y += (d0v >> 16) & 0x7fffu; p[u].z += d1v & 0x7fffu; p[u].w += (d1v >> 16) & 0x7fffu;
            *reinterpret_cast<uint4 *>(pass + at[u]) = p[u];
            if (!(d0v | d1v)) continue;
            const uint32_t o = om[u];
            // one bit per byte (cell): touched by this scan / hit by this scan / occupied before (bit 6
            // is set in 100 only) / never touched before (bit 4 is set in 50 only)
            const uint32_t tb = ((d0v & 0xffffu) ? 1u : 0u) | ((d0v >> 16) ? 0x100u : 0u) | ((d1v & 0xffffu) ? 0x10000u : 0u) | ((d1v >> 16) ? 0x1000000u : 0u);
            const uint32_t fb = ((d0v >> 15) & 1u) | (((d0v >> 31) & 1u) << 8) | (((d1v >> 15) & 1u) << 16) | ((d1v >> 31) << 24);
            const uint32_t was = (o >> 6) & 0x01010101u, fresh = (o >> 4) & 0x01010101u;
            const uint32_t pmax = max(max(p[u].x, p[u].y), max(p[u].z, p[u].w));
            // a byte changes iff the cell was touched, was not occupied, and is fresh (50 -> 0 or 100),
            // hit now (-> 100) or at / over the pass threshold now (-> 100)
            if (((tb & ~was) & (fresh | fb)) != 0u || pmax >= pthr) {
                uint32_t occ = was | fb;
                occ |= (p[u].x >= pthr ? 1u : 0u) | (p[u].y >= pthr ? 0x100u : 0u) | (p[u].z >= pthr ? 0x10000u : 0u) | (p[u].w >= pthr ? 0x1000000u : 0u);
                const uint32_t tm = tb * 255u;
                const uint32_t out = (o & ~tm) | ((occ * 100u) & tm);
                if (out != o) *reinterpret_cast<uint32_t *>(pm + at[u]) = out;
            }
        }
    }
}

// Tail of a window workgroup: its visits are summed in LDS (*wg_visits, zeroed at the start) and go out as ONE global add.
__device__ __forceinline__ void finish_workgroup(const GridDev &g, unsigned long long *wg_visits, unsigned nvis, int tid)
{
    const unsigned tot = wave_sum_u32(nvis);
    if ((tid & 63) == 0 && tot) atomicAdd(wg_visits, (unsigned long long)tot);
    __syncthreads();
    if (tid == 0 && *wg_visits) atomicAdd(visit_slot(g.visits), *wg_visits);
}

// Shared-map form: groups of scans of a replay cast into a map that other workgroups write too.
// __launch_bounds__(1024, 8): eight waves per SIMD, i.e. TWO 1024-thread workgroups on a CU, are part of the contract.  Without
// the second figure the compiler used 93 scalar registers; a wave is given 16 more for the trap handler, 112 with the granule,
// and a SIMD's 800 then hold seven waves, 28 a CU: the second workgroup's 16 waves never fit, whatever the LDS request and
// whatever hipOccupancyMaxActiveBlocksPerMultiprocessor answered (stamps with the CU's id: one resident at a time).  With it
// the kernel stays at 78 (16 scalars live in lanes of a vector register; no scratch).
template <class Src>
__global__ void __launch_bounds__(1024, 8) k_grid_update_win(GridDev g, Src src, int group_size, const int32_t *__restrict__ got,
                                                          int sort_cap, int win_cells, int split, int lds_hits)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const WinLds lds(smem, group_size, sort_cap, win_cells);
    ScanConst *sc = lds.sc; WinCtl *ctl = lds.ctl; int *hist = lds.hist; unsigned *win = lds.win;
    lds_guard_fill(lds.guard);
    STAMP_DECL;

    const int tid = threadIdx.x;
    const int l = blockIdx.y;
    // split: TWO workgroups per group of scans (see the planner below), each with a window of its own
    const int my_half = split ? (int)(blockIdx.x & 1u) : -1;
    const int s0 = (int)(split ? blockIdx.x >> 1 : blockIdx.x) * group_size;
    const int cnt = min(group_size, src.scans_per_traj() - s0);
    const int gi = got ? got[l] : src.own_grid(l);
    uint32_t *pass = g.pass + (size_t)gi * g.xw * g.yw, *hit = g.hit + (size_t)gi * g.xw * g.yw;
    const int n = src.n, nrays = cnt * n;

    // rows of an even number of cells: two neighbouring counters are one aligned 8-byte word, and the two
    // 16-bit counts of a window dword are flushed by ONE 64-bit atomic (flush_window)
    const bool pair64 = (g.yw & 1) == 0 && (((size_t)gi * g.xw * g.yw) & 1) == 0;
    const int ymask = pair64 ? 1 : 0;
    if (tid < cnt) { src.scan_const(l, s0 + tid, g, sc[tid]); ctl->first_bad[tid] = INT_MAX; }
    if (tid == 0) {
        ctl->bbox[0] = ctl->bbox[1] = INT_MAX; ctl->bbox[2] = ctl->bbox[3] = INT_MIN; ctl->next_ray = 0; ctl->visits = 0ull;
        for (int q = 0; q < 4; ++q) { ctl->qbox[q][0] = ctl->qbox[q][1] = INT_MAX; ctl->qbox[q][2] = ctl->qbox[q][3] = INT_MIN; }
        ctl->phases = 1; ctl->parity = 0;
    }
    // Direction quadrants (DESIGN.md "K4a"): a ray never crosses the column or the row of its origin, so the rays of the four
    // direction quadrants (end cell right / left of, above / below the origin) touch four nearly disjoint parts of the group's
    // bounding box.  When the box of a workgroup's rays does not fit the window it is cut at the origins' column, and a half that
    // still does not fit at their row: every part gets the window to itself, one PHASE after the other; every ray is still walked
    // once, and none of its cells takes the checked walk with scattered global atomics.
    // A group of more than kMaxSortRays rays is neither sorted nor cut: one window, the rays in their own order.
    const bool sorted = nrays <= sort_cap;
    unsigned short *bins = reinterpret_cast<unsigned short *>(win);   // scratch until the window is zeroed
    for (int k = tid; k < 4 * kSortBins; k += blockDim.x) hist[k] = 0;
    __syncthreads();
    STAMP(0);                                   // scan constants

    // pass 1: which phase of which workgroup casts a ray is decided behind the barrier, when the boxes are known
    // (bits 7-8: quadrant, bit 9: beam parity); rays with nothing to cast are nobody's
    win_pass1(g, src, sc, l, s0, cnt, n, sorted, ctl->bbox, ctl->first_bad, [&](int r, int i, bool casts, int quad, int lbin) {
        bins[r] = casts ? (unsigned short)(lbin | (quad << 7) | ((i & 1) << 9)) : (unsigned short)0xffffu;
    });
    if (tid == 0) {
        // the quadrants' boxes, and the parts (sets of quadrants) this workgroup casts, one phase each: launch_shapes.h
        const int *bb = ctl->bbox;
        if (bb[0] <= bb[2]) {
            int ox0 = INT_MAX, oy0 = INT_MAX, ox1 = INT_MIN, oy1 = INT_MIN;
            for (int k = 0; k < cnt; ++k) { ox0 = min(ox0, sc[k].pcx); ox1 = max(ox1, sc[k].pcx); oy0 = min(oy0, sc[k].pcy); oy1 = max(oy1, sc[k].pcy); }
            quadrant_boxes(bb, ox0, oy0, ox1, oy1, ctl->qbox);
        }
        auto fits = [&](unsigned mask) -> bool { int o[4]; return !box_of(ctl->qbox, mask, g.xw, g.yw, ymask, o) || box_fits(o, win_cells); };
        unsigned part[4] = {0u, 0u, 0u, 0u};
        int nph = 1, parity = 0;
        pick_parts(split != 0, my_half, sorted, fits, part, nph, parity);
        for (int q = 0; q < 4; ++q) ctl->phq[q] = -1;
        for (int ph = 0; ph < nph; ++ph) {
            for (int q = 0; q < 4; ++q)
                if (part[ph] >> q & 1u) ctl->phq[q] = ph;
            int o[4];
            const bool any = box_of(ctl->qbox, part[ph], g.xw, g.yw, ymask, o);
            fit_window(g, any, o, ymask, sc[0], win_cells, ctl->phw[ph]);
        }
        ctl->phases = nph; ctl->parity = parity;
        if (!sorted) { ctl->seg[0] = 0; ctl->seg[1] = nrays; }       // (else: the counting sort's)
    }
    __syncthreads();
    STAMP(1);                                   // pass 1: endpoints, bounding boxes, phases
    const int phases = ctl->phases;
    if (sorted) {                                                    // this workgroup's rays and their phases
        const bool parity = ctl->parity != 0;
        for (int r = tid; r < nrays; r += blockDim.x) {
            const unsigned b = bins[r];
            if (b == 0xffffu) continue;
            const int ph = ctl->phq[(b >> 7) & 3u];
            const bool mine = ph >= 0 && (!parity || (int)((b >> 9) & 1u) == my_half);
            const unsigned fin = (unsigned)ph * kSortBins + (b & 127u);
            bins[r] = mine ? (unsigned short)fin : (unsigned short)0xffffu;
            if (mine) atomicAdd(&hist[fin], 1);
        }
        __syncthreads();
        counting_sort<8>(hist, bins, lds.order, nrays, ctl->seg);    // by (phase, length bin)
    }
    unsigned nvis = 0;
    int W = ctl->phw[0][2], H = ctl->phw[0][3];                      // (after the loop: of the last phase with rays, for the stamps)
    bool covers = ctl->phw[0][4] != 0;
    for (int ph = 0; ph < phases; ++ph) {
        const int seg0 = ctl->seg[ph], seg1 = ctl->seg[ph + 1];
        if (seg0 == seg1) continue;                                   // (uniform) a part without rays
        const int *o = ctl->phw[ph];
        const int wx0 = o[0], wy0 = o[1];
        W = o[2]; H = o[3]; covers = o[4] != 0;         // the window holds every in-map cell the phase's rays can touch
        const int Hp2 = (H + 1) >> 1;                   // dwords per window row
        __syncthreads();                                              // the previous phase's flush has read the window
        if (tid == 0) ctl->next_ray = 0;
        for (int w = tid; w < W * Hp2; w += blockDim.x) win[w] = 0u;
        __syncthreads();
        STAMP(2);                                   // sort + zero
        // pass 2: walk the rays (the reference's float-error Bresenham, bresenham.py:45-55)
        const unsigned short *ord = sorted ? lds.order + seg0 : nullptr;
        // sorted rays leave their hits in the order's dead slots; they are counted in the window behind the flush (flush_hits)
        unsigned short *park = sorted && lds_hits ? lds.order + seg0 : nullptr;
        if (covers) nvis += cast_rays<true>(g, src, sc, l, s0, n, seg1 - seg0, &ctl->next_ray, ord, win, wx0, wy0, W, H, Hp2, pass, hit, ctl->first_bad, park);
        else        nvis += cast_rays<false>(g, src, sc, l, s0, n, seg1 - seg0, &ctl->next_ray, ord, win, wx0, wy0, W, H, Hp2, pass, hit, ctl->first_bad, park);
        __syncthreads();
        STAMP(3);                                   // walk
        flush_window(win, pass, g.yw, wx0, wy0, W, Hp2, pair64, park != nullptr);
        if (park) flush_hits(win, park, seg1 - seg0, hit, g.yw, wx0, wy0, 2 * Hp2);
    }
    finish_workgroup(g, &ctl->visits, nvis, tid);
    STAMP(4);                                   // flush
    STAMP_VAL((ctl->parity << 8) | (covers ? 1 : 0) | (phases << 4) | ((unsigned)(W * ((H + 1) & ~1)) << 12));
    STAMP_END(5);                               // [5] lifetime, [6] workgroups
    lds_guard_check(lds.guard, g.status);
}

// Owner form: the workgroup is the only writer of its map, which has a live pmap, and the launch is not one for the single-scan
// owner kernels below (several scans in one group: context option "grid_group"; a scan of more than 1 024 beams; three hit levels;
// rows that are no multiple of 16 cells).  One window, then the workgroup finishes every cell its rays could touch, pmap included.
template <class Src>
__global__ void __launch_bounds__(1024) k_grid_update_own(GridDev g, Src src, int group_size, int sort_cap, int win_cells)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const WinLds lds(smem, group_size, sort_cap, win_cells);
    ScanConst *sc = lds.sc; WinCtl *ctl = lds.ctl; int *hist = lds.hist; unsigned *win = lds.win;
    lds_guard_fill(lds.guard);
    STAMP_DECL;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
    const int l = blockIdx.y;
    const int s0 = (int)blockIdx.x * group_size;
    const int cnt = min(group_size, src.scans_per_traj() - s0);
    const int gi = src.own_grid(l);
    uint32_t *pass = g.pass + (size_t)gi * g.xw * g.yw, *hit = g.hit + (size_t)gi * g.xw * g.yw;
    int8_t *pm = g.pmap_live + (size_t)gi * g.xw * g.yw;
    const int n = src.n, nrays = cnt * n;

    // rows that are a multiple of 4 cells: the sweep is a plain vectorised read-modify-write of the touched rectangle
    // that adds the window's counts itself, so there is no flush
    const bool fused = (g.yw & 3) == 0 && (((size_t)gi * g.xw * g.yw) & 3) == 0;
    const bool pair64 = (g.yw & 1) == 0 && (((size_t)gi * g.xw * g.yw) & 1) == 0;   // (see k_grid_update_win)
    const int ymask = fused ? 3 : pair64 ? 1 : 0;
    if (tid < cnt) { src.scan_const(l, s0 + tid, g, sc[tid]); ctl->first_bad[tid] = INT_MAX; }
    if (tid == 0) {
        ctl->bbox[0] = ctl->bbox[1] = INT_MAX; ctl->bbox[2] = ctl->bbox[3] = INT_MIN; ctl->next_ray = 0; ctl->visits = 0ull;
        ctl->strips = 0; ctl->strip_w = 0;
    }
    const bool sorted = nrays <= sort_cap;
    unsigned short *bins = reinterpret_cast<unsigned short *>(win);   // scratch until the window is zeroed
    for (int k = tid; k < kSortBins; k += blockDim.x) hist[k] = 0;
    __syncthreads();
    STAMP(0);                                   // scan constants

    win_pass1(g, src, sc, l, s0, cnt, n, sorted, ctl->bbox, ctl->first_bad, [&](int r, int, bool, int, int lbin) {
        bins[r] = (unsigned short)lbin;                              // parked in the (not yet zeroed) window
        atomicAdd(&hist[lbin], 1);
    });
    if (tid == 0) {
        int o[4] = {ctl->bbox[0], ctl->bbox[1], ctl->bbox[2], ctl->bbox[3]};
        int *w = ctl->phw[0];
        const bool any = clamp_box(g.xw, g.yw, o, 0);
        // Single-scan strip form (below): one scan, one hit occupies, and the window, widened to whole 64-byte pieces of the
        // counter rows (16 cells) and cut into S strips of at most Ws rows, holds every cell.
        if (any && fused && cnt == 1 && nrays < 32768 && g.hit_levels == 1 && (g.yw & 15) == 0) {
            const int ya = o[1] & ~15, Ha = ((o[3] | 15) + 1) - ya, Wb = o[2] - o[0] + 1;
            int S = (int)(((long)Wb * Ha + win_cells - 1) / win_cells), Ws = (Wb + S - 1) / S;
            while ((long)Ws * Ha > win_cells && S < Wb) { ++S; Ws = (Wb + S - 1) / S; }
            if ((long)Ws * Ha <= win_cells) { w[0] = o[0]; w[1] = ya; w[2] = Wb; w[3] = Ha; w[4] = 1; ctl->strips = S; ctl->strip_w = Ws; }
        }
        if (!ctl->strips) {
            o[1] &= ~ymask;
            fit_window(g, any, o, ymask, sc[0], win_cells, w);
        }
    }
    __syncthreads();
    STAMP(1);                                   // pass 1: endpoints, bounding box, window
    if (sorted) counting_sort<kSortBins / kWave>(hist, bins, lds.order, nrays, nullptr);   // by length bin
    const unsigned short *ord = sorted ? lds.order : nullptr;
    const int wx0 = ctl->phw[0][0], wy0 = ctl->phw[0][1], W = ctl->phw[0][2], H = ctl->phw[0][3];
    const bool covers = ctl->phw[0][4] != 0;
    const int Hp2 = (H + 1) >> 1;                                    // dwords per window row
    const int strips = ctl->strips, strip_w = ctl->strip_w;
    unsigned nvis = 0;
    if (strips) {
        // Single-scan strip form: no cell is updated by a global atomic and nothing an atomic wrote is read (as in owner_cast); a
        // box larger than the window is cut into strips of rows, each walked (cast_rays_strip) and swept (sweep_strip) in turn
        const uint32_t pthr = g.pass_thresh[0];
        const int qrow = H >> 2;                                      // H is a multiple of 16 here
        const unsigned qinv = (unsigned)((0x100000000ull + (unsigned)qrow - 1) / (unsigned)qrow);   // q / qrow == umulhi(q, qinv), q < 2^16
        for (int strip = 0; strip < strips; ++strip) {
            const int sx0 = wx0 + strip * strip_w, SW = min(strip_w, wx0 + W - sx0);
            if (strip) __syncthreads();                               // the previous strip's sweep has read the window
            for (int w = tid; w < SW * Hp2; w += blockDim.x) win[w] = 0u;
            if (tid == 0) ctl->next_ray = 0;
            __syncthreads();
            STAMP(2);                                   // (sort +) zero
            nvis += cast_rays_strip(g, src, sc[0], l, s0, nrays, &ctl->next_ray, ord, win, sx0, wy0, SW, H, Hp2, hit, ctl->first_bad[0]);
            __syncthreads();
            STAMP(3);                                   // walk
            sweep_strip(win, pass, pm, g.yw, sx0, wy0, SW, H, qrow, qinv, pthr);
            STAMP_SYNC();
            STAMP(4);                                   // sweep
        }
        STAMP_COUNT(7, strips);
    } else {
        for (int w = tid; w < W * Hp2; w += blockDim.x) win[w] = 0u;
        __syncthreads();
        STAMP(2);                                   // sort + zero
        // pass 2: walk the rays (the reference's float-error Bresenham, bresenham.py:45-55)
        if (covers) nvis += cast_rays<true>(g, src, sc, l, s0, n, nrays, &ctl->next_ray, ord, win, wx0, wy0, W, H, Hp2, pass, hit, ctl->first_bad);
        else        nvis += cast_rays<false>(g, src, sc, l, s0, n, nrays, &ctl->next_ray, ord, win, wx0, wy0, W, H, Hp2, pass, hit, ctl->first_bad);
        __syncthreads();
        STAMP(3);                                   // walk
        if (!fused) flush_window(win, pass, g.yw, wx0, wy0, W, Hp2, pair64);
        // Once its own atomics (hits, out-of-window passes, the flush) have landed, the workgroup finishes every cell its rays could
        // have touched - the box of pass 1, clamped to the map - in one sweep that re-thresholds pmap.  Plain loads are safe: the
        // counters were only touched by this workgroup's atomics (done, fenced) and nothing of this map is in this CU's L1.
        owner_fence();
        __syncthreads();
        const int x0 = max(ctl->bbox[0], 0), y0 = max(ctl->bbox[1], 0), x1 = min(ctl->bbox[2], g.xw - 1), y1 = min(ctl->bbox[3], g.yw - 1);
        const OccRule rule = OccRule::of(g);
        if (x0 <= x1 && y0 <= y1 && fused) {
            // the window's pass counts are added here, with plain 16-byte read-modify-writes
            const int ya = y0 & ~3, qrow = ((y1 | 3) + 1 - ya) >> 2, rows = x1 - x0 + 1;
            const int total = rows * qrow;
            // (pm is a char pointer and may alias anything for the compiler: the loads of a batch
            // are issued before its stores by hand)
            constexpr int kBatch = 4;                                     // 16-byte read-modify-writes a lane keeps in flight
            for (int q0 = tid; q0 < total; q0 += kBatch * blockDim.x) {
                uint4 p[kBatch], h[kBatch];
                size_t at[kBatch];
                bool add[kBatch];
#pragma unroll
                for (int u = 0; u < kBatch; ++u) {
                    int q = min(q0 + u * (int)blockDim.x, total - 1);
                    int r = q / qrow, c = q - r * qrow;
                    int x = x0 + r, y = ya + 4 * c;
                    at[u] = (size_t)x * g.yw + y;
                    p[u] = *reinterpret_cast<const uint4 *>(pass + at[u]);
                    h[u] = *reinterpret_cast<const uint4 *>(hit + at[u]);
                    unsigned wx = (unsigned)(x - wx0), wy = (unsigned)(y - wy0);   // wy is a multiple of 4 when inside
                    unsigned d0 = 0, d1 = 0;
                    if (wx < (unsigned)W && wy < (unsigned)H) {
                        unsigned di = wx * Hp2 + (wy >> 1);
                        d0 = win[di];
                        d1 = (wy >> 1) + 1 < (unsigned)Hp2 ? win[di + 1] : 0u;
                    }
                    add[u] = (d0 | d1) != 0;
                    p[u].x += d0 & 0xffffu; p[u].y += d0 >> 16;
                    p[u].z += d1 & 0xffffu; p[u].w += d1 >> 16;
                }
#pragma unroll
                for (int u = 0; u < kBatch; ++u) {
                    if (q0 + u * (int)blockDim.x >= total) continue;
                    if (add[u]) *reinterpret_cast<uint4 *>(pass + at[u]) = p[u];
                    uint32_t out = rule.value(p[u].x, h[u].x) | rule.value(p[u].y, h[u].y) << 8 |
                                   rule.value(p[u].z, h[u].z) << 16 | rule.value(p[u].w, h[u].w) << 24;
                    *reinterpret_cast<uint32_t *>(pm + at[u]) = out;
                }
            }
        } else if (x0 <= x1 && y0 <= y1) {
            for (int x = x0 + wave; x <= x1; x += nwaves) {
                size_t rowb = (size_t)x * g.yw;
                for (int y = y0 + lane; y <= y1; y += kWave) pm[rowb + y] = (int8_t)rule.value(pass[rowb + y], hit[rowb + y]);
            }
        }
    }
    finish_workgroup(g, &ctl->visits, nvis, tid);
    STAMP(4);                                   // flush / sweep
    STAMP_VAL((covers ? 1 : 0) | (1 << 4) | ((unsigned)(W * ((H + 1) & ~1)) << 12));
    STAMP_END(5);                               // [5] lifetime, [6] workgroups
    lds_guard_check(lds.guard, g.status);
}

// ---------------------------------------------------------------------------------
// Single-scan owner kernel (DESIGN.md "K4 owner"): ONE scan cast into a map that this workgroup
// owns for the whole launch - the per-particle maps of BASELINE.json configs[2], and
// Mapping.update of one scan - with the live pmap kept current.  No cell is updated by a global
// atomic and nothing an atomic wrote is read back:
//   * every ray's walk state lives in registers (up to kOwnerRays rays per lane, longest rays in
//     the lowest waves), so a bounding box larger than the LDS window is handled by cutting it
//     into strips of rows (x ranges) that are walked and swept in turn, in ascending x.  The
//     reference walks along +x (or +y for steep lines) after its endpoint swaps, so the map x of
//     a walk never decreases except for steep lines that step towards -x: every other ray resumes
//     in a strip where it left the previous one and is walked exactly ONCE; those (a quarter of
//     the rays, and only when there is more than one strip) restart from their first cell in
//     every strip, because a walk cannot be entered midway - its state is a rounded running sum
//     (bresenham.py:45-55: the same operations in the same order either way);
//   * the path's last cell is the endpoint cell itself (the path runs start -> end inclusive):
//     it takes the hit without being walked to - a fire-and-forget atomic on the hit counter,
//     which is never read, and bit 15 of its 16-bit window cell;
//   * the sweep of a strip reads the window, adds the pass counts into whole 64-byte pieces of the
//     counter rows (plain 16-byte loads / stores of touched pieces only) and re-thresholds pmap
//     from the window's flag bits, the new pass counts and the live pmap's previous value: with
//     one hit occupying (the reference's +20 > 10), pmap == 100 says "hit before or pass >=
//     threshold" and counters only grow, so an occupied cell stays occupied; otherwise hit == 0
//     and the new pass count decides (mapping.py:42-50).
// Rays that leave the map (mapping.py:41 drops their outside cells) are rare and take a plain
// bounds-checked walk per strip.
// ---------------------------------------------------------------------------------
// (kOwnerThreads, kOwnerMaxRays: launch_shapes.h)

struct OwnRay {
    int lx, h;            // current cell: map x, halfword index in the strip's window
    int k, kend, klast;   // next walk step, last walk step, walk step of the path's last cell (takes the hit instead)
    int dlx_k, dlx_y;     // map-x step per walk step / per y advance
    int dh_k, dh_y;       // window halfword step per walk step / per y advance
    int ly;               // map y of the current cell (kept current between strips only)
    double error, derr;
    __device__ __forceinline__ void start(const Ray &rr, int H)
    {
        const CellWalk w(rr);                                        // (its fields are kept here: the walk is suspended between strips)
        k = 0; kend = rr.dx; klast = w.klast;
        lx = w.lx; ly = w.ly;
        dlx_k = w.ax_x; dlx_y = w.ay_x;
        dh_k = w.stride_k(H); dh_y = w.stride_y(H);
        error = w.error; derr = w.derr;
        h = 0;
    }
};

// Control block of owner_cast, in the LDS region of the window kernels' (WinCtl)
struct OwnCtl {
    int bbox[4];                     // x0, y0, x1, y1 of everything the scan's rays can touch
    int win[4];                      // x0, y0, W, H of the rows and cells the strips cover
    int halves, split;               // cut at the origin's column `split` instead of into strips
    int strips, strip_w;
    alignas(8) unsigned long long visits;   // of the whole workgroup: ONE global add, at the very end
    int unsafe;                      // some ray leaves the map
    int first_bad;                   // the scan's first beam that Python's int() would raise on
};
static_assert(sizeof(OwnCtl) <= kWinBoxInts * 4, "the control block outgrew its LDS region");

template <class Src, int kOwnerRays>
__device__ __forceinline__ void owner_cast(const GridDev &g, const Src &src, int sort_cap, int win_cells, const int l)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    ScanConst *sc = reinterpret_cast<ScanConst *>(smem);
    OwnCtl *ctl = reinterpret_cast<OwnCtl *>(smem + win_sc_bytes(1));
    int *hist = reinterpret_cast<int *>(ctl) + kWinBoxInts;          // [2][kSortBins]: (direction half,) length bin
    unsigned short *order = reinterpret_cast<unsigned short *>(hist + 2 * kSortBins);
    unsigned *win = reinterpret_cast<unsigned *>(order + sort_cap);
    char *guard = reinterpret_cast<char *>(win) + (size_t)win_cells * 2;
    lds_guard_fill(guard);
    STAMP_DECL;

    const int tid = threadIdx.x, lane = tid & 63;
    const int gi = src.own_grid(l), n = src.n;
    uint32_t *pass = g.pass + (size_t)gi * g.xw * g.yw, *hit = g.hit + (size_t)gi * g.xw * g.yw;
    int8_t *pm = g.pmap_live + (size_t)gi * g.xw * g.yw;
    unsigned short *bins = reinterpret_cast<unsigned short *>(win);   // scratch until the window is first zeroed

    if (tid == 0) {
        src.scan_const(l, 0, g, sc[0]);
        ctl->bbox[0] = ctl->bbox[1] = INT_MAX; ctl->bbox[2] = ctl->bbox[3] = INT_MIN; ctl->visits = 0ull; ctl->unsafe = 0; ctl->first_bad = INT_MAX;
    }
    if (tid < 2 * kSortBins) hist[tid] = 0;
    __syncthreads();
    STAMP(0);
    const ScanConst c0 = sc[0];

    // pass 1: endpoints, bounding box, length histogram
    int bx0 = INT_MAX, by0 = INT_MAX, bx1 = INT_MIN, by1 = INT_MIN, bad = 0;
    for (int r = tid; r < n; r += blockDim.x) {
        int pox = 0, poy = 0, len = 0, b2 = 0;
        if (src.ray(l, 0, r, c0, g, pox, poy, b2)) {
            bx0 = min(bx0, min(pox, c0.pcx)); bx1 = max(bx1, max(pox, c0.pcx));
            by0 = min(by0, min(poy, c0.pcy)); by1 = max(by1, max(poy, c0.pcy));
            len = max(abs(pox - c0.pcx), abs(poy - c0.pcy));
        }
        // the scan stops at its first beam that Python's int() would raise on (mapping.py:29-36: the
        // beams before it have been applied when the exception leaves update(), and the error is that
        // beam's)
        if (b2) atomicMin(&ctl->first_bad, r);
        // longest first; rays that run towards larger x behind those that run towards smaller x (see `halves`)
        int bin = kSortBins - 1 - min(len >> 2, kSortBins - 1) + (pox >= c0.pcx ? kSortBins : 0);
        bins[r] = (unsigned short)bin;
        atomicAdd(&hist[bin], 1);
    }
    bx0 = wave_min_i32(bx0); by0 = wave_min_i32(by0); bx1 = wave_max_i32(bx1); by1 = wave_max_i32(by1);
    if (lane == 0 && bx0 <= bx1) {
        atomicMin(&ctl->bbox[0], bx0); atomicMin(&ctl->bbox[1], by0); atomicMax(&ctl->bbox[2], bx1); atomicMax(&ctl->bbox[3], by1);
    }
    __syncthreads();
    if (tid == 0) {
        if (ctl->first_bad != INT_MAX) {                             // the first bad beam's own error (NaN or overflow)
            int pox, poy, b2 = 0;
            (void)src.ray(l, 0, ctl->first_bad, c0, g, pox, poy, b2);
            atomicOr(g.status, b2);
        }
        // window = bounding box clamped to the map, rows widened to whole 16-cell pieces, cut into
        // S strips of at most Ws rows that each fit the window
        int x0 = max(ctl->bbox[0], 0), y0 = max(ctl->bbox[1], 0), x1 = min(ctl->bbox[2], g.xw - 1), y1 = min(ctl->bbox[3], g.yw - 1);
        int S = 0, Ws = 0, ya = 0, Ha = 0;
        if (x0 <= x1 && y0 <= y1) {
            ya = y0 & ~15; Ha = ((y1 | 15) + 1) - ya;
            const int Wb = x1 - x0 + 1;
            S = (int)(((long)Wb * Ha + win_cells - 1) / win_cells); Ws = (Wb + S - 1) / S;
            while ((long)Ws * Ha > win_cells) { ++S; Ws = (Wb + S - 1) / S; }   // (the host made sure one row fits: yw <= win_cells)
        }
        // Direction halves (as in k_grid_update_win): a box that needs two or more strips is cut at the origin's
        // column instead when both sides then fit - a ray never crosses that column, so each ray is walked once,
        // in the half it runs into, without a bounds test; strips walk some rays again and test every step.
        int halves = 0;
        const int split = min(max(c0.pcx, x0), x1);
        if (S >= 2 && (long)max(split - x0 + 1, x1 - split + 1) * Ha <= win_cells) { halves = 1; S = 2; }
        ctl->win[0] = x0; ctl->win[1] = ya; ctl->win[2] = x1 - x0 + 1; ctl->win[3] = Ha;
        ctl->strips = S; ctl->strip_w = Ws; ctl->halves = halves; ctl->split = split;
    }
    counting_sort<2 * kSortBins / kWave>(hist, bins, order, n, nullptr);   // by (half, length bin)
    STAMP(1);
    const int wx0 = ctl->win[0], wy0 = ctl->win[1], W = ctl->win[2], H = ctl->win[3], strips = ctl->strips, strip_w = ctl->strip_w;
    const bool halves = ctl->halves != 0;
    const int split = ctl->split;
    const int Hp2 = H >> 1;

    // this lane's rays: sorted rays tid, tid + blockDim, ...
    OwnRay ry[kOwnerRays];
    int pox[kOwnerRays], poy[kOwnerRays];
    // 0: nothing to walk; 1: all cells in the map, map x never decreases along the walk; 2: all cells in
    // the map, map x decreases (steep, towards -x): restarted in every strip; 3: leaves the map
    unsigned kind[kOwnerRays];
    unsigned nvis = 0;
    int unsafe = 0;
#pragma unroll
    for (int j = 0; j < kOwnerRays; ++j) {
        kind[j] = 0u; pox[j] = poy[j] = 0;
        Ray rr = Ray::none();
        ry[j].start(rr, H);                                          // kend = -1: never active
        const int sr = tid + j * (int)blockDim.x;
        if (sr >= n || strips == 0) continue;
        int b2 = 0;
        if ((int)order[sr] >= ctl->first_bad) continue;                    // at or after the first bad beam: not cast
        if (!src.ray(l, 0, (int)order[sr], c0, g, pox[j], poy[j], b2)) continue;
        if (!ray_setup(c0.pcx, c0.pcy, pox[j], poy[j], rr)) continue;          // identical cells: empty path (bresenham.py:10-11)
        const bool inmap = (unsigned)c0.pcx < (unsigned)g.xw && (unsigned)c0.pcy < (unsigned)g.yw &&
                           (unsigned)pox[j] < (unsigned)g.xw && (unsigned)poy[j] < (unsigned)g.yw;
        if (!inmap) { kind[j] = 3u; unsafe = 1; continue; }
        kind[j] = (rr.steep && rr.ystep < 0 && strips > 1 && !halves) ? 2u : 1u;
        nvis += (unsigned)rr.dx + 1u;                                // every cell of the path is in the map (mapping.py:41)
        ry[j].start(rr, H);
    }
    if (unsafe) ctl->unsafe = 1;
    __syncthreads();
    const bool any_unsafe = ctl->unsafe != 0;

    const uint32_t pthr = g.pass_thresh[0];
    const int qrow = H >> 2;                                         // quads per window row (H is a multiple of 16)
    const unsigned qinv = qrow ? (unsigned)((0x100000000ull + (unsigned)qrow - 1) / (unsigned)qrow) : 0u;   // q / qrow == umulhi(q, qinv)
    for (int strip = 0; strip < strips; ++strip) {
        const int sx0 = halves ? (strip ? split : wx0) : wx0 + strip * strip_w;
        const int SW = halves ? (strip ? wx0 + W - split : split - wx0 + 1) : min(strip_w, wx0 + W - sx0);
        if (strip) __syncthreads();                                  // the previous strip's sweep has read the window
        {
            uint4 *w4 = reinterpret_cast<uint4 *>(win);
            for (int w = tid; w < (SW * Hp2) >> 2; w += blockDim.x) w4[w] = make_uint4(0u, 0u, 0u, 0u);   // H % 16 == 0: whole uint4s
        }
        __syncthreads();
        STAMP(2);
        // hits: the path's last cell is the endpoint cell (mapping.py:44-45)
#pragma unroll
        for (int j = 0; j < kOwnerRays; ++j) {
            if (kind[j] == 0u) continue;
            if (halves && (pox[j] >= c0.pcx ? 1 : 0) != strip) continue;     // (the origin's column lies in both halves)
            const unsigned wx = (unsigned)(pox[j] - sx0), wy = (unsigned)(poy[j] - wy0);
            if (wx < (unsigned)SW && wy < (unsigned)H) {             // (the strips tile the bounding box clamped to the map)
                atomicOr(&win[wx * Hp2 + (wy >> 1)], 0x8000u << ((wy & 1u) * 16u));
                atomicAdd(&hit[(size_t)pox[j] * g.yw + poy[j]], 1u);
                if (kind[j] == 3u) ++nvis;
            }
        }
        // walk (bresenham.py:45-55)
        if (halves) {
            // every ray of this half, start to end, unchecked (see cast_rays): all its cells lie in the half's window
#pragma unroll
            for (int j = 0; j < kOwnerRays; ++j) {
                const OwnRay &o = ry[j];
                const bool mine = kind[j] == 1u && (pox[j] >= c0.pcx ? 1 : 0) == strip;
                if (!__any(mine)) continue;
                const unsigned a2 = lds_addr(win) + 2u * (unsigned)((o.lx - sx0) * H + (o.ly - wy0));
                double error = 0.0;
                // pass cells: all but the path's last; a reversed path's first walk step is the hit cell
                lds_walk(a2, 2 * o.dh_k, 2 * o.dh_y, mine ? o.kend : 0, o.derr, error, mine && o.klast == 0);
            }
        } else
#pragma unroll
        for (int j = 0; j < kOwnerRays; ++j) {
            OwnRay &o = ry[j];
            const bool desc = kind[j] == 2u;
            if (desc) {                                              // restarts from its first cell (which lies to the right)
                Ray rr;
                ray_setup(c0.pcx, c0.pcy, pox[j], poy[j], rr);
                o.start(rr, H);
            }
            // the window halfword of the current cell, relative to this strip
            o.h = (o.lx - sx0) * H + (o.ly - wy0);
            // ascending: walks until it leaves the strip to the right; descending: until it has left it to the left
            const int lo = desc ? sx0 : INT_MIN, hi = desc ? INT_MAX : sx0 + SW;
            for (;;) {
                bool moved = false;
#pragma unroll
                for (int u = 0; u < 4; ++u) {                        // (four steps per wave-wide check; branch-free conditions)
                    const bool act = (o.k <= o.kend) & (o.lx >= lo) & (o.lx < hi);
                    moved |= act;
                    if (act) {
                        const bool cnt = ((unsigned)(o.lx - sx0) < (unsigned)SW) & (o.k != o.klast);
                        if (cnt) atomicAdd(&win[o.h >> 1], 1u << ((o.h & 1) * 16));   // mapping.py:43
                        const bool stepy = walk_step(o.error, o.derr);
                        o.h += o.dh_k + (stepy ? o.dh_y : 0);
                        o.lx += o.dlx_k + (stepy ? o.dlx_y : 0);
                        ++o.k;
                    }
                }
                if (!__any(moved)) break;
            }
            o.ly = wy0 + (o.h - (o.lx - sx0) * H);                   // map y of the cell the ray stands on now
        }
        if (any_unsafe) {
            // rays with cells outside the map: plain walk of the whole ray, counting this strip's cells
#pragma unroll
            for (int j = 0; j < kOwnerRays; ++j) {
                if (kind[j] != 3u) continue;
                if (halves && (pox[j] >= c0.pcx ? 1 : 0) != strip) continue;   // (walked once, in the half they run into)
                Ray rr;
                ray_setup(c0.pcx, c0.pcy, pox[j], poy[j], rr);
                const int klast = rr.flag ? 0 : rr.dx;
                double error = 0.0;
                int y = rr.y0;
                for (int k = 0; k <= rr.dx; ++k) {
                    const int x = rr.x0 + k;
                    const unsigned wx = (unsigned)((rr.steep ? y : x) - sx0), wy = (unsigned)((rr.steep ? x : y) - wy0);
                    if (k != klast && wx < (unsigned)SW && wy < (unsigned)H) {
                        ++nvis;
                        atomicAdd(&win[wx * Hp2 + (wy >> 1)], 1u << ((wy & 1u) * 16u));
                    }
                    if (walk_step(error, rr.derr)) y += rr.ystep;
                }
            }
        }
        __syncthreads();
        STAMP(3);
        sweep_strip(win, pass, pm, g.yw, sx0, wy0, SW, H, qrow, qinv, pthr);
        STAMP_SYNC();
        STAMP(4);
    }
    unsigned tot = wave_sum_u32(nvis);
    int anybad = bad;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) anybad |= __shfl_xor(anybad, off, kWave);
    if (lane == 0) {
        if (tot) atomicAdd(&ctl->visits, (unsigned long long)tot);
        if (anybad) atomicOr(g.status, anybad);
    }
    __syncthreads();
    if (tid == 0 && ctl->visits) atomicAdd(visit_slot(g.visits), ctl->visits);
    STAMP_COUNT(7, strips);
    STAMP_END(5);
    lds_guard_check(guard, g.status);
}

// The general owner kernel has two launch forms: one workgroup per map (blockIdx.y), or - behind the
// byte-window kernel below - a fixed number of workgroups that work off the list of maps that kernel
// left for it (redo[0]: count, redo[1]: workgroups done, redo[2..]: map numbers; normally empty).
template <class Src, int kOwnerRays>
__global__ void __launch_bounds__(kOwnerThreads, kOwnerRays == 1 ? 2 * kOwnerThreads / 256 : kOwnerThreads / 256)
k_grid_update_owner(GridDev g, Src src, int sort_cap, int win_cells)
{
    owner_cast<Src, kOwnerRays>(g, src, sort_cap, win_cells, (int)blockIdx.y);
}

template <class Src, int kOwnerRays>
__global__ void __launch_bounds__(kOwnerThreads) k_grid_update_owner_redo(GridDev g, Src src, int sort_cap, int win_cells, int32_t *redo)
{
    const int count = redo[0];
    for (int it = blockIdx.x; it < count; it += gridDim.x) {
        owner_cast<Src, kOwnerRays>(g, src, sort_cap, win_cells, redo[2 + it]);
        __syncthreads();                                             // the next map re-uses the LDS regions
    }
    // every workgroup has read the count before it reports here: the last one empties the list for the next launch
    if (threadIdx.x == 0 && atomicAdd(&redo[1], 1) == (int)gridDim.x - 1) { redo[0] = 0; redo[1] = 0; }
}

// ---------------------------------------------------------------------------------
// Single-scan owner kernel with a BYTE window (DESIGN.md "K4 owner8"): the plain case of the kernel above -
// every beam valid, every ray inside the map, at most one ray per lane - with 8-bit window cells, so that the
// whole bounding box of a scan (236 x 212 cells for the 10 m x 8 m benchmark room at 0.05 m) is ONE window of
// ~50 KB and three workgroups share a CU.  One phase per map: no strips, no direction halves, every ray walked
// once without bounds tests, one sweep.
//   * a window byte = 7-bit pass count + bit 7 "a hit fell here".  The scan's origin cell is the first cell of
//     every path and would count all n rays: it is left out of the walk and its count (the number of non-empty
//     rays) is added by the sweep.  Any other cell sees only the rays whose direction lies within a cell's width
//     of it: 54 of 360 next to the origin on the benchmark scan.
//   * nothing bounds a byte for arbitrary input (n identical rays), and a count of 128 would spill into the flag
//     and the neighbouring cell.  So the walk is CHECKED before anything is written to the map: the sum of all
//     window bytes (flags masked) must equal the number of cells the rays passed, which the set-up knows
//     (sum of dx - 1).  Every overflow event lowers the masked byte sum (by 128, 127 or 126 ...) and nothing
//     raises it, so equality proves that no byte overflowed.  On a mismatch - and for every case this kernel
//     does not handle: a bad beam, a ray leaving the map, a box larger than the window - the map's number goes
//     on the re-do list and the general kernel above casts it; this kernel has then written nothing to it.
//   * set-up with two barriers: the beam loads are in flight while LDS is initialised; the counting sort by
//     length (longest rays in the lowest waves) takes the rank inside a bin from the histogram atomic's return
//     value and the bin's offset from a wave-level scan that every wave does for itself; the sorted end cells
//     travel through LDS as packed 16-bit pairs instead of being loaded and computed a second time.
//   * the sweep goes by window rows: a wave takes a row (64 quads of it at a time), so the map addresses are a
//     scalar row offset plus a per-lane constant, and reads / writes the counters and pmap with non-temporal buffer
//     loads and stores whose per-lane offset lies beyond the buffer for lanes with nothing to do: BATCH rows per
//     wave in flight, no branches, no lane masks.  Counters and pmap rule exactly as in the kernel above
//     (mapping.py:42-50); the pmap arithmetic runs only for quads where something can change.
//   * what bounds it (tools/ubench_rmw.hip, profiles/r03_ubench_rmw.txt): the chip moves this traffic - 64-byte
//     pieces read and written back in place, scattered over 14 GB of maps - at 3.8 TB/s with the default cache
//     policy and 4.75 TB/s non-temporal; a plain streaming copy reaches 4.5 TB/s (reads alone 6.3, writes alone 4.4).
// ---------------------------------------------------------------------------------
// (kOwn8Bins, kOwn8BoxInts, kOwn8Threads, kOwn8LdsBytes - half a CU's LDS - and own8_fixed_bytes: launch_shapes.h)
constexpr int kOwn8MaxLen = 2048;
constexpr int kOwn8Batch = 8;           // window rows a wave keeps in flight in the sweep (4: 15 % slower, 12: 10 % slower; 512 threads: equal)
// cache policy of the sweep's counter and pmap traffic (buffer aux bits: 1 sc0, 2 nt, 16 sc1): every byte is read and
// written once per launch, and non-temporal loads AND stores run the in-place read-modify-write 24 % faster than the
// default policy (tools/ubench_rmw.hip: 4.75 against 3.83 TB/s on this access pattern; nt on the stores alone: no gain)
constexpr int kOwn8Aux = 2;
constexpr int kOwn8PerCU = 163840 / kOwn8LdsBytes;      // workgroups per CU the register budget is set for

typedef unsigned short u16x2_t __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
constexpr int kBufferRsrcWord3 = 0x00020000;     // raw buffer, 32-bit data format (gfx9 / CDNA)
__device__ __forceinline__ unsigned pk_min_u16(unsigned a, unsigned b)
{
    return __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_bit_cast(u16x2_t, a), __builtin_bit_cast(u16x2_t, b)));
}
__device__ __forceinline__ unsigned pk_max_u16(unsigned a, unsigned b)
{
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(u16x2_t, a), __builtin_bit_cast(u16x2_t, b)));
}
__device__ __forceinline__ void lds_or_u32(unsigned addr, unsigned v)
{
    (void)__hip_atomic_fetch_or((lds_u32_t *)(uintptr_t)addr, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// New value of a quad's four pmap bytes (mapping.py:47-50) from their old value and what the scan did to the cells (one bit
// per byte - 7: touched, 6: hit, 5: pass count at or over the threshold now): a touched cell shows 100 if it was occupied
// (bit 6 is set in 100 only, not in 0 or 50), is hit now or is over the threshold, else 0; an untouched cell keeps its byte.
__device__ __forceinline__ uint32_t own8_pmap_bytes(uint32_t o, uint32_t e)
{
    const uint32_t tb = (e >> 7) & 0x01010101u;
    const uint32_t occ = ((o >> 6) | (e >> 6) | (e >> 5)) & 0x01010101u;
    const uint32_t tm = tb * 255u;
    return (o & ~tm) | ((occ * 100u) & tm);
}

template <class Src, int THREADS, int BATCH>
__global__ void __launch_bounds__(THREADS, (kOwn8PerCU * THREADS + 255) / 256) k_grid_update_owner8(GridDev g, Src src, int win_bytes, int32_t *__restrict__ redo)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int *box = reinterpret_cast<int *>(smem);                        // [0..3] bounding box, [4] odd case seen, [5] cells the rays pass, [6] window byte sum
    int *hist = box + kOwn8BoxInts;                                  // [kOwn8Bins] rays per length bin
    unsigned *slots = reinterpret_cast<unsigned *>(hist + kOwn8Bins);   // [THREADS] end cells in sorted order
    unsigned *win = slots + THREADS;                                 // [W][Hs] bytes
    char *guard = reinterpret_cast<char *>(win) + win_bytes;
    lds_guard_fill(guard);
    STAMP_DECL;

    const int tid = threadIdx.x, lane = tid & 63;
    const int l = blockIdx.y, gi = src.own_grid(l), n = src.n;
    auto give_up = [&]() {                                           // (uniform) leave the map to the general kernel
        if (tid == 0) redo[2 + atomicAdd(&redo[0], 1)] = l;
    };

    // this lane's beam: loads first, LDS set-up while they are in flight
    typename Src::Beam beam = src.fetch(l, 0, tid < n ? tid : 0);
    ScanConst c0;
    src.scan_const(l, 0, g, c0);
    if (tid < kOwn8BoxInts) box[tid] = tid < 2 ? INT_MAX : (tid < 4 ? INT_MIN : 0);
    if (tid < kOwn8Bins) hist[tid] = 0;
    {
        uint4 *w4 = reinterpret_cast<uint4 *>(win);
        for (int w = tid; w < (win_bytes >> 4); w += THREADS) w4[w] = make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();
    STAMP(0);

    // pass 1: end cell, length bin, bounding box (mapping.py:30-36)
    int pox = 0, poy = 0, b2 = 0;
    const bool ok = tid < n && src.ray(beam, c0, g, pox, poy, b2);
    const bool inmap = (unsigned)c0.pcx < (unsigned)g.xw && (unsigned)c0.pcy < (unsigned)g.yw &&
                       (unsigned)pox < (unsigned)g.xw && (unsigned)poy < (unsigned)g.yw;
    // int() would raise / the ray leaves the map / a ray longer than the lengths for which "the float walk ends
    // in the cell of its other end" has been checked exhaustively (dx <= 2100: tests/test_walk_ends.py)
    const int len = max(abs(pox - c0.pcx), abs(poy - c0.pcy));
    const bool odd = (tid < n && b2 != 0) || (ok && (!inmap || len > kOwn8MaxLen));
    const bool valid = ok && inmap && len > 0 && len <= kOwn8MaxLen;   // identical cells: empty path (bresenham.py:10-11)
    int bin = 0, idx = 0;
    if (valid) {
        bin = kOwn8Bins - 1 - min(len >> 2, kOwn8Bins - 1);          // longest first
        idx = atomicAdd(&hist[bin], 1);
    }
    const unsigned pk = (unsigned)pox | ((unsigned)poy << 16);       // (both < 65 536 when valid)
    {
        unsigned lo = valid ? pk : 0xffffffffu, hi = valid ? pk : 0u;
        int cells = valid ? len - 1 : 0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            lo = pk_min_u16(lo, (unsigned)__shfl_xor((int)lo, off, kWave));
            hi = pk_max_u16(hi, (unsigned)__shfl_xor((int)hi, off, kWave));
            cells += __shfl_xor(cells, off, kWave);
        }
        const unsigned long long anyv = __ballot(valid), anyodd = __ballot(odd);
        if (lane == 0) {
            if (anyv) {
                atomicMin(&box[0], (int)(lo & 0xffffu)); atomicMin(&box[1], (int)(lo >> 16));
                atomicMax(&box[2], (int)(hi & 0xffffu)); atomicMax(&box[3], (int)(hi >> 16));
                atomicAdd(&box[5], cells);
            }
            if (anyodd) box[4] = 1;
        }
    }
    __syncthreads();
    STAMP(1);
    if (box[4]) { give_up(); return; }
    // counting sort: every wave scans the histogram for itself (two bins per lane)
    const int h0 = hist[2 * lane], h1 = hist[2 * lane + 1];
    int inc = h0 + h1;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) { const int v = __shfl_up(inc, off, kWave); if (lane >= off) inc += v; }
    const int nv = __shfl(inc, kWave - 1, kWave);                    // non-empty rays
    if (nv == 0) return;                                             // nothing to cast (mapping.py:38-39: empty paths)
    const int x0 = min(box[0], c0.pcx), y0 = min(box[1], c0.pcy), x1 = max(box[2], c0.pcx), y1 = max(box[3], c0.pcy);
    // window rows of whole 64-byte pieces of the counter rows (16 cells = 4 quads = 4 lanes of the sweep): a piece
    // the scan touched is read and written back whole - runs that start or end inside a piece cost the memory
    // system 11 % of its rate for this traffic (tools/ubench_rmw.hip: 4.29 against 4.84 TB/s)
    const int y4 = y0 & ~15, Hs = ((y1 | 15) + 1) - y4, W = x1 - x0 + 1;
    if ((long)W * Hs > (long)win_bytes) { give_up(); return; }
    {
        const int excl = inc - (h0 + h1);
        int base = __shfl(excl, bin >> 1, kWave);
        const int first = __shfl(h0, bin >> 1, kWave);
        if (bin & 1) base += first;
        if (valid) slots[base + idx] = pk;
    }
    __syncthreads();
    STAMP(2);

    // this lane's ray: the tid-th longest
    const bool have = tid < nv;
    const unsigned e = have ? slots[tid] : 0u;
    const int ex = (int)(e & 0xffffu), ey = (int)(e >> 16);
    Ray rr = Ray::none();
    if (have) (void)ray_setup(c0.pcx, c0.pcy, ex, ey, rr);
    const unsigned wbase = lds_addr(win);
    if (have) {                                                      // the path's last cell is the end cell: the hit (mapping.py:44-45)
        const unsigned b = (unsigned)((ex - x0) * Hs + (ey - y4));
        lds_or_u32(wbase + (b & ~3u), 0x80u << ((b & 3u) * 8u));
    }
    {
        // the walk (bresenham.py:45-55) without its two end steps: walk step 0 is the origin cell (or, for a
        // reversed path, the hit cell) and step dx the hit cell (or the origin): dx - 1 cells in between
        CellWalk w(rr);
        const unsigned a = wbase + (unsigned)((w.lx - x0) * Hs + (w.ly - y4));   // byte counters
        lds_walk(a, w.stride_k(Hs), w.stride_y(Hs), have ? rr.dx - 1 : 0, w.derr, w.error, have);
    }
    __syncthreads();
    STAMP(3);

    // From here on a wave works on whole window rows (map x = x0 + r), 64 quads of a row at a time (a quad: 4 cells,
    // one window dword, 16 bytes of counters, 4 of pmap): row and segment are wave-uniform, so the window index and the
    // map addresses are a scalar base plus a per-lane constant and cost no vector instruction.
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int NW = THREADS / kWave;
    const int qrow = Hs >> 2, nseg = (qrow + kWave - 1) >> 6;

    // the check: masked byte sum of the window == cells the rays passed
    {
        unsigned acc = 0u;
        for (int seg = 0; seg < nseg; ++seg) {
            const int c = seg * kWave + lane;
            if (c < qrow)
                for (int r = wv; r < W; r += NW) acc = __builtin_amdgcn_sad_u8(win[r * qrow + c] & 0x7f7f7f7fu, 0u, acc);
        }
        acc = wave_sum_u32(acc);
        if (lane == 0 && acc) atomicAdd(&box[6], (int)acc);
    }
    __syncthreads();
    if (box[6] != box[5]) { give_up(); return; }

    uint32_t *pass = g.pass + (size_t)gi * g.xw * g.yw, *hit = g.hit + (size_t)gi * g.xw * g.yw;
    int8_t *pm = g.pmap_live + (size_t)gi * g.xw * g.yw;
    if (tid == 0) atomicAdd(visit_slot(g.visits), (unsigned long long)(box[5] + 2 * nv));   // every cell of every path is in the map (:41)

    // sweep.  Counters and pmap go through buffer loads / stores: the map's row is the scalar offset, the lane's quad
    // the vector offset, and a lane with nothing to do gets an offset beyond the buffer - the hardware then neither
    // reads nor writes for it - so a batch of rows is straight-line code without branches or lane masks.
    const uint32_t pthr = g.pass_thresh[0];
    const int org_r = c0.pcx - x0, org_q = (c0.pcy - y4) >> 2;       // the origin cell's row, quad ...
    const unsigned org_b = (unsigned)(c0.pcy - y4) & 3u;             // ... and byte in the quad
    const __amdgpu_buffer_rsrc_t rs_pass = __builtin_amdgcn_make_buffer_rsrc(pass, 0, g.xw * g.yw * 4, kBufferRsrcWord3);
    const __amdgpu_buffer_rsrc_t rs_pm = __builtin_amdgcn_make_buffer_rsrc(pm, 0, g.xw * g.yw, kBufferRsrcWord3);
    constexpr unsigned kSkip = 0x80000000u;                          // (beyond any map: xw * yw * 4 < 2^31, checked by the launcher)
    for (int seg = 0; seg < nseg; ++seg) {
        const int c = seg * kWave + lane;
        const bool incol = c < qrow;
        const bool org_lane = c == org_q;
        for (int r0 = wv; r0 < W; r0 += NW * BATCH) {
            u32x4_t p[BATCH];
            uint32_t om[BATCH], dd[BATCH], vo[BATCH], vp[BATCH], ev[BATCH];
            auto rowoff_of = [&](int u) -> uint32_t {                // (wave-uniform) first cell of the segment in map row x0 + r
                const int rc = min(r0 + u * NW, W - 1);
                return (uint32_t)((x0 + rc) * g.yw + y4 + seg * 4 * kWave);
            };
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                const int r = r0 + u * NW;                           // (wave-uniform)
                const int rc = min(r, W - 1);
                dd[u] = (incol && r < W) ? win[rc * qrow + c] : 0u;
                // the four lanes of a piece decide together (rows start on a piece, 64 lanes are 16 pieces)
                const unsigned long long m = __ballot(dd[u] != 0u || (r == org_r && org_lane));
                const bool live = ((m >> (lane & 60)) & 0xFull) != 0ull && incol;
                vo[u] = live ? (unsigned)lane << 4 : kSkip;         // byte offset of the lane's quad in the counter row
                p[u] = __builtin_amdgcn_raw_buffer_load_b128(rs_pass, vo[u], rowoff_of(u) << 2, kOwn8Aux);
            }
            // pmap (mapping.py:47-50).  A touched cell shows 0 or 100 afterwards; its byte CHANGES only if the cell was never
            // touched before (then its old pass count is 0), or is hit now and was not occupied, or its pass count is at or
            // over the threshold now.  The old bytes are read where they can matter.  Up front: quads a hit fell in.  The
            // other two cases are known once the counters are here and are rare once a map has seen a scan or two: those
            // quads read pmap late (below).  The up-front reads are issued BEHIND the batch's counter loads: a wave's loads
            // return in order, and a lone lane's pmap line coming from memory between two rows' counters held every later
            // row of the batch back.  (Per 10 000 maps: pmap read for every live quad, as until round 3, 0.671 ms and
            // 3.20 GB; for the quads that need it, each between its row's counters and the next row's, 0.722 ms; behind the
            // counter loads 0.640 ms and 2.94 GB; listed in LDS and settled after the sweep in one round 0.718 ms - that
            // round trip is paid at the end of every workgroup's life, with nothing left to overlap it.)
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                vp[u] = (vo[u] != kSkip && (dd[u] & 0x80808080u) != 0u) ? (unsigned)lane << 2 : kSkip;
                om[u] = __builtin_amdgcn_raw_buffer_load_b32(rs_pm, vp[u], rowoff_of(u), kOwn8Aux);
            }
            bool late_any = false;
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                const int r = r0 + u * NW;
                const uint32_t d = dd[u], dm = d & 0x7f7f7f7fu;
                u32x4_t q = p[u];
                // one bit per cell (bit 7 of its byte): its pass count was 0 before this scan
                const uint32_t z7 = (q.x == 0u ? 0x80u : 0u) | (q.y == 0u ? 0x8000u : 0u) | (q.z == 0u ? 0x800000u : 0u) | (q.w == 0u ? 0x80000000u : 0u);
                q.x += dm & 0xffu; q.y += (dm >> 8) & 0xffu; q.z += (dm >> 16) & 0xffu; q.w += dm >> 24;   // mapping.py:43
                // one bit per cell (bit 7 of its byte): passed or hit by this scan
                uint32_t t7 = ((dm + 0x7f7f7f7fu) | d) & 0x80808080u;
                if (r == org_r) {                                    // (wave-uniform) every non-empty path starts in the origin cell
                    if (org_lane) {
                        q.x += org_b == 0u ? (uint32_t)nv : 0u; q.y += org_b == 1u ? (uint32_t)nv : 0u;
                        q.z += org_b == 2u ? (uint32_t)nv : 0u; q.w += org_b == 3u ? (uint32_t)nv : 0u;
                        t7 |= 0x80u << (8u * org_b);
                    }
                }
                __builtin_amdgcn_raw_buffer_store_b128(q, rs_pass, vo[u], rowoff_of(u) << 2, kOwn8Aux);
                // what the scan did to the quad's cells, one bit per byte - 7: touched, 6: hit, 5: count at or over the threshold
                const uint32_t ge5 = (q.x >= pthr ? 0x20u : 0u) | (q.y >= pthr ? 0x2000u : 0u) | (q.z >= pthr ? 0x200000u : 0u) | (q.w >= pthr ? 0x20000000u : 0u);
                ev[u] = t7 | ((d >> 1) & 0x40404040u) | ge5;
                if (vp[u] == kSkip && vo[u] != kSkip && ((t7 & z7) != 0u || (ge5 & (t7 >> 2)) != 0u)) {
                    vp[u] = ((unsigned)lane << 2) | 1u;              // (bit 0: read late)
                    late_any = true;
                }
            }
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {                        // the quads read up front
                if (vp[u] == kSkip || (vp[u] & 1u)) continue;
                const uint32_t out = own8_pmap_bytes(om[u], ev[u]);
                if (out != om[u]) __builtin_amdgcn_raw_buffer_store_b32(out, rs_pm, vp[u], rowoff_of(u), kOwn8Aux);
            }
            if (__any(late_any)) {
#pragma unroll
                for (int u = 0; u < BATCH; ++u)
                    om[u] = __builtin_amdgcn_raw_buffer_load_b32(rs_pm, (vp[u] != kSkip && (vp[u] & 1u)) ? vp[u] & ~3u : kSkip, rowoff_of(u), kOwn8Aux);
#pragma unroll
                for (int u = 0; u < BATCH; ++u) {
                    if (vp[u] == kSkip || !(vp[u] & 1u)) continue;
                    const uint32_t out = own8_pmap_bytes(om[u], ev[u]);
                    if (out != om[u]) __builtin_amdgcn_raw_buffer_store_b32(out, rs_pm, vp[u] & ~3u, rowoff_of(u), kOwn8Aux);
                }
            }
        }
    }
    // the hits last (mapping.py:45): fire-and-forget atomics, which the sweep's loads would otherwise queue behind
    if (have) atomicAdd(&hit[(size_t)ex * g.yw + ey], 1u);
    STAMP_SYNC();
    STAMP(4);
    STAMP_END(5);
    lds_guard_check(guard, g.status);
}

// CUs and LDS bytes per CU of the current device (cached per device): the launch shapes below count workgroups against them
struct ChipShape { int cus; long lds_per_cu; };
static ChipShape chip_shape()
{
    static std::mutex mu;
    static std::vector<std::pair<int, ChipShape>> seen;
    int dev = 0;
    ChipShape c{kChipCus, (long)kLdsPerCu};                          // MI355X, should a query fail
    if (hipGetDevice(&dev) != hipSuccess) return c;
    std::lock_guard<std::mutex> lock(mu);
    for (const auto &e : seen)
        if (e.first == dev) return e.second;
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) c.cus = v;
    // (gfx950 reports 160 KiB here; a workgroup may ask for all of it)
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) == hipSuccess && v > 0) c.lds_per_cu = v;
    (void)hipGetLastError();
    seen.push_back({dev, c});
    return c;
}

// SLAM_WIN_RESIDENCY=1 in the environment: what the runtime says about how many workgroups of a k_grid_update_win launch a CU
// holds, to stderr, for every such launch while the switch is set (the figures of DESIGN.md "K4a" round 6 come from here)
static void report_win_residency(const void *kernel, int threads, size_t lds, int win_cells, long wgs)
{
    const char *on = getenv("SLAM_WIN_RESIDENCY");
    if (!on || !*on || *on == '0') return;
    int per_cu = -1;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, lds);
    if (e != hipSuccess) (void)hipGetLastError();
    fprintf(stderr, "k_grid_update_win: %d threads, %zu bytes of LDS (window %d cells), %ld workgroups: %d resident per CU%s\n",
            threads, lds, win_cells, wgs, per_cu, e == hipSuccess ? "" : " (the query failed)");
}

template <class Src>
static hipError_t launch_win(const GridDev &g, const Src &src, int L, int scans, int n, int group, const int32_t *got,
                             hipStream_t s, int split_pref = -1, int hits_pref = -1)
{
    // the shape is plan_win's (launch_shapes.h); here: the attributes it asks for, and the kernel of its form
    const ChipShape chip = chip_shape();
    WinRequest req{L, scans, n, group, got != nullptr, g.pmap_live != 0, src.maps_are_private(), g.hit_levels, g.xw, g.yw,
                   g.redo != nullptr, split_pref, hits_pref, chip.cus, chip.lds_per_cu, kLdsGuard};
    const WinShape p = plan_win(req);
    const bool owner = p.form != kWinFormWin && p.form != kWinFormOwn;
    const void *const standing[] = {reinterpret_cast<const void *>(&k_grid_update_win<Src>), reinterpret_cast<const void *>(&k_grid_update_own<Src>),
                                    reinterpret_cast<const void *>(&k_grid_update_owner<Src, 1>), reinterpret_cast<const void *>(&k_grid_update_owner<Src, 2>),
                                    reinterpret_cast<const void *>(&k_grid_update_owner_redo<Src, 1>)};
    for (int k = 0; k < (owner ? 5 : 2); ++k) {
        hipError_t e = allow_dynamic_lds(standing[k], (int)win_lds_max());
        if (e != hipSuccess) return e;
    }
    if (p.live_dirty && g.live_dirty) *g.live_dirty = true;
    if (p.lds_attr) {
        hipError_t e = allow_dynamic_lds(standing[p.form == kWinFormOwn ? 1 : 0], (int)p.lds_attr);
        if (e != hipSuccess) return e;
    }
    const dim3 grid(p.grid_x, p.grid_y), block(p.threads);
    switch (p.form) {
    case kWinFormOwner8ThenRedo:
        SLAM_LAUNCH((k_grid_update_owner8<Src, kOwn8Threads, kOwn8Batch>), grid, dim3(kOwn8Threads), p.own8_lds, s, g, src, p.own8_win, g.redo);
        SLAM_LAUNCH((k_grid_update_owner_redo<Src, 1>), dim3(p.redo_grid), block, p.lds, s, g, src, p.sort_cap, p.win_cells, g.redo);
        break;
    case kWinFormOwner1: SLAM_LAUNCH((k_grid_update_owner<Src, 1>), grid, block, p.lds, s, g, src, p.sort_cap, p.win_cells); break;
    case kWinFormOwner2: SLAM_LAUNCH((k_grid_update_owner<Src, 2>), grid, block, p.lds, s, g, src, p.sort_cap, p.win_cells); break;
    case kWinFormOwn: SLAM_LAUNCH((k_grid_update_own<Src>), grid, block, p.lds, s, g, src, group, p.sort_cap, p.win_cells); break;
    default:
        report_win_residency(standing[0], p.threads, p.lds, p.win_cells, p.wgs);
        SLAM_LAUNCH((k_grid_update_win<Src>), grid, block, p.lds, s, g, src, group, got, p.sort_cap, p.win_cells, p.split, p.lds_hits);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------
// Tiled ray casting for maps far larger than one LDS window (DESIGN.md "K4 tiles"; the
// 2000x2000 @ 0.02 m map of BASELINE.json configs[4], where a scan's rays cover ~800 k cells
// and the window kernel fell back to scattered global atomics for most of them).
//
// The float-error Bresenham walk (bresenham.py:45-55) cannot be entered in the middle: its
// state is a rounded running sum.  So every ray is walked ONCE (k_ray_bits), touching no map
// cell, and the walk is recorded as one bit per step - "y advanced after this step" - plus a
// running count of set bits per 32-step word.  With those, the cell of step k is
// (x0 + k, y0 + ystep * popcount(bits[0..k))) for any k, so a second kernel (k_tile_cast) can
// give every (map tile, scan group) pair its own workgroup: it enters each ray where it
// crosses the tile, accumulates the tile's pass counts in LDS exactly like the window kernel,
// and flushes the non-zero cells row by row.  The cells visited are the reference's by
// construction (same walk, recorded instead of applied).  Hits (one per ray) and the visit
// counter are handled by the first kernel; rays of 2048 steps or more take the direct path
// there.
// ---------------------------------------------------------------------------------
constexpr int kTileSteps = 2048;                 // rays with dx < kTileSteps are recorded
constexpr int kTileWords = kTileSteps / 32;
constexpr int kTileSide = 192;        // 192 x 192 16-bit cells = the 72 KiB window

struct RayRec {
    int x0, y0, dx, yend;                        // walk coordinates; yend = y of the cell at step dx
    uint32_t flags;                              // 1: steep, 2: reversed (path runs end -> start), 4: ystep > 0, 8: valid
    int pad[3];
};

struct TileScratch {
    RayRec *recs;                                // [rays]
    uint32_t *bits;                              // [rays][kTileWords]
    unsigned short *prefix;                      // [rays][kTileWords]: set bits before each word
    int *gbox;                                   // [groups][4]: map-space bounding box of a group's recorded rays
};

__global__ void __launch_bounds__(256) k_tile_init(int *gbox, int groups)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < groups) { gbox[4 * i] = gbox[4 * i + 1] = INT_MAX; gbox[4 * i + 2] = gbox[4 * i + 3] = INT_MIN; }
}

// Pass A: block (scan, stream) walks the scan's rays once.
template <class Src>
__global__ void __launch_bounds__(256) k_ray_bits(GridDev g, Src src, TileScratch ts, int group_size)
{
    __shared__ ScanConst sc;
    __shared__ int box[4];
    const int s = blockIdx.x, l = blockIdx.y, n = src.n;
    const int scans = src.scans_per_traj();
    const int groups_per_traj = (scans + group_size - 1) / group_size;
    const int group = l * groups_per_traj + s / group_size;
    uint32_t *pass = g.pass, *hit = g.hit;       // single shared map (the launcher guarantees it)
    __shared__ int first_bad;
    if (threadIdx.x == 0) {
        src.scan_const(l, s, g, sc);
        box[0] = box[1] = INT_MAX; box[2] = box[3] = INT_MIN;
        first_bad = INT_MAX;
    }
    __syncthreads();
    // the scan stops at its first beam that Python's int() would raise on (mapping.py:29-36: the beams before it have been
    // applied when the exception leaves update(), and the error is that beam's): find it before anything is recorded or cast
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        int pox, poy, b2 = 0;
        (void)src.ray(l, s, i, sc, g, pox, poy, b2);
        if (b2) atomicMin(&first_bad, i);
    }
    __syncthreads();
    const int stop = first_bad;
    unsigned nvis = 0;
    int bad = 0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const size_t rid = ((size_t)l * scans + s) * n + i;
        RayRec rec;
        rec.flags = 0; rec.x0 = rec.y0 = rec.dx = rec.yend = 0; rec.pad[0] = rec.pad[1] = rec.pad[2] = 0;
        int pox, poy, b2 = 0;
        Ray ry;
        const bool valid = i <= stop && src.ray(l, s, i, sc, g, pox, poy, b2) && ray_setup(sc.pcx, sc.pcy, pox, poy, ry);
        // the common ray: recorded, and both ends (hence every cell) inside the map.  Only the walk's
        // decisions are needed - one bit per step - so the loop is the error recurrence alone
        // (bresenham.py:51-55), all lanes at the same step; the path's last cell is the endpoint cell
        // itself and takes its hit without being walked to (mapping.py:44-45).
        const bool plain = valid && ry.dx < kTileSteps && (unsigned)sc.pcx < (unsigned)g.xw && (unsigned)sc.pcy < (unsigned)g.yw &&
                           (unsigned)pox < (unsigned)g.xw && (unsigned)poy < (unsigned)g.yw;
        {
            uint32_t *bw = ts.bits + rid * kTileWords;
            unsigned short *pw = ts.prefix + rid * kTileWords;
            const int dx = plain ? ry.dx : -1;
            const double derr = plain ? ry.derr : 0.0;
            double error = 0.0;
            uint32_t count = 0, before_last = 0;
            for (int k0 = 0; __any(k0 <= dx); k0 += 32) {
                if (k0 <= dx) {
                    uint32_t word = 0;
                    const int nb = min(32, dx - k0 + 1);
                    // (whole words: the steps past the ray's end are computed and masked off - nothing reads
                    // the recurrence after them - so there is no lane mask per step)
#pragma unroll 8
                    for (int b = 0; b < 32; ++b) {
                        word |= walk_step(error, derr) ? (1u << b) : 0u;
                    }
                    if (nb < 32) word &= (1u << nb) - 1u;
                    pw[k0 >> 5] = (unsigned short)count;
                    bw[k0 >> 5] = word;
                    if (k0 + 32 > dx) before_last = count + __popc(word & ((1u << (dx - k0)) - 1u));   // y advances before step dx
                    count += __popc(word);
                }
            }
            if (plain) {
                nvis += (unsigned)ry.dx + 1u;                         // mapping.py:41: every cell is in the map
                atomicAdd(&hit[(size_t)pox * g.yw + poy], 1u);
                rec.yend = ry.y0 + ry.ystep * (int)before_last;
                rec.x0 = ry.x0; rec.y0 = ry.y0; rec.dx = ry.dx;
                rec.flags = 8u | (ry.steep ? 1u : 0u) | (ry.flag ? 2u : 0u) | (ry.ystep > 0 ? 4u : 0u);
                int a0 = ry.x0, a1 = ry.x0 + ry.dx, b0 = min(ry.y0, rec.yend), b1 = max(ry.y0, rec.yend);
                int mx0 = ry.steep ? b0 : a0, mx1 = ry.steep ? b1 : a1, my0 = ry.steep ? a0 : b0, my1 = ry.steep ? a1 : b1;
                atomicMin(&box[0], mx0); atomicMin(&box[1], my0); atomicMax(&box[2], mx1); atomicMax(&box[3], my1);
            }
        }
        if (valid && !plain) {                                       // leaves the map, or too long to record: the step-by-step form
            const bool record = ry.dx < kTileSteps;
            uint32_t *bw = ts.bits + rid * kTileWords;
            unsigned short *pw = ts.prefix + rid * kTileWords;
            // (x0 + k, y and walk_step, not CellWalk: with it the compiler allots this kernel 4 more VGPRs)
            const int klast = ry.flag ? 0 : ry.dx;
            double error = 0.0;
            int y = ry.y0, hx = -1, hy = -1;
            uint32_t word = 0, count = 0;
            for (int k = 0; k <= ry.dx; ++k) {
                if (record && (k & 31) == 0) pw[k >> 5] = (unsigned short)count;
                int x = ry.x0 + k;
                int lx = ry.steep ? y : x, ly = ry.steep ? x : y;
                bool inmap = (unsigned)lx < (unsigned)g.xw && (unsigned)ly < (unsigned)g.yw;
                nvis += inmap ? 1u : 0u;
                if (k == klast) { hx = lx; hy = ly; }
                else if (!record && inmap) atomicAdd(&pass[(size_t)lx * g.yw + ly], 1u);
                if (k == ry.dx) rec.yend = y;
                if (walk_step(error, ry.derr)) { y += ry.ystep; word |= 1u << (k & 31); ++count; }
                if (record && ((k & 31) == 31 || k == ry.dx)) { bw[k >> 5] = word; word = 0; }
            }
            if ((unsigned)hx < (unsigned)g.xw && (unsigned)hy < (unsigned)g.yw) atomicAdd(&hit[(size_t)hx * g.yw + hy], 1u);
            if (record) {
                rec.x0 = ry.x0; rec.y0 = ry.y0; rec.dx = ry.dx;
                rec.flags = 8u | (ry.steep ? 1u : 0u) | (ry.flag ? 2u : 0u) | (ry.ystep > 0 ? 4u : 0u);
                int a0 = ry.x0, a1 = ry.x0 + ry.dx, b0 = min(ry.y0, rec.yend), b1 = max(ry.y0, rec.yend);
                int mx0 = ry.steep ? b0 : a0, mx1 = ry.steep ? b1 : a1, my0 = ry.steep ? a0 : b0, my1 = ry.steep ? a1 : b1;
                atomicMin(&box[0], mx0); atomicMin(&box[1], my0); atomicMax(&box[2], mx1); atomicMax(&box[3], my1);
            }
        }
        bad |= b2;
        ts.recs[rid] = rec;
    }
    __syncthreads();
    if (threadIdx.x == 0 && box[0] <= box[2]) {
        atomicMin(&ts.gbox[4 * group], box[0]); atomicMin(&ts.gbox[4 * group + 1], box[1]);
        atomicMax(&ts.gbox[4 * group + 2], box[2]); atomicMax(&ts.gbox[4 * group + 3], box[3]);
    }
    unsigned tot = wave_sum_u32(nvis);
    int anybad = bad;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) anybad |= __shfl_xor(anybad, off, kWave);
    if ((threadIdx.x & 63) == 0) {
        if (tot) atomicAdd(visit_slot(g.visits), (unsigned long long)tot);
        if (anybad) atomicOr(g.status, anybad);
    }
}

// Pass B: workgroup (tile, group): the pass counts of one map tile from one group of scans.
__global__ void __launch_bounds__(1024) k_tile_cast(GridDev g, TileScratch ts, int tiles_x, int rays_per_group, long total_rays)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned *win = reinterpret_cast<unsigned *>(smem);
    __shared__ int next_ray;
    const int tile = blockIdx.x, group = blockIdx.y;
    const int tx0 = (tile % tiles_x) * kTileSide, ty0 = (tile / tiles_x) * kTileSide;
    const int W = min(kTileSide, g.xw - tx0), H = min(kTileSide, g.yw - ty0);
    const int tx1 = tx0 + W - 1, ty1 = ty0 + H - 1;
    const int *gb = ts.gbox + 4 * group;
    if (gb[0] > tx1 || gb[2] < tx0 || gb[1] > ty1 || gb[3] < ty0) return;   // nothing of this group comes near the tile
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
    const int Hp2 = (H + 1) >> 1;
    const int Hs = Hp2 | 1;                      // odd row stride: rows start in different LDS banks
    char *guard = smem + (size_t)kTileSide * ((kTileSide / 2) | 1) * 4;
    lds_guard_fill(guard);
    for (int w = tid; w < W * Hs; w += blockDim.x) win[w] = 0u;
    if (tid == 0) next_ray = 0;
    __syncthreads();
    const long rbase = (long)group * rays_per_group;
    const int nrays = (int)min((long)rays_per_group, total_rays - rbase);
    uint32_t *pass = g.pass;
    for (;;) {
        int base = 0;
        if (lane == 0) base = atomicAdd(&next_ray, kWave);
        base = __builtin_amdgcn_readfirstlane(base);
        if (base >= nrays) break;
        if (base + lane >= nrays) continue;
        const size_t rid = (size_t)(rbase + base + lane);
        const RayRec rec = ts.recs[rid];
        if (!(rec.flags & 8u)) continue;
        const bool steep = rec.flags & 1u;
        const int ystep = (rec.flags & 4u) ? 1 : -1;
        const int klast = (rec.flags & 2u) ? 0 : rec.dx;
        // tile range along the walk axis (a) and the other axis (b), in walk coordinates
        const int a0 = steep ? ty0 : tx0, a1 = steep ? ty1 : tx1, b0 = steep ? tx0 : ty0, b1 = steep ? tx1 : ty1;
        const int k0 = max(0, a0 - rec.x0), k1 = min(rec.dx, a1 - rec.x0);
        if (k0 > k1 || min(rec.y0, rec.yend) > b1 || max(rec.y0, rec.yend) < b0) continue;
        const uint32_t *bw = ts.bits + rid * kTileWords;
        int w = k0 >> 5;
        uint32_t word = bw[w];
        int y = rec.y0 + ystep * ((int)ts.prefix[rid * kTileWords + w] + __popc(word & ((1u << (k0 & 31)) - 1u)));
        word >>= (k0 & 31);
        // The cell of walk step k as the LDS byte address of its 16-bit counter, advanced incrementally (while
        // the ray is outside the tile's rows the address is virtual: it is only used inside them).  The path's
        // last cell takes the hit and no pass count (mapping.py:44-45): it is the ray's first or last step and is
        // trimmed off the range here.
        const int HW = 2 * Hs;                                       // 16-bit counters per window row
        const int da_k = 2 * (steep ? 1 : HW), da_y = 2 * (steep ? ystep * HW : ystep);
        unsigned a2 = lds_addr(win) + 2u * (unsigned)(steep ? (y - b0) * HW + (rec.x0 + k0 - a0) : (rec.x0 + k0 - a0) * HW + (y - b0));
        int k = k0, kk1 = k1 - (klast == k1 ? 1 : 0);
        if (klast == k0) {                                           // (klast == 0 == k0: the word holds bit 0 still)
            const unsigned bit = word & 1u;
            y += bit ? ystep : 0;
            a2 += (unsigned)(da_k + (bit ? da_y : 0));
            word >>= 1;
            ++k;
            if ((k & 31) == 0 && k <= kk1) word = bw[++w];           // (only for a one-bit first word: dx >= 1, so never; kept for safety)
        }
        bool gone = false;
        while (k <= kk1 && !gone) {
            const int kend = min(kk1, (w << 5) + 31);
            const uint32_t next = (w + 1) * 32 <= k1 ? bw[w + 1] : 0u;   // in flight while this word is walked
            const int nb = kend - k + 1;
            const uint32_t bits = nb == 32 ? word : (word & ((1u << nb) - 1u));
            const int pc = __popc(bits);
            const int yafter = y + ystep * pc;                       // y of the step after this word's last
            if (ystep > 0 ? yafter < b0 : yafter > b1) {             // the whole word stays short of the tile's rows
                y = yafter; k = kend + 1; a2 += (unsigned)(nb * da_k + pc * da_y); word = next; ++w;
                continue;
            }
            // every step of the word inside the rows (y is monotone: both ends inside): no checks, four steps
            // per wave-wide test
            const int ylast = yafter - ((bits >> (nb - 1)) & 1u ? ystep : 0);   // y AT the word's last step
            const bool inside = y >= b0 && y <= b1 && ylast >= b0 && ylast <= b1;
            if (__any(inside)) {
                int rem = inside ? nb : 0;
                auto step = [&]() {
                    lds_add_u32(a2 & ~3u, 1u << ((a2 << 3) & 31u));
                    a2 += (unsigned)(da_k + ((word & 1u) ? da_y : 0));
                    word >>= 1;
                };
                for (;;) {
                    const bool full = rem >= 4;
                    if (!__any(full)) break;
                    if (full) { step(); step(); step(); step(); rem -= 4; }
                }
#pragma unroll
                for (int u = 0; u < 3; ++u)
                    if (rem > u) step();
                if (inside) { y = yafter; k = kend + 1; word = next; ++w; }
            }
            if (!inside) {                                           // the word in which the ray enters or leaves the rows
                for (; k <= kend; ++k) {
                    if (ystep > 0 ? y > b1 : y < b0) { gone = true; break; }   // left the tile for good
                    if (y >= b0 && y <= b1) lds_add_u32(a2 & ~3u, 1u << ((a2 << 3) & 31u));
                    const unsigned bit = word & 1u;
                    y += bit ? ystep : 0;
                    a2 += (unsigned)(da_k + (bit ? da_y : 0));
                    word >>= 1;
                }
                word = next;
                ++w;
            }
        }
    }
    __syncthreads();
    const int rot = (int)((blockIdx.x * 37u + blockIdx.y * 11u) % (unsigned)W);
    for (int rr = wave; rr < W; rr += nwaves) {
        const int row = rr + rot < W ? rr + rot : rr + rot - W;
        size_t gbase = (size_t)(tx0 + row) * g.yw + ty0;
        // pairs of counters are aligned 8-byte words (see the window kernel).  gbase counts from g.pass itself: the tiles are
        // never given a map offset (plan_cast sends grid_of_traj to the wedges or the window), so its parity is the address's.
        // A cast into map gi would have to test (gi * xw * yw + gbase) & 1, as k_wedge_cast does.
        if ((gbase & 1) == 0) {
            for (int d = lane; d < Hp2; d += kWave) {
                unsigned v = win[row * Hs + d];
                if (v) atomicAdd(reinterpret_cast<unsigned long long *>(&pass[gbase + 2 * d]),
                                 (unsigned long long)(v & 0xffffu) | ((unsigned long long)(v >> 16) << 32));
            }
            continue;
        }
        for (int d = lane; d < Hp2; d += kWave) {
            unsigned v = win[row * Hs + d];
            unsigned p0 = v & 0xffffu, p1 = v >> 16;
            if (p0) atomicAdd(&pass[gbase + 2 * d], p0);
            if (p1) atomicAdd(&pass[gbase + 2 * d + 1], p1);
        }
    }
    lds_guard_check(guard, g.status);
}

// the pieces of a tile cast, bound to the members of `ts`
static Layout tile_pieces(TileScratch &ts, long rays, long groups)
{
    return Layout().add(ts.recs, rays).add(ts.bits, (size_t)rays * kTileWords).add(ts.prefix, (size_t)rays * kTileWords).add(ts.gbox, (size_t)groups * 4);
}

// The casts for large maps take at most kMaxLaunchGroups groups of scans in one launch (k_tile_cast: a row of gridDim.y per
// group; k_wedge_cast: a unit number of 20 bits, group x class).  A larger cast goes as successive launches on the same
// stream, over whole trajectories, or over scan ranges where one trajectory alone has more groups (ranges of whole groups
// of G scans).  The counters are integer sums and the visit counter one more, so the split gives the maps of one launch
// bit for bit; `one(src, L, scans, got)` is the launcher of a piece, whose scratch the next piece reuses in stream order.
constexpr int kMaxLaunchGroups = 65535;

template <class Src, class One>
static hipError_t launch_in_chunks(const Src &src, int L, int scans, int G, const int32_t *got, One &&one)
{
    if (src.maps_are_private()) return hipErrorInvalidValue;        // (the maps travel in `got` here)
    const int groups_per_traj = (scans + G - 1) / G;
    if (groups_per_traj <= kMaxLaunchGroups) {
        const int per = kMaxLaunchGroups / groups_per_traj;
        for (int l0 = 0; l0 < L; l0 += per) {
            hipError_t e = one(src.trajectories_from(l0), std::min(per, L - l0), scans, got ? got + l0 : nullptr);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    const int span = kMaxLaunchGroups * G;
    for (int l = 0; l < L; ++l)
        for (int k0 = 0; k0 < scans; k0 += span) {
            const int cnt = std::min(span, scans - k0);
            hipError_t e = one(src.trajectories_from(l).scans_from(k0, cnt), 1, cnt, got ? got + l : nullptr);
            if (e != hipSuccess) return e;
        }
    return hipSuccess;
}

template <class Src>
static hipError_t launch_tiles(const GridDev &g, const Src &src, int L, int scans, int n, int group, void *scratch, size_t cap, hipStream_t s)
{
    if (scans < 1) return hipSuccess;
    // scans per (tile, group) workgroup: 16 by default (1080 beams, 2000 x 2000 cells, three overlapping replays:
    // 8 -> 0.79, 12 -> 0.85, 16 -> 0.86, 24 -> 0.88, 32 -> 0.83 M scans/s; alone 16 equals 8 and 32 is 14 % slower)
    int G = group > 0 ? group : 16;
    G = std::min(G, std::max(1, 65535 / n));
    G = std::min(G, scans);
    if ((long)G * n > 65535) return hipErrorInvalidValue;   // (the tile counters and a group's ray numbers are 16-bit)
    if (L > 1)                                    // a group is a contiguous range of ray ids: it must not straddle streams
        while (scans % G != 0) --G;
    const int groups_per_traj = (scans + G - 1) / G;
    const long groups = (long)L * groups_per_traj, rays = (long)L * scans * n;
    if (groups > kMaxLaunchGroups)
        return launch_in_chunks(src, L, scans, G, nullptr, [&](const Src &cs, int cl, int cscans, const int32_t *) {
            return launch_tiles(g, cs, cl, cscans, n, G, scratch, cap, s);
        });
    TileScratch ts;
    if (!tile_pieces(ts, rays, groups).place(scratch, cap)) return hipErrorInvalidValue;
    if (g.pmap_live && g.live_dirty) *g.live_dirty = true;
    // the family is three launches: bracket it with recorded events when timing is armed
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    const bool timed = launch_events(&ev0, &ev1);
    if (timed) (void)hipEventRecord(ev0, s);
    hipLaunchKernelGGL(k_tile_init, dim3((groups + 255) / 256), dim3(256), 0, s, ts.gbox, (int)groups);
    hipLaunchKernelGGL((k_ray_bits<Src>), dim3(scans, L), dim3(256), 0, s, g, src, ts, G);
    const int tiles_x = (g.xw + kTileSide - 1) / kTileSide, tiles_y = (g.yw + kTileSide - 1) / kTileSide;
    size_t lds = (size_t)kTileSide * ((kTileSide / 2) | 1) * 4 + kLdsGuard;
    {
        hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(&k_tile_cast), (int)lds);
        if (e != hipSuccess) return e;
    }
    // 1024 lanes: the kernel is bound by the latency of its loads and LDS atomics (measured 2.35 ms
    // with 512, 2.14 ms with 1024 on the 1080-beam / 2000x2000 replay; tiles of 128 or 224 cells are slower)
    hipLaunchKernelGGL(k_tile_cast, dim3(tiles_x * tiles_y, (unsigned)groups), dim3(1024), lds, s, g, ts, tiles_x, G * n, rays);
    if (timed) (void)hipEventRecord(ev1, s);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------
// Wedge ray casting for maps far larger than one LDS window (DESIGN.md "K4 wedges"): the rays of a group of
// scans are dealt to workgroups by DIRECTION - steep or not, pointing up or down the walk axis, slope class - so
// that a workgroup's rays fan out from (nearly) one origin inside a narrow wedge, and the wedge is swept in BANDS
// along the walk axis: zero the window, walk every ray through the band, flush, next band.  A ray's walk
// (bresenham.py:45-55) always ascends along its walk axis after the reference's endpoint swaps, which is the
// band axis of its own steepness class: every ray is walked exactly ONCE, start to end, its state (step, y, float
// error) resting in registers between bands - nothing is recorded, nothing re-entered.
// The window of a band is a PARALLELOGRAM: rows follow the wedge with an integer shear M in {-1, 0, 1} per step
// of the walk axis (the slope class's nearest integer), so the LDS index stays LINEAR in the cell,
//     index = (a - a_lo) * ca + (y - M a - v_lo) * cv          (a: walk axis, y: the other axis)
// and the unchecked walk of cast_rays applies unchanged with strides (ca - M cv) per step and (+-cv) per y step.
// A band takes as many rows as its parallelogram leaves room for (the wedge's width at the band's far end plus the
// drift |slope - M| <= 1/2 per row).  k_wedge_sort prepares the group: end cells, direction class and a counting
// sort by (class, length) so that lanes hold the longest rays of their class first; hits, the visit counter and
// the odd rays (leaving the map, bad beams) are its business, as they were k_ray_bits'.
// ---------------------------------------------------------------------------------
constexpr int kWedgeSlopes = 4;                       // slope classes per (steepness, direction): equal parts of [-1, 1] (8: 10 % slower)
constexpr int kWedgeClasses = 4 * kWedgeSlopes;       // x (steep?) x (walk runs away from / towards the origin)
constexpr int kWedgeLenBins = 64;
constexpr int kWedgeThreads = 512;
constexpr int kWedgeSlots = 4;                        // rays per lane and pass
constexpr int kWedgeCells = 37888;                    // 16-bit window cells (74 KiB): two workgroups per CU
constexpr int kWedgePartMin = kWedgeThreads * kWedgeSlots;   // rays per part of a unit (the scratch is sized for it)

struct WedgeScratch {
    uint32_t *ends;            // [rays] end cell, x | y << 16
    uint32_t *orgs;            // [scans] origin cell
    unsigned short *list;      // [rays] ray numbers inside their group, sorted by (class, length descending)
    int *offs;                 // [groups][kWedgeClasses + 1] class boundaries in the group's list
    uint32_t *cost;            // [groups][kWedgeClasses] cells the class's rays pass (from the length bins: to +-8 cells a ray)
    uint32_t *order;           // [1 + groups * kWedgeClasses + rays / kWedgePartMin] parts listed, then the parts (unit | part << 20), the most cells first
    const int32_t *got;        // nullable [L]: map of trajectory l (null: every trajectory casts into map 0)
};

__device__ __forceinline__ int wedge_class(const Ray &r, int ddx, int ddy)
{
    // minor over major displacement in [-1, 1], as the walk sees it (after the swaps the walk ascends along its axis)
    const int maj = r.steep ? ddy : ddx, mnr = r.steep ? ddx : ddy;
    const int q = min(kWedgeSlopes - 1, (int)(((long)(mnr * (maj < 0 ? -1 : 1) + abs(maj)) * kWedgeSlopes) / (2L * abs(maj))));
    return ((r.steep ? 2 : 0) + (r.flag ? 1 : 0)) * kWedgeSlopes + q;
}
__host__ __device__ inline int wedge_shear(int cls)      // nearest integer of the class's slopes
{
    const int q = cls % kWedgeSlopes;                     // slopes [-1 + 2 q / Q, -1 + 2 (q + 1) / Q): middle (2 q + 1 - Q) / Q
    const int mid2 = 2 * (2 * q + 1 - kWedgeSlopes);      // twice the middle, times Q
    return mid2 >= kWedgeSlopes ? 1 : (mid2 <= -kWedgeSlopes ? -1 : 0);
}

template <class Src>
__global__ void __launch_bounds__(1024) k_wedge_sort(GridDev g, Src src, WedgeScratch ws, int group_size)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    ScanConst *sc = reinterpret_cast<ScanConst *>(smem);                                   // [group_size]
    int *hist = reinterpret_cast<int *>(smem + win_sc_bytes(group_size));                  // [kWedgeClasses * kWedgeLenBins]
    int *wsum = hist + kWedgeClasses * kWedgeLenBins;                                       // [64] cross-wave scan (16 used); before it: every scan's first bad beam
    unsigned short *keys = reinterpret_cast<unsigned short *>(wsum + kWinMaxGroup);         // [group_size * n]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l = blockIdx.y, n = src.n, scans = src.scans_per_traj();
    const int groups_per_traj = (scans + group_size - 1) / group_size;
    const int s0 = blockIdx.x * group_size, cnt = min(group_size, scans - s0);
    const long group = (long)l * groups_per_traj + blockIdx.x;
    const long ray0 = ((long)l * scans + s0) * n;                     // first ray of the group in ends[]
    const size_t map_off = (size_t)(ws.got ? ws.got[l] : 0) * g.xw * g.yw;   // the trajectory's map (one shared map without `got`)
    uint32_t *pass = g.pass + map_off, *hit = g.hit + map_off;
    if (tid < cnt) {
        src.scan_const(l, s0 + tid, g, sc[tid]);
        ws.orgs[(long)l * scans + s0 + tid] = (uint32_t)(sc[tid].pcx & 0xffff) | ((uint32_t)(sc[tid].pcy & 0xffff) << 16);
    }
    for (int k = tid; k < kWedgeClasses * kWedgeLenBins; k += blockDim.x) hist[k] = 0;
    int *fb = wsum;                                                  // [cnt <= 64 ints, ahead of the scan that uses wsum] every scan's first bad beam
    if (tid < kWinMaxGroup) fb[tid] = INT_MAX;
    __syncthreads();
    const int nrays = cnt * n;
    // every scan stops at its first beam that Python's int() would raise on (mapping.py:29-36: the beams before it have been
    // applied when the exception leaves update(), and the error is that beam's): find it before any hit or count is added
    for (int r = tid; r < nrays; r += blockDim.x) {
        const int s = r / n, i = r - s * n;
        int pox, poy, b2 = 0;
        (void)src.ray(l, s0 + s, i, sc[s], g, pox, poy, b2);
        if (b2) atomicMin(&fb[s], i);
    }
    __syncthreads();
    unsigned nvis = 0;
    int bad = 0;
    for (int r = tid; r < nrays; r += blockDim.x) {
        const int s = r / n, i = r - s * n;
        int pox, poy, b2 = 0;
        Ray ry;
        const bool valid = i <= fb[s] && src.ray(l, s0 + s, i, sc[s], g, pox, poy, b2) && ray_setup(sc[s].pcx, sc[s].pcy, pox, poy, ry);
        const bool plain = valid && (unsigned)sc[s].pcx < (unsigned)g.xw && (unsigned)sc[s].pcy < (unsigned)g.yw &&
                           (unsigned)pox < (unsigned)g.xw && (unsigned)poy < (unsigned)g.yw;
        unsigned short key = 0xffffu;
        if (plain) {                                                 // every cell in the map: the path's last cell takes the hit (mapping.py:44-45)
            nvis += (unsigned)ry.dx + 1u;
            atomicAdd(&hit[(size_t)pox * g.yw + poy], 1u);
            ws.ends[ray0 + r] = (uint32_t)pox | ((uint32_t)poy << 16);
            const int cls = wedge_class(ry, pox - sc[s].pcx, poy - sc[s].pcy);
            key = (unsigned short)(cls * kWedgeLenBins + (kWedgeLenBins - 1 - min(ry.dx >> 4, kWedgeLenBins - 1)));   // longest first
            atomicAdd(&hist[key], 1);
        } else if (valid) {                                          // leaves the map: the step-by-step form with direct atomics
            const int klast = ry.flag ? 0 : ry.dx;
            double error = 0.0;
            int y = ry.y0, hx = -1, hy = -1;
            for (int k = 0; k <= ry.dx; ++k) {
                const int x = ry.x0 + k;
                const int lx = ry.steep ? y : x, ly = ry.steep ? x : y;
                const bool inmap = (unsigned)lx < (unsigned)g.xw && (unsigned)ly < (unsigned)g.yw;
                nvis += inmap ? 1u : 0u;
                if (k == klast) { hx = lx; hy = ly; }
                else if (inmap) atomicAdd(&pass[(size_t)lx * g.yw + ly], 1u);
                if (walk_step(error, ry.derr)) y += ry.ystep;
            }
            if ((unsigned)hx < (unsigned)g.xw && (unsigned)hy < (unsigned)g.yw) atomicAdd(&hit[(size_t)hx * g.yw + hy], 1u);
        }
        keys[r] = key;
        bad |= b2;
    }
    __syncthreads();
    // exclusive scan of the bins: kBinsPerThread consecutive bins per thread (1 024 threads), wave scans, then the waves' totals
    {
        constexpr int kBinsPerThread = kWedgeClasses * kWedgeLenBins / 1024;
        static_assert(kBinsPerThread >= 1 && kBinsPerThread * 1024 == kWedgeClasses * kWedgeLenBins && kWedgeLenBins % kBinsPerThread == 0, "bins per thread");
        int v[kBinsPerThread], sum = 0;
#pragma unroll
        for (int u = 0; u < kBinsPerThread; ++u) { v[u] = hist[tid * kBinsPerThread + u]; sum += v[u]; }
        {
            // cells a class's rays pass, from its length bins (16 cells wide): what k_wedge_order sorts the units by.  One bin
            // per thread and kWedgeLenBins = 64 bins per class: a class is a wave.
            static_assert(kBinsPerThread == 1 && kWedgeLenBins == kWave, "a class's bins are one wave");
            const unsigned c = wave_sum_u32((unsigned)v[0] * (unsigned)((kWedgeLenBins - 1 - lane) * 16 + 8));
            if (lane == 0) ws.cost[group * kWedgeClasses + wave] = c;
        }
        int inc = sum;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) { const int t = __shfl_up(inc, off, kWave); if (lane >= off) inc += t; }
        if (lane == kWave - 1) wsum[wave] = inc;
        __syncthreads();
        int run = inc - sum;
        for (int w = 0; w < wave; ++w) run += wsum[w];
#pragma unroll
        for (int u = 0; u < kBinsPerThread; ++u) {
            const int bin = tid * kBinsPerThread + u;
            hist[bin] = run;
            if ((bin & (kWedgeLenBins - 1)) == 0) ws.offs[group * (kWedgeClasses + 1) + bin / kWedgeLenBins] = run;
            run += v[u];
        }
        if (tid == blockDim.x - 1) ws.offs[group * (kWedgeClasses + 1) + kWedgeClasses] = run;
    }
    __syncthreads();
    for (int r = tid; r < nrays; r += blockDim.x)
        if (keys[r] != 0xffffu) ws.list[ray0 + atomicAdd(&hist[keys[r]], 1)] = (unsigned short)r;
    unsigned tot = wave_sum_u32(nvis);
    int anybad = bad;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) anybad |= __shfl_xor(anybad, off, kWave);
    if (lane == 0) {
        if (tot) atomicAdd(visit_slot(g.visits), (unsigned long long)tot);
        if (anybad) atomicOr(g.status, anybad);
    }
}

// The work of a launch in the order k_wedge_cast takes it: a (group, class) unit is cut into PARTS of at most `part_rays` rays
// of its length-sorted list, and the parts are sorted by decreasing work; workgroup b casts part order[1 + b] and the
// hardware starts workgroups in index order, so the longest parts start first.  Before (stamps, round 4: 1 008 units on 512
// workgroup slots) unit lifetimes ranged to 2.7 x the mean and the longest unit alone lasted 400 of the launch's 480 us.
// Counting sort by the logarithm of a part's share of its unit's cost (256 buckets, order inside a bucket arbitrary).
// order[0]: parts listed; an entry is unit | part << 20.
__global__ void __launch_bounds__(1024) k_wedge_order(WedgeScratch ws, int units, int part_rays)
{
    __shared__ int hist[256];
    const int tid = threadIdx.x;
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    auto parts_of = [&](int u) -> int {
        const int g = u / kWedgeClasses, c = u - g * kWedgeClasses;
        const int nr = ws.offs[(size_t)g * (kWedgeClasses + 1) + c + 1] - ws.offs[(size_t)g * (kWedgeClasses + 1) + c];
        return (nr + part_rays - 1) / part_rays;                      // (a class without rays: no part)
    };
    auto bucket = [](uint32_t c) -> int { return 255 - min(255, (int)(__log2f((float)c + 1.0f) * 9.0f)); };   // log2 < 32: 9 per octave
    for (int u = tid; u < units; u += blockDim.x) {
        const int np = parts_of(u);
        if (np > 0) atomicAdd(&hist[bucket(ws.cost[u] / (uint32_t)np)], np);
    }
    __syncthreads();
    if (tid < 64) {                                                  // exclusive scan of the 256 buckets by one wave
        int h4[4], tot = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { h4[k] = hist[4 * tid + k]; tot += h4[k]; }
        int inc = tot;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) { const int v = __shfl_up(inc, off, kWave); if (tid >= off) inc += v; }
        int run = inc - tot;
#pragma unroll
        for (int k = 0; k < 4; ++k) { hist[4 * tid + k] = run; run += h4[k]; }
        if (tid == 63) ws.order[0] = (uint32_t)inc;
    }
    __syncthreads();
    for (int u = tid; u < units; u += blockDim.x) {
        const int np = parts_of(u);
        if (np <= 0) continue;
        const int base = atomicAdd(&hist[bucket(ws.cost[u] / (uint32_t)np)], np);
        for (int k = 0; k < np; ++k) ws.order[1 + base + k] = (uint32_t)u | ((uint32_t)k << 20);
    }
}

struct WedgeRay {
    int x0, y;             // walk origin along the axis; current y (the other axis, in walk coordinates)
    int k, kend;           // next walk step that passes a cell, last such step (the path's last cell - the hit - is neither)
    int ystep;
    double error, derr;
};

__global__ void __launch_bounds__(kWedgeThreads, 2 * kWedgeThreads / 256) k_wedge_cast(GridDev g, WedgeScratch ws, int n, int group_size, int scans, int part_rays)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int *box = reinterpret_cast<int *>(smem);                          // [0] a_min [1] a_max [2] v_lo [3] v_hi [4] rows of the band
    unsigned *win = reinterpret_cast<unsigned *>(smem + 64);
    char *guard = reinterpret_cast<char *>(win) + (size_t)kWedgeCells * 2;
    lds_guard_fill(guard);
    STAMP_DECL;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = kWedgeThreads >> 6;
    if (blockIdx.x >= ws.order[0]) return;                               // (the grid is sized for the largest possible number of parts)
    const uint32_t entry = ws.order[1 + blockIdx.x];                     // the parts with the most cells first
    const uint32_t unit = entry & 0xfffffu, part = entry >> 20;
    const int cls = (int)(unit % kWedgeClasses);
    const long group = unit / kWedgeClasses;
    const int groups_per_traj = (scans + group_size - 1) / group_size;
    const int l = (int)(group / groups_per_traj), s0 = (int)(group % groups_per_traj) * group_size;
    const long ray0 = ((long)l * scans + s0) * n;
    const int lo = ws.offs[group * (kWedgeClasses + 1) + cls] + (int)part * part_rays;
    const int hi = min(ws.offs[group * (kWedgeClasses + 1) + cls + 1], lo + part_rays);
    if (lo >= hi) return;
    const bool steep = (cls / kWedgeSlopes) >= 2;
    const int M = wedge_shear(cls);
    const size_t map_off = (size_t)(ws.got ? ws.got[l] : 0) * g.xw * g.yw;   // the trajectory's map, in cells of g.pass
    uint32_t *pass = g.pass + map_off;
    const unsigned wbase = lds_addr(win);

    for (int c0 = lo; c0 < hi; c0 += kWedgeThreads * kWedgeSlots) {     // (one pass unless a class holds more than 2 048 rays)
        WedgeRay wr[kWedgeSlots];
        int amin = INT_MAX, amax = INT_MIN;
#pragma unroll
        for (int j = 0; j < kWedgeSlots; ++j) {
            const int pos = c0 + j * kWedgeThreads + tid;                // slot 0 holds the class's longest rays
            WedgeRay &w = wr[j];
            w.x0 = 0; w.y = 0; w.k = 1; w.kend = 0; w.ystep = 1; w.error = 0.0; w.derr = 0.0;
            if (pos < hi) {
                const int r = (int)ws.list[ray0 + pos];
                const uint32_t e = ws.ends[ray0 + r], o = ws.orgs[(long)l * scans + s0 + r / n];
                Ray ry;
                (void)ray_setup((int)(o & 0xffffu), (int)(o >> 16), (int)(e & 0xffffu), (int)(e >> 16), ry);
                w.x0 = ry.x0; w.y = ry.y0; w.ystep = ry.ystep; w.derr = ry.derr;
                w.k = 0; w.kend = ry.dx - 1;                             // walk steps 0 .. dx - 1 pass, step dx is the hit ...
                if (ry.flag) {                                           // ... or, for a reversed path, step 0 is the hit: start one step in
                    if (walk_step(w.error, w.derr)) w.y += w.ystep;
                    w.k = 1; w.kend = ry.dx;
                }
                if (w.k <= w.kend) { amin = min(amin, w.x0 + w.k); amax = max(amax, w.x0 + w.kend); }
            }
        }
        if (tid == 0) { box[0] = INT_MAX; box[1] = INT_MIN; }
        __syncthreads();
        amin = wave_min_i32(amin); amax = wave_max_i32(amax);
        if (lane == 0 && amin <= amax) { atomicMin(&box[0], amin); atomicMax(&box[1], amax); }
        __syncthreads();
        STAMP(0);                                   // ray set-up
        const int a_first = box[0] & ~1, a_end = box[1];               // (even band starts: pairs of counters line up for the flush)
        for (int a_lo = a_first; a_lo <= a_end;) {
            // rows of this band (even): try what is left (at most 512), shrink to what the parallelogram's width allows.
            // Along a ray the sheared coordinate v = y - M a moves one way only (each step changes it by 0 or by the
            // class's sign), so a ray's range in the band is spanned by its values on entry and on exit; the walk stays
            // within half a cell of its line (|error| <= 1/2), which bounds the exit value before the ray is walked.
            int rows = (min(a_end - a_lo + 1, 512) + 1) & ~1;
            int v_lo = 0, v_hi = -1, Hw = 0;
            for (int attempt = 0; attempt < 2; ++attempt) {
                if (tid == 0) { box[2] = INT_MAX; box[3] = INT_MIN; }
                __syncthreads();
                int vl = INT_MAX, vh = INT_MIN;
#pragma unroll
                for (int j = 0; j < kWedgeSlots; ++j) {
                    const WedgeRay &w = wr[j];
                    const int a_in = w.x0 + w.k, a_out = min(w.x0 + w.kend, a_lo + rows - 1);
                    if (w.k <= w.kend && a_in <= a_out) {
                        const double adv = (double)(a_out - a_in) * w.derr + w.error;     // y steps up to the exit, +- 1/2
                        const int yo_lo = w.y + (w.ystep > 0 ? (int)floor(adv - 0.5) : -(int)ceil(adv + 0.5));
                        const int yo_hi = w.y + (w.ystep > 0 ? (int)ceil(adv + 0.5) : -(int)floor(adv - 0.5));
                        const int vi = w.y - M * a_in, vo0 = yo_lo - M * a_out, vo1 = yo_hi - M * a_out;
                        vl = min(vl, min(vi, vo0)); vh = max(vh, max(vi, vo1));
                    }
                }
                vl = wave_min_i32(vl); vh = wave_max_i32(vh);
                if (lane == 0 && vl <= vh) { atomicMin(&box[2], vl); atomicMax(&box[3], vh); }
                __syncthreads();
                v_lo = box[2]; v_hi = box[3];
                if (v_lo > v_hi) break;                                  // no ray has a cell in these rows
                v_lo &= ~1;                                              // (even: pairs of counters line up for the flush)
                Hw = ((v_hi - v_lo + 1) + 1) & ~1;                       // parallelogram width, even
                const int fit = (kWedgeCells / Hw) & ~1;
                if (fit < 2) break;                                      // not even two rows fit: the band goes by direct atomics (below)
                if (rows <= fit) break;
                rows = fit;                                              // fewer rows: the extents can only shrink
                if (attempt == 1) break;
                __syncthreads();
            }
            if (v_lo > v_hi) { a_lo += rows; __syncthreads(); continue; }
            if ((long)Hw * 2 > kWedgeCells) {
                // rays of one class that lie too far apart for any window (scans of a group cast from origins all over a
                // large map): this band's cells go straight to the counters, one atomic each - slow, exact, rare
#pragma unroll
                for (int j = 0; j < kWedgeSlots; ++j) {
                    WedgeRay &w = wr[j];
                    while (w.k <= w.kend && w.x0 + w.k < a_lo + rows) {
                        const int a = w.x0 + w.k;
                        atomicAdd(&pass[steep ? (size_t)w.y * g.yw + a : (size_t)a * g.yw + w.y], 1u);   // mapping.py:43
                        if (walk_step(w.error, w.derr)) w.y += w.ystep;
                        ++w.k;
                    }
                }
                a_lo += rows;
                __syncthreads();
                continue;
            }
            // physical layout: rows of C halfwords.  Not steep: a row per walk-axis step (map x), columns along map y.
            // Steep: a row per sheared column (map x again), columns along the walk axis (map y) - contiguous in the map either way
            const int C = steep ? rows : Hw, P = steep ? Hw : rows;
            const int ca = steep ? 1 : C, cv = steep ? C : 1;
            for (int w4 = tid; w4 < (P * C) >> 3; w4 += kWedgeThreads) reinterpret_cast<uint4 *>(win)[w4] = make_uint4(0u, 0u, 0u, 0u);
            for (int w1 = ((P * C) >> 3) * 4 + tid; w1 < (P * C) >> 1; w1 += kWedgeThreads) win[w1] = 0u;
            __syncthreads();
            STAMP(1);                               // band geometry + zero
            const int dh_a = ca - M * cv;
#pragma unroll
            for (int j = 0; j < kWedgeSlots; ++j) {
                WedgeRay &w = wr[j];
                const int a_in = w.x0 + w.k;
                int rem = (w.k <= w.kend && a_in < a_lo + rows) ? min(w.x0 + w.kend, a_lo + rows - 1) - a_in + 1 : 0;
                if (!__any(rem > 0)) continue;
                unsigned a2 = wbase + 2u * (unsigned)((a_in - a_lo) * ca + (w.y - M * a_in - v_lo) * cv);
                // lds_walk's loop with y carried along, kept here: through lds_walk (y as one more in/out parameter) the
                // compiler allots this kernel 115 VGPRs instead of 125 and moves the band geometry to the scalar unit
                const int da_k = 2 * dh_a, da_y = 2 * w.ystep * cv;
                double error = w.error;                                  // resumes where the previous band ended
                int y = w.y;
                const int took = rem;
                auto step = [&]() {
                    lds_add_u32(a2 & ~3u, 1u << ((a2 << 3) & 31u));      // mapping.py:43
                    const bool stepy = walk_step(error, w.derr);
                    a2 += (unsigned)(da_k + (stepy ? da_y : 0));
                    y += stepy ? w.ystep : 0;
                };
                for (;;) {
                    const bool full = rem >= 4;
                    if (!__any(full)) break;
                    if (full) { step(); step(); step(); step(); rem -= 4; }
                }
#pragma unroll
                for (int u = 0; u < 3; ++u)
                    if (rem > u) step();
                w.error = error; w.y = y; w.k += took;
            }
            __syncthreads();
            STAMP(3);                               // walk
            // flush: a wave per MAP row (map x), lanes along map y, two cells per lane as one 64-bit add where the pair is
            // aligned.  Not steep, or steep without shear: a map row is a physical row of the window.  Steep with shear: the
            // cells of map row x lie on a diagonal of the window (column c = map y - a_lo in physical row x - M y - v_lo),
            // read with per-lane addresses.
            const bool diag = steep && M != 0;
            const int nrows = diag ? P + C - 1 : P;                      // map rows the parallelogram touches
            const int x_first = !steep ? a_lo : (M == 0 ? v_lo : v_lo + (M > 0 ? M * a_lo : M * (a_lo + C - 1)));
            const unsigned short *winh = reinterpret_cast<const unsigned short *>(win);
            const int rot = (int)((blockIdx.x * 37u + blockIdx.y * 11u) % (unsigned)nrows);
            for (int pr = wave; pr < nrows; pr += nwaves) {
                const int p = pr + rot < nrows ? pr + rot : pr + rot - nrows;
                const int mx = x_first + p;
                if ((unsigned)mx >= (unsigned)g.xw) continue;            // (rows beyond the rays' reach hold nothing)
                const int my0 = steep ? a_lo : v_lo + M * mx;            // map y of column 0
                const size_t gbase = (size_t)mx * g.yw + my0;
                // The 64-bit add needs an 8-byte address: the parity that counts is the cell's in g.pass (an 8-byte
                // aligned allocation), not in the map - a map of an odd number of cells puts every odd-numbered map at
                // 4 mod 8 (the window kernels: pair64).  With rows of an odd length every other row goes cell by cell.
                // A pair's second cell may lie one past its row's end (C and Hw are even, yw need not be): its count is
                // zero, it is the next row's or the next map's first cell, and past the last map it is the padding
                // that an odd number of cells leaves in front of hit[] (slam_grid_create rounds pass[] up).
                const bool pair = (((map_off + gbase) & 1) == 0);
                for (int d = lane; d < (C >> 1); d += kWave) {
                    unsigned v;
                    if (!diag) v = win[p * (C >> 1) + d];
                    else {
                        const int p0 = mx - v_lo - M * (a_lo + 2 * d), p1 = p0 - M;     // physical rows of the pair's two cells
                        const unsigned c0 = (unsigned)p0 < (unsigned)P ? winh[p0 * C + 2 * d] : 0u;
                        const unsigned c1 = (unsigned)p1 < (unsigned)P ? winh[p1 * C + 2 * d + 1] : 0u;
                        v = c0 | (c1 << 16);
                    }
                    if (!v) continue;
                    if (pair) atomicAdd(reinterpret_cast<unsigned long long *>(&pass[gbase + 2 * d]), (unsigned long long)(v & 0xffffu) | ((unsigned long long)(v >> 16) << 32));
                    else {
                        if (v & 0xffffu) atomicAdd(&pass[gbase + 2 * d], v & 0xffffu);
                        if (v >> 16) atomicAdd(&pass[gbase + 2 * d + 1], v >> 16);
                    }
                }
            }
            a_lo += rows;
            __syncthreads();
            STAMP(4);                               // flush
        }
    }
    STAMP_END(5);
    lds_guard_check(guard, g.status);
}

// the pieces of a wedge cast, bound to the members of `ws`
static Layout wedge_pieces(WedgeScratch &ws, long rays, long scans, long groups)
{
    return Layout().add(ws.ends, rays).add(ws.orgs, scans).add(ws.offs, (size_t)groups * (kWedgeClasses + 1)).add(ws.cost, (size_t)groups * kWedgeClasses)
        .add(ws.order, 1 + (size_t)groups * kWedgeClasses + (size_t)rays / kWedgePartMin).add(ws.list, rays);
}

template <class Src>
static hipError_t launch_wedges(const GridDev &g, const Src &src, int L, int scans, int n, int group, void *scratch, size_t cap, hipStream_t s, const int32_t *got)
{
    if (scans < 1) return hipSuccess;
    int G = group > 0 ? group : 16;
    G = std::min(G, std::max(1, 65535 / n));
    G = std::min(G, scans);
    if ((long)G * n > 65535) return hipErrorInvalidValue;   // (ray numbers inside a group are 16-bit: keys[], ws.list[])
    if (g.xw > 65535 || g.yw > 65535) return hipErrorInvalidValue;   // (end cells travel as 16-bit pairs)
    const int groups_per_traj = (scans + G - 1) / G;
    const long groups = (long)L * groups_per_traj, rays = (long)L * scans * n;
    if (groups > kMaxLaunchGroups)
        return launch_in_chunks(src, L, scans, G, got, [&](const Src &cs, int cl, int cscans, const int32_t *cgot) {
            return launch_wedges(g, cs, cl, cscans, n, G, scratch, cap, s, cgot);
        });
    WedgeScratch ws;
    if (!wedge_pieces(ws, rays, (long)L * scans, groups).place(scratch, cap)) return hipErrorInvalidValue;
    ws.got = got;
    if (g.pmap_live && g.live_dirty) *g.live_dirty = true;
    const size_t lds_a = win_sc_bytes(G) + (size_t)(kWedgeClasses * kWedgeLenBins + kWinMaxGroup) * 4 + (size_t)G * n * 2;
    const size_t lds_b = 64 + (size_t)kWedgeCells * 2 + kLdsGuard;
    hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(&k_wedge_sort<Src>), (int)lds_a);
    if (e == hipSuccess) e = allow_dynamic_lds(reinterpret_cast<const void *>(&k_wedge_cast), (int)lds_b);
    if (e != hipSuccess) return e;
    SLAM_LAUNCH((k_wedge_sort<Src>), dim3(groups_per_traj, L), dim3(1024), lds_a, s, g, src, ws, G);
    // rays per part: what a workgroup's lanes hold in one pass.  (Smaller parts balance the launch better and cost more than they
    // gain - every part of a class zeroes and flushes the class's bands again: 1 024 rays 0.533 ms, 512 rays 0.667 ms against 0.516.)
    const int part_rays = kWedgeThreads * kWedgeSlots;
    const long max_parts = groups * kWedgeClasses + rays / part_rays;      // (every unit's last part may be short)
    SLAM_LAUNCH(k_wedge_order, dim3(1), dim3(1024), 0, s, ws, (int)(groups * kWedgeClasses), part_rays);
    SLAM_LAUNCH(k_wedge_cast, dim3((unsigned)max_parts), dim3(kWedgeThreads), lds_b, s, g, ws, n, G, scans, part_rays);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------
// Which engine casts a batch of scans.  big: the map has more than eight windows of cells (xw * yw > 8 * kWinCells);
// wok: the direction wedges take the map (grid_mode != 2, both sides <= 65 535 cells, as the end cells travel as 16-bit
// pairs).  First match wins:
//
//   entry                                  condition                                           path
//   slam_grid_update[_dev]                 grid_of_batch given                                 Direct (any mode)
//                                          mode 1, 2 or 4, n <= 8192, (big or mode 2, 4)       Wedges if wok, else Tiles
//                                          mode != 0, n <= 65 535                              Window
//                                          otherwise                                           Direct
//   slam_replay*, slam_grid_update_scans*  mode 1, 2 or 4, n <= 8192, (big or mode 2, 4),      Wedges if wok, else Tiles
//                                          and with grid_of_traj given also wok
//                                          mode != 0                                           Window (with centres: one stream)
//                                          mode 0 with centres                                 SLAM_ERR_INVALID (the caller's)
//                                          mode 0                                              Direct
//   slam_particles* with a grid            always, any mode and map size                       Window
//
// Window is launch_win; the table in the header of the window section ("Which kernel casts a launch") says which of the
// window kernels takes it.  The replay entries take at most 65 535 beams, so one Window rule serves both forms.
// n <= 8192 (kTileMaxBeams): ray numbers inside a group of the tiles and wedges are 16-bit.
// ---------------------------------------------------------------------------------
constexpr int kTileMaxBeams = 8192;

CastPath plan_cast(const GridDev &g, int mode, const CastRequest &r)
{
    if (r.particles) return CastPath::Window;
    if (r.ox && r.maps) return CastPath::Direct;
    const bool big = (long)g.xw * g.yw > 8L * kWinCells;
    const bool wok = mode != 2 && g.xw <= 65535 && g.yw <= 65535;
    if ((mode == 1 || mode == 2 || mode == 4) && r.n <= kTileMaxBeams && (big || mode == 2 || mode == 4) && (!r.maps || wok))
        return wok ? CastPath::Wedges : CastPath::Tiles;
    return mode != 0 && r.n <= 65535 ? CastPath::Window : CastPath::Direct;
}

size_t cast_layout_bytes(CastPath p, long rays, long scans, long groups)
{
    TileScratch ts;
    WedgeScratch ws;
    if (p == CastPath::Wedges) return wedge_pieces(ws, rays, scans, groups).bytes();
    if (p == CastPath::Tiles) return tile_pieces(ts, rays, groups).bytes();
    return 0;
}

size_t cast_scratch_bytes(CastPath p, const CastRequest &r)
{
    // the wedges keep 6 bytes per ray (end cell, sorted ray number), the recorded walks ~400; groups: one per scan bounds them
    const long scans = (long)r.L * r.scans;
    return cast_layout_bytes(p, scans * r.n, scans, scans);
}

template <class Src>
static hipError_t launch_cast(const GridDev &g, CastPath p, const Src &src, const CastRequest &r, void *scratch, size_t cap, hipStream_t s)
{
    switch (p) {
    case CastPath::Wedges: return launch_wedges(g, src, r.L, r.scans, r.n, r.group, scratch, cap, s, r.maps);
    case CastPath::Tiles: return launch_tiles(g, src, r.L, r.scans, r.n, r.group, scratch, cap, s);
    case CastPath::Window:
        return launch_win(g, src, r.L, r.scans, r.n, pick_group(r.group, (long)r.L * r.scans, r.scans, r.n), r.maps, s, r.split, r.lds_hits);
    case CastPath::Direct: break;
    }
    if (g.pmap_live && g.live_dirty) *g.live_dirty = true;
    const int block = std::min(256, std::max(kWave, (r.n + kWave - 1) / kWave * kWave));
    SLAM_LAUNCH((k_grid_update<Src>), dim3(r.scans, r.L), dim3(block), 0, s, g, src, r.maps);
    return hipGetLastError();
}

hipError_t launch_cast(const GridDev &g, CastPath p, const CastRequest &r, void *scratch, size_t scratch_bytes, hipStream_t s)
{
    if (r.ox) return launch_cast(g, p, ExplicitSource{r.ox, r.oy, r.cx, r.cy, r.scans, r.n}, r, scratch, scratch_bytes, s);
    if (r.per_filter) {
        ParticleSource src(r.ranges, r.cos_t, r.sin_t, r.poses, r.acc, r.n, r.per_filter);
        src.l0 = r.first_particle;
        return launch_cast(g, p, src, r, scratch, scratch_bytes, s);
    }
    const ReplaySource src{r.ranges, r.cos_t, r.sin_t, r.poses, r.scans + 1, r.n, r.particles ? 0L : (long)(r.scans + 1) * r.n,
                           r.particles, r.centres, r.heading_cs};
    return launch_cast(g, p, src, r, scratch, scratch_bytes, s);
}

__global__ void __launch_bounds__(256) k_grid_finalize(const uint32_t *__restrict__ pass, const uint32_t *__restrict__ hit,
                                                       size_t cells, OccRule rule, int8_t *__restrict__ pmap)
{
    size_t stride = (size_t)gridDim.x * blockDim.x * 4;
    for (size_t c = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; c < cells; c += stride) {
        if (c + 4 <= cells) {
            uint4 p = *reinterpret_cast<const uint4 *>(pass + c);
            uint4 h = *reinterpret_cast<const uint4 *>(hit + c);
            uint32_t out = rule.value(p.x, h.x) | rule.value(p.y, h.y) << 8 | rule.value(p.z, h.z) << 16 |
                           rule.value(p.w, h.w) << 24;
            *reinterpret_cast<uint32_t *>(pmap + c) = out;
        } else {
            for (size_t e = c; e < cells; ++e) pmap[e] = (int8_t)rule.value(pass[e], hit[e]);
        }
    }
}

hipError_t launch_grid_finalize(const GridDev &g, int g0, int gcount, int8_t *pmap, hipStream_t s)
{
    size_t per = (size_t)g.xw * g.yw, cells = per * gcount;
    size_t blocks = (cells / 4 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    if (blocks < 1) blocks = 1;
    OccRule rule = OccRule::of(g);
    SLAM_LAUNCH(k_grid_finalize, dim3(blocks), dim3(256), 0, s, g.pass + per * g0, g.hit + per * g0, cells, rule, pmap);
    return hipGetLastError();
}

// datamap view of the counters: free_inc*pass + hit_inc*hit (mapping.py:43,45).
__global__ void __launch_bounds__(256) k_grid_datamap(const uint32_t *__restrict__ pass, const uint32_t *__restrict__ hit,
                                                      size_t cells, double free_inc, double hit_inc, double *__restrict__ out)
{
    for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += (size_t)gridDim.x * blockDim.x)
        out[c] = free_inc * (double)pass[c] + hit_inc * (double)hit[c];
}

hipError_t launch_grid_datamap(const GridDev &g, int gi, double *datamap, hipStream_t s)
{
    size_t per = (size_t)g.xw * g.yw;
    size_t blocks = (per + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    SLAM_LAUNCH(k_grid_datamap, dim3(blocks), dim3(256), 0, s, g.pass + per * gi, g.hit + per * gi, per, g.free_inc,
                       g.hit_inc, datamap);
    return hipGetLastError();
}

// publishMap layout (slam_ekf.py:270-271): data[y*xw + x] = pmap[x][y]; 32x32 LDS tile
// transpose so both sides are coalesced.
__global__ void __launch_bounds__(256) k_grid_transpose(const int8_t *__restrict__ pmap, int xw, int yw, int8_t *__restrict__ data)
{
    __shared__ int8_t tile[32][33];
    int x0 = blockIdx.x * 32, y0 = blockIdx.y * 32;
    int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    for (int r = ty; r < 32; r += 8) {
        int x = x0 + r, y = y0 + tx;
        if (x < xw && y < yw) tile[r][tx] = pmap[(size_t)x * yw + y];
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        int y = y0 + r, x = x0 + tx;
        if (x < xw && y < yw) data[(size_t)y * xw + x] = tile[tx][r];
    }
}

hipError_t launch_grid_transpose(const int8_t *pmap, int xw, int yw, int8_t *data, hipStream_t s)
{
    SLAM_LAUNCH(k_grid_transpose, dim3((xw + 31) / 32, (yw + 31) / 32), dim3(256), 0, s, pmap, xw, yw, data);
    return hipGetLastError();
}

// bresenham(start, end).path (bresenham.py:2-58): one lane per line.
__global__ void __launch_bounds__(256) k_bresenham(const int32_t *__restrict__ starts, const int32_t *__restrict__ ends, int B,
                                                   const int64_t *__restrict__ offsets, int32_t *__restrict__ lens,
                                                   int32_t *__restrict__ cells)
{
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    Ray r;
    if (!ray_setup(starts[2 * b], starts[2 * b + 1], ends[2 * b], ends[2 * b + 1], r)) { lens[b] = 0; return; }
    lens[b] = r.dx + 1;
    if (!cells) return;
    int32_t *out = cells + 2 * offsets[b];
    double error = 0.0;
    int y = r.y0;
    for (int k = 0; k <= r.dx; ++k) {
        int x = r.x0 + k;
        int j = r.flag ? r.dx - k : k;                               // path.reverse(), :57-58
        out[2 * (size_t)j] = r.steep ? y : x;
        out[2 * (size_t)j + 1] = r.steep ? x : y;
        y += walk_step(error, r.derr) ? r.ystep : 0;
    }
}

hipError_t launch_bresenham(const int32_t *starts, const int32_t *ends, int B, const int64_t *offsets, int32_t *lens,
                            int32_t *cells, hipStream_t s)
{
    SLAM_LAUNCH(k_bresenham, dim3((B + 255) / 256), dim3(256), 0, s, starts, ends, B, offsets, lens, cells);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------
// Maps that follow their ancestors (slam_grid_copy_maps): bandwidth work.
// ---------------------------------------------------------------------------------
// n dwords by the whole workgroup: 16 bytes per lane where source and destination are equally aligned (a map's base is
// g * xw * yw * 4 bytes and need not be 16-byte aligned), the head, the tail and unequal alignment dword by dword.
__device__ __forceinline__ void copy_dwords(uint32_t *__restrict__ dst, const uint32_t *__restrict__ src, long n)
{
    const uintptr_t ad = reinterpret_cast<uintptr_t>(dst), as = reinterpret_cast<uintptr_t>(src);
    if (((ad ^ as) & 15) != 0) {
        for (long i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
        return;
    }
    const long head = std::min(n, (long)(((16 - (ad & 15)) & 15) / 4)), body = (n - head) / 4;
    for (long i = threadIdx.x; i < head; i += blockDim.x) dst[i] = src[i];
    const uint4 *s4 = reinterpret_cast<const uint4 *>(src + head);
    uint4 *d4 = reinterpret_cast<uint4 *>(dst + head);
    for (long i = threadIdx.x; i < body; i += blockDim.x) d4[i] = s4[i];
    for (long i = head + 4 * body + threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
}

// the same for the bytes of the live pmap: a dword per lane where both are equally aligned
__device__ __forceinline__ void copy_bytes(int8_t *__restrict__ dst, const int8_t *__restrict__ src, long n)
{
    const uintptr_t ad = reinterpret_cast<uintptr_t>(dst), as = reinterpret_cast<uintptr_t>(src);
    if (((ad ^ as) & 3) != 0) {
        for (long i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
        return;
    }
    const long head = std::min(n, (long)((4 - (ad & 3)) & 3)), body = (n - head) / 4;
    for (long i = threadIdx.x; i < head; i += blockDim.x) dst[i] = src[i];
    const uint32_t *s4 = reinterpret_cast<const uint32_t *>(src + head);
    uint32_t *d4 = reinterpret_cast<uint32_t *>(dst + head);
    for (long i = threadIdx.x; i < body; i += blockDim.x) d4[i] = s4[i];
    for (long i = head + 4 * body + threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
}

// Group = (destination k, chunk ch of its cells), taken grid-stride.  Map first + k becomes a copy of map src[k]; kept
// (copied 0) when that is itself or no map; left alone (copied -1) when the source is a destination of this call - the one
// extra load - so that no map is read that the launch writes.
__global__ void __launch_bounds__(kCopyThreads) k_grid_copy_maps(GridDev g, const int32_t *__restrict__ src, int first, int count,
                                                                long chunks, int32_t *__restrict__ copied)
{
    const long cells = (long)g.xw * g.yw, groups = (long)count * chunks;
    for (long grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int k = (int)(grp / chunks);
        const long ch = grp % chunks;
        const int d = first + k, s = src[k];
        int what = 1;
        if (s == d || (unsigned)s >= (unsigned)g.G) what = 0;
        else if (s >= first && s - first < count && src[s - first] != s) what = -1;
        if (ch == 0 && threadIdx.x == 0 && copied) copied[k] = what;
        if (what != 1) continue;
        const long c0 = ch * kCopyChunkCells, len = std::min((long)kCopyChunkCells, cells - c0);
        const size_t so = (size_t)s * cells + c0, dof = (size_t)d * cells + c0;
        copy_dwords(g.pass + dof, g.pass + so, len);
        copy_dwords(g.hit + dof, g.hit + so, len);
        if (g.pmap_live) copy_bytes(g.pmap_live + dof, g.pmap_live + so, len);
    }
}

hipError_t launch_grid_copy_maps(const GridDev &g, const int32_t *src, int first, int count, int32_t *copied_out, hipStream_t s)
{
    const CopyShape p = plan_copy_maps((long)g.xw * g.yw, count);
    SLAM_LAUNCH(k_grid_copy_maps, dim3((unsigned)p.grid), dim3(p.threads), 0, s, g, src, first, count, p.chunks, copied_out);
    return hipGetLastError();
}

}  // namespace slam
