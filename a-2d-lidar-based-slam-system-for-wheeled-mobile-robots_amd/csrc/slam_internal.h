// Internal declarations shared by the kernel files and the C-ABI layer of libslamhip.so.
// gfx950 (MI355X) only; wavefront = 64.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "slam_hip.h"
#include "slam_refine.h"
#include "slam_track.h"
#include "launch_shapes.h"

#include <hip/hip_ext.h>

namespace slam {

// Kernel timing: when the ABI layer has opened a timing bracket (slam_timing_enable; `Timed` in
// slam_abi.hip), every launch inside it asks the bracket for a fresh pair of events and carries
// them as the dispatch's own start / stop events (hipExtLaunchKernelGGL), so they bracket exactly
// the kernel's execution - what rocprofv3's kernel trace reports - and no marker packets are put
// into the queue.  A family that is several launches (the byte-window ray cast and its fallback,
// the wedge sort and cast) is the sum of its launches.
struct LaunchTimer {
    void *self;
    bool (*next)(void *self, hipEvent_t *e0, hipEvent_t *e1);
};
extern thread_local LaunchTimer g_launch_timer;
inline bool launch_events(hipEvent_t *e0, hipEvent_t *e1)
{
    return g_launch_timer.self && g_launch_timer.next(g_launch_timer.self, e0, e1);
}

#define SLAM_LAUNCH(kernel, grid, block, shmem, stream, ...)                                                          \
    do {                                                                                                              \
        hipEvent_t e0_ = nullptr, e1_ = nullptr;                                                                      \
        if (::slam::launch_events(&e0_, &e1_))                                                                        \
            hipExtLaunchKernelGGL(kernel, grid, block, shmem, stream, e0_, e1_, 0, __VA_ARGS__);                      \
        else                                                                                                          \
            hipLaunchKernelGGL(kernel, grid, block, shmem, stream, __VA_ARGS__);                                      \
    } while (0)


// hipFuncSetAttribute(MaxDynamicSharedMemorySize) applies to the CURRENT device: the largest size set so far is remembered
// per (device, function), so a second device used by the same process gets the attribute too and a later launch that
// needs more LDS than any before it raises it.
hipError_t allow_dynamic_lds(const void *kernel, int bytes);

// (kWave, kMaxWaves and kLdsGuard, the guard bytes of the LDS-guard debug build: launch_shapes.h)
constexpr int kMaxRayCells = 1 << 20;    // longest ray the grid kernels will walk (cells)

enum : int { kStatusNaN = 1, kStatusOverflow = 2, kStatusGuard = 4 };

#if defined(__HIPCC__)
__device__ __forceinline__ void lds_guard_fill(char *p)
{
    for (int i = threadIdx.x; i < kLdsGuard / 4; i += blockDim.x) reinterpret_cast<unsigned *>(p)[i] = 0xA5A5A5A5u;
}
__device__ __forceinline__ void lds_guard_check(const char *p, int *status)
{
    if (kLdsGuard == 0) return;
    __syncthreads();
    bool bad = false;
    for (int i = threadIdx.x; i < kLdsGuard / 4; i += blockDim.x) bad |= reinterpret_cast<const unsigned *>(p)[i] != 0xA5A5A5A5u;
    if (bad && status) atomicOr(status, kStatusGuard);
}

// a 64-bit value across a wave: lane `src`'s v
template <typename T>
__device__ __forceinline__ T shfl64(T v, int src)
{
    static_assert(sizeof(T) == 8, "64-bit values");
    unsigned long long u;
    memcpy(&u, &v, 8);
    const unsigned hi = __shfl((unsigned)(u >> 32), src, kWave), lo = __shfl((unsigned)u, src, kWave);
    u = ((unsigned long long)hi << 32) | lo;
    memcpy(&v, &u, 8);
    return v;
}
#endif

// ---- ICP ---------------------------------------------------------------------------
struct IcpArgs {
    // Either point buffers ...
    const void *tar, *src;     // [2][n] per set, storage type = template T
    // ... or raw scans (fused polar->Cartesian, used by the replay / particle pipelines): scan k
    // of a stream is the source, scan k-1 the target; the points are formed in registers with the
    // same arithmetic as k_scan_to_points (one multiply, then rounding to T) and never touch HBM.
    const float *ranges;       // nullable; [.. scans ..][n]
    const double *cos_t, *sin_t;
    long tar_scan_stride, src_scan_stride;   // floats between consecutive pairs' scans (0: shared)
    const double *prior;       // nullable [B][6]
    long tar_stride, src_stride;  // elements between consecutive sets (0: shared)
    int ppt;                   // replay addressing: pairs per trajectory (0: plain batch)
    int B, n_tar, n_src, max_iter;
    double tol;
    double *T_out;             // [B][9]
    int32_t *iters_out;        // nullable [B]
    double *err_out;           // nullable [B]
    int *status = nullptr;     // sticky status word of the context (LDS guard builds)
    int qpt_pref = 0;          // queries per lane in batched launches: 0 = by batch size (context option "icp_qpt")
    void *zero_ptr = nullptr;  // nullable: zero_bytes bytes (a multiple of 4, 16-byte aligned start) that the launch clears on its way -
    size_t zero_bytes = 0;     //   the counters of the map the replay's ray cast fills next (slam_replay_dev, option "replay_reset")
    int polar_copy = 0;        // set by launch_icp: the kernel carves the unpadded second copy of the target (nn_polar)
    int team_cap = 0;          // set by launch_icp: room in the LDS list of first-iteration queries without a beam window (nn_listed), 0: none
    int team_mode = 0;         // context option "icp_team": 0 = on where it applies, 1 = off (the box search takes every such query)
    int one_wave = -1;         // context option "icp_one_wave": -1 = one wave per pair where a full-chip launch allows it, 0 = never, 1 = wherever a pair fits
    int f32_filter = -1;       // context option "icp_f32_filter": the one-wave shape scans its beam windows in float32 first, float64 decides: -1 = on, 0 = off, 1 = on
    int batch_invariant = 0;   // 1: launch_icp picks a shape that does not depend on B (the node replay: results independent of the batch)
};

hipError_t launch_icp(const IcpArgs &a, int dtype, hipStream_t s);
hipError_t launch_nn(const void *src, const void *tar, int B, int n_src, int n_tar, int dtype, double *dist,
                     int32_t *idx, hipStream_t s);
hipError_t launch_kabsch(const double *src, const double *tar, int B, int n, double *T_out, hipStream_t s);
hipError_t launch_scan_to_points(const float *ranges, const double *cos_t, const double *sin_t, long total,
                                 int n, int clip_inf, int dtype, void *pts, hipStream_t s);
// prior: nullable [L][6] (n must be 1): the step composed is T.[prior; 0 0 1] (particle hypotheses).
// heading_cs: nullable [L][2] (n must be 1): cos / sin of the new headings, for the ray cast that follows.
hipError_t launch_pose_compose(const double *T, const double *pose0, int L, int n, double *poses, hipStream_t s,
                               const double *prior = nullptr, double *heading_cs = nullptr);

#ifdef SLAM_STAMPS_ICP
hipError_t debug_polar_lanes(unsigned long long out[6], bool clear);   // diagnostic build: lane efficiency counters of nn_polar (slam_stamps.h)
#endif

// ---- grid --------------------------------------------------------------------------
constexpr int kMaxHitLevels = 8;
constexpr int kVisitSlots = 256;         // power of two
constexpr int kVisitStride = 8;          // unsigned long longs between slots (64 bytes)
#if defined(__HIPCC__)
__device__ __forceinline__ unsigned long long *visit_slot(unsigned long long *visits)
{
    return visits + (size_t)((blockIdx.x + blockIdx.y * 131u) & (unsigned)(kVisitSlots - 1)) * kVisitStride;
}
#endif

struct GridDev {
    int G, xw, yw;
    double scale, off_x, off_y;
    uint32_t *pass, *hit;          // [G][xw][yw]
    // In-bounds cell visits since reset: kVisitSlots counters, one per 64-byte line; a workgroup adds
    // to the slot of its block index and slam_grid_visits sums them.  (One shared counter made every
    // wave of a 10 000-workgroup launch queue on one address: 80 000 serialised atomics, 1.6 ms.)
    unsigned long long *visits;
    int *status;                   // sticky kStatus* bits (context-wide)
    // Occupied rule on the integer counters (see slam_grid_create): a cell with h hits and p
    // passes is occupied iff h >= hit_levels or p >= pass_thresh[h].
    int hit_levels;                // 1 for the reference's +20 (one hit occupies), 3 for the online variant's +4
    uint32_t pass_thresh[kMaxHitLevels];
    // Live pmap (slam_grid_live_pmap): [G][xw][yw] int8 kept current by ray casts that own their
    // map exclusively (one workgroup per map); any other update sets *live_dirty (host flag) and
    // the next finalize / read refreshes it with a full pass.
    int8_t *pmap_live;
    bool *live_dirty;
    // Re-do list of the single-scan owner kernels (allocated with the live pmap): [0] maps listed, [1] workgroups
    // of the general kernel that have read the list, [2 + k] map numbers.  Empty between launches.
    int32_t *redo;
    double free_inc, hit_inc;
};

// A ray cast of a batch of scans: plan_cast picks the engine and launch_cast places that engine's pieces (grid_kernels.hip:
// TileScratch, WedgeScratch; none for Direct and Window) in the `scratch_bytes` bytes at `scratch`, or fails with
// hipErrorInvalidValue before its first kernel when they end beyond them.  cast_layout_bytes is where the pieces of a launch of
// `rays` rays in `scans` scans and `groups` groups end, and cast_scratch_bytes that of a whole request with one group per scan:
// no piece shrinks as a count grows, so it covers every launch of the request and every chunk of an oversize one.  The request holds either explicit world-frame endpoints (ox != nullptr:
// Mapping.update's own arguments, `scans` scans of one stream) or a replay: scan k of trajectory l is
// ranges[(l * (scans + 1) + k + 1) * n], cast from poses[l][k] (slam_ekf.py:89).
enum class CastPath { Direct, Window, Tiles, Wedges };
struct CastRequest {
    const double *ox = nullptr, *oy = nullptr, *cx = nullptr, *cy = nullptr;      // [scans][n], [scans]
    const float *ranges = nullptr;
    const double *cos_t = nullptr, *sin_t = nullptr, *poses = nullptr;
    const double *centres = nullptr;       // nullable [L][scans][2]: ray origins that are not the pose (one stream)
    const double *heading_cs = nullptr;    // nullable [L][scans][2]: cos / sin of the poses' headings
    int L = 1, scans = 0, n = 0;
    const int32_t *maps = nullptr;         // nullable: the map of every scan (explicit) or trajectory (replay)
    bool particles = false;                // every trajectory reads the same two scans and casts into map l of its own
    // with `particles` (slam_grid_update_particles): per_filter = P > 0: trajectory l is particle first_particle + l of F filters
    // of P; it reads scan (first_particle + l) / P of ranges [F][n] and poses[l], and casts nothing when acc[l] is SLAM_MCL_DEAD
    int per_filter = 0;
    long first_particle = 0;
    const int32_t *acc = nullptr;          // nullable [L]
    int group = 0, split = -1;             // scans per workgroup (0: automatic); window split in two (-1: automatic, 0, 1)
    int lds_hits = -1;                     // context option "win_lds_hits": hits of sorted window rays counted in LDS, one add per end cell: -1 = in chip-filling launches, 0 = off, 1 = on
};
CastPath plan_cast(const GridDev &g, int grid_mode, const CastRequest &r);
size_t cast_layout_bytes(CastPath p, long rays, long scans, long groups);
size_t cast_scratch_bytes(CastPath p, const CastRequest &r);
hipError_t launch_cast(const GridDev &g, CastPath p, const CastRequest &r, void *scratch, size_t scratch_bytes, hipStream_t s);
hipError_t launch_grid_finalize(const GridDev &g, int g0, int gcount, int8_t *pmap, hipStream_t s);
// slam_grid_copy_maps: map first + k becomes a copy of map src[k], counters and (when kept) live pmap; copied_out nullable [count]
hipError_t launch_grid_copy_maps(const GridDev &g, const int32_t *src, int first, int count, int32_t *copied_out, hipStream_t s);
hipError_t launch_grid_datamap(const GridDev &g, int gi, double *datamap, hipStream_t s);
hipError_t launch_grid_transpose(const int8_t *pmap, int xw, int yw, int8_t *data, hipStream_t s);
hipError_t launch_bresenham(const int32_t *starts, const int32_t *ends, int B, const int64_t *offsets,
                            int32_t *lens, int32_t *cells, hipStream_t s);

// ---- rays traced through a map (raycast_kernels.hip) ----------------------------------
struct RaycastArgs {
    GridDev g;
    const uint32_t *mask = nullptr;          // [G][xw][ceil(yw / 32)]: bit ly % 32 of word [lx][ly / 32] = pmap == 100 (launch_raycast_pack)
    int wpr = 0;                             // set by launch_raycast: mask words per row
    const double *poses = nullptr;           // [B][3]
    const int32_t *maps = nullptr;           // nullable [B]: the map of every hypothesis (an entry outside [0, G): a NaN / BAD row)
    const double *cos_t = nullptr, *sin_t = nullptr;
    int B = 0, n = 0, skip = 0;
    float max_range = 0.f;                   // ray cast: every beam's range
    float *ranges_out = nullptr;             // ray cast: [B][n]
    int32_t *cells_out = nullptr;            // ray cast: nullable [B][n][2]
    const float *ranges = nullptr;           // score: [B][n], or one [n] with range_stride 0
    long range_stride = 0;
    int32_t *counts_out = nullptr;           // score (non-null selects it): [B][SLAM_RAY_CLASSES], zero on entry
    int8_t *class_out = nullptr;             // score: nullable [B][n]
    int hyps_per_block = 1;                  // set by launch_raycast (staged engine)
};
size_t raycast_mask_words(const GridDev &g);
// true: the staged engine (mask in LDS); lds_mode is the context option "raycast_lds"
bool choose_raycast_path(const GridDev &g, int lds_mode, long B, int n);
hipError_t launch_raycast_pack(const GridDev &g, uint32_t *mask, hipStream_t s);
hipError_t launch_raycast(RaycastArgs a, bool staged, hipStream_t s);

// ---- view gain: the cells a scan from a pose would reveal (view_kernels.hip) --------------
struct ViewArgs {
    GridDev g;
    const uint32_t *occ = nullptr;           // [G][xw][wpr]: bit ly % 32 of word [lx][ly / 32] = pmap == 100 (launch_view_pack)
    const uint32_t *unk = nullptr;           // the same for pmap == 50
    int wpr = 0;                             // words per map row
    const double *poses = nullptr;           // [B][3]
    const int32_t *maps = nullptr;           // nullable [B]: NULL = every view reads map 0 (an entry outside [0, G): a row of -1)
    const double *cos_t = nullptr, *sin_t = nullptr;
    int B = 0, n = 0, skip = 0;
    float max_range = 0.f;
    int lds_mode = -1;                       // context option "gain_lds"
    uint32_t *slots = nullptr;               // global engine: [its workgroups][xw * wpr] window words
    int32_t *counts_out = nullptr;           // [B][SLAM_VIEW_COUNTS]
    uint32_t *seen_out = nullptr;            // nullable [B][xw][wpr]
};
// occ, unk: the two planes, raycast_mask_words(g) words each
hipError_t launch_view_pack(const GridDev &g, uint32_t *occ, uint32_t *unk, hipStream_t s);
// the LDS engine over the views it takes, then the global engine over the rest, as p says
hipError_t launch_view(const ViewArgs &a, const ViewShape &p, hipStream_t s);

// ---- distance field of the grid and the window matcher on it (match_kernels.hip) ---------
struct MatchArgs {
    GridDev g;
    const int16_t *field = nullptr;          // [G][xw][yw] (launch_distance_field)
    const float *ranges = nullptr;           // [B][n], or one [n] with range_stride 0
    long range_stride = 0;
    const double *centres = nullptr;         // [B][2]
    const int32_t *maps = nullptr;           // nullable [B]: the map of every hypothesis (an entry outside [0, G): all outputs -1)
    const double *cos_t = nullptr, *sin_t = nullptr;
    const double *rot_cs = nullptr;          // [B][K][2] cos / sin of every rotation
    int B = 0, n = 0, K = 0, nx = 0, ny = 0;
    double step = 0.0;
    float max_range = 0.f;
    int cap = 0;
    unsigned long long *keys = nullptr;      // workspace [B], every byte 0xff on entry: min of (cost << 32 | flat index)
    int32_t *best_out = nullptr, *best_cost_out = nullptr;   // [B]
    int32_t *used_out = nullptr;             // nullable [B]
    int32_t *cost_out = nullptr;             // nullable [B][K][2 nx + 1][2 ny + 1]
    int kc = 1, chunks = 1;                  // set by launch_match: rotations per workgroup, workgroups per hypothesis
};
size_t field_rowd_bytes(const GridDev &g);   // workspace of launch_distance_field
// mask: launch_raycast_pack's words; rowd: field_rowd_bytes(g) bytes of workspace; field [G][xw][yw]; 1 <= cap <= 32767
hipError_t launch_distance_field(const GridDev &g, const uint32_t *mask, int cap, uint8_t *rowd, int16_t *field, hipStream_t s);
hipError_t launch_match(MatchArgs a, hipStream_t s);

// ---- refinement of a scan-to-map pose below the cell (refine_kernels.hip, include/slam_refine.h) ----
struct RefineArgs {
    GridDev g;
    const int16_t *field = nullptr;          // [G][xw][yw] (launch_distance_field at the same cap)
    const float *ranges = nullptr;           // [B][n], or one [n] with range_stride 0
    long range_stride = 0;
    const double *poses = nullptr;           // [B][3]
    const int32_t *maps = nullptr;           // nullable [B]: the map of every hypothesis (an entry outside [0, G): SLAM_REFINE_NO_MAP)
    const double *cos_t = nullptr, *sin_t = nullptr;
    int B = 0, n = 0, iters = 0;
    double damping = 0.0;
    double step_xy = 0.0, step_rad = 0.0;    // the clamps of a step: step_cells / scale metres, radians
    float max_range = 0.f;
    int cap = 0;
    double *pose_out = nullptr;              // [B][3]
    double *cost_out = nullptr;              // [B][2]
    int32_t *used_out = nullptr;             // nullable [B]
    double *normal_out = nullptr;            // nullable [B][9]
    int32_t *status_out = nullptr;           // [B]
};
hipError_t launch_refine(const RefineArgs &a, hipStream_t s);

// ---- the scan-to-map tracker's steps around the matcher, the refinement and the cast (track_kernels.hip, include/slam_track.h) ----
// Everything but the caller's arrays is workspace of slam_track_dev, [L] rows each, rewritten for every scan.
struct TrackArgs {
    const float *ranges = nullptr;           // [L][S][n]
    const double *motion = nullptr;          // nullable [L][S][3]
    const double *rot_off = nullptr;         // [K]
    const double *rot_off_cs = nullptr;      // [K][2]
    int L = 0, S = 0, n = 0, K = 0, nx = 0, ny = 0;
    double step = 0.0;
    int min_used = 1, map0 = 0;
    double gate_dist = 0.0, gate_turn = 0.0;
    double scale = 0.0, off_x = 0.0, off_y = 0.0;            // the grid's index rule
    double *state = nullptr;                 // [L][8], in and out
    double *poses_out = nullptr;             // [L][S][3]
    int32_t *info_out = nullptr;             // [L][S][4]
    double *trace_out = nullptr;             // nullable [L][S][13]
    float *scan = nullptr;                   // [L][n]: this scan's rows
    double *pred = nullptr;                  // [L][5]: pred, c0, s0
    double *centres = nullptr;               // [L][2]      the matcher's inputs ...
    double *rot_cs = nullptr;                // [L][K][2]
    int32_t *match_maps = nullptr;           // [L]: map0 + l, or -1 for a first scan
    unsigned long long *keys = nullptr;      // [L]
    int32_t *best = nullptr, *best_cost = nullptr, *used = nullptr;      // ... and its outputs
    double *start = nullptr;                 // [L][3]      the refinement's start poses (the matched poses) ...
    int32_t *refine_maps = nullptr;          // [L]: map0 + l, or -1 where nothing is refined
    double *refined = nullptr, *refine_cost = nullptr;       // [L][3], [L][2]: ... and its outputs
    int32_t *refine_status = nullptr;        // [L]
    int32_t *acc = nullptr;                  // [L]: the cast's skip marks (SLAM_MCL_DEAD: not integrated)
    double *cast_pose = nullptr;             // [L][3]: the pose each scan is cast from
};
hipError_t launch_track_predict(const TrackArgs &a, int s, hipStream_t st);
hipError_t launch_track_seed(const TrackArgs &a, hipStream_t st);
hipError_t launch_track_decide(const TrackArgs &a, int s, hipStream_t st);

// ---- global scan localisation on a pyramid of the field (locate_kernels.hip) --------------
// Level h of the pyramid: P_h[x][y] for -pad <= x < xw, -pad <= y < yw (pad = 2^h - 1) at base[(gi * X + x + pad) * Y + y + pad];
// cap everywhere else.  Level 0 is the field itself.
struct LocateLevel {
    const int16_t *base = nullptr;
    int pad = 0, X = 0, Y = 0;
};
struct LocateArgs {
    GridDev g;
    LocateLevel lvl[kLocateMaxLevels + 1];
    const float *ranges = nullptr;           // [B][n], or one [n] with range_stride 0
    long range_stride = 0;
    const int32_t *maps = nullptr;           // nullable [B]
    const double *cos_t = nullptr, *sin_t = nullptr;
    const double *rot_cs = nullptr;          // [K][2]
    const int32_t *region = nullptr;         // nullable [B][4]
    int B = 0, n = 0, K = 0, H = 0;
    int max_ni = 0, max_nj = 0;              // what the lists were sized for: a larger region makes its hypothesis invalid
    float max_range = 0.f;
    int cap = 0;
    // workspace, per hypothesis
    unsigned long long *key_top = nullptr;   // [B] 0xff on entry: min of (LB << 32 | node index) over the level-H nodes
    unsigned long long *key_leaf = nullptr;  // [B] 0xff on entry: min of (cost << 32 | flat) over the sweep's level-0 survivors
    int32_t *bound = nullptr;                // [B] U, written by the descent
    int32_t *used = nullptr;                 // [B] used beams, -1: the hypothesis names no map / no region
    unsigned long long *evaluated = nullptr; // [B][H + 1] zero on entry: nodes evaluated per level below H
    // workspace, per chunk of pairs
    int32_t *list[kLocateMaxLevels + 1] = {nullptr};   // [h]: [list_cap[h]][2] survivors of level h: pair, I * nJ_h + J
    long list_cap[kLocateMaxLevels + 1] = {0};
    unsigned *list_len = nullptr;            // [kLocateMaxLevels + 1] zero at the start of a chunk
    int32_t *table = nullptr;                // [chunk pairs][n][2] (ax, ay) of a pair's used beams that are on, packed to the front
    int32_t *table_cnt = nullptr;            // [chunk pairs][2] how many of them, and how many used beams are off
    int32_t *best_out = nullptr, *best_cost_out = nullptr, *used_out = nullptr;   // [B][3], [B], nullable [B]
    int64_t *stats_out = nullptr;            // nullable [B][H + 2]
};
size_t locate_pyramid_cells(const GridDev &g, int H);   // int16 cells of levels 1 .. H of all G maps
// pyr: locate_pyramid_cells(g, H) int16; fills a.lvl[0 .. H] and builds levels 1 .. H from `field`
hipError_t launch_locate_pyramid(LocateArgs &a, const int16_t *field, int16_t *pyr, hipStream_t s);
// the whole search on a built pyramid: top level, descent, sweep in chunks of pairs, finish
hipError_t launch_locate(const LocateArgs &a, const LocateShape &p, hipStream_t s);

// ---- map frontiers: clustered exploration goals (frontier_kernels.hip) --------------------
// The label word of a cell (workspace, [chunk][xw][yw] int32) through the phases:
//   -1            not a frontier cell
//   v >= 0        a frontier cell whose parent (after k_frontier_flatten: whose root) is flat cell v of its query
//   v <= -2       a root, from k_frontier_flatten on: -(size + 1) until k_frontier_rank, then -(row + 2) for a cluster
//                 with a row in the table and kFrontierNoRow for one without (too small, or behind max_clusters)
constexpr int32_t kFrontierNoRow = INT32_MIN;
struct FrontierArgs {
    GridDev g;
    const int16_t *field = nullptr;          // [G][xw][yw] when min_clear2 > 0
    const int32_t *maps = nullptr;           // nullable [B]: NULL = query b reads map b
    int B = 0, radius = 0, min_unknown = 0, min_clear2 = 0, min_size = 0, M = 0;
    int32_t *lab = nullptr;                  // workspace [chunk queries][xw * yw]
    int32_t *seg = nullptr;                  // workspace [chunk queries][segs][2]: kept roots, frontier cells of a segment
    int32_t *count_out = nullptr;            // [B][2]
    int32_t *clusters_out = nullptr;         // [B][M][8], nullable when M == 0
    int64_t *sums_out = nullptr;             // [B][M][2], nullable when M == 0
    int32_t *labels_out = nullptr;           // nullable [B][xw][yw]
};
// every phase of queries b0 .. b0 + nb - 1 (nb <= p.chunk_queries), enqueued on s
hipError_t launch_frontiers(const FrontierArgs &a, const FrontierShape &p, long b0, long nb, hipStream_t s);

// ---- travel-cost field: reachable cells, costs and paths (travel_kernels.hip) --------------
// A cost word through the phases: kTravelUnreached until a source reaches the cell, then the least cost found so far
// (only ever lowered); k_travel_finish turns what is left of kTravelUnreached into -1.
constexpr int32_t kTravelUnreached = 0x3fffffff;     // + kTravelDiagonal does not overflow
constexpr int32_t kTravelClean = INT32_MAX;          // the pending key of a tile that is not dirty
struct TravelArgs {
    GridDev g;
    const int16_t *field = nullptr;          // [G][xw][yw] when min_clear2 > 0
    const int32_t *maps = nullptr;           // nullable [B]: NULL = query b reads map b
    const int32_t *sources = nullptr;        // [B][S][2]
    const int32_t *goals = nullptr;          // nullable [B][Q][2]
    int B = 0, S = 0, foot = 0, through_unknown = 0, min_clear2 = 0, Q = 0, path_cap = 0;
    int32_t *ws_cost = nullptr;              // workspace [chunk queries][xw * yw] when cost_out is NULL
    unsigned long long *mask = nullptr;      // workspace [chunk queries][xw][tiles_y]: bit y % 64 of word y / 64 of row x
    int32_t *dirty = nullptr;                // workspace [chunk queries][tiles]: the pending key, kTravelClean for none
    int32_t *status_out = nullptr;           // [B]
    int32_t *cost_out = nullptr;             // nullable [B][xw][yw]: the relaxation runs in it
    int8_t *dir_out = nullptr;               // nullable [B][xw][yw]
    int32_t *goal_cost_out = nullptr;        // [B][Q] with goals
    int32_t *path_len_out = nullptr;         // [B][Q] with goals
    int32_t *path_out = nullptr;             // [B][Q][path_cap][2], nullable when path_cap == 0
};
// every phase of queries b0 .. b0 + nb - 1 (nb <= p.chunk_queries), enqueued on s
hipError_t launch_travel(const TravelArgs &a, const TravelShape &p, long b0, long nb, hipStream_t s);

// ---- Monte Carlo localisation on the distance field (mcl_kernels.hip) ---------------------
constexpr int kMclScanBlock = 1024;          // particles per workgroup of the prefix sum: fixed, so a filter's sums do not depend on the batch
inline int mcl_scan_blocks(int P) { return (P + kMclScanBlock - 1) / kMclScanBlock; }
struct MclWeighArgs {
    GridDev g;
    const int16_t *field = nullptr;          // [G][xw][yw] (launch_distance_field)
    double *poses = nullptr;                 // [F][P][3], moved in place when motion is given
    const double *motion = nullptr;          // nullable [F][3]
    const double *noise = nullptr;           // nullable [F][P][3]
    const float *ranges = nullptr;           // [F][n]
    const double *cos_t = nullptr, *sin_t = nullptr;
    const int32_t *maps = nullptr;           // nullable [F]: the map of every filter (an entry outside [0, G): every particle dead)
    int own_maps = 0;                        // 1 (slam_mcl_weigh_maps): a map per PARTICLE, pmaps[f][p] or, pmaps null, map f * P + p
    const int32_t *pmaps = nullptr;          // nullable [F][P] (own_maps only; an entry outside [0, G): that particle dead)
    int F = 0, P = 0, n = 0;
    float max_range = 0.f;
    int cap = 0;
    int32_t *acc = nullptr;                  // nullable [F][P]
    int32_t *cost_out = nullptr;             // nullable [F][P]
    int32_t *used_out = nullptr;             // nullable [F]
    int chunks = 1;                          // set by launch_mcl_weigh: workgroups per filter
};
struct MclResampleArgs {
    const double *poses = nullptr;           // [F][P][3]
    int32_t *acc = nullptr;                  // [F][P]
    const uint32_t *table = nullptr;         // [T]
    int T = 0, shift = 0;
    const double *u0 = nullptr;              // [F]
    double ess_frac = 0.0;
    int F = 0, P = 0;
    double *poses_out = nullptr;             // [F][P][3]
    int32_t *ancestors_out = nullptr;        // nullable [F][P]
    double *est_out = nullptr;               // [F][4]
    int32_t *info_out = nullptr;             // [F][4]
    // workspace, nblk = mcl_scan_blocks(P):
    unsigned long long *keys = nullptr;      // [F], every byte 0xff on entry: min of (acc, index) over the live particles
    int32_t *live = nullptr;                 // [F], zero on entry
    unsigned long long *cum = nullptr;       // [F][P] inclusive prefix sums of the weights within each scan block
    unsigned long long *bsum = nullptr;      // [F][nblk] block sums, then their exclusive scan
    unsigned long long *bq = nullptr;        // [F][nblk] block sums of squares
    double *bpart = nullptr;                 // [F][nblk][4] block sums of w x, w y, w sin, w cos
    unsigned long long *fpar = nullptr;      // [F][2]: S if the filter resamples else 0, and the offset o
    int nblk = 1;                            // set by launch_mcl_resample
};
// shape: the context option "mcl_shape" (-1: by beam count, 0: lanes over particles, 1: a wave per particle)
hipError_t launch_mcl_weigh(MclWeighArgs a, int shape, hipStream_t s);
hipError_t launch_mcl_resample(MclResampleArgs a, hipStream_t s);
constexpr int kMclSettleMaxP = 4096;         // three int arrays of P in LDS: 48 KiB
// slam_mcl_settle: every surviving particle keeps its slot; every output but settled is nullable
struct MclSettleArgs {
    const int32_t *ancestors = nullptr;      // [F][P]; an entry outside [0, P) is clamped into it
    const double *poses_src = nullptr;       // nullable [F][P][3]
    int F = 0, P = 0, map0 = 0;
    int32_t *settled = nullptr;              // [F][P]
    double *poses_out = nullptr;             // [F][P][3]
    int32_t *map_src = nullptr;              // [F][P]
    int32_t *moved = nullptr;                // [F]
    int *status = nullptr;
};
hipError_t launch_mcl_settle(const MclSettleArgs &a, hipStream_t s);

// ---- scan-to-map observation ---------------------------------------
hipError_t launch_map_obstacles(const int8_t *map, int width, int height, int wire, double resolution, double origin_x,
                                double origin_y, double *ox, double *oy, int cap, int *count, hipStream_t s);
hipError_t launch_virtual_scan(const double *ox, const double *oy, int K, const double *poses, int B, double angle_min,
                               double angle_increment, int n, double *ranges, hipStream_t s);
hipError_t launch_ranges64_to_points(const double *ranges, const double *cos_t, const double *sin_t, int B, int n,
                                     double *pts, hipStream_t s);

// ---- batched W9 node (Localization.laserCallback, W9/localization.py:66-126; localization_kernels.hip) ----
constexpr int kLocMaxBeams = 4096;           // beam bins of a trajectory in LDS (8 B each)
constexpr int kLocStateDoubles = 16;         // per trajectory: xEst[3], xOdom[3], PEst[9], status
struct LocArgs {
    int L, S, M, n, n_scan;
    int step;                                // the step whose virtual scan and source this call prepares; it finishes step - 1
    int body;                                // 0: the last call, which only finishes step n_scan - 1
    const float *ranges;                     // [S][n_scan][n]
    const int32_t *stream_of_traj, *map_of_traj;   // nullable [L]
    const double *ox, *oy;                   // [K] every map's obstacles, concatenated
    const int64_t *obs_off;                  // [M + 1], clamped to [0, K]
    long K;
    const double *pose0;                     // nullable [L][3]
    const double *cos_t, *sin_t;
    double angle_min, angle_increment;
    const double *T_stream;                  // [S][2 n_scan - 1][9]: T2 of step s at s, T1 of step s >= 1 at n_scan + s - 1
    const double *T_step;                    // [L][9] what the scan matcher made of the pair this kernel prepared last
    const int32_t *iters_step;               // [L]
    double *state;                           // [L][kLocStateDoubles]
    double *tar_pts, *src_pts;               // [L][2][n] the pair of the scan matcher launch that follows
    double *xest_out, *xodom_out;            // [L][n_scan][3]
    double *P_final_out;                     // [L][9]
    int32_t *status_out;                     // [L] SLAM_LOC_*
    double *T_obs_out, *T_odom_out;          // nullable [L][n_scan][9]
    int32_t *iters_obs_out;                  // nullable [L][n_scan]
    double *tar_pts_out;                     // nullable [L][n_scan][2][n]
    int *status;
};
hipError_t launch_loc_step(const LocArgs &a, hipStream_t s);
// the pairs of the stream-only solves as point sets: pairs [S][2 n_scan - 1][2][2][n] (target, then source)
hipError_t launch_loc_stream_pairs(const float *ranges, const double *cos_t, const double *sin_t, int S, int n_scan, int n,
                                   double *pairs, hipStream_t s);

// ---- DWA local planner (dwa_kernels.hip) ----------------------------------------------
// The fields of SLAM_DWA_CONFIG_LEN in the order include/slam_hip.h documents (dwa.py:23-45).
struct DwaConfig {
    double max_speed, min_speed, max_yawrate, max_accel, max_dyawrate, dt, v_reso, yawrate_reso, predict_time,
        to_goal_cost_gain, speed_cost_gain, obstacle_cost_gain, robot_type, robot_radius, robot_width, robot_length;
};
constexpr int kDwaTile = 4096;               // obstacles staged in LDS at a time (16 B each)
constexpr int kDwaMaxBeams = kDwaTile - 1;   // scans form: the sentinel and every beam fit one tile
constexpr long kDwaMaxGroups = 1L << 20;     // workgroups per launch; more planners are taken grid-stride
struct DwaArgs {
    const double *states, *goals;            // [B][5], [B][2]
    // explicit obstacles: [.][2][M] (x row, then y row), ob_stride doubles between planners (0: one shared set);
    // counts nullable ([.] with count_stride 0 or 1): planner b uses min(counts[b], M) of them
    const double *obs = nullptr;
    long ob_stride = 0;
    int M = 0;
    const int32_t *counts = nullptr;
    long count_stride = 0;
    // scans form (ranges != nullptr): [.][n] float32, scan_stride floats between planners (0: shared)
    const float *ranges = nullptr;
    const double *cos_t = nullptr, *sin_t = nullptr;
    long scan_stride = 0;
    int n = 0;
    double threshold = 0.0;
    long B = 0;
    int rows = 0;                            // trajectory rows: 1 + the passes of the predict_time loop
    int nv_cap = 0, nw_cap = 0;              // bound on the sample axes for this config (slam_dwa_shape)
    int tile_cap = 0;                        // obstacles per LDS tile
    DwaConfig cfg;
    double *u_out, *cost_out;                // [B][2], [B]
    int32_t *index_out;                      // [B]
    int32_t *counts_out = nullptr;           // nullable [B][2]
    double *costs_out = nullptr;             // nullable [B][s_cap]
    int s_cap = 0;
    double *traj_out = nullptr;              // nullable [B][rows][5]
    int *status = nullptr;
};
hipError_t launch_dwa(const DwaArgs &a, hipStream_t s);

// ---- A* global planner (astar_kernels.hip) ----------------------------------------------
constexpr int kAstarMaxSpan = 4096;          // inflated extent: one 64-column word per lane of the row walk
constexpr int kAstarMaxSlots = 4096;         // resident waves of the search (one workspace slot each)
constexpr size_t kAstarSlotBudget = 1ull << 30;   // bytes of search workspace a call may take
// per cell of a slot: state byte, open-list position, entry cell, entry g, closed list (int32 each), entry key
constexpr size_t kAstarSlotBytesPerCell = 1 + 4 * 4 + 8;
struct AstarArgs {
    const int8_t *imaps;                     // inflated row-major maps [G][H][W]
    int G, H, W;
    const int32_t *starts, *goals;           // [B][2] (row, col) before find_path's -1
    const int32_t *map_of_query;             // nullable [B]; NULL: map 0 (G == 1) or map b (G == B)
    long B;
    int path_cap;
    int32_t *status, *path_len, *path, *expansions;   // [B], [B], [B][path_cap][2], [B]
    // workspace: `slots` slots of H * W cells each; state bytes zero on entry
    int slots;
    uint8_t *state;
    int32_t *pos, *ocell, *og, *closed;
    unsigned long long *okey;
};
// dil: workspace [G][span][(span + 63) / 64] words; out: inflated row-major maps [G][H][W]
hipError_t launch_astar_inflate(const int8_t *maps, int G, int H, int W, int wire, int span, int r,
                                unsigned long long *dil, int8_t *out, int *status, hipStream_t s);
hipError_t launch_astar(const AstarArgs &a, hipStream_t s);

// ---- landmark extraction, landmark EKF and the node's kept scans (landmark_kernels.hip) ------
constexpr int kLandmarkMaxBeams = 4096;      // a scan's points and its four index arrays fit LDS (32 B per beam)
constexpr int kEkfMaxLm = 32;                // 67 x 67 covariance and its per-step copy: 75 KiB of LDS
constexpr long kLandmarkMaxGroups = 1L << 20;   // workgroups per launch; more scans / trajectories are taken grid-stride
struct LandmarkArgs {
    const float *ranges;                     // [S][n]
    const double *cos_t, *sin_t;             // [n]
    long S;
    int n;
    double range_threshold, radius_max_th;
    int lm_cap;
    int32_t *count, *overflow, *ids;         // [S], [S], [S][lm_cap]
    double *means, *z;                       // [S][lm_cap][2] each
    int32_t *labels;                         // nullable [S][n-1]
    int *status;
};
struct EkfArgs {
    long B;
    int steps_max, max_lm;
    const double *x0;                        // nullable [B][3]
    const int32_t *steps;                    // [B]; the trajectory runs steps[b] - steps_bias steps, clamped to [0, steps_max]
    int steps_bias;
    const double *u;                         // [B][steps_max][3], or null: taken from T [B][steps_max][9] (T2u)
    const double *T;
    const double *z;                         // observation rows (range, bearing)
    // rows of step (b, s): z_off[b * steps_max + s] .. z_off[.. + 1], clamped to [0, nz] ...
    const int64_t *z_off;
    long nz;
    // ... or (kept != null) the lm_count[scan] rows from scan * lm_cap on, scan = b * (steps_max + 1) + kept[b][s + 1]
    const int32_t *kept, *lm_count, *lm_overflow;
    int lm_cap;
    double *x_out, *P_out;                   // [B][N], [B][N][N], N = 3 + 2 max_lm, zero beyond the state
    int32_t *nlm_hist;                       // [B][steps_max], -1 for steps that did not happen
    int32_t *status_out;                     // [B] SLAM_NODE_*
    int32_t *nlm_out;                        // nullable [B]
    double *x_hist;                          // nullable [B][steps_max][3], NaN for steps that did not happen
    double *cast_poses;                      // nullable [B][steps_max][3], (inf, 0, 0) for steps that did not happen
    int *status;
};
size_t landmark_lds_bytes(int n);
size_t ekf_lds_bytes(int max_lm);
hipError_t launch_landmarks(const LandmarkArgs &a, hipStream_t s);
hipError_t launch_ekf_lm(const EkfArgs &a, hipStream_t s);
hipError_t launch_node_keep(const int32_t *lm_count, int L, int n_scan, int32_t *kept, int32_t *kept_count, hipStream_t s);
hipError_t launch_node_gather(const float *ranges, const int32_t *kept, const int32_t *kept_count, int L, int n_scan, int n,
                              float *out, hipStream_t s);

}  // namespace slam
