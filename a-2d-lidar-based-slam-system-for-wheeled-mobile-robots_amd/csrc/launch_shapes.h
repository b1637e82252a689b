// Launch shapes of the LDS-window ray cast (grid_kernels.hip) and of the scan matcher (icp_kernels.hip): the constants, the
// LDS size functions the kernels carve their regions by, and the two planners that decide a launch.  Plain C++17, no HIP
// header: a planner is a pure function of its request - no device call, no global state - so the launchers (launch_win,
// launch_icp_t), the introspection entries of the C ABI (slam_plan_win, slam_plan_win_phases, slam_plan_icp, slam_plan_query) and the tests
// all ask the same code.  Every function that counts guard bytes takes them as a parameter (default: this build's), so
// that one build answers for the shipped and for the LDS-guard build alike.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#if defined(__HIPCC__)
#define SLAM_HD __host__ __device__
#else
#define SLAM_HD
#endif

namespace slam {

constexpr int kWave = 64;
constexpr int kMaxWaves = 16;            // 1024-thread workgroups

// Debug build (-DSLAM_LDS_GUARD, `make guard`): every kernel with dynamic LDS gets kLdsGuard
// extra bytes behind its last region, fills them with a pattern and checks them before it
// exits; a changed word raises kStatusGuard (SLAM_ERR_HIP from slam_check_status).  GPU
// AddressSanitizer is not available on the target pool; this catches the overrun class that
// matters here (a region sized too small, e.g. a window row count rounded the wrong way).
#ifdef SLAM_LDS_GUARD
constexpr int kLdsGuard = 512;
#else
constexpr int kLdsGuard = 0;
#endif

constexpr size_t kLdsPerCu = 160 * 1024;     // LDS of a CU of gfx950: a workgroup may ask for all of it, a launch that asks for more fails
constexpr size_t kLdsDefault = 64 * 1024;    // what a kernel gets without hipFuncSetAttribute(MaxDynamicSharedMemorySize)
constexpr int kChipCus = 256;                // MI355X, should the device query fail

// sizes of what the kernels keep in LDS (each asserted next to its struct or use)
constexpr size_t kScanConstBytes = 48;       // sizeof(ScanConst): four doubles, four ints
constexpr size_t kDouble2Bytes = 16;         // sizeof(double2)
constexpr size_t kFloat2Bytes = 8;           // sizeof(float2)
constexpr size_t kBoxBytes = 32;             // sizeof(Box): four doubles
constexpr size_t kListSlotBytes = kDouble2Bytes + sizeof(int);   // a slot of the first-iteration list (nn_listed): double2 + int

// ---------------------------------------------------------------------------------
// LDS-window ray cast
// ---------------------------------------------------------------------------------
constexpr int kWinCells = 36864;     // 16-bit cells: 72 KiB of LDS
constexpr int kWinMaxGroup = 64;     // scans per workgroup
constexpr int kSortBins = 128;        // ray-length histogram (4 cells per bin)
constexpr int kMaxSortRays = 8192;    // rays per workgroup that can be length-sorted (u16 ids in LDS)
static_assert(kMaxSortRays <= 0xffff, "flush_hits counts a sorted phase's hits in 16-bit window cells: one count per ray at most");
constexpr int kRaysPerLane = 4;     // lanes per workgroup = rays / kRaysPerLane (rays are dealt to waves dynamically)
constexpr unsigned kNoHit = 0xffffu; // a slot of the sorted order without a hit for flush_hits (cast_rays): a window index must stay below it
constexpr int kWinBoxInts = 160;     // ints of LDS set aside for the control block
// the window takes most of a CU's LDS, so a CU runs one or two workgroups: the flush / the
// exclusive sweep (a streaming pass over the touched rectangle) need lanes for memory
// operations in flight even when there are few rays (measured on 10 000 single-scan groups:
// 2.88 ms with 128 threads, 2.05 ms with 512)
constexpr int kWinMinThreads = 512;

// single-scan owner forms (k_grid_update_owner, k_grid_update_owner8): what the decision reads of them
constexpr int kOwnerThreads = 512;   // 8 waves: two workgroups per CU at up to 128 VGPRs
constexpr int kOwnerMaxRays = 2;                    // rays per lane (template parameter: 1 up to 512 beams)
constexpr int kOwnerRedoMaxGrid = 256;              // workgroups of the re-do launch behind the byte-window kernel
constexpr int kOwn8Bins = 128;
constexpr int kOwn8BoxInts = 16;
constexpr int kOwn8Threads = 384;       // >= kOwn8Bins, a multiple of 64: six waves, one ray per lane up to 384 beams
// LDS of a workgroup: half a CU's 160 KiB.  (Three workgroups per CU with 52.5 KiB each - the benchmark scan's box just fit -
// were measured no faster: the kernel goes at the pace of the memory system, not of the workgroups in flight.)
constexpr int kOwn8LdsBytes = 81920;
SLAM_HD inline size_t own8_fixed_bytes(int threads) { return (size_t)(kOwn8BoxInts + kOwn8Bins) * 4 + (size_t)threads * 4; }

SLAM_HD inline size_t win_sc_bytes(int group) { return ((size_t)group * kScanConstBytes + 15) & ~(size_t)15; }
SLAM_HD inline int win_sort_cap(long rays) { return rays <= kMaxSortRays ? (int)((rays + 7) & ~7L) : 0; }   // 16-byte multiple
SLAM_HD inline size_t win_lds_bytes(int group, int sort_cap, int win_cells, int guard = kLdsGuard)
{
    return win_sc_bytes(group) + kWinBoxInts * 4 + 4 * kSortBins * 4 + (size_t)sort_cap * 2 + (size_t)win_cells * 2 + guard;
}
// Window capacity (16-bit cells) of a launch: kWinCells, or, for small groups, whatever still lets two
// workgroups share a CU's 160 KiB (a single 360-beam scan: 40 288 cells instead of 36 864 - the
// bounding box of a scan of the 10 m x 8 m benchmark room, padded to 16-cell pieces, is 35-37 k cells)
// two_per_cu (plan_win: a shared-map launch of sorted rays with more workgroups than the chip has CUs): the same carving even
// where it comes out BELOW kWinCells, so that two workgroups are resident on a CU - one walks while the other sorts, zeroes or
// flushes.  A group of 16 scans of 360 beams gets 33 216 cells (measured, profiles/win_two_per_cu.txt: one workgroup resident
// per CU before, two now; the 32-trajectory launch 0.736 -> 0.705 ms).
// The floor: a smaller window costs phases (more groups whose halves no longer fit), and below some size that must cost more
// than the second resident gains.  Measured at the largest sorted groups of 360 beams, 20 and 22 scans (31 680 and 30 912 cells;
// 24 x 360 is 8 640 rays, not sorted, and keeps its window anyway): 0.776 -> 0.688 and 0.723 -> 0.668 ms, MORE than group 16
// gains, and with one resident a window of 30 720 cells cost 1 %, of 24 576 cells 8 %.  Nothing measured argues for a floor
// above the smallest window the carving can ask for at all - 8 192 sorted rays in 64 scans: 29 632 cells -, so that is the floor;
// it is also what keeps the window large enough for the 16-bit keys pass 1 parks in it.
constexpr int kWinHalfSlack = 512;                                   // a little room for allocation granules
constexpr int kWinTwoFloor = 29632;
SLAM_HD inline int win_cells_for(int group, int sort_cap, bool two_per_cu = false, long lds_per_cu = (long)kLdsPerCu, int guard = kLdsGuard)
{
    const long half = lds_per_cu / 2 - kWinHalfSlack;
    long other = (long)win_lds_bytes(group, sort_cap, 0, guard);
    long cells = ((half - other) / 2) & ~15L;
    if (cells > kWinCells) return (int)cells;
    return two_per_cu && cells >= kWinTwoFloor ? (int)cells : kWinCells;
}
static_assert(kWinTwoFloor >= kMaxSortRays && kWinTwoFloor % 16 == 0, "pass 1 parks a 16-bit key per sorted ray in the window");

// group == 0: automatic.  Measured on the 1k-scan replay (profiles/r01_*): the kernel is
// fastest with about one workgroup per two CUs (8 scans each); more, smaller groups re-flush
// the same map region more often, fewer leave CUs idle.
inline int pick_group(int group, long total_scans, int scans_per_traj, int n)
{
    int gmax = std::min(kWinMaxGroup, 65535 / std::max(n, 1));
    if (gmax < 1) return 0;                                          // n too large for the packed counters
    if (group <= 0) {
        long want = (total_scans + 127) / 128;
        group = (int)std::min<long>(std::max<long>(want, 1), 12);   // (5 000-scan replays, four overlapping: 12 -> 9.3, 16 -> 8.9 M scans/s)
    }
    group = std::min(std::min(group, gmax), std::max(scans_per_traj, 1));
    return group;
}

// Which kernel casts a launch (the table in the header of grid_kernels.hip's window section; first match wins)
enum WinForm : int {
    kWinFormWin = 0,                 // k_grid_update_win: a map that other workgroups write too
    kWinFormOwn = 1,                 // k_grid_update_own: the map's only writer
    kWinFormOwner1 = 2,              // k_grid_update_owner<1>: one scan, one ray per lane
    kWinFormOwner2 = 3,              // k_grid_update_owner<2>: one scan, two rays per lane
    kWinFormOwner8ThenRedo = 4,      // k_grid_update_owner8, then k_grid_update_owner_redo<1> for what it left
};

struct WinRequest {
    int L, scans, n, group;          // streams, scans per stream, beams per scan, scans per workgroup (pick_group)
    bool has_got;                    // the caller names each stream's map (`got`)
    bool pmap_live, maps_are_private;
    int hit_levels, xw, yw;
    bool has_redo;                   // the grid has a re-do list
    int split_pref = -1, hits_pref = -1;   // context options "grid_split" and "win_lds_hits": -1 = the library's choice
    int cus = kChipCus;
    long lds_per_cu = (long)kLdsPerCu;
    int guard = kLdsGuard;
};

struct WinShape {
    int form;                        // WinForm
    int grid_x, grid_y, threads;
    size_t lds;                      // dynamic LDS of the launch
    size_t lds_attr;                 // LDS size to allow by attribute; 0: the standing one (win_lds_max) is enough
    int exclusive, sort_cap, win_cells, split, lds_hits;
    int two_per_cu;                  // the window was carved for two workgroups per CU
    long wgs;                        // workgroups of the launch (0 for the single-scan owner forms: not counted there)
    int own8_lds, own8_win;          // kWinFormOwner8ThenRedo: dynamic LDS and window bytes of the byte-window kernel ...
    int redo_grid;                   // ... and the grid of the re-do launch behind it (which takes threads, lds, sort_cap, win_cells)
    bool live_dirty;                 // the live pmap no longer follows the counters
};

// the LDS size every window kernel is allowed from its first launch on
SLAM_HD inline size_t win_lds_max(int guard = kLdsGuard) { return win_lds_bytes(kWinMaxGroup, kMaxSortRays, kWinCells, guard); }

inline WinShape plan_win(const WinRequest &r)
{
    WinShape p{};
    const size_t lds_max = win_lds_max(r.guard);
    int groups = (r.scans + r.group - 1) / r.group;
    long rays = (long)r.group * r.n;
    long want = (rays + kRaysPerLane - 1) / kRaysPerLane;
    int threads = want >= kMaxWaves * kWave ? kMaxWaves * kWave : (int)(((want + kWave - 1) / kWave) * kWave);
    if (threads < 128) threads = 128;
    // one workgroup per map and no other writer: single stream (L == 1) or one map per stream
    const int exclusive = r.pmap_live && groups == 1 && !r.has_got && (r.L == 1 || r.maps_are_private);
    p.live_dirty = r.pmap_live && !exclusive;
    if (threads < kWinMinThreads) threads = kWinMinThreads;
    const int sort_cap = win_sort_cap((long)r.group * r.n);
    const int own_cells = win_cells_for(r.group, sort_cap, false, (long)kLdsPerCu, r.guard);   // every launch but the chip-filling shared-map one below
    p.exclusive = exclusive; p.sort_cap = sort_cap;
    // one scan per map, cast by the map's only writer, live pmap, the reference's one-hit-occupies rule
    if (exclusive && r.group == 1 && r.scans == 1 && r.hit_levels == 1 && (r.yw & 15) == 0 && (((size_t)r.xw * r.yw) & 3) == 0 &&
        r.yw <= own_cells && r.n <= kOwnerMaxRays * kOwnerThreads) {
        p.win_cells = own_cells;
        p.lds = win_lds_bytes(1, sort_cap, p.win_cells, r.guard);
        p.grid_x = 1; p.grid_y = r.L; p.threads = kOwnerThreads;
        // the plain case (all of a closed room's scans) goes through the byte-window kernel, three workgroups per CU;
        // whatever it leaves on the re-do list is cast by the general kernel behind it
        if (r.has_redo && r.n <= kOwn8Threads && r.n <= kOwnerThreads && r.xw <= 65535 && r.yw <= 65535 && (long)r.xw * r.yw < (1L << 29)) {
            p.form = kWinFormOwner8ThenRedo;
            p.own8_lds = kOwn8LdsBytes + r.guard; p.own8_win = (int)(kOwn8LdsBytes - own8_fixed_bytes(kOwn8Threads));
            p.redo_grid = std::min(r.L, kOwnerRedoMaxGrid);
        } else
            p.form = r.n <= kOwnerThreads ? kWinFormOwner1 : kWinFormOwner2;
        return p;
    }
    // Two workgroups per group where the rays are sorted and the map is not the workgroup's own - a group whose box fits one
    // window is shared by beam parity, else one workgroup takes the rays right of the origins' column and one those left of it
    // (k_grid_update_win): a launch that cannot fill the chip on its own (a 1 000-scan replay is 125 groups on 256 CUs) runs
    // 11 % shorter that way (0.088 -> 0.078 ms); when launches of several contexts share the chip the duplicated first pass
    // costs 4 % of the throughput, so callers that overlap replays switch it off (context option "grid_split")
    const int split = (!exclusive && sort_cap > 0 && (r.split_pref > 0 || (r.split_pref < 0 && (long)groups * r.L <= (3L * r.cus) / 4))) ? 1 : 0;
    // A launch of at most one workgroup per CU asks for more than half a CU's LDS, so that no CU gets two of its workgroups
    // while others stay empty: the dispatcher does not spread a small grid by itself (stamps, round 4: of 250 workgroups on
    // 256 CUs the slowest took 1.8 x the mean with the same number of cells to walk - it shared its CU with another one).
    const long wgs = (long)(split ? 2 * groups : groups) * r.L;
    // A launch of more workgroups than the chip has CUs, on the other hand, wants TWO of them on every CU: one workgroup's phases
    // run one after the other behind barriers, and only a second one can fill the CU while the first sorts, zeroes or flushes.
    // At kWinCells a group of 8 to 16 scans of 360 beams asks for 82 - 89 KB, which is one per CU; such a launch gets the smaller
    // window that leaves room for two (win_cells_for).  Sorted rays only: the unsorted form cannot cut a box that no longer fits.
    const bool two_per_cu = !exclusive && sort_cap > 0 && wgs > r.cus;
    const int win_cells = two_per_cu ? win_cells_for(r.group, sort_cap, true, r.lds_per_cu, r.guard) : own_cells;
    size_t lds = win_lds_bytes(r.group, sort_cap, win_cells, r.guard);
    // (only where a CU's LDS really is more than twice a workgroup's need, and the larger request is one the device grants)
    const size_t half_cu = (size_t)(r.lds_per_cu / 2);
    if (split && wgs <= r.cus && lds <= half_cu && half_cu + 512 <= (size_t)r.lds_per_cu) lds = half_cu + 512;
    // Hits of sorted rays counted in the window, one global add per distinct end cell (flush_hits; a window index must fit 16
    // bits).  Left to the library: in launches of more workgroups than the chip has CUs, like the smaller window - there the
    // launch lasts as long as its memory-side atomics take and the second resident hides flush_hits' two barriers (one-lane
    // benchmark launch 0.705 -> 0.601 ms); a lone replay of 250 workgroups sends a thirtieth of the atomics, has its CU to
    // itself, and was 5 % LONGER with the hits counted (profiles/win_lds_hits.txt).
    const int lds_hits = sort_cap > 0 && win_cells < (int)kNoHit && (r.hits_pref > 0 || (r.hits_pref < 0 && wgs > r.cus)) ? 1 : 0;
    // the map's only writer (then there is one group, and no `got`) finishes its cells itself, pmap included
    p.form = exclusive ? kWinFormOwn : kWinFormWin;
    p.grid_x = split ? 2 * groups : groups; p.grid_y = r.L; p.threads = threads;
    p.lds = lds; p.lds_attr = lds > lds_max ? lds : 0;
    p.win_cells = win_cells; p.split = split; p.lds_hits = lds_hits; p.two_per_cu = two_per_cu ? 1 : 0; p.wgs = wgs;
    return p;
}

// ---- the phases of a shared-map workgroup (k_grid_update_win, one lane, behind pass 1) ----------------------------

SLAM_HD inline int shape_min(int a, int b) { return a < b ? a : b; }
SLAM_HD inline int shape_max(int a, int b) { return a > b ? a : b; }

// o[4] (x0, y0, x1, y1) clamped to the map, its first row moved down to a multiple of ymask + 1 cells (1: the window's
// dwords line up with 8-byte pairs of counters, 3: with the quads of the fused sweep).  False: nothing of it is in the map.
SLAM_HD inline bool clamp_box(int xw, int yw, int *o, int ymask)
{
    o[0] = shape_max(o[0], 0); o[1] = shape_max(o[1], 0); o[2] = shape_min(o[2], xw - 1); o[3] = shape_min(o[3], yw - 1);
    o[1] &= ~ymask;
    return o[0] <= o[2] && o[1] <= o[3];
}
SLAM_HD inline bool box_fits(const int *o, int win_cells)   // (rows are stored padded to an even height)
{
    return (long)(o[2] - o[0] + 1) * ((o[3] - o[1] + 2) & ~1) <= win_cells;
}
// A quadrant's rays lie between the group's origins and the edges of its bounding box on the quadrant's side (every ray
// lies in the box of its two ends): the box of quadrant q from the box of everything, bb, and the extremes of the origins.
// (For a bb that is not empty; with an empty one every quadrant's box stays the empty box.)
SLAM_HD inline void quadrant_boxes(const int *bb, int ox0, int oy0, int ox1, int oy1, int (*qbox)[4])
{
    for (int q = 0; q < 4; ++q) {
        qbox[q][0] = (q & 1) ? shape_max(ox0, bb[0]) : bb[0]; qbox[q][2] = (q & 1) ? bb[2] : shape_min(ox1, bb[2]);
        qbox[q][1] = (q & 2) ? shape_max(oy0, bb[1]) : bb[1]; qbox[q][3] = (q & 2) ? bb[3] : shape_min(oy1, bb[3]);
    }
}
// union of the quadrants in mask -> clamped box; false: empty
SLAM_HD inline bool box_of(const int (*qbox)[4], unsigned mask, int xw, int yw, int ymask, int *o)
{
    o[0] = o[1] = INT32_MAX; o[2] = o[3] = INT32_MIN;
    for (int q = 0; q < 4; ++q) {
        const int *b = qbox[q];
        if ((mask >> q & 1u) && b[0] <= b[2]) { o[0] = shape_min(o[0], b[0]); o[1] = shape_min(o[1], b[1]); o[2] = shape_max(o[2], b[2]); o[3] = shape_max(o[3], b[3]); }
    }
    return clamp_box(xw, yw, o, ymask);
}
// The parts (sets of quadrants) a workgroup casts, one phase each: into part[4] (zeroes on entry), nph (1 on entry) and
// parity (0 on entry).  fits(mask): whether the box of the quadrants in mask fits the window (asked in this order, and
// only when needed).
template <class Fits>
SLAM_HD inline void pick_parts(bool split, int my_half, bool sorted, Fits &&fits, unsigned *part, int &nph, int &parity)
{
    if (split) {
        // Two workgroups per group.  When the group's whole box fits one window, both take that window and share the rays evenly,
        // by beam parity (neighbouring beams are about equally long; the direction halves of a scan taken off-centre differ up to
        // 3 : 1 in cells to walk).  Else a workgroup per direction half, cut again at the origins' row if the half does not fit.
        const unsigned mine = my_half ? 0xAu : 0x5u;             // quadrants right / left of the origins' column
        if (fits(0xFu)) { part[0] = 0xFu; parity = 1; }
        else if (fits(mine)) part[0] = mine;
        else { part[0] = mine & 0x3u; part[1] = mine & 0xCu; nph = 2; }
    } else {
        // One workgroup: the same cuts, decided per direction half - a half that fits is one phase, one that does not is cut
        // at the origins' row: two, three or four phases (a window carved for two workgroups per CU is a tenth smaller, and
        // it is mostly ONE half of a group's box that then no longer fits).
        if (!sorted || fits(0xFu)) part[0] = 0xFu;               // (the quadrants together: the box of everything)
        else {
            const bool left = fits(0x5u), right = fits(0xAu);
            if (left && right) { part[0] = 0x5u; part[1] = 0xAu; nph = 2; }
            else if (left) { part[0] = 0x5u; part[1] = 2u; part[2] = 8u; nph = 3; }
            else if (right) { part[0] = 1u; part[1] = 4u; part[2] = 0xAu; nph = 3; }
            else { part[0] = 1u; part[1] = 2u; part[2] = 4u; part[3] = 8u; nph = 4; }
        }
    }
}

// ---------------------------------------------------------------------------------
// Scan matcher
// ---------------------------------------------------------------------------------
constexpr int kNNBlock = 16;
constexpr int kNNStride = kNNBlock + 1;   // LDS slots per block: the pad spreads the blocks over the banks
constexpr int kPolarTail = 4;                 // NaN points behind the beam-window search's copy of the target
constexpr int kIcpExtraLds = 32;               // flag words: source set collapsed, count of listed queries, re-do
// cross-wave stage of the reductions ([2][nwaves][8] doubles: seven values in the one-pass iteration; 128 B a wave, so
// what follows stays 16-byte aligned) and of the collapsed-set test ([2][nwaves][4]: matched point of the wave's first
// query, "this wave saw another"), two alternating buffers each
constexpr int kRedStride = 8;
constexpr int kWaveQpt = 6;                   // queries per lane of the one-wave shape
constexpr int kWaveRound = 4 * 1024;          // pairs resident at once in this shape: 4 per SIMD, 1 024 SIMDs
constexpr long kIcpFullChipWaves = 7500;      // waves at two queries per lane from which the automatic preference is three
constexpr size_t kIcpWaveFullLds = 10 * 1024; // the automatic one-wave shape: while 16 pairs fit a CU's LDS

// LDS image of the target: float64 (x, y) pairs padded with NaN points to a whole number
// of blocks (NaN never wins a comparison), then one bounding box per block.
SLAM_HD inline int nn_blocks(int n_tar) { return (n_tar + kNNBlock - 1) / kNNBlock; }
SLAM_HD inline int nn_boxes_padded(int n_tar) { return (nn_blocks(n_tar) + 3) / 4 * 4; }   // multiple of 4
SLAM_HD inline int nn_boxes4(int n_tar) { return nn_boxes_padded(n_tar) / 4; }
SLAM_HD inline size_t nn_lds_bytes(int n_tar)
{
    return (size_t)nn_blocks(n_tar) * kNNStride * kDouble2Bytes +
           (size_t)(nn_boxes_padded(n_tar) + nn_boxes4(n_tar)) * kBoxBytes;
}
SLAM_HD inline size_t icp_polar_bytes(int n_tar) { return (size_t)(n_tar + kPolarTail) * kDouble2Bytes; }
SLAM_HD inline size_t icp_red_bytes(int nwaves) { return (size_t)2 * nwaves * (kRedStride + 4) * sizeof(double) + 8 * sizeof(double); }   // + what a pair's first wave hands the others (kLead)
SLAM_HD inline int icp_wave_points(int n_tar)
{
    const int whole = nn_blocks(n_tar) * kNNBlock, tail = n_tar + kPolarTail;
    return whole > tail ? whole : tail;
}
// (f32: the float32 image serves the first iteration too, so it cannot lie over the list as it first did - the list of that
// form is kept in registers instead, a word a query dealt to the lanes by a lane exchange, and takes no LDS.  360 beams:
// 8 768 B with a list of 96 slots of 20 B, 9 792 B with the image of 368 points, 16 pairs a CU either way; image and
// 20-byte slots side by side would be 11 712 B and 13)
SLAM_HD inline size_t icp_wave_lds_bytes(int n_tar, int cap, bool f32)   // (without the guard: the kernel puts it behind)
{
    const size_t behind = f32 ? (size_t)icp_wave_points(n_tar) * kFloat2Bytes : (size_t)cap * kListSlotBytes;
    return (size_t)icp_wave_points(n_tar) * kDouble2Bytes + (size_t)(nn_boxes_padded(n_tar) + nn_boxes4(n_tar)) * kBoxBytes + behind;
}
SLAM_HD inline int icp_block(int n_src, int qpt)
{
    int per = (n_src + qpt - 1) / qpt;
    int blk = ((per + kWave - 1) / kWave) * kWave;
    return blk < kWave ? kWave : blk;
}
// dynamic LDS of a workgroup launch before the unpadded copy and the list
SLAM_HD inline size_t icp_base_lds_bytes(int n_tar, int block, int guard = kLdsGuard)
{
    return nn_lds_bytes(n_tar) + icp_red_bytes(block / kWave) + kIcpExtraLds + guard;
}

enum IcpForm : int {
    kIcpFormInvalid = 0,             // no launch: more LDS than a CU has
    kIcpFormWaveF32 = 1,             // k_icp<T, true>: one wave per pair, float32 pre-filter
    kIcpFormWaveF64 = 2,             // k_icp<T, false>: one wave per pair
    kIcpFormWorkgroup = 3,           // k_icp<T, qpt, unroll>: one workgroup per pair
};

struct IcpRequest {
    int B, n_src, n_tar;
    bool is_scan;                    // the clouds are raw scans (IcpArgs::ranges), not point buffers
    int qpt_pref = 0, batch_invariant = 0, one_wave = -1, f32_filter = -1, team_mode = 0;   // as in IcpArgs
    int guard = kLdsGuard;
};

struct IcpShape {
    int form;                        // IcpForm
    int pref, preferred;             // the preferred queries per lane, and whether they replaced the size-derived ones
    int qpt, unroll, block;          // k_icp<T, qpt, unroll> (the one-wave forms: kWaveQpt, 0, kWave)
    size_t lds;                      // dynamic LDS of the launch
    int polar_copy, team_cap, cap_wanted;   // IcpArgs::polar_copy and ::team_cap; the list before the LDS cuts it
    bool raise_attr;                 // lds is more than a kernel gets by default
    size_t nn_bytes;                 // nn_lds_bytes(n_tar): where the regions behind the padded image start
};

inline IcpShape plan_icp(const IcpRequest &a)
{
    IcpShape p{};
    p.nn_bytes = nn_lds_bytes(a.n_tar);
    int qpt = (a.n_src + 1023) / 1024;
    // Queries per lane for batches (a handful of pairs cannot fill the chip anyway: one query per lane
    // gives the lowest latency, 0.13 instead of 0.15 ms for the drop-in ICP.process call).  Fewer waves per
    // pair repeat the per-iteration fixed work less often: three queries per lane are fastest when
    // the chip is full (10 000 pairs: 0.510 against 0.536 ms; four overlapping 999-pair replays: 6.2
    // against 6.0 M scans/s); a launch that cannot fill the chip on its own runs shorter with two
    // (999 pairs alone: 0.121 against 0.140 ms).  a.qpt_pref: 0 = by batch size, else 1..3.  "Full" goes by the waves the
    // batch would have at two queries per lane: from 7 500 on - 2 500 pairs of 360 beams, 834 pairs of 1 080 (999 such pairs
    // alone: 0.338 ms with three queries per lane against 0.364 with two) - the chip holds them in more than one round.
    const long waves_at_two = (long)a.B * ((a.n_src + 127) / 128);
    // a.batch_invariant (slam_node_replay_dev): the shape must not follow the batch size, so that a trajectory's transforms
    // are the same bits whether it runs alone or among thousands - two queries per lane for every B, never the automatic
    // one-wave shape; an explicit "icp_qpt" / "icp_one_wave" = 1 still holds, for every B alike.
    int pref = a.qpt_pref > 0 ? a.qpt_pref : (a.batch_invariant ? 2 : waves_at_two >= kIcpFullChipWaves ? 3 : 2);
    p.pref = pref;
    if ((a.B > 64 || a.batch_invariant) && qpt < pref && a.n_src > 64 * pref) { qpt = pref; p.preferred = 1; }
    if (qpt > 4) qpt = 8;                     // the shapes that exist: 1, 2, 3, 4, 8 queries per lane
    // One wave per pair with six queries per lane (k_icp<T>): no barriers, the per-iteration fixed work paid once per
    // pair.  For launches that fill the chip several times over on their own, where instructions are time: the preference
    // resolves to the full-chip shape (given or automatic) and the batch is at least FOUR rounds of this shape's own
    // workgroups - 4 resident per SIMD on 1 024 SIMDs, 16 384 pairs.  A launch of a round or two ends on its longest pairs,
    // and a pair is slower alone in this shape (six queries in sequence: 0.28 against 0.20 ms for 999 pairs when it was
    // first tried, in the era of lone launches), so every smaller launch - the particle batches of 10 000 and their chunks
    // among them, which were not measured in this shape - keeps the shape it had.  Measured on the benchmark's launches of
    // 31 968 pairs (7.8 rounds), two contexts: 17.46 against 15.50 M scans/s, a step of 1.831 instead of 2.062 ms
    // (profiles/icp_one_wave.txt).  Automatic only for scans (the box search of a point cloud would read the unpadded image
    // throughout) and while 16 pairs fit a CU's LDS.  a.one_wave: -1 = by this rule, 0 = never, 1 = wherever a pair fits
    // (context option "icp_one_wave").
    {
        const int cap = (a.is_scan && a.team_mode == 0) ? ((a.n_src + 3) / 4 + 15) / 16 * 16 : 0;   // the list: a quarter of the queries (a fifth is listed on the benchmark scans)
        // a.f32_filter: -1 / 1 = the float32 pre-filter of every iteration's beam windows (scans only: a point cloud has no
        // windows), 0 = the float64 scan alone (context option "icp_f32_filter"; no result depends on it)
        const bool f32 = a.f32_filter != 0 && a.is_scan;
        const size_t lds = icp_wave_lds_bytes(a.n_tar, cap, f32) + a.guard;
        const bool fits = a.n_src <= kWave * kWaveQpt && lds <= kLdsDefault;
        const bool full = !a.batch_invariant && pref == 3 && a.B >= 4 * kWaveRound && a.n_src > kWave * 3 && a.is_scan && lds - a.guard <= kIcpWaveFullLds;   // (the shipped layout's size: the debug build's guard does not choose the shape)
        if (fits && (a.one_wave == 1 || (a.one_wave < 0 && full))) {
            p.form = f32 ? kIcpFormWaveF32 : kIcpFormWaveF64;
            p.qpt = kWaveQpt; p.block = kWave; p.lds = lds; p.team_cap = p.cap_wanted = cap;
            return p;
        }
    }
    const int block = icp_block(a.n_src, qpt);
    const size_t lds_base = icp_base_lds_bytes(a.n_tar, block, a.guard);
    // second, unpadded copy of the target for the beam-window search: only for scans, and only while both copies fit
    // (up to 4 557 beams; larger scans, up to the documented 8 192, and point clouds go by the box search alone)
    p.polar_copy = (a.is_scan && lds_base + icp_polar_bytes(a.n_tar) <= kLdsPerCu) ? 1 : 0;
    size_t lds = lds_base + (p.polar_copy ? icp_polar_bytes(a.n_tar) : 0);
    // the list of first-iteration queries without a usable window (nn_listed): room for half of the queries - on the
    // benchmark scans a fifth of them is listed - as far as the CU's LDS goes; a full list leaves the rest to the box search
    p.team_cap = 0;
    if (p.polar_copy && a.team_mode == 0) {
        long cap = ((a.n_src + 1) / 2 + 15) / 16 * 16;
        p.cap_wanted = (int)cap;
        const long room = ((long)kLdsPerCu - (long)lds) / (long)kListSlotBytes;
        cap = cap < room ? cap : room / 16 * 16;
        p.team_cap = cap > 0 ? (int)cap : 0;
    }
    lds += (size_t)p.team_cap * kListSlotBytes;
    p.qpt = qpt; p.block = block; p.lds = lds;
    // (candidates per trip of the beam-window search: see nn_polar.  Four
    // per trip are as fast as two when the chip is full and faster when it is not - four overlapping 999-pair
    // replays 8.5 -> 8.9 M scans/s - since the candidates come from the unpadded copy.)
    p.unroll = qpt <= 3 ? 4 : 2;
    p.raise_attr = lds > kLdsDefault;
    p.form = (lds > kLdsPerCu || qpt > 8) ? kIcpFormInvalid : kIcpFormWorkgroup;   // (qpt > 8: n_src > 8192)
    return p;
}

// ---------------------------------------------------------------------------------
// In-place copy of maps (k_grid_copy_maps, slam_grid_copy_maps)
// ---------------------------------------------------------------------------------
// A workgroup takes (destination k, chunk of cells): kCopyChunkCells cells of both counter arrays (and of the live pmap),
// 16 bytes per lane and trip where source and destination are equally aligned.  The chunk is a multiple of four cells, so
// a chunk's start has its map's alignment.  More groups than kCopyMaxGroups are taken grid-stride.
constexpr int kCopyThreads = 256;
constexpr int kCopyChunkCells = 8192;        // 32 KiB of each counter array per workgroup: 8 trips of 16 bytes per lane
constexpr long kCopyMaxGroups = 1L << 20;
static_assert(kCopyChunkCells % 4 == 0, "a chunk's first cell keeps its map's 16-byte alignment");
struct CopyShape {
    long chunks = 0;       // workgroups per destination
    long groups = 0;       // count * chunks
    long grid = 0;         // workgroups launched
    int threads = kCopyThreads;
};
inline CopyShape plan_copy_maps(long cells, long count)
{
    CopyShape p;
    if (cells < 1 || count < 1) return p;
    p.chunks = (cells + kCopyChunkCells - 1) / kCopyChunkCells;
    p.groups = p.chunks * count;
    p.grid = std::min(p.groups, kCopyMaxGroups);
    return p;
}

// ---------------------------------------------------------------------------------
// Global scan localisation (locate_kernels.hip, slam_grid_locate)
// ---------------------------------------------------------------------------------
// Two shapes, by what the node counts of a search say:
//   dense   the top level, every node of every rotation: a workgroup takes (pair = hypothesis x rotation, tile of nodes),
//           stages the rotation's cell offsets in LDS once and runs its lanes over the tile's nodes, each lane looping
//           over the beams - as k_match does.  A tile is kLocateTileRounds rounds of the workgroup, so that the staging
//           (a few float64 products per beam) is paid once per 4 096 nodes and a brute-force rotation of a large map
//           still spreads over many workgroups.
//   sparse  the survivors' children: a lane per child, looping over its pair's row of a table of packed offsets that the
//           dense pass of the chunk left in global memory; grid-stride over a list whose length is read on the device;
//           the launch is sized by the chip, not the list.  (A wave per node with its lanes over the beams - what lists
//           of tens to thousands of nodes suggest - was built first and measured: the offsets formed in float64 per
//           node and one atomic per survivor made 64 scans slower than brute force)
// The node lists and the table live in a budget (context option "locate_ws_mb"): level h of one pair holds at most every
// node of that level (an empty map: everything ties and survives), kLocateNodeBytes each; pairs are taken in chunks that fit.
constexpr int kLocateMaxLevels = 8;
constexpr int kLocateMaxBeams = 4096;
constexpr int kLocateThreads = 256;
constexpr int kLocateTileRounds = 16;
constexpr size_t kLocateOffsetBytes = 8;     // an (ax, ay) pair of int32 in LDS
constexpr size_t kLocateNodeBytes = 8;       // a list entry: pair, I * nJ + J
constexpr long kLocateMaxBlocks = 1L << 20;  // workgroups of a dense launch; more groups are taken grid-stride
constexpr int kLocateSweepBlocks = 2048;     // workgroups of a sparse launch: eight per CU of 256

SLAM_HD inline long locate_level_nodes(int ni, int nj, int h)
{
    const long s = 1L << h;
    return ((ni + s - 1) / s) * ((nj + s - 1) / s);
}
// worst-case bytes of one pair's lists: the survivors of levels H .. 1
SLAM_HD inline long locate_pair_bytes(int ni, int nj, int H)
{
    long nodes = 0;
    for (int h = 1; h <= H; ++h) nodes += locate_level_nodes(ni, nj, h);
    return nodes * (long)kLocateNodeBytes;
}
// a pair's row of the sweep's offset table and its two counts (H = 0 keeps neither lists nor table)
SLAM_HD inline long locate_table_bytes(int n) { return (long)n * (long)kLocateOffsetBytes + 8; }
SLAM_HD inline size_t locate_dense_lds(int n, int guard = kLdsGuard) { return (size_t)n * kLocateOffsetBytes + guard; }
SLAM_HD inline int locate_dense_threads(long nodes)
{
    return (int)std::min((long)kLocateThreads, (nodes + kWave - 1) / kWave * kWave);
}

struct LocateRequest {
    long pairs = 0;              // B * K
    int n = 0, ni = 0, nj = 0;   // beams; the largest region of the batch
    int H = 0;
    long ws_bytes = 0;           // the list budget
    int guard = kLdsGuard;
};
struct LocateShape {
    bool ok = false;             // false: one pair's worst-case lists do not fit the budget
    int dense_threads = 0, dense_lds = 0;
    long tile = 0, tiles = 0;    // top-level nodes per workgroup, workgroups per pair
    long pair_bytes = 0;         // lists and table row of one pair
    long chunk_pairs = 0, chunks = 0;
    long level_nodes[kLocateMaxLevels + 1] = {0};   // worst-case nodes of level h of one pair
    int sweep_threads = kLocateThreads;
};
inline LocateShape plan_locate(const LocateRequest &r)
{
    LocateShape p;
    if (r.pairs < 1 || r.n < 1 || r.ni < 1 || r.nj < 1 || r.H < 0 || r.H > kLocateMaxLevels) return p;
    for (int h = 0; h <= r.H; ++h) p.level_nodes[h] = locate_level_nodes(r.ni, r.nj, h);
    const long top = p.level_nodes[r.H];
    p.dense_threads = locate_dense_threads(top);
    p.dense_lds = (int)locate_dense_lds(r.n, r.guard);
    p.tile = (long)p.dense_threads * kLocateTileRounds;
    p.tiles = (top + p.tile - 1) / p.tile;
    p.pair_bytes = locate_pair_bytes(r.ni, r.nj, r.H) + (r.H ? locate_table_bytes(r.n) : 0);
    p.chunk_pairs = p.pair_bytes ? std::min(r.pairs, r.ws_bytes / p.pair_bytes) : r.pairs;   // H = 0 keeps no list
    if (p.chunk_pairs < 1) return p;
    p.chunks = (r.pairs + p.chunk_pairs - 1) / p.chunk_pairs;
    p.ok = true;
    return p;
}

// ---------------------------------------------------------------------------------
// Map frontiers (frontier_kernels.hip, slam_grid_frontiers)
// ---------------------------------------------------------------------------------
// One query = one map.  Its cells are cut into tiles of kFrontierTileX x kFrontierTileY (lanes along y, the fast axis); a
// workgroup forms the frontier bits of a tile from the counters (with a halo of max(radius, 1) cells in LDS), labels the
// tile in LDS and writes one int32 label per cell.  The unions across tile borders are one work item per border cell
// (the rows x = k * TileX and the columns y = k * TileY), through global atomics.  Every later phase is a pass over the
// query's cells in segments of kFrontierSeg cells; the ordered table comes from per-segment counts of kept roots.
// Workspace of a query (context option "frontier_ws_mb"): 4 bytes per cell of labels and 8 bytes per segment of counts;
// queries are taken in chunks that fit.
constexpr int kFrontierTileX = 32;
constexpr int kFrontierTileY = 64;
constexpr int kFrontierThreads = 256;
constexpr int kFrontierMaxRadius = 8;
constexpr int kFrontierSeg = 1024;            // cells per segment of the passes behind the labelling: four per lane
constexpr int kFrontierMaxClusters = 65536;
constexpr long kFrontierMaxBlocks = 1L << 20; // workgroups of a launch; more groups are taken grid-stride

SLAM_HD inline int frontier_halo(int radius) { return radius > 1 ? radius : 1; }
// dynamic LDS of the tile kernel: labels int32 [TileX * TileY], cell codes uint8 [(TileX + 2h) * (TileY + 2h)], the
// window's row sums uint8 [(TileX + 2h) * TileY], rounded up to 16 bytes, then the guard
SLAM_HD inline size_t frontier_lds_bytes(int radius, int guard = kLdsGuard)
{
    const size_t h = (size_t)frontier_halo(radius);
    const size_t b = (size_t)kFrontierTileX * kFrontierTileY * 4 + (kFrontierTileX + 2 * h) * (kFrontierTileY + 2 * h) +
                     (kFrontierTileX + 2 * h) * kFrontierTileY;
    return (b + 15) / 16 * 16 + (size_t)guard;
}
SLAM_HD inline long frontier_segs(long cells) { return (cells + kFrontierSeg - 1) / kFrontierSeg; }
SLAM_HD inline long frontier_query_bytes(long cells) { return cells * 4 + frontier_segs(cells) * 8; }

struct FrontierRequest {
    long B = 0;
    int xw = 0, yw = 0, radius = 0;
    long ws_bytes = 0;
    int guard = kLdsGuard;
};
struct FrontierShape {
    bool ok = false;             // false: one query's workspace does not fit the budget
    int tiles_x = 0, tiles_y = 0;
    long tiles = 0;              // workgroups of the tile kernel per query
    long border = 0;             // work items of the border unions per query
    long segs = 0;               // segments per query
    long query_bytes = 0;
    long chunk_queries = 0, chunks = 0;
    int lds = 0, threads = kFrontierThreads;
};
inline FrontierShape plan_frontiers(const FrontierRequest &r)
{
    FrontierShape p;
    if (r.B < 1 || r.xw < 1 || r.yw < 1 || r.radius < 0 || r.radius > kFrontierMaxRadius) return p;
    const long cells = (long)r.xw * r.yw;
    p.tiles_x = (r.xw + kFrontierTileX - 1) / kFrontierTileX;
    p.tiles_y = (r.yw + kFrontierTileY - 1) / kFrontierTileY;
    p.tiles = (long)p.tiles_x * p.tiles_y;
    p.border = (long)(p.tiles_x - 1) * r.yw + (long)(p.tiles_y - 1) * r.xw;
    p.segs = frontier_segs(cells);
    p.query_bytes = frontier_query_bytes(cells);
    p.lds = (int)frontier_lds_bytes(r.radius, r.guard);
    p.chunk_queries = std::min(r.B, r.ws_bytes / p.query_bytes);
    if (p.chunk_queries < 1) return p;
    p.chunks = (r.B + p.chunk_queries - 1) / p.chunk_queries;
    p.ok = true;
    return p;
}

// ---------------------------------------------------------------------------------
// Travel-cost field (travel_kernels.hip, slam_grid_travel)
// ---------------------------------------------------------------------------------
// One query = one map and its sources.  The map's cells are cut into tiles of kTravelTile x kTravelTile; the bits of the
// traversable set T lie in rows padded to whole tiles of y, one 64-bit word per (row, tile column).  ONE workgroup owns
// the whole relaxation of a query: it takes the dirty tile with the lowest pending border cost, relaxes it with a one-cell
// halo in LDS until nothing changes and marks the neighbours whose facing border went down.  With that order a tile's
// pending keys rise strictly and each is the final cost of one of the 4 * kTravelTile + 4 cells around it (DESIGN.md
// section 19), which bounds the activations of a query by tiles * kTravelTripsPerTile.
// Workspace of a query (context option "travel_ws_mb"): 4 bytes per cell of costs unless cost_out takes them, 8 bytes
// per (row, tile column) of T, 4 bytes per tile of pending keys; queries are taken in chunks that fit.
constexpr int kTravelTile = 64;
constexpr int kTravelThreads = 1024;
constexpr int kTravelStraight = 10, kTravelDiagonal = 14;
constexpr int kTravelMaxSources = 64, kTravelMaxFoot = 8, kTravelMaxGoals = 65536;
constexpr int kTravelTripsPerTile = 4 * kTravelTile + 6;      // the first activation, one per cell around the tile, one to spare
constexpr long kTravelMaxBlocks = 1L << 20;   // workgroups of a launch; more groups are taken grid-stride

// dynamic LDS of the relaxation: costs int32 [(Tile + 2)^2], T bytes [(Tile + 2)^2] rounded up to 16, 64 words of
// selection keys and marks, then the guard
SLAM_HD inline size_t travel_lds_bytes(int guard = kLdsGuard)
{
    const size_t halo = (size_t)(kTravelTile + 2) * (kTravelTile + 2);
    return halo * 4 + (halo + 15) / 16 * 16 + 64 * 4 + (size_t)guard;
}

struct TravelRequest {
    long B = 0;
    int xw = 0, yw = 0;
    bool own_costs = true;       // cost_out is NULL: the costs live in the workspace
    long ws_bytes = 0;
    int guard = kLdsGuard;
};
struct TravelShape {
    bool ok = false;             // false: one query's workspace does not fit the budget
    int tiles_x = 0, tiles_y = 0;
    long tiles = 0;
    long mask_words = 0;         // 64-bit words of T per query: xw * tiles_y
    long trips = 0;              // bound on the tile activations of a query
    long query_bytes = 0;
    long chunk_queries = 0, chunks = 0;
    int lds = 0, threads = kTravelThreads;
};
inline TravelShape plan_travel(const TravelRequest &r)
{
    TravelShape p;
    if (r.B < 1 || r.xw < 1 || r.yw < 1) return p;
    const long cells = (long)r.xw * r.yw;
    p.tiles_x = (r.xw + kTravelTile - 1) / kTravelTile;
    p.tiles_y = (r.yw + kTravelTile - 1) / kTravelTile;
    p.tiles = (long)p.tiles_x * p.tiles_y;
    p.mask_words = (long)r.xw * p.tiles_y;
    p.trips = p.tiles * kTravelTripsPerTile;
    p.query_bytes = (r.own_costs ? cells * 4 : 0) + p.mask_words * 8 + (p.tiles * 4 + 7) / 8 * 8;
    p.lds = (int)travel_lds_bytes(r.guard);
    p.chunk_queries = std::min(r.B, r.ws_bytes / p.query_bytes);
    if (p.chunk_queries < 1) return p;
    p.chunks = (r.B + p.chunk_queries - 1) / p.chunk_queries;
    p.ok = true;
    return p;
}

// ---------------------------------------------------------------------------------
// View gain (view_kernels.hip, slam_grid_view_gain)
// ---------------------------------------------------------------------------------
// One view = one pose and its beams.  Its BOX is the bounding box of its start and end cells, clipped to the map and
// padded to whole 32-cell words in y: box_rows rows of box_words words.  One workgroup owns a view: it keeps one bit per
// cell of the box (the WINDOW), sets the bits of the cells its beams see and counts them against the map's class bits.
// The window lies in LDS when it is at most kViewLdsBytes (the bound of the staged ray cast: two workgroups share a
// compute unit's 160 KiB), else in the call's workspace, one slot of a whole map's words per workgroup of the global
// engine (context option "gain_ws_mb"): chunk_views slots, over which the views are taken grid-stride in `chunks` passes.
constexpr size_t kViewLdsBytes = 64 * 1024;
constexpr int kViewThreads = 256;
constexpr long kViewMaxBlocks = 16384;       // workgroups of a launch; more views are taken grid-stride

// Which engine takes a view whose window has `window_words` words ("gain_lds": -1 automatic, 0 global, 1 LDS wherever
// the window fits): the ONE place that decides, asked by plan_view and by both kernels.
// The automatic rule follows tools/bench_gain.py (profiles/gain_bench.json): automatic means LDS
// wherever the window fits.  Course map at 400 x 400, views at its 60 frontier representatives, 360 beams to 30 m, ms
// per call, LDS / global:
//     B          1            64           256          8 192        1 024 maps x 256
//     gain    0.349/0.414  0.348/0.423  0.347/0.455  5.45/6.14    172.7/186.1         global 8 - 31 % slower everywhere
// Nothing measured speaks for the global engine where LDS fits.  (Supposed, not measured: the marks of a view land in
// few words - beams share their cells near the origin - and an OR at the L2 costs more than one in LDS.)
SLAM_HD inline bool view_fits_lds(long window_words) { return window_words * 4 <= (long)kViewLdsBytes; }
SLAM_HD inline bool choose_view_lds(long window_words, int lds_mode)
{
    if (!view_fits_lds(window_words) || lds_mode == 0) return false;
    return true;                             // 1, and automatic
}

struct ViewRequest {
    long B = 0;
    int xw = 0, yw = 0;
    int box_rows = 0, box_words = 0;     // the box asked about (0: the whole map)
    int lds_mode = -1;
    long ws_bytes = 0;
    int guard = kLdsGuard;
};
struct ViewShape {
    bool ok = false;             // false: the global engine may be needed and one view's slot does not fit the budget
    int row_words = 0;           // words per map row: ceil(yw / 32)
    long map_words = 0;          // xw * row_words: seen_out words of a view, and the words of a global slot
    long window_words = 0;       // of the box asked about
    long lds_bytes = 0;          // of that window in LDS, guard included
    bool engine_lds = false;     // the engine that box takes
    bool needs_global = false;   // some box of this map may go to the global engine
    bool needs_lds = false;      // ... to the LDS engine
    long launch_lds = 0;         // dynamic LDS of the LDS engine's launch: the largest window that can fit, and the guard
    long view_bytes = 0;         // bytes of a global slot
    long chunk_views = 0, chunks = 0;
    long grid_lds = 0, grid_global = 0;
    int threads = kViewThreads;
};
inline ViewShape plan_view(const ViewRequest &r)
{
    ViewShape p;
    if (r.B < 1 || r.xw < 1 || r.yw < 1) return p;
    p.row_words = (r.yw + 31) / 32;
    p.map_words = (long)r.xw * p.row_words;
    const int rows = r.box_rows > 0 ? std::min(r.box_rows, r.xw) : r.xw;
    const int words = r.box_words > 0 ? std::min(r.box_words, p.row_words) : p.row_words;
    p.window_words = (long)rows * words;
    p.lds_bytes = p.window_words * 4 + r.guard;
    p.engine_lds = choose_view_lds(p.window_words, r.lds_mode);
    p.needs_lds = r.lds_mode != 0;
    p.needs_global = !choose_view_lds(p.map_words, r.lds_mode);
    p.launch_lds = std::min(p.map_words * 4, (long)kViewLdsBytes) + r.guard;
    p.view_bytes = p.map_words * 4;
    p.chunk_views = std::min(r.B, r.ws_bytes / p.view_bytes);
    p.grid_lds = p.needs_lds ? std::min(r.B, kViewMaxBlocks) : 0;
    if (p.chunk_views < 1) {
        p.chunk_views = 0;
        p.ok = !p.needs_global;
        return p;
    }
    p.chunk_views = std::min(p.chunk_views, kViewMaxBlocks);
    p.chunks = (r.B + p.chunk_views - 1) / p.chunk_views;
    p.grid_global = p.needs_global ? p.chunk_views : 0;
    p.ok = true;
    return p;
}

// ---------------------------------------------------------------------------------
// Refinement of a scan-to-map pose (refine_kernels.hip, slam_grid_refine)
// ---------------------------------------------------------------------------------
// One WAVE owns a hypothesis through all its iterations: its lanes take the beams, its sums go through a butterfly and
// every lane solves the same 3 x 3 system.  Four waves share a 256-thread workgroup (no LDS, no barrier: they only share
// the launch), so a launch has ceil(B / 4) workgroups, kRefineMaxBlocks at most; the hypotheses beyond
// kRefineMaxBlocks * kRefineWaves are taken grid-stride.  Nothing here depends on n: a hypothesis's sums must not
// depend on the batch, so the shape may not either.
constexpr int kRefineWaves = 4;              // hypotheses per workgroup
constexpr int kRefineThreads = kRefineWaves * kWave;
constexpr long kRefineMaxBlocks = 16384;     // workgroups of a launch: 64 waves a CU of a 256-CU chip, eight rounds of residency
struct RefineShape {
    long blocks = 0;             // workgroups the batch needs
    long grid = 0;               // workgroups launched
    long pass = 0;               // hypotheses one sweep of the launch takes: grid * kRefineWaves
    int threads = kRefineThreads;
};
SLAM_HD inline RefineShape plan_refine(long B)
{
    RefineShape p;
    if (B < 1) return p;
    p.blocks = (B + kRefineWaves - 1) / kRefineWaves;
    p.grid = p.blocks < kRefineMaxBlocks ? p.blocks : kRefineMaxBlocks;
    p.pass = p.grid * kRefineWaves;
    return p;
}

// ---------------------------------------------------------------------------------
// The scan-to-map tracker's own steps (track_kernels.hip, slam_track)
// ---------------------------------------------------------------------------------
// Two shapes for L trajectories.  "Rows": one workgroup of a wave per trajectory, whose lanes copy the scan's n ranges
// and form the K rotations while lane 0 predicts (k_track_predict).  "Lanes": one lane per trajectory, 256 to a workgroup
// (k_track_seed, k_track_decide).  Both take the trajectories beyond kTrackMaxBlocks workgroups grid-stride.
constexpr int kTrackRowThreads = kWave;
constexpr int kTrackThreads = 256;
constexpr long kTrackMaxBlocks = 65536;
struct TrackShape {
    long row_grid = 0, lane_grid = 0;        // workgroups of the two shapes
    int row_threads = kTrackRowThreads, lane_threads = kTrackThreads;
};
SLAM_HD inline TrackShape plan_track(long L)
{
    TrackShape p;
    if (L < 1) return p;
    p.row_grid = L < kTrackMaxBlocks ? L : kTrackMaxBlocks;
    const long lanes = (L + kTrackThreads - 1) / kTrackThreads;
    p.lane_grid = lanes < kTrackMaxBlocks ? lanes : kTrackMaxBlocks;
    return p;
}

}  // namespace slam
