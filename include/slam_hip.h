/*
 * slam_hip.h - C ABI of libslamhip.so: the MI355X (gfx950) implementation of the
 * per-scan SLAM hot path of zjwzcx/A-2D-LiDAR-based-SLAM-System-for-Wheeled-Mobile-Robots.
 *
 * The reference has no FFI layer (it is pure Python 2 / NumPy); its boundary for this
 * path is the Python class API of course_agv_slam/scripts.  Each entry
 * point below names the reference interface it replaces.  Reference paths:
 *   W12m = "W12_LiDAR SLAM/w12-mapping/course_agv_slam/scripts"
 *   W7   = "W7_Dead Reckoning (ICP)/course_agv_slam/scripts"
 * The ctypes binding a maintainer of the reference would add is shown in INTEGRATION.md
 * and implemented in the package's _abi.py.
 *
 * Conventions
 *  - plain C types only; every function returns 0 (SLAM_OK) or a negative SLAM_ERR_*;
 *    slam_last_error() returns the message of the calling thread's last failure.
 *  - a slam_ctx owns one HIP stream (or borrows the caller's) and a device workspace;
 *    use one context per host thread.  Nothing here falls back to the CPU: without a
 *    usable gfx950 device slam_create fails.
 *  - functions without suffix take HOST pointers, copy in, run the kernels, copy out and
 *    synchronise; *_dev functions take DEVICE pointers (e.g. torch.Tensor.data_ptr()),
 *    only enqueue work on the context's stream and do not synchronise.
 *  - point sets are structure-of-arrays: one set is 2*n values, the n x coordinates
 *    then the n y coordinates ("[2][n]").  The reference's third row of ones
 *    (icp.py:42-49) is not stored.  `dtype` is the STORAGE type of a point buffer
 *    (SLAM_F64 / SLAM_F32 / SLAM_F16); all arithmetic is float64 regardless.
 *  - T is a 3x3 row-major float64 matrix [[R, t], [0, 0, 1]] exactly as ICP.process
 *    returns it; poses are (x, y, theta) float64.
 *  - grids are [xw][yw] row-major (x outer) as mapping.py:14-15.
 */
#ifndef SLAM_HIP_H
#define SLAM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLAM_ABI_VERSION 1

typedef struct slam_ctx slam_ctx;
typedef struct slam_grid slam_grid;

enum {
    SLAM_OK = 0,
    SLAM_ERR_INVALID = -1,  /* bad argument (null pointer, non-positive size, unknown dtype) */
    SLAM_ERR_HIP = -2,      /* a HIP runtime call or kernel launch failed                    */
    SLAM_ERR_NOMEM = -3,    /* device or host allocation failed                              */
    SLAM_ERR_NAN = -4,      /* NaN world coordinate: the reference raises ValueError from
                               int(nan) at mapping.py:33                                     */
    SLAM_ERR_OVERFLOW = -5, /* infinite / unrepresentable cell index: the reference raises
                               OverflowError from int(inf) at mapping.py:33-36 (or would walk
                               a ray of more than 2^20 cells)                                */
    SLAM_ERR_NODEVICE = -6  /* no gfx950 device visible                                      */
};

enum { SLAM_F64 = 0, SLAM_F32 = 1, SLAM_F16 = 2 };

/* kernel families timed by slam_timing_* */
enum { SLAM_K_POINTS = 0, SLAM_K_ICP = 1, SLAM_K_COMPOSE = 2, SLAM_K_GRID = 3, SLAM_K_FINALIZE = 4,
       SLAM_K_NN = 5, SLAM_K_KABSCH = 6, SLAM_K_BRESENHAM = 7, SLAM_K_COUNT = 8 };

int slam_abi_version(void);
const char *slam_last_error(void);

/* ---- context ------------------------------------------------------------------ */
/* device: HIP ordinal.  stream: a hipStream_t to enqueue on (e.g. torch's current
 * stream), or NULL to create a private one. */
int slam_create(int device, void *stream, slam_ctx **out);
int slam_destroy(slam_ctx *ctx);
int slam_synchronize(slam_ctx *ctx);
/* Order the context's work against another HIP stream of the caller WITHOUT a host synchronise (stream: a
 * hipStream_t, e.g. torch's current stream, on which the RCCL collectives of torch.distributed are ordered; NULL: the
 * legacy default stream).  direction 0: `stream` waits for everything this context has enqueued so far - on its own
 * stream and on its internal ones ("pipeline" map / pose stages, chunked particle ray casts); direction 1: everything
 * the context enqueues from now on waits for what `stream` holds at this moment.  The reference has no counterpart
 * (one Python thread, W12m/slam_ekf.py:63-95); this is what makes a device pointer handed out by
 * slam_grid_counters_dev / slam_grid_live_pmap safe to use from a stream the library does not own:
 *   slam_grid_counters_dev(...); slam_stream_order(ctx, s, 0); <all_reduce on s>; slam_stream_order(ctx, s, 1); */
int slam_stream_order(slam_ctx *ctx, void *stream, int direction);
/* Synchronise and return-and-clear the sticky data error raised by kernels since the
 * last call (SLAM_OK, SLAM_ERR_NAN or SLAM_ERR_OVERFLOW). */
int slam_check_status(slam_ctx *ctx);
/* Tuning knobs.  Maps, cell indices, nearest-neighbour indices and iteration counts never depend on them; the launch
 * shape of the scan matcher ("icp_qpt", "icp_one_wave", and the batch size itself) decides the order in which a pair's sums are added,
 * so transforms and poses of two shapes agree to rounding (1e-13), not bit for bit.
 * "grid_mode": 1 = automatic (default): ray casting through an LDS window per group of scans,
 *   or - for one shared map much larger than a window - rays dealt by direction and swept in
 *   bands through a sheared window (wedges); 0 = direct global atomics; 2 = walks recorded once
 *   and cast tile by tile, wherever that applies; 3 = always the window; 4 = wedges wherever
 *   they apply.
 * "grid_group": scans per workgroup / per tile group, 0 = automatic.
 * "grid_split": LDS-window ray cast with two workgroups per group of scans, one per direction
 *   half (a ray never crosses the column of its origin): -1 = automatic (default: when the launch
 *   cannot fill the chip on its own - shorter launch, a little more total work), 0 = never
 *   (callers that overlap launches of several contexts), 1 = always.
 * "icp_qpt": queries per lane of batched scan matching, 1..3; 0 = by batch size (two for
 *   launches that cannot fill the chip on their own, three from 2 500 pairs of 360 beams or
 *   834 of 1 080 - 7 500 waves at two queries per lane; callers that overlap several smaller
 *   launches set 3).  3 means "the shapes for a full chip": three queries per lane, or - see
 *   "icp_one_wave" - one wave per pair where the launch is that large on its own.
 * "icp_one_wave": scan matching by ONE wave per pair, six queries per lane, for pairs of up to 384
 *   source points: fewer instructions per pair and no barriers, a longer solve of the single pair.
 *   -1 = automatic (default): where the queries per lane resolve to 3 (given or by batch size), the
 *   launch holds at least 16 384 pairs (four rounds of the pairs resident in this shape), the clouds
 *   are scans and 16 pairs fit a compute unit's LDS; 0 = never; 1 = wherever a pair fits.  Same matches and iteration counts;
 *   transforms agree with the other shapes to rounding, as above.
 * "icp_f32_filter": the one-wave shape scans the beam windows of its iterations, the first included, in float32
 *   first and forms in float64 only the winner's distance, wherever every lane of the wave has PROVED its
 *   nearest target (it beats the runner-up by more than float32 can be wrong); any other wave runs the
 *   float64 scan as before.  -1 = the library's choice (default: on), 0 = off, 1 = on.  No result depends
 *   on it - bit-identical transforms, poses and iteration counts; an A/B switch.
 * "win_lds_hits": the shared-map LDS-window ray cast (groups of scans of a replay, up to 8 192 rays a group)
 *   counts the hits of its rays per end cell in the window, behind the flush of the pass counts, and sends
 *   one global add per distinct end cell instead of one per ray.  -1 = the library's choice (default: in
 *   launches of more workgroups than the chip has compute units, where the launch waits for its memory-side
 *   atomics), 0 = off, 1 = wherever the rays are sorted.  No result depends on it - the counters are integers; an A/B switch.
 * "replay_reset": 1 = slam_replay_dev starts its map from zero (as slam_grid_reset before it would),
 *   clearing the counters inside its scan-matching launch: one dispatch less per replay.  0
 *   (default): the map accumulates across replays until slam_grid_reset.
 * "icp_team": first-iteration queries of a scan without a usable beam window (range jumps between
 *   the two scans): 0 = compacted into a list and searched apart from the lanes that own them
 *   (default), 1 = by the box search of the owning lane.  Same results; an A/B switch.
 * "pipeline": 1 = slam_replay_dev with a map runs as three stages on three streams of the
 *   context (scan matching | pose composition | slam_grid_reset -> ray cast ->
 *   slam_grid_finalize_dev), so the map stage of one replay overlaps the scan matching of the
 *   next; give consecutive replays different poses_out and T_out buffers to benefit (a buffer an
 *   earlier stage is still reading is waited for).  Results of the later stages (poses_out,
 *   pmap_dev) are visible after slam_synchronize / a device synchronise, or to any later call
 *   on this context.  0 = everything on the context's stream (default).
 * "particle_chunks": k > 1 = slam_particles_dev cuts its batch into k chunks: scan matching and pose step of chunk
 *   i + 1 on the context's stream beside the ray cast of chunk i on a second stream.  The call still returns with the
 *   context's stream ordered behind ALL of its work (the second stream is joined at the end), so buffers may be
 *   reused by later calls as with any *_dev entry point.  Measured slower than one piece on MI355X;
 *   0 / 1 = off (default).
 * "raycast_lds": where slam_grid_raycast / slam_grid_scan_score read the map's occupied bits from: 0 = global
 *   memory, one lane per ray (any map size); 1 = a copy in LDS per workgroup wherever the map's bit mask fits
 *   64 KiB (512 K cells), else as 0; -1 = automatic (default).  Same bits either way; an A/B switch.
 * "mcl_shape": launch shape of slam_mcl_weigh: 0 = a workgroup's lanes run over the particles, each lane looping over
 *   the beams; 1 = a wave per particle, its lanes over the beams; -1 = the library's choice by beam count (default).
 *   Same bits either way; an A/B switch.
 * "locate_ws_mb": MiB that the node lists of slam_grid_locate may take in the context's workspace, in (0, 2^20],
 *   fractions allowed; default 64.  The (hypothesis, rotation) pairs of a call are cut into chunks whose worst-case
 *   lists fit; a call whose single pair does not fit is SLAM_ERR_INVALID.  No result depends on it.
 * "frontier_ws_mb": MiB that the labels of slam_grid_frontiers may take in the context's workspace, in (0, 2^20],
 *   fractions allowed; default 256.  The queries of a call are cut into chunks that fit; a call whose single query
 *   does not fit is SLAM_ERR_INVALID.  No result depends on it.
 * "travel_ws_mb": MiB that the costs, the traversable bits and the tile keys of slam_grid_travel may take in the
 *   context's workspace, in (0, 2^20], fractions allowed; default 256.  The queries of a call are cut into chunks that
 *   fit; a call whose single query does not fit is SLAM_ERR_INVALID.  No result depends on it.
 * "gain_lds", "gain_ws_mb": the engine and the workspace of slam_grid_view_gain (see there). */
int slam_set_option(slam_ctx *ctx, const char *name, double value);
/* Per-kernel-family timing with HIP events on the context's stream (bench.py roofline).
 * on: 0 = off, 1 = every family, 2 * mask = only the families in mask (bit SLAM_K_*): events on a
 * dispatch cost throughput (3-4 % with four replays overlapping), a caller that needs one family's
 * times pays for one.  read: synchronises, adds up elapsed ms and launch counts since the last reset. */
int slam_timing_enable(slam_ctx *ctx, int on);
int slam_timing_read(slam_ctx *ctx, double ms_out[SLAM_K_COUNT], int64_t launches_out[SLAM_K_COUNT]);

/* Introspection of launch decisions: what the library WOULD launch for a request, decided by the same functions its
 * launchers call.  No context and no device call: each works on a machine without a GPU.  Stable in meaning, not a
 * promise that shapes stay: a later version may decide differently for the same request.  cus / lds_per_cu: the chip the
 * launch is planned for (MI355X: 256 CUs, 163 840 bytes).  guard: guard bytes behind every dynamic LDS region, 0 in the
 * shipped build, 512 in the LDS-guard debug build; negative = those of the build that was loaded.
 *
 * slam_plan_win: the LDS-window ray cast of L streams of `scans` scans of n beams in groups of `group` scans per workgroup
 * into a map of xw x yw cells.  has_got: the caller names every stream's map; pmap_live, maps_are_private, hit_levels,
 * has_redo: the grid's state (a live pmap, a map per stream, 1 or 3 hit levels, a re-do list); split_pref / hits_pref: the
 * context options "grid_split" / "win_lds_hits" (-1: the library's choice). */
enum { SLAM_WIN_FORM_WIN = 0, SLAM_WIN_FORM_OWN = 1, SLAM_WIN_FORM_OWNER1 = 2, SLAM_WIN_FORM_OWNER2 = 3,
       SLAM_WIN_FORM_OWNER8_THEN_REDO = 4 };
typedef struct slam_win_plan {
    int form;                 /* SLAM_WIN_FORM_*: shared-map kernel, the map's only writer, its single-scan forms */
    int grid_x, grid_y, threads;
    int lds;                  /* dynamic LDS of the launch, bytes */
    int lds_attr;             /* LDS size the launch must be allowed by attribute first; 0: the standing allowance does */
    int exclusive, sort_cap, win_cells, split, lds_hits;   /* kernel arguments */
    int two_per_cu;           /* the window was carved so that two workgroups fit a CU */
    int wgs;                  /* workgroups (0 for the single-scan owner forms) */
    int own8_lds, own8_win;   /* OWNER8_THEN_REDO: dynamic LDS and window bytes of the byte-window launch ... */
    int redo_grid;            /* ... and workgroups of the re-do launch behind it (threads, lds, sort_cap, win_cells are its) */
    int live_dirty;           /* the launch leaves the live pmap behind the counters */
} slam_win_plan;
int slam_plan_win(int L, int scans, int n, int group, int has_got, int pmap_live, int maps_are_private, int hit_levels, int xw,
                  int yw, int has_redo, int split_pref, int hits_pref, int cus, int lds_per_cu, int guard, slam_win_plan *out);
/* slam_plan_win_phases: how one workgroup of the shared-map kernel cuts its group's rays into phases, each with the window
 * to itself.  bbox: x0, y0, x1, y1 (cells) of everything the group's rays can touch; origins: min x, min y, max x, max y of
 * the scans' origin cells; ymask: 1 where the map's rows hold an even number of cells (the window's rows then start on an
 * even cell), else 0; win_cells: the window's capacity (slam_win_plan.win_cells); sorted: the rays are sorted
 * (slam_win_plan.sort_cap > 0); half: -1 = one workgroup per group, 0 / 1 = the workgroup of a split launch that takes the
 * rays left / right of the origins' column.  Per phase: the quadrants it casts (bit q: end cell right of the origin for
 * q & 1, above it for q & 2), their box clamped to the map (any = 0: nothing of it is in the map; the box is then
 * meaningless), and whether the box fits the window (0: a sub-rectangle gets the window, the rest goes by global atomics). */
typedef struct slam_win_phases {
    int nph, parity;          /* phases; 1: two workgroups share one window's rays by beam parity */
    int part[4];
    int box[4][4];            /* x0, y0, x1, y1 */
    int any[4], fits[4];
} slam_win_phases;
int slam_plan_win_phases(const int32_t bbox[4], const int32_t origins[4], int xw, int yw, int ymask, int win_cells, int sorted,
                         int half, slam_win_phases *out);
/* slam_plan_icp: the scan matcher for B pairs of n_src against n_tar points.  is_scan: the clouds are raw scans (the replay
 * and particle entry points), not point buffers; qpt_pref, one_wave, f32_filter, team_mode: the context options "icp_qpt",
 * "icp_one_wave", "icp_f32_filter", "icp_team"; batch_invariant: the node replay's shape that does not follow B. */
enum { SLAM_ICP_FORM_INVALID = 0, SLAM_ICP_FORM_WAVE_F32 = 1, SLAM_ICP_FORM_WAVE_F64 = 2, SLAM_ICP_FORM_WORKGROUP = 3 };
typedef struct slam_icp_plan {
    int form;                 /* SLAM_ICP_FORM_*: no launch (more LDS than a CU has), one wave per pair, one workgroup per pair */
    int pref, preferred;      /* preferred queries per lane; whether they replaced the size-derived ones */
    int qpt, unroll, block;   /* queries per lane, candidates per trip of the beam-window search, threads */
    int lds;                  /* dynamic LDS of the launch, bytes */
    int polar_copy, team_cap, cap_wanted;   /* unpadded copy of the target in LDS; slots of the first-iteration list, and before the LDS cut it */
    int raise_attr;           /* lds is more than a kernel gets by default */
    int nn_bytes;             /* bytes of the padded target image and its boxes */
} slam_icp_plan;
int slam_plan_icp(int B, int n_src, int n_tar, int is_scan, int qpt_pref, int batch_invariant, int one_wave, int f32_filter,
                  int team_mode, int guard, slam_icp_plan *out);
/* slam_plan_query: a constant or an LDS size function of the two planners by its name in csrc/launch_shapes.h, e.g.
 * "kWinCells", "win_lds_bytes" (a, b, c = group, sort_cap, win_cells), "win_cells_for" (group, sort_cap, two_per_cu),
 * "win_sort_cap" (rays), "nn_lds_bytes" / "icp_polar_bytes" (n_tar), "icp_red_bytes" (waves), "icp_block" (n_src, qpt);
 * "locate_level_nodes" (ni, nj, level), "locate_pair_bytes" / "locate_tile" / "locate_tiles" (ni, nj, levels),
 * "locate_dense_lds" (n), "locate_dense_threads" (nodes), "locate_chunk_pairs" (budget in KiB, a pair's bytes, pairs);
 * "frontier_tiles" / "frontier_tiles_x" / "frontier_tiles_y" / "frontier_border" / "frontier_segs" /
 * "frontier_query_bytes" (xw, yw), "frontier_lds" (radius), "frontier_chunk_queries" (budget in KiB, a query's bytes, B);
 * "travel_tiles" / "travel_tiles_x" / "travel_tiles_y" / "travel_mask_words" / "travel_trips" (xw, yw),
 * "travel_query_bytes" (xw, yw, 1 when the costs live in the workspace), "travel_lds", "travel_chunk_queries" / "travel_chunks"
 * (budget in KiB, a query's bytes, B);
 * "wedge_ws_bytes" / "tile_ws_bytes" (scans of the cast = L * scans, beams, groups): the bytes at which the device workspace
 * of the wedge / tile ray cast ends, every piece on a 256-byte boundary, computed in 64 bits;
 * "grid_state_bytes" (G, xw, yw): the bytes a reset of such a grid object clears (both counters of every map, the visit slots);
 * arguments a function does not take are ignored.  SLAM_ERR_INVALID for a name it does not know. */
int slam_plan_query(const char *name, int a, int b, int c, int guard, int64_t *out);

/* ---- ICP ------------------------------------------------------------------------ */
/* Replaces ICP.laserToNumpy (W7/icp.py:182-195) and SLAM_EKF.laserToNumpy
 * (W12m/slam_ekf.py:115-123; clip_inf != 0 applies its inf -> 30 m rule, :119).
 * ranges [B][n] float32; cos_t, sin_t [n] = cos/sin(numpy.linspace(angle_min, angle_max, n))
 * computed by the caller; pts_out [B][2][n] of `dtype`. */
int slam_scan_to_points(slam_ctx *ctx, const float *ranges, const double *cos_t, const double *sin_t,
                        int B, int n, int clip_inf, int dtype, void *pts_out);
int slam_scan_to_points_dev(slam_ctx *ctx, const float *ranges, const double *cos_t, const double *sin_t,
                            int B, int n, int clip_inf, int dtype, void *pts_out);

/* Replaces ICP.findNearest(src, tar) (W12m/icp.py:90-114): brute-force nearest
 * neighbour, lowest index on ties OF THE DISTANCE - the reference compares sqrt of the
 * fused square, so squares that differ in the last places but share a square root tie too
 * (tests/golden/g9, g10) - and (distance 0, index 0) when nothing compares less
 * than inf.  src [B][2][n_src], tar [B][2][n_tar]; dist [B][n_src], idx [B][n_src]. */
int slam_nn(slam_ctx *ctx, const void *src, const void *tar, int B, int n_src, int n_tar, int dtype,
            double *dist, int32_t *idx);
int slam_nn_dev(slam_ctx *ctx, const void *src, const void *tar, int B, int n_src, int n_tar, int dtype,
                double *dist, int32_t *idx);

/* Replaces ICP.getTransform(src, tar) (W12m/icp.py:149-179): rigid 2-D fit of paired
 * rows; src, tar [B][2][n] float64; T_out [B][9].
 * DOCUMENTED DEVIATION: when every row of src or of tar is ONE point (bitwise), W = BB^T.AA is
 * mathematically zero and every rotation is optimal; the reference's SVD then sees the rounding
 * noise of np.mean and returns an arbitrary rotation (tests/golden/g8_collapsed.npz holds eight,
 * 16 .. 170 degrees).  This function returns the canonical R = I, t = centroid_tar - centroid_src;
 * both answers move the source centroid onto the matched point. */
int slam_kabsch2d(slam_ctx *ctx, const double *src, const double *tar, int B, int n, double *T_out);
int slam_kabsch2d_dev(slam_ctx *ctx, const double *src, const double *tar, int B, int n, double *T_out);

/* Replaces ICP.process(tar_pc, src_pc) (W12m/icp.py:38-88) and the loop body of
 * ICP.laserCallback (W7/icp.py:74-92) for B independent pairs in one launch.
 * tar [B][2][n_tar] (or one shared set when tar_shared != 0), src likewise.
 * prior: NULL, or [B][6] row-major 2x3 matrices applied to the source points first
 * (x' = p0*x + p1*y + p2; y' = p3*x + p4*y + p5): the perturbed-prior particle batch of
 * BASELINE.json configs[2]; the returned T maps the perturbed source.
 * T_out [B][9]; iters_out [B] and mean_err_out [B] may be NULL.
 * n_tar, n_src <= 8192.  The rigid fit of every iteration follows slam_kabsch2d, including its
 * canonical R = I for collapsed correspondences (every source point matched to one target). */
int slam_icp_batch(slam_ctx *ctx, const void *tar, const void *src, int B, int n_tar, int n_src,
                   int dtype, int tar_shared, int src_shared, const double *prior, int max_iter,
                   double tol, double *T_out, int32_t *iters_out, double *mean_err_out);
int slam_icp_batch_dev(slam_ctx *ctx, const void *tar, const void *src, int B, int n_tar, int n_src,
                       int dtype, int tar_shared, int src_shared, const double *prior, int max_iter,
                       double tol, double *T_out, int32_t *iters_out, double *mean_err_out);

/* Replaces the pose part of ICP.publishResult(T) (W7/icp.py:153-158 = W12m/icp.py:185-190)
 * applied along L trajectories of n steps: T [L][n][9], pose0 [L][3] -> poses_out [L][n][3]
 * (pose after each step; theta is not wrapped). */
int slam_pose_compose(slam_ctx *ctx, const double *T, const double *pose0, int L, int n, double *poses_out);
int slam_pose_compose_dev(slam_ctx *ctx, const double *T, const double *pose0, int L, int n, double *poses_out);

/* ---- occupancy grid --------------------------------------------------------------- */
/* Replaces Mapping.__init__(xw, yw, xyreso) (W12m/mapping.py:8-20) for G independent
 * maps.  Cell index rule: int(scale * (x + off)) truncated toward zero; the reference
 * hard-codes scale = off_x = off_y = 10 (:33-36).  free_inc / hit_inc / thresh are the
 * +0.01 / +20 / >10 of :43-47 (hit_inc = 4 gives the w12-mapping-online variant,
 * W12o/mapping.py:46).  Evidence is held as integer pass / hit counters; a cell with h hits
 * and p passes is occupied iff the float64 running sum "h x hit_inc, then p x free_inc"
 * (sequential IEEE adds, hits first) exceeds thresh.  For hit_inc > thresh that is the
 * reference's answer whatever the order of arrival; for the +4 variant the reference's own
 * answer is order-dependent when p sits exactly on a threshold, and this canonical order
 * decides.  At most 8 hits may be needed to exceed thresh (else SLAM_ERR_INVALID). */
int slam_grid_create(slam_ctx *ctx, int G, int xw, int yw, double scale, double off_x, double off_y,
                     double free_inc, double hit_inc, double thresh, slam_grid **out);
int slam_grid_destroy(slam_ctx *ctx, slam_grid *grid);
int slam_grid_reset(slam_ctx *ctx, slam_grid *grid);

/* Replaces Mapping.update(ox, oy, center_x, center_y) (W12m/mapping.py:22-51) for B
 * scans: ox, oy [B][n] world-frame beam endpoints, cx, cy [B] ray origins;
 * grid_of_batch [B] selects the map each scan is cast into (NULL: all into map 0). */
int slam_grid_update(slam_ctx *ctx, slam_grid *grid, const double *ox, const double *oy, const double *cx,
                     const double *cy, int B, int n, const int32_t *grid_of_batch);
int slam_grid_update_dev(slam_ctx *ctx, slam_grid *grid, const double *ox, const double *oy,
                         const double *cx, const double *cy, int B, int n, const int32_t *grid_of_batch);

/* Replaces the map-building lines of SLAM_EKF.laserCallback for S scans at once:
 * obs = u2T(xEst).dot(laserToNumpy(msg)) (inf -> 30 m) and mapping.update(obs[0], obs[1],
 * centre) (W12m/slam_ekf.py:88-90, :115-123).  ranges float32 [S][n]; poses [S][3] = xEst of
 * each scan; centres [S][2] = the ray origins, or NULL to cast from the pose as w12-mapping
 * does.  w12-mapping-online takes the centre from /tf instead (W12o/slam_ekf.py:71-77,104).
 * All S scans go into map 0. */
int slam_grid_update_scans(slam_ctx *ctx, slam_grid *grid, const float *ranges, const double *cos_t,
                           const double *sin_t, const double *poses, const double *centres, int S, int n);
int slam_grid_update_scans_dev(slam_ctx *ctx, slam_grid *grid, const float *ranges, const double *cos_t,
                               const double *sin_t, const double *poses, const double *centres, int S, int n);

/* Read map g back (what Mapping.update returns, mapping.py:51, plus the state behind it).
 * Any output may be NULL.  pmap [xw][yw] int8 in {0, 50, 100}; datamap [xw][yw] float64
 * = free_inc*pass + hit_inc*hit; pass, hit [xw][yw] uint32. */
int slam_grid_read(slam_ctx *ctx, slam_grid *grid, int g, int8_t *pmap, double *datamap, uint32_t *pass,
                   uint32_t *hit);
/* Device addresses of the evidence counters, pass and hit, each uint32 [G][xw][yw]: for
 * checkpoint / restore and for merging maps that several GPUs built from disjoint scans - one
 * all_reduce(SUM) over the ranks, in place (integer sums commute, so the merged map is
 * bit-identical for any rank count).  Work enqueued on the context's stream after
 * this call sees every earlier update; a live pmap is marked stale.  The call orders nothing against
 * OTHER streams: a consumer on a stream of its own (a collective on torch's current stream) first makes
 * that stream wait for the context, and the context wait for it afterwards, with slam_stream_order -
 * dist.all_reduce_grid of the Python package does exactly that. */
int slam_grid_counters_dev(slam_ctx *ctx, slam_grid *grid, uint32_t **pass_dev, uint32_t **hit_dev);

/* Keep pmap [G][xw][yw] int8 resident and current on the device and return its address.
 * Ray casts that are the only writer of their map in a launch (one scan group per map: the
 * per-particle maps of slam_particles, Mapping.update of one scan) re-threshold just the cells
 * they could have touched, so no finalize pass over the whole map is needed afterwards; any
 * other update marks it stale and the next finalize / read refreshes it with a full pass.
 * slam_grid_finalize_dev(pmap_dev == that address) then costs nothing when it is current. */
int slam_grid_live_pmap(slam_ctx *ctx, slam_grid *grid, int8_t **pmap_dev_out);
/* Device-side finalize of all G maps into pmap_dev [G][xw][yw] int8 (no synchronise). */
int slam_grid_finalize_dev(slam_ctx *ctx, slam_grid *grid, int8_t *pmap_dev);
/* Replaces the data layout of SLAM_EKF.publishMap (W12m/slam_ekf.py:270-271):
 * data[y*xw + x] = int8(pmap[x][y]). */
int slam_grid_occupancy_data(slam_ctx *ctx, slam_grid *grid, int g, int8_t *data);
/* Number of in-bounds cell visits accumulated since creation / reset (SURVEY.md 8d "C"). */
int slam_grid_visits(slam_ctx *ctx, slam_grid *grid, uint64_t *visits_out);

/* ---- rays traced through a map ------------------------------------------------------- */
/* The read side of the grid; the reference has no counterpart (it only writes its map).  Both operators rest on
 *   trace(map, start, end, skip): with path = bresenham(start, end).path (W12m/bresenham.py:2-58, the cells
 *   Mapping.update visits, in its order), the smallest path index j >= skip whose cell is in bounds and has
 *   pmap == 100 (pmap as slam_grid_finalize_dev gives it), or -1; and the path length Lp.
 * The calls see every update enqueued before them on the context's stream and change nothing in the grid; the
 * context's sticky status is left untouched.  poses [B][3]; grid_of_batch [B] names the map of every hypothesis
 * (NULL: all read map 0; the host forms reject an entry outside [0, G), the device forms give that hypothesis
 * NaN / SLAM_RAY_BAD rows); cos_t, sin_t [n] as for slam_scan_to_points.  1 <= n <= 4096, B >= 1, B * n < 2^31,
 * 0 <= skip <= 2^20 (skip = 1 leaves the ray's own cell out).  Under slam_timing_* the pass that packs the
 * occupied bits counts as SLAM_K_FINALIZE, the trace as SLAM_K_GRID.
 *
 * slam_grid_raycast: the scan the map would give.  Beam i of hypothesis b ends where slam_grid_update_scans would
 * put a beam of range max_range (finite, > 0) cast from poses[b]: obs = u2T(pose).dot(pc), the ray origin is the
 * pose, both cells by int(scale * (v + off)) (W12m/slam_ekf.py:88-90, :115-123; mapping.py:33-36).
 * ranges_out [B][n] float32: the distance sqrt(dx*dx + dy*dy), in float64 and rounded once, from (x, y) of the
 * pose to the centre ((cx + 0.5) / scale - off_x, (cy + 0.5) / scale - off_y) of the cell found; +inf when the
 * ray meets no occupied cell; NaN for a non-finite pose or a cell index beyond 2^20.  cells_out (nullable)
 * [B][n][2] int32: the cell found, (-1, -1) otherwise. */
int slam_grid_raycast(slam_ctx *ctx, slam_grid *grid, const double *poses, int B, const int32_t *grid_of_batch,
                      const double *cos_t, const double *sin_t, int n, float max_range, int skip, float *ranges_out,
                      int32_t *cells_out);
int slam_grid_raycast_dev(slam_ctx *ctx, slam_grid *grid, const double *poses, int B, const int32_t *grid_of_batch,
                          const double *cos_t, const double *sin_t, int n, float max_range, int skip, float *ranges_out,
                          int32_t *cells_out);
/* slam_grid_scan_score: how a measured scan sits in the map.  ranges float32 [B][n], or one [n] for every
 * hypothesis when shared != 0.  Every beam is formed exactly as slam_grid_update_scans forms it (inf -> 30 m,
 * slam_ekf.py:119), traced to its own end cell, and put into one class: */
enum {
    SLAM_RAY_EMPTY = 0,     /* Lp == 0: the beam ends in the cell it starts in                         */
    SLAM_RAY_HIT = 1,       /* j == Lp - 1: the first occupied cell is the beam's end cell             */
    SLAM_RAY_BLOCKED = 2,   /* 0 <= j < Lp - 1: an occupied cell in front of the end cell              */
    SLAM_RAY_FREE = 3,      /* j == -1, the end cell is in bounds and its pmap is not 50               */
    SLAM_RAY_UNKNOWN = 4,   /* j == -1, the end cell is in bounds and its pmap is 50                   */
    SLAM_RAY_OUT = 5,       /* j == -1, the end cell is out of bounds                                  */
    SLAM_RAY_BAD = 6,       /* NaN / cell index beyond 2^20 (what raises in mapping.py:33-36), bad map */
    SLAM_RAY_CLASSES = 7
};
/* counts_out [B][SLAM_RAY_CLASSES] int32: beams per class (integer tallies: a hypothesis gets the same counts
 * alone, in any batch and in any order); class_out (nullable) [B][n] int8. */
int slam_grid_scan_score(slam_ctx *ctx, slam_grid *grid, const float *ranges, int shared, const double *poses, int B,
                         const int32_t *grid_of_batch, const double *cos_t, const double *sin_t, int n, int skip,
                         int32_t *counts_out, int8_t *class_out);
int slam_grid_scan_score_dev(slam_ctx *ctx, slam_grid *grid, const float *ranges, int shared, const double *poses, int B,
                             const int32_t *grid_of_batch, const double *cos_t, const double *sin_t, int n, int skip,
                             int32_t *counts_out, int8_t *class_out);

/* ---- view gain: the cells a scan from a pose would reveal ---------------------------------- */
/* What a robot would SEE from a pose, as a set of cells; the reference has no counterpart.  View b is poses[b] and
 * n beams formed exactly as slam_grid_raycast forms them (every range max_range, finite and > 0; the origin at the
 * pose; both cells through int(scale * (v + off))).  grid_of_batch as for the ray cast: NULL = every view reads
 * map 0.  For beam i with path = bresenham(start, end).path and (j, Lp) = trace(map, start, end, skip) the beam sees
 * the path indices skip <= k <= j when j >= 0 (the found cell included) and skip <= k < Lp when j == -1; a path cell
 * outside the map is seen by nobody.  S(b) is the set of in-bounds cells seen by any beam of the view. */
#define SLAM_VIEW_UNKNOWN 0   /* |S| with pmap == 50                                               */
#define SLAM_VIEW_FREE 1      /* |S| with pmap == 0                                                */
#define SLAM_VIEW_OCCUPIED 2  /* |S| with pmap == 100: the distinct first-hit cells                */
#define SLAM_VIEW_OPEN 3      /* beams with a valid end cell and j == -1                           */
#define SLAM_VIEW_COUNTS 4
/* counts_out [B][SLAM_VIEW_COUNTS] int32, pmap as slam_grid_finalize_dev would give it now.  seen_out (nullable)
 * uint32 [B][xw][ceil(yw / 32)]: bit y & 31 of word y >> 5 in row x is set iff (x, y) is in S(b); bits at y >= yw
 * are 0.  A beam whose end cell the index rule rejects (NaN, beyond 2^20) is skipped and not counted as OPEN.  A view
 * with a non-finite pose or a start index beyond 2^20 gets a row of -1 and zero seen words; so does, in the device
 * form, a view whose map entry is outside [0, G) (the host form rejects such an entry).  Neither raises the sticky
 * status.  Every view answers the same alone, in any batch, in any order, under any chunking and under either engine
 * (integer counts of a set).  The call sees every update enqueued before it on the context's stream, changes
 * nothing in the grid, keeps nothing between calls and leaves the sticky status untouched.
 * 1 <= n <= 4096, B >= 1, B * n < 2^31, 0 <= skip <= 2^20; with seen_out B * xw * ceil(yw / 32) < 2^31.
 * Context options: "gain_lds" - where a view's bit window lies: 1 = in LDS wherever the window of its box (the
 *   bounding box of its start and end cells, clipped to the map, whole words in y) fits 64 KiB, else in the
 *   workspace; 0 = always in the workspace (global atomics); -1 = automatic (default).  Same bits either way.
 *   "gain_ws_mb" - MiB the workspace windows may take, in (0, 2^20], fractions allowed; default 256.  One window slot
 *   holds a whole map's words; the views are taken over the slots that fit and no result depends on the cut; a call
 *   that may need a slot and whose single slot does not fit is SLAM_ERR_INVALID.
 * Under slam_timing_* the pass that packs the class bits counts as SLAM_K_FINALIZE, the rest as SLAM_K_GRID. */
int slam_grid_view_gain(slam_ctx *ctx, slam_grid *grid, const double *poses, int B, const int32_t *grid_of_batch,
                        const double *cos_t, const double *sin_t, int n, float max_range, int skip, int32_t *counts_out,
                        uint32_t *seen_out);
int slam_grid_view_gain_dev(slam_ctx *ctx, slam_grid *grid, const double *poses, int B, const int32_t *grid_of_batch,
                            const double *cos_t, const double *sin_t, int n, float max_range, int skip, int32_t *counts_out,
                            uint32_t *seen_out);

/* ---- distance field of the map and the window scan-to-map matcher --------------------------- */
/* Where a scan fits a map best; the reference has no counterpart.  Both calls see every update enqueued before
 * them on the context's stream, change nothing in the grid and leave the context's sticky status untouched.
 * "Occupied" is what the ray cast reads: pmap == 100 as slam_grid_finalize_dev would give it NOW.  The occupied
 * bits and the field of all G maps are REBUILT at the start of every call (slam_grid_match builds a field of its
 * own in the context's workspace); nothing is kept between calls.  Under slam_timing_* building the field counts
 * as SLAM_K_FINALIZE, the match as SLAM_K_GRID.
 *
 * slam_grid_distance_field: field_out [G][xw][yw] int16, in pmap's cell order,
 *   field[g][x][y] = min(cap, min over cells (u, v) of map g with pmap == 100 of (x-u)^2 + (y-v)^2),
 * the squared cell distance to the nearest occupied cell, exact for every 1 <= cap <= 32767; cap everywhere on a
 * map with no occupied cell. */
int slam_grid_distance_field(slam_ctx *ctx, slam_grid *grid, int cap, int16_t *field_out);
int slam_grid_distance_field_dev(slam_ctx *ctx, slam_grid *grid, int cap, int16_t *field_out);
/* slam_grid_match: every pose of a window around a start pose, scored on the field.  Hypothesis b reads map
 * gi = grid_of_batch[b] (NULL: map 0) around centre (cx, cy) = centres[b]; ranges float32 [B][n], or one [n] for
 * every hypothesis when shared != 0; cos_t, sin_t [n] as for slam_scan_to_points; rot_cs [B][K][2] the cosine and
 * sine of every rotation (made by the caller, as the beam tables are).  Candidate (k, i, j), 0 <= k < K,
 * 0 <= i <= 2*nx, 0 <= j <= 2*ny, has flat index (k*(2*nx+1) + i)*(2*ny+1) + j and
 *   px = cx + (double)(i - nx) * step,  py = cy + (double)(j - ny) * step,  c = rot_cs[b][k][0],  s = rot_cs[b][k][1];
 *   per beam t:  rr = (double)ranges[t];  used iff isfinite(rr) && ranges[t] < max_range (compared as float32);
 *                lx = cos_t[t]*rr;  ly = sin_t[t]*rr;
 *                x = c*lx + (-s)*ly + px*1.0;  y = s*lx + c*ly + py*1.0     (u2T(pose).dot(pc), W12m/slam_ekf.py:88-90,
 *                                                                             no fused multiply-add)
 *                cell = (int(scale*(x + off_x)), int(scale*(y + off_y)))     (mapping.py:33-36)
 *                cost += field[gi][cell] if the cell is in bounds, else cap  (also for NaN / a cell index beyond 2^20)
 * Costs are int32 sums over the used beams.  best_out [B]: the flat index of the smallest cost, ties to the LOWEST
 * flat index; best_cost_out [B] its cost; used_out (nullable) [B] the number of used beams; cost_out (nullable)
 * [B][K][2*nx+1][2*ny+1] every candidate's cost.  A scan with no used beam: cost 0 everywhere, best 0, used 0.
 * A hypothesis whose centre is not finite or whose centre cell index is beyond 2^20, or whose grid_of_batch entry
 * is outside [0, G) (host and device form alike), gets best -1, cost -1, used 0 and costs of -1; the others of
 * the batch are unaffected, and every hypothesis gets the same outputs alone, in any batch and in any order.
 * 1 <= cap <= 32767, 1 <= n <= 4096, n * cap < 2^31, B >= 1, B * n < 2^31, K >= 1, nx, ny >= 0,
 * K*(2*nx+1)*(2*ny+1) <= 2^24, B * K < 2^31, step finite and > 0, max_range > 0 (+inf: every finite range is used);
 * anything else is SLAM_ERR_INVALID and leaves the context as it was. */
int slam_grid_match(slam_ctx *ctx, slam_grid *grid, const float *ranges, int shared, const double *centres, int B,
                    const int32_t *grid_of_batch, const double *cos_t, const double *sin_t, int n, const double *rot_cs, int K,
                    int nx, int ny, double step, float max_range, int cap, int32_t *best_out, int32_t *best_cost_out,
                    int32_t *used_out, int32_t *cost_out);
int slam_grid_match_dev(slam_ctx *ctx, slam_grid *grid, const float *ranges, int shared, const double *centres, int B,
                        const int32_t *grid_of_batch, const double *cos_t, const double *sin_t, int n, const double *rot_cs,
                        int K, int nx, int ny, double step, float max_range, int cap, int32_t *best_out,
                        int32_t *best_cost_out, int32_t *used_out, int32_t *cost_out);

/* ---- global scan localisation: exact branch and bound on a pyramid of the field ------------- */
/* slam_grid_locate: the best pose of a scan over a whole map (or a rectangle of it) and a table of rotations -
 * "where in this map was this scan taken?" - exact, integer end to end, batched over (scan, map) pairs.  The
 * reference has no counterpart.  It changes nothing in the grid, leaves the context's sticky status untouched and
 * sees every update enqueued before it on the context's stream.
 *
 * Inputs.  ranges float32 [B][n], or one [n] for every hypothesis when shared != 0; grid_of_batch [B] (NULL: map 0);
 * cos_t, sin_t [n] as for slam_scan_to_points; rot_cs [K][2] the cosine and sine of every rotation, made by the
 * caller and shared by all hypotheses; region int32 [B][4] = (i0, j0, ni, nj), the robot cells searched (NULL: the
 * whole map); levels = H, 0 <= H <= 8; max_range, cap as for slam_grid_match.
 *
 * Field.  The field slam_grid_distance_field gives NOW at this cap, rebuilt at the start of the call for all G maps;
 * on it a pyramid P_1 .. P_H (below) for all G maps, in the context's workspace: a grid of many maps pays for all of
 * them, 2 bytes per cell of the field plus about 2 * H bytes per cell of the pyramid.  Nothing is kept between calls.
 * Under slam_timing_* field and pyramid count as SLAM_K_FINALIZE, the search as SLAM_K_GRID.
 *
 * Scan discretisation, once per rotation k with c = rot_cs[k][0], s = rot_cs[k][1].  Beam t is used iff
 * isfinite(rr) && ranges[t] < max_range (compared as float32), rr = (double)ranges[t].  For a used beam
 *   lx = cos_t[t]*rr;  ly = sin_t[t]*rr;  rx = c*lx + (-s)*ly;  ry = s*lx + c*ly     (no fused multiply-add)
 *   ax = (int)floor(scale*rx + 0.5);  ay = (int)floor(scale*ry + 0.5)
 * A used beam whose scale*rx or scale*ry is not finite, or is 2^20 or more in magnitude, is "off": it adds cap to
 * every candidate.
 *
 * Candidates.  (k, i, j), 0 <= k < K, i0 <= i < i0 + ni, j0 <= j < j0 + nj, is the robot at the CENTRE of cell (i, j)
 * with rotation k:
 *   cost = sum over the used beams of E(i + ax, j + ay),  E(x, y) = field[gi][x][y] inside the map, cap outside; int32.
 * This is the DISCRETISED-SCAN cost, not slam_grid_match's expression: a shift of the robot by whole cells shifts every
 * end cell by the same cells, by definition (slam_grid_match rounds every beam's end for every candidate anew).  That
 * is what makes the bound below exact.  The pose of a candidate is x = ((double)i + 0.5) / scale - off_x,
 * y = ((double)j + 0.5) / scale - off_y, theta = atan2(s, c).
 *
 * Answer.  The smallest (cost, flat), flat = (k*ni + (i - i0))*nj + (j - j0).  best_out [B][3] = (k, i, j);
 * best_cost_out [B]; used_out (nullable) [B] the number of used beams; stats_out (nullable) int64 [B][H + 2], below.
 * A hypothesis whose grid_of_batch entry is outside [0, G) gets best (-1, -1, -1), cost -1, used 0 and stats of 0; the
 * others of the batch are unaffected.  A scan with no used beam answers (0, i0, j0), cost 0, used 0 and stats of 0;
 * no search is run for it.
 *
 * The search is part of the contract (stats_out is tested).  P_h[x][y] = min over 0 <= a, b < 2^h of E(x + a, y + b)
 * for every integer (x, y); P_0 = E.  Node (h, k, I, J), 0 <= I < nI_h = ceil(ni / 2^h), 0 <= J < nJ_h = ceil(nj / 2^h),
 * covers the cells i0 + I*2^h .. i0 + (I+1)*2^h - 1 of the region and likewise in j; its bound is
 *   LB = sum over the used beams of P_h[i0 + I*2^h + ax][j0 + J*2^h + ay]      (an off beam adds cap).
 * A child's bound is never below its parent's; at level 0 the bound is the cost.  The children of (h, k, I, J) are
 * (h - 1, k, 2I + a, 2J + b), a, b in {0, 1}, those inside the level's node counts (they intersect the region).
 *   1. The incumbent.  Take the level-H node of smallest (LB, node index (k*nI_H + I)*nJ_H + J) and descend to level
 *      0, at every level to the child of smallest (LB, I, J).  U is the cost of the leaf reached; it is fixed before
 *      the sweep and never tightened during it.
 *   2. The sweep.  Every level-H node is evaluated; a node survives iff LB <= U; every child of a survivor is
 *      evaluated; at level 0 the survivors' keys cost << 32 | flat are minimised.
 * stats_out[b][h], h = 0 .. H, is the number of nodes evaluated at level h in the sweep; stats_out[b][H + 1] is U.
 * Because U is fixed first, every output, the statistics included, is the same alone, in any batch, in any order and
 * for any chunking (below).  H = 0 is brute force through the same code.
 *
 * Workspace.  The survivors of a level are kept in lists, sized for the worst case (an empty map: everything ties
 * and survives): 8 bytes per node of levels 1 .. H of every (hypothesis, rotation) pair.  The context option
 * "locate_ws_mb" bounds them; the pairs are taken in chunks whose lists fit, and no result depends on the cut.
 *
 * 1 <= cap <= 32767, 1 <= n <= 4096, n * cap < 2^31, B >= 1, K >= 1, B * K < 2^31, 0 <= H <= 8, max_range > 0 (+inf:
 * every finite range is used), every region inside the map with ni, nj >= 1, K * ni * nj < 2^31 for the largest
 * region, and the lists of ONE pair within "locate_ws_mb"; anything else is SLAM_ERR_INVALID, enqueues nothing and
 * leaves the context as it was.  In the device form `region` is device memory the host cannot check: K * xw * yw
 * < 2^31 is required whenever it is given, the lists are sized for the whole map, and a hypothesis whose region is
 * empty or not inside the map is answered like one whose map entry is outside [0, G). */
int slam_grid_locate(slam_ctx *ctx, slam_grid *grid, const float *ranges, int shared, int B, const int32_t *grid_of_batch,
                     const double *cos_t, const double *sin_t, int n, const double *rot_cs, int K, const int32_t *region,
                     int levels, float max_range, int cap, int32_t *best_out, int32_t *best_cost_out, int32_t *used_out,
                     int64_t *stats_out);
int slam_grid_locate_dev(slam_ctx *ctx, slam_grid *grid, const float *ranges, int shared, int B, const int32_t *grid_of_batch,
                         const double *cos_t, const double *sin_t, int n, const double *rot_cs, int K, const int32_t *region,
                         int levels, float max_range, int cap, int32_t *best_out, int32_t *best_cost_out, int32_t *used_out,
                         int64_t *stats_out);

/* ---- map frontiers: clustered exploration goals --------------------------------------------- */
/* slam_grid_frontiers: "where should the robot go next to see more of this map?" in the sense of Yamauchi - the free
 * cells that border unexplored space, grouped into 8-connected clusters, one member cell per cluster as a goal; integer
 * end to end, batched over maps.  The reference has no counterpart.  The call changes nothing in the grid, leaves the
 * context's sticky status untouched, sees every update enqueued before it on the context's stream and keeps nothing
 * between calls.  Under slam_timing_* the field counts as SLAM_K_FINALIZE, everything else as SLAM_K_GRID.
 *
 * Which map.  Query b reads map gi = grid_of_batch[b]; with grid_of_batch NULL gi = b, and B <= G is required (the
 * same map B times over is pointless, so NULL does not mean map 0 here).
 *
 * Which values.  pmap is what slam_grid_finalize_dev would give NOW: 0 free, 50 unknown, 100 occupied.
 *
 * Frontier cell.  F(x, y) iff all of
 *   - pmap[x][y] == 0;
 *   - at least one of the four neighbours (x+-1, y), (x, y+-1) that lie inside the map is 50 (a neighbour outside the
 *     map is not unknown; a cell with only a diagonal unknown neighbour does not qualify);
 *   - min_unknown == 0, or the number of cells equal to 50 among the cells of the (2*radius+1)^2 window centred on
 *     (x, y) that lie inside the map is at least min_unknown (a scan's rays leave unknown gaps between them: the plain
 *     rule alone marks thousands of cells inside explored space);
 *   - min_clear2 == 0, or field[gi][x][y] >= min_clear2, the field slam_grid_distance_field gives NOW at `cap`.
 * With min_clear2 == 0 no field is built and cap is ignored.  Otherwise the field is rebuilt for ALL G maps, as
 * slam_grid_match does: a grid of many maps pays for all of them, whatever B is.
 *
 * Clusters.  The 8-connected components of F; the label of a component is the smallest flat index x*yw + y of its
 * cells.  Of each: size; sx, sy the sums of x and of y (int64); the box x0, y0, x1, y1, inclusive; the rounded centroid
 * cxr = (2*sx + size) / (2*size), cyr likewise (integer division); the representative: the member with the smallest
 * (x-cxr)^2 + (y-cyr)^2, ties to the lowest flat index.  (The centroid of a crescent is no frontier cell and may lie in
 * a wall; the representative always is a frontier cell.)
 *
 * Outputs.  count_out [B][2]: the number of clusters with size >= min_size - the TRUE number, also beyond
 * max_clusters - and the number of frontier cells.  clusters_out [B][M][8], M = max_clusters, rows (label, size, rep_x,
 * rep_y, x0, y0, x1, y1), and sums_out [B][M][2], rows (sx, sy): the kept clusters in ASCENDING LABEL order, the first
 * min(count, M) of them; every later row is -1.  labels_out (nullable) [B][xw][yw]: the label of every frontier cell,
 * those of clusters below min_size included, -1 elsewhere.  With M == 0 the two tables may be NULL.  clusters_out must
 * be 8-byte aligned (the device form).  A query whose map entry is outside [0, G) gets counts (-1, -1), rows of -1 and
 * labels of -1, in both forms; the others are unaffected.  Every query gets the same outputs alone, in any batch, in
 * any order and under any chunking (below).
 *
 * Workspace.  In the context's workspace, 4 bytes per cell per query of labels and 8 bytes per 1024 cells of counts,
 * bounded by the context option "frontier_ws_mb"; the queries are taken in chunks that fit and no result depends on the
 * cut.
 *
 * B >= 1; 0 <= radius <= 8; 0 <= min_unknown <= (2*radius+1)^2; min_clear2 >= 0, and 1 <= cap <= 32767 and
 * min_clear2 <= cap when min_clear2 > 0; min_size >= 1; 0 <= max_clusters <= 65536; B * max(M, 1) < 2^31; a map of at
 * most 32768 cells in either axis; the workspace of ONE query within "frontier_ws_mb"; anything else is
 * SLAM_ERR_INVALID, enqueues nothing and leaves the context as it was. */
int slam_grid_frontiers(slam_ctx *ctx, slam_grid *grid, int B, const int32_t *grid_of_batch, int radius, int min_unknown,
                        int min_clear2, int cap, int min_size, int max_clusters, int32_t *count_out, int32_t *clusters_out,
                        int64_t *sums_out, int32_t *labels_out);
int slam_grid_frontiers_dev(slam_ctx *ctx, slam_grid *grid, int B, const int32_t *grid_of_batch, int radius, int min_unknown,
                            int min_clear2, int cap, int min_size, int max_clusters, int32_t *count_out, int32_t *clusters_out,
                            int64_t *sums_out, int32_t *labels_out);

/* ---- travel-cost field: reachable cells, costs and paths -------------------------------------- */
/* slam_grid_travel: "what does it cost to drive from here to every cell of this map, and how?" - the cost-to-go field
 * from the robot's cell over the traversable cells, the move back from every cell and the paths to a list of goals (the
 * representatives of slam_grid_frontiers, say); integer end to end, one answer, batched over maps.  The reference has no
 * counterpart.  The call changes nothing in the grid, leaves the context's sticky status untouched, sees every update
 * enqueued before it on the context's stream and keeps nothing between calls.  Under slam_timing_* the field counts as
 * SLAM_K_FINALIZE, everything else as SLAM_K_GRID.
 *
 * Which map.  Query b reads map gi = grid_of_batch[b]; with grid_of_batch NULL gi = b, and B <= G is required, as for
 * the frontiers.
 *
 * Which values.  pmap is what slam_grid_finalize_dev would give NOW: 0 free, 50 unknown, 100 occupied.
 *
 * Sources.  sources [B][S][2], cells (x, y).  An entry outside the map is skipped; a query with no source inside its
 * map answers -1 everywhere with status 0.
 *
 * Traversable set T of a query.  A cell of the map is in T iff
 *   (a) it lies within Chebyshev distance `foot` of a source of the query that lies inside the map - the robot stands
 *       there, whatever the map says (its own cell turns occupied once enough rays have started in it) - or
 *   (b) its class is travelable: pmap == 0, or with through_unknown != 0 also pmap == 50; AND its clearance is enough:
 *       min_clear2 == 0, or field[gi][x][y] >= min_clear2, the field slam_grid_distance_field gives NOW at `cap`.
 * With min_clear2 == 0 no field is built and cap is ignored.  Otherwise the field is rebuilt for ALL G maps, as the
 * frontiers and the matcher do.
 *
 * Moves.  Direction codes d = 0..7 = (1,0), (0,1), (-1,0), (0,-1), (1,1), (-1,1), (-1,-1), (1,-1); codes 0 to 3 cost
 * SLAM_TRAVEL_STRAIGHT, codes 4 to 7 SLAM_TRAVEL_DIAGONAL.  A move from u to v is allowed iff both cells are in T; a
 * diagonal move also needs the two cells it passes between, (ux+dx, uy) and (ux, uy+dy), in T: no corner cutting, two
 * occupied cells that touch diagonally are a wall.  The graph is undirected.
 *
 * Outputs.  cost_out (nullable) [B][xw][yw], pmap's cell order: the least sum of move costs from any source; a source
 * has 0; a cell that no source reaches, or that is not in T, has -1.  dir_out (nullable) int8 [B][xw][yw]: the LOWEST
 * code d such that the move from the cell in direction d is allowed and cost[neighbour] + w_d == cost[cell]; sources
 * and unreached cells have -1.  dir_out is defined from the final costs, not from the order anything ran in, so both
 * arrays are unique, and every query answers the same alone, in any batch, in any order and under any chunking (below).
 *
 * Goals (optional).  goals (nullable) [B][Q][2]; goal_cost_out [B][Q]: the goal cell's cost, -1 for a goal outside the
 * map or unreached; path_len_out [B][Q]: the TRUE number of cells of the path that follows dir from the goal to a
 * source, both ends included - 1 for a goal on a source, 0 where the cost is -1; path_out (nullable when path_cap == 0)
 * [B][Q][path_cap][2]: the path source first, min(len, path_cap) cells of it, every later row -1.  Entries of -1 are
 * legal goals and answer -1 / 0, so the rep_x, rep_y columns of slam_grid_frontiers' table go straight in.  With goals
 * NULL or Q == 0 the three goal outputs are not touched.
 *
 * status_out [B]: 0 answered; -1 the map entry is outside [0, G) - then every output of the query is -1 and the lengths
 * are 0, in both forms, the others unaffected; SLAM_TRAVEL_TRIPS a hard trip bound of the relaxation was reached - the
 * query's outputs are then not answers.  (Costs only decrease, so the relaxation ends; the tile with the lowest pending
 * cost goes first, which bounds the activations of a tile by the cells around it: DESIGN.md section 19.)
 *
 * Workspace.  In the context's workspace per query: 4 bytes per cell of costs when cost_out is NULL (otherwise the
 * relaxation runs in cost_out), the bits of T in rows padded to 64, 4 bytes per tile of 64 x 64 cells; bounded by the
 * context option "travel_ws_mb"; the queries are taken in chunks that fit and no result depends on the cut.
 *
 * B >= 1; 1 <= S <= 64; 0 <= foot <= 8; min_clear2 >= 0, and 1 <= cap <= 32767 and min_clear2 <= cap when
 * min_clear2 > 0; 0 <= Q <= 65536; 0 <= path_cap <= xw*yw; B * max(Q, 1) * max(path_cap, 1) < 2^31; 14 * xw * yw <
 * 2^31; B <= G without routing; the workspace of ONE query within "travel_ws_mb"; status_out and sources not NULL; at
 * least one of cost_out, dir_out and the goal outputs (goals with Q > 0, goal_cost_out, path_len_out, and path_out
 * when path_cap > 0) asked for; anything else is SLAM_ERR_INVALID, enqueues nothing and leaves the context as it was. */
#define SLAM_TRAVEL_STRAIGHT 10
#define SLAM_TRAVEL_DIAGONAL 14
#define SLAM_TRAVEL_TRIPS 1
int slam_grid_travel(slam_ctx *ctx, slam_grid *grid, int B, const int32_t *grid_of_batch, const int32_t *sources, int S, int foot,
                     int through_unknown, int min_clear2, int cap, const int32_t *goals, int Q, int path_cap, int32_t *status_out,
                     int32_t *cost_out, int8_t *dir_out, int32_t *goal_cost_out, int32_t *path_len_out, int32_t *path_out);
int slam_grid_travel_dev(slam_ctx *ctx, slam_grid *grid, int B, const int32_t *grid_of_batch, const int32_t *sources, int S, int foot,
                         int through_unknown, int min_clear2, int cap, const int32_t *goals, int Q, int path_cap, int32_t *status_out,
                         int32_t *cost_out, int8_t *dir_out, int32_t *goal_cost_out, int32_t *path_len_out, int32_t *path_out);

/* ---- Monte Carlo localisation on the distance field ----------------------------------------- */
/* F particle filters of P particles each, weighed against their filter's scan on the field above and resampled on
 * the device; the reference has no counterpart.  State: poses float64 [F][P][3] (x, y, theta; theta is not
 * wrapped) and acc int32 [F][P], a particle's accumulated cost since its filter last resampled (the integer
 * log-weight, >= 0).  acc == SLAM_MCL_DEAD marks a dead particle; it stays dead until a resample replaces it.
 * Filter f reads map grid_of_filter[f] (NULL: map 0).  Everything that decides an index is integer: a filter gets
 * the same outputs alone, in any batch and in any order.  Both calls change nothing in the grid and leave the
 * context's sticky status untouched.  Under slam_timing_* building the field counts as SLAM_K_FINALIZE, the weigh
 * and the resampling as SLAM_K_GRID.
 *
 * slam_mcl_weigh: moves the particles, then scores the filter's scan from every particle.
 *   motion (nullable) [F][3]; noise (nullable, only together with motion) [F][P][3], made by the caller (no random
 *   numbers are drawn on the device):  d = motion[f] + noise[f][p] componentwise (absent noise: motion[f]), then
 *     x' = (x + cos(th)*dx) - sin(th)*dy;  y' = (y + sin(th)*dx) + cos(th)*dy;  th' = th + dth     (icp.py:185-190)
 *   is written back to poses and the cost is taken from the NEW pose (motion NULL: poses is not written).
 *   Cost: c = cos(th), s = sin(th) on the device; per beam t of ranges [F][n] exactly slam_grid_match's expression
 *   with px, py the particle's position: used iff isfinite(rr) && ranges[t] < max_range (as float32);
 *   lx = cos_t[t]*rr; ly = sin_t[t]*rr; x = c*lx + (-s)*ly + px*1.0; y = s*lx + c*ly + py*1.0; both through
 *   int(scale*(v + off)); cost += field[gi][cell] if the cell is in bounds, else cap.  No used beam: cost 0.
 *   A particle is dead if a component of its (new) pose is not finite, if its own cell index is NaN or beyond 2^20,
 *   if its filter's grid_of_filter entry is outside [0, G), or if it arrives with acc == SLAM_MCL_DEAD: its
 *   cost_out is -1 and its acc SLAM_MCL_DEAD (its pose is still moved).  A live one: acc = min(acc + cost, 2^30).
 *   acc (nullable: nothing is accumulated), cost_out (nullable) int32 [F][P]; used_out (nullable) [F] the number of
 *   used beams of the filter's scan (whatever its map entry).
 *   field (nullable) int16 [G][xw][yw]: a field made by slam_grid_distance_field_dev at the SAME cap; it is used
 *   and nothing is built (a static map costs no rebuild per scan).  NULL: the field of all G maps is rebuilt in the
 *   context's workspace at the start of the call, as slam_grid_match does.  In the host form `field` is a host array.
 *
 * slam_mcl_resample: weights, estimate, effective sample size and systematic resampling.
 *   amin = the smallest acc among filter f's live particles; a live particle has
 *     w[p] = min(table[min((acc[p] - amin) >> shift, T - 1)], 2^20),  a dead one 0;
 *   S = sum w, Q = sum w^2 (uint64);  ESS = (double)S * (double)S / (double)Q, 0 when S == 0.
 *   est_out [F][4] float64 = (sum w x / S, sum w y / S, atan2(sum w sin th, sum w cos th), ESS), taken BEFORE
 *   resampling over the particles of non-zero weight (summation order: the library's, fixed for a given P); the
 *   first three are NaN when S == 0.  info_out [F][4] int32 = (best, live, resampled, amin): best the live particle
 *   of lowest acc, ties to the lowest index, -1 when none is alive; amin 0 when none is alive.
 *   Filter f resamples iff S > 0 and ESS < ess_frac * P (+inf: always, 0: never - a pure estimate).  Then
 *     o = min((uint64)(u0[f] * (double)S), S - 1);  slot j has threshold t_j = o + j*S;  cum = inclusive prefix sums
 *     of w;  ancestor a_j = the smallest i with cum[i] * P > t_j;  poses_out[j] = poses[a_j];  acc[j] = 0.
 *   A filter that does not resample copies its poses, keeps acc and gets the identity in ancestors_out (nullable
 *   int32 [F][P]).  poses_out [F][P][3] must not be poses.  u0 [F] must lie in [0, 1): the host form rejects
 *   anything else, in the device form that is the caller's duty (a value outside is clamped into the range, NaN
 *   counts as 0).  table uint32 [T]: the host form rejects an entry above 2^20, the device form clamps it.
 *
 * F >= 1, 1 <= P <= 2^20, F * P < 2^31, 1 <= n <= 4096, F * n < 2^31, 1 <= cap <= 32767, max_range > 0, noise only
 * with motion, 1 <= T <= 65536, 0 <= shift <= 30, ess_frac >= 0 and not NaN, required pointers non-null; anything
 * else is SLAM_ERR_INVALID, enqueues nothing and leaves the context as it was. */
#define SLAM_MCL_DEAD 2147483647
int slam_mcl_weigh(slam_ctx *ctx, slam_grid *grid, double *poses, const double *motion, const double *noise,
                   const float *ranges, const double *cos_t, const double *sin_t, const int32_t *grid_of_filter, int F, int P,
                   int n, float max_range, int cap, const int16_t *field, int32_t *acc, int32_t *cost_out, int32_t *used_out);
int slam_mcl_weigh_dev(slam_ctx *ctx, slam_grid *grid, double *poses, const double *motion, const double *noise,
                       const float *ranges, const double *cos_t, const double *sin_t, const int32_t *grid_of_filter, int F,
                       int P, int n, float max_range, int cap, const int16_t *field, int32_t *acc, int32_t *cost_out,
                       int32_t *used_out);
int slam_mcl_resample(slam_ctx *ctx, const double *poses, int32_t *acc, const uint32_t *table, int T, int shift,
                      const double *u0, double ess_frac, int F, int P, double *poses_out, int32_t *ancestors_out,
                      double *est_out, int32_t *info_out);
int slam_mcl_resample_dev(slam_ctx *ctx, const double *poses, int32_t *acc, const uint32_t *table, int T, int shift,
                          const double *u0, double ess_frac, int F, int P, double *poses_out, int32_t *ancestors_out,
                          double *est_out, int32_t *info_out);

/* ---- grid FastSLAM: a map per particle that follows resampling --------------------------------- */
/* Particle (f, p) of F filters of P particles owns map map0 + f*P + p of the grid.  A step of the filter is five calls:
 * slam_mcl_weigh_maps (every particle on ITS OWN map), slam_mcl_resample, slam_mcl_settle (every survivor keeps its
 * slot), slam_grid_copy_maps (only the maps of slots whose particle died are copied, in place, from a survivor's map
 * that nobody overwrites) and slam_grid_update_particles (the scan integrated from every particle).  The reference has
 * no counterpart.  Everything that decides an index is integer.  The new kernels count as SLAM_K_GRID, the field build
 * as SLAM_K_FINALIZE.  A failed up-front check is SLAM_ERR_INVALID, enqueues nothing and leaves the context as it was.
 *
 * slam_mcl_weigh_maps: slam_mcl_weigh with grid_of_particle int32 [F][P] where grid_of_filter stands; NULL: particle
 *   (f, p) reads map f*P + p, which needs F*P <= G.  Every other argument and rule is slam_mcl_weigh's, with the
 *   PARTICLE's map entry outside [0, G) in place of the filter's among the "dead" rules.
 *
 * slam_mcl_settle: per filter, cnt[i] = the number of slots j with ancestors[j] == i.  A slot with cnt[i] >= 1 gets
 *   settled[i] = i; the free slots (cnt == 0), in ascending order, receive in ascending order the surplus list: every i
 *   repeated cnt[i] - 1 times (the two lists are equally long).  The identity gives the identity; the ancestors need
 *   not be monotone.  No slot that is a source (settled[j] for some j != itself) is a destination.
 *   poses_out[j] = poses_src[settled[j]] (poses_src: the particles BEFORE slam_mcl_resample gathered them; must not be
 *   poses_out); map_src_out[f][p] = map0 + f*P + settled[f][p]; moved_out[f] = the slots with settled[j] != j.
 *   ancestors, settled_out int32 [F][P]; poses_src, poses_out, map_src_out, moved_out nullable.  F >= 1,
 *   1 <= P <= 4096, F*P < 2^31, map0 >= 0, map0 + F*P < 2^31.  The host form rejects an ancestor outside [0, P), the
 *   device form clamps it into the range.
 *
 * slam_grid_copy_maps: for k < count, map d = first + k becomes a copy of map s = src[k]: pass, hit and, when the grid
 *   keeps one, the live pmap (one that was current stays current).  s == d or s outside [0, G): the map is kept and
 *   copied_out[k] (nullable int32 [count]) is 0.  A source that is itself a destination of this call (first <= s <
 *   first + count and src[s - first] != s) is SLAM_ERR_INVALID in the host form; in the device form that destination is
 *   left unchanged and copied_out[k] is -1.  Otherwise copied_out[k] is 1.  first >= 0, count >= 1, first + count <= G.
 *   The visit counters of slam_grid_visits are not touched.
 *
 * slam_grid_update_particles: for every (f, p) exactly what slam_grid_update_scans does for the one scan ranges[f]
 *   (float32 [F][n]) at pose poses[f][p] (float64 [F][P][3]; centres NULL, inf -> 30 m), into map map0 + f*P + p.  A
 *   particle with acc[f][p] == SLAM_MCL_DEAD (acc nullable int32 [F][P]) casts nothing and raises no sticky status.
 *   n <= 65535, map0 >= 0, map0 + F*P <= G.  The host form ends with the status check of slam_grid_update_scans. */
int slam_mcl_weigh_maps(slam_ctx *ctx, slam_grid *grid, double *poses, const double *motion, const double *noise,
                        const float *ranges, const double *cos_t, const double *sin_t, const int32_t *grid_of_particle, int F,
                        int P, int n, float max_range, int cap, const int16_t *field, int32_t *acc, int32_t *cost_out,
                        int32_t *used_out);
int slam_mcl_weigh_maps_dev(slam_ctx *ctx, slam_grid *grid, double *poses, const double *motion, const double *noise,
                            const float *ranges, const double *cos_t, const double *sin_t, const int32_t *grid_of_particle,
                            int F, int P, int n, float max_range, int cap, const int16_t *field, int32_t *acc,
                            int32_t *cost_out, int32_t *used_out);
int slam_mcl_settle(slam_ctx *ctx, const int32_t *ancestors, const double *poses_src, int F, int P, int map0,
                    int32_t *settled_out, double *poses_out, int32_t *map_src_out, int32_t *moved_out);
int slam_mcl_settle_dev(slam_ctx *ctx, const int32_t *ancestors, const double *poses_src, int F, int P, int map0,
                        int32_t *settled_out, double *poses_out, int32_t *map_src_out, int32_t *moved_out);
int slam_grid_copy_maps(slam_ctx *ctx, slam_grid *grid, const int32_t *src, int first, int count, int32_t *copied_out);
int slam_grid_copy_maps_dev(slam_ctx *ctx, slam_grid *grid, const int32_t *src, int first, int count, int32_t *copied_out);
int slam_grid_update_particles(slam_ctx *ctx, slam_grid *grid, const float *ranges, const double *cos_t, const double *sin_t,
                               const double *poses, const int32_t *acc, int F, int P, int n, int map0);
int slam_grid_update_particles_dev(slam_ctx *ctx, slam_grid *grid, const float *ranges, const double *cos_t,
                                   const double *sin_t, const double *poses, const int32_t *acc, int F, int P, int n, int map0);

/* Replaces bresenham(start, end).path (W12m/bresenham.py:2-58), B lines at once.
 * starts, ends [B][2] int32.  lens_out [B] receives each path length; cells_out (may be
 * NULL) receives the paths, line b at cells_out + 2*offsets[b] (x, y interleaved), with
 * room for max(|dx|,|dy|)+1 cells each. */
int slam_bresenham_batch(slam_ctx *ctx, const int32_t *starts, const int32_t *ends, int B,
                         const int64_t *offsets, int32_t *lens_out, int32_t *cells_out, int64_t total_cells);

/* ---- fused replay ------------------------------------------------------------------ */
/* The per-scan unit of BASELINE.json (one ICP.process + one Mapping.update) over L scan
 * streams of n_scan scans: SLAM_EKF.laserCallback (W12m/slam_ekf.py:63-95) without its
 * out-of-scope EKF / landmark steps, the map being cast from the dead-reckoned ICP pose
 * (slam_node_replay below is the node with them).
 * ranges [L][n_scan][n] float32; pose0 [L][3]; grid may be NULL (ICP + poses only);
 * grid_of_traj [L] or NULL (all into map 0).
 * poses_out [L][n_scan-1][3]; T_out [L][n_scan-1][9], iters_out [L][n_scan-1] may be NULL.
 * dtype: storage type of the intermediate point buffers the ICP reads. */
int slam_replay(slam_ctx *ctx, const float *ranges, const double *cos_t, const double *sin_t, int L,
                int n_scan, int n, int dtype, int max_iter, double tol, const double *pose0,
                slam_grid *grid, const int32_t *grid_of_traj, double *poses_out, double *T_out,
                int32_t *iters_out);
/* Device form.  pts_ws is unused (may be NULL): polar->Cartesian is fused into the ICP
 * kernel, which forms the points of storage type `dtype` in registers; the parameter is
 * kept for ABI stability. */
int slam_replay_dev(slam_ctx *ctx, const float *ranges, const double *cos_t, const double *sin_t, int L,
                    int n_scan, int n, int dtype, int max_iter, double tol, const double *pose0,
                    slam_grid *grid, const int32_t *grid_of_traj, void *pts_ws, double *poses_out,
                    double *T_out, int32_t *iters_out);

/* ---- particle hypotheses (BASELINE.json configs[2]) --------------------------------- */
/* The same two operators batched over P pose hypotheses of ONE scan pair (the reference
 * has no particle filter; this is ICP.process + Mapping.update evaluated P times with
 * perturbed priors).  ranges2 [2][n] float32: previous scan (target) then current scan
 * (source).  prior [P][6] (nullable): 2x3 matrix applied to the source points before the
 * solve; the hypothesis' motion is then M = T.[prior; 0 0 1].  pose_prev [P][3].
 * Per hypothesis p: T_p = ICP.process(tar, prior_p . src) (W12m/icp.py:38-88);
 * pose_p = pose_prev_p (+) M_p (icp.py:185-190); the current scan is ray-cast from pose_p
 * into map p of `grid` (needs G >= P maps; W12m/mapping.py:22-51).
 * poses_out [P][3]; T_out [P][9]; iters_out [P] (host form: T_out / iters_out nullable). */
int slam_particles(slam_ctx *ctx, const float *ranges2, const double *cos_t, const double *sin_t, int n, int dtype,
                   const double *prior, const double *pose_prev, int P, int max_iter, double tol, slam_grid *grid,
                   double *poses_out, double *T_out, int32_t *iters_out);
/* Device form: T_out is required; pts_ws is unused (may be NULL), as in slam_replay_dev. */
int slam_particles_dev(slam_ctx *ctx, const float *ranges2, const double *cos_t, const double *sin_t, int n, int dtype,
                       const double *prior, const double *pose_prev, int P, int max_iter, double tol, slam_grid *grid,
                       void *pts_ws, double *poses_out, double *T_out, int32_t *iters_out);

/* ---- scan-to-map observation -------------------------------------- */
/* W9 = "W9_Fusion Localization (LiDAR Odometry)/course_agv_slam/scripts".
 * Replaces the obstacle extraction of Localization.updateMap (W9/localization.py:54-60):
 * cells > 20 or < -0.5 (occupied and unknown) -> (tx*resolution + origin_x, ty*resolution +
 * origin_y).  map: int8 [height*width]; wire_layout != 0: OccupancyGrid order data[y*width + x]
 * (what the reference receives), else [x][y] (Mapping.pmap order).  Up to cap points are
 * written (in arbitrary order); *count_out receives the number found. */
int slam_map_obstacles(slam_ctx *ctx, const int8_t *map, int width, int height, int wire_layout, double resolution,
                       double origin_x, double origin_y, double *ox, double *oy, int cap, int *count_out);
int slam_map_obstacles_dev(slam_ctx *ctx, const int8_t *map, int width, int height, int wire_layout, double resolution,
                           double origin_x, double origin_y, double *ox, double *oy, int cap, int *count_dev);

/* Replaces Localization.laserEstimation(msg, x) (W9/localization.py:128-150) for B pose
 * hypotheses: obstacle points (ox, oy)[K], poses [B][3] -> ranges_out [B][n] float64, the
 * scan the map would produce (100.0 where no obstacle falls into a beam's bin). */
int slam_virtual_scan(slam_ctx *ctx, const double *ox, const double *oy, int K, const double *poses, int B,
                      double angle_min, double angle_increment, int n, double *ranges_out);
int slam_virtual_scan_dev(slam_ctx *ctx, const double *ox, const double *oy, int K, const double *poses, int B,
                          double angle_min, double angle_increment, int n, double *ranges_out);

/* Replaces Localization.laserToNumpy (W9/localization.py:168-174) for float64 ranges (the
 * virtual scan above is float64, not a float32 wire message): ranges [B][n] ->
 * pts_out [B][2][n] float64. */
int slam_scan_to_points_f64(slam_ctx *ctx, const double *ranges, const double *cos_t, const double *sin_t, int B, int n,
                            double *pts_out);
int slam_scan_to_points_f64_dev(slam_ctx *ctx, const double *ranges, const double *cos_t, const double *sin_t, int B,
                                int n, double *pts_out);

/* Replaces Localization.calc_map_observation(msg) (W9/localization.py:152-157) for B pose
 * hypotheses: virtual scan of the map from poses[b] -> laserToNumpy (:168-174) -> ICP.process
 * against the current scan's points src ([B][2][n] float64, or one shared [2][n] set when
 * src_shared != 0).  cos_t, sin_t [n] as for slam_scan_to_points.  T_out [B][9];
 * iters_out [B] nullable. */
int slam_map_observation(slam_ctx *ctx, const double *ox, const double *oy, int K, const double *poses,
                         const double *src, int B, int n, int src_shared, const double *cos_t, const double *sin_t,
                         double angle_min, double angle_increment, int max_iter, double tol, double *T_out,
                         int32_t *iters_out);
/* Device form: needs workspaces vranges_ws [B][n] and vpts_ws [B][2][n] (float64). */
int slam_map_observation_dev(slam_ctx *ctx, const double *ox, const double *oy, int K, const double *poses,
                             const double *src, int B, int n, int src_shared, const double *cos_t,
                             const double *sin_t, double angle_min, double angle_increment, int max_iter, double tol,
                             double *vranges_ws, double *vpts_ws, double *T_out, int32_t *iters_out);

/* ---- DWA local planner --------------------------------------------------------------- */
/* NAV = "W12_LiDAR SLAM/w12-mapping/course_agv_nav/scripts".  Replaces dwa_control(x, config,
 * goal, ob) (NAV/dwa.py:10-16, with calc_dynamic_window :65-83 and calc_control_and_trajectory
 * :85-113) for B planners in one launch; the local planner node runs it on every control step
 * (NAV/local_planner.py:135-150).
 * config: double[SLAM_DWA_CONFIG_LEN], the fields of Config (NAV/dwa.py:23-45) in this order:
 *   max_speed, min_speed, max_yawrate, max_accel, max_dyawrate, dt, v_reso, yawrate_reso,
 *   predict_time, to_goal_cost_gain, speed_cost_gain, obstacle_cost_gain,
 *   robot_type (0 = RobotType.circle, 1 = RobotType.rectangle), robot_radius, robot_width, robot_length.
 *   Every value must be finite; dt, v_reso and yawrate_reso must be > 0 (the reference loops
 *   forever or raises) and predict_time >= 0 (else its trajectory has no last row).
 * Semantics are the reference's as it executes (DESIGN.md "DWA local planner"):
 *  - samples: numpy float arange of both window axes, v outer: sample s = iv * nw + iw (:95-96);
 *  - rollout: row 0 = the state, then one row per pass of `while time <= predict_time`
 *    (time accumulated in float64, :115-124); each step yaw, then x, then y (:57-63);
 *  - rectangle robots collide iff some (row, obstacle) pair has |tx-ox| <= robot_length/2 and
 *    |ty-oy| <= robot_width/2 in the PLANNING frame: the reference's rotation is a no-op
 *    (`np.reshape(-1, 1)` is [-1], :138) and is reproduced, not fixed; circle robots iff some
 *    hypot <= robot_radius; the obstacle cost is inf on collision, else 1 / min hypot (:126-160);
 *  - final cost to_goal + speed + obstacle gains, summed left to right (0 * inf = NaN, :101-105);
 *  - selection as `if min_cost >= final_cost` from inf (:108): NaN never wins, ties go to the
 *    LARGER index; no winner (empty window, all NaN): u = (0, 0), index -1, cost inf;
 *  - a state whose v or omega is not finite plans an empty window (the reference raises for inf).
 * states [B][5] (x, y, yaw, v, omega); goals [B][2].  obstacles: [B][2][M] structure-of-arrays
 * (M x values, then M y values: the layout slam_map_obstacles_dev writes with oy = ox + M), or one
 * shared [2][M] set when shared != 0.  counts: NULL (every planner uses M obstacles) or [B]
 * (one value when shared): planner b uses the first min(counts[b], M).  The host form rejects a
 * count outside [1, M] (np.min of an empty set raises in the reference); in the device form a
 * count < 1 gives index -1.
 * Outputs: u_out [B][2], cost_out [B] (the winner's final cost), index_out [B];
 * nullable: counts_out [B][2] (nv, nw), costs_out [B][s_cap] (every sample's final cost; samples
 * at s >= s_cap are not written), traj_out [B][rows][5] (the winner's trajectory; with no winner
 * row 0 is the state and the other rows NaN).  rows and the sample bound come from slam_dwa_shape.
 * Obstacle sets of any size are staged through LDS in tiles; B is bounded by memory. */
#define SLAM_DWA_CONFIG_LEN 16
int slam_dwa(slam_ctx *ctx, const double *states, const double *goals, const double *obstacles, const int32_t *counts,
             int M, int shared, const double *config, int B, double *u_out, double *cost_out, int32_t *index_out,
             int32_t *counts_out, double *costs_out, int s_cap, double *traj_out);
int slam_dwa_dev(slam_ctx *ctx, const double *states, const double *goals, const double *obstacles,
                 const int32_t *counts, int M, int shared, const double *config, int B, double *u_out,
                 double *cost_out, int32_t *index_out, int32_t *counts_out, double *costs_out, int s_cap,
                 double *traj_out);
/* The same with the obstacles of LocalPlanner.laserCallback (NAV/local_planner.py:57-68)
 * formed inside the launch: the sentinel (100, 100), then (cos_t[i] * r, sin_t[i] * r) for every
 * beam i with r < threshold (inf and NaN ranges drop out).  ranges [B][n] float32 (one shared
 * scan when shared != 0), n <= 4095; cos_t, sin_t [n] = cos / sin(angle_min + angle_increment * i)
 * computed by the caller; threshold = max_speed * predict_time in the reference (:34). */
int slam_dwa_scans(slam_ctx *ctx, const double *states, const double *goals, const float *ranges, int n, int shared,
                   const double *cos_t, const double *sin_t, double threshold, const double *config, int B,
                   double *u_out, double *cost_out, int32_t *index_out, int32_t *counts_out, double *costs_out,
                   int s_cap, double *traj_out);
int slam_dwa_scans_dev(slam_ctx *ctx, const double *states, const double *goals, const float *ranges, int n,
                       int shared, const double *cos_t, const double *sin_t, double threshold, const double *config,
                       int B, double *u_out, double *cost_out, int32_t *index_out, int32_t *counts_out,
                       double *costs_out, int s_cap, double *traj_out);
/* Host only, no context: validate a config (as above) and return the trajectory rows of
 * predict_trajectory (NAV/dwa.py:115-124) and upper bounds of the two sample axes over every
 * state (nv <= nv_cap, nw <= nw_cap; size costs_out with s_cap = nv_cap * nw_cap).  Configs whose
 * rows exceed 65 536 or whose nv_cap * nw_cap exceeds 2^20 are rejected (SLAM_ERR_INVALID). */
int slam_dwa_shape(const double *config, int *rows_out, int *nv_cap_out, int *nw_cap_out);

/* ---- A* global planner --------------------------------------------------------------- */
/* NAV as above.  Replaces find_path(map, start, goal).start_find() (NAV/global_planner.py:133-238)
 * for B queries over G maps in one call; the global planner node runs it on every goal
 * (NAV/global_planner.py:87-98).  Semantics are the reference's as it executes (DESIGN.md "A* global planner"):
 *  - maps: G int8 maps of H rows x W columns (row = y, column = x); wire_layout != 0: OccupancyGrid
 *    order data[y*W + x] (what map_callback reshapes, :61-70), else [x][y] (Mapping.pmap order,
 *    what slam_grid_live_pmap holds).  100 and -1 are obstacles, 0 is free, any other value
 *    (99, SLAM_EKF's 50 for unknown cells) is neither;
 *  - inflation (:148-155, with 129 -> span and 2 -> r): the in-place loop over rows and columns
 *    [r, span - r) writing 99 over the (2r+1)^2 window of every cell that still holds 100 or -1
 *    when the loop reaches it - a greedy set, not a dilation; inflating twice changes nothing;
 *  - start / goal [B][2] (row, col) as find_path receives them: it subtracts 1 from both (:137-142);
 *  - search (:157-238): 8 moves of cost 10, h = 10 * Manhattan distance, neighbours row offset
 *    outer, column offset inner; an open cell is replaced in place only if its f is strictly
 *    larger; the pop is the first open-list entry of the smallest f below 100 000, else entry 0;
 *    the goal is tested when popped.
 * Per query: status_out [B] (SLAM_ASTAR_*), path_len_out [B] (cells of the path, also when
 * TRUNCATED), path_out [B][path_cap][2] (row, col) start -> goal (nullable when path_cap is 0; the
 * entries past a query's path are not written),
 * expansions_out [B] = len(close_list) (the start plus every non-goal pop; for NO_PATH and EDGE the
 * cells closed before the search stopped).  inflated_out: nullable [G][H][W] row-major, the map
 * start_find leaves in GlobalPlanner.map.
 * Rejected up front (SLAM_ERR_INVALID): span > min(H, W) (the reference raises IndexError),
 * H > W (its state_map is W x W), r < 0, span < 0 or span > 4096, H * W >= 2^31, map_of_query NULL
 * with G != 1 and G != B; the host form also rejects a map_of_query entry outside [0, G) (the
 * device form reports SLAM_ASTAR_BAD_MAP).  Workspace: G * (H * W + span * (span + 63) / 8) bytes
 * and up to 1 GB of search slots (25 bytes per cell each), on the context. */
enum {
    SLAM_ASTAR_OK = 0,
    SLAM_ASTAR_INVALID_START = 1,   /* the start cell is not 0 after inflation: `return "None"` (:157-159)   */
    SLAM_ASTAR_INVALID_GOAL = 2,    /* the goal cell is not 0 after inflation: `return "None"` (:160-162)    */
    SLAM_ASTAR_NO_PATH = 3,         /* the open list ran empty, start == goal included: IndexError (:172)    */
    SLAM_ASTAR_EDGE = 4,            /* an expansion would index outside [0,H) x [0,W), or the shifted start or
                                       goal lies outside: the reference wraps a -1 index or raises IndexError */
    SLAM_ASTAR_TRUNCATED = 5,       /* path longer than path_cap: the first path_cap cells written           */
    SLAM_ASTAR_BAD_MAP = 6          /* device form: map_of_query entry outside [0, G)                        */
};
int slam_astar(slam_ctx *ctx, const int8_t *maps, int G, int H, int W, int wire_layout, int span, int r,
               const int32_t *starts, const int32_t *goals, const int32_t *map_of_query, int B, int path_cap,
               int32_t *status_out, int32_t *path_len_out, int32_t *path_out, int32_t *expansions_out,
               int8_t *inflated_out);
int slam_astar_dev(slam_ctx *ctx, const int8_t *maps, int G, int H, int W, int wire_layout, int span, int r,
                   const int32_t *starts, const int32_t *goals, const int32_t *map_of_query, int B, int path_cap,
                   int32_t *status_out, int32_t *path_len_out, int32_t *path_out, int32_t *expansions_out,
                   int8_t *inflated_out);
/* The inflation alone (:148-155): the map start_find leaves behind in GlobalPlanner.map (the
 * reference mutates it in place), inflated_out [G][H][W] row-major; same checks as slam_astar. */
int slam_astar_inflate(slam_ctx *ctx, const int8_t *maps, int G, int H, int W, int wire_layout, int span, int r,
                       int8_t *inflated_out);
int slam_astar_inflate_dev(slam_ctx *ctx, const int8_t *maps, int G, int H, int W, int wire_layout, int span, int r,
                           int8_t *inflated_out);

/* ---- landmark EKF-SLAM node ------------------------------------------- */
/* Replaces Extraction.process(msg) (W12m/extraction.py:24-89) and SLAM_EKF.observation(lm)
 * (W12m/slam_ekf.py:96-106) for S scans in one launch.  ranges [S][n] float32, cos_t / sin_t [n] as for
 * slam_scan_to_points; the points are formed as laserToNumpy does (inf -> 30 m, slam_ekf.py:115-123).
 * The rules are the reference's as it executes: only the first n-1 points are labelled (:36); the point that
 * closes a cluster belongs to it and a cluster needs two earlier members to be closed (:41-45); cluster
 * numbers advance on every gap; a cluster still open at the end is never tested; the gap is
 * sqrt(dx*dx + dy*dy) < range_threshold (:37) and the extent the largest pairwise distance < radius_max_th
 * (:47-49).  A NaN range compares false everywhere: it ends a cluster and is no landmark's member.
 * Per scan: count_out [S] landmarks (at most lm_cap; overflow_out [S] is 1 when the scan had more, the first
 * lm_cap are kept), ids_out [S][lm_cap] their cluster numbers (-1 in unused slots), means_out [S][lm_cap][2]
 * the sensor-frame means (running sums in index order, :81-87: bit-equal to the reference), z_out
 * [S][lm_cap][2] the rows (hypot, pi_2_pi(atan2)) of observation; labels_out: nullable [S][n-1], every
 * point's cluster number or -1.  1 <= n <= 4096, 1 <= lm_cap <= 1024. */
int slam_landmarks(slam_ctx *ctx, const float *ranges, const double *cos_t, const double *sin_t, int S, int n,
                   double range_threshold, double radius_max_th, int lm_cap, int32_t *count_out, int32_t *overflow_out,
                   int32_t *ids_out, double *means_out, double *z_out, int32_t *labels_out);
int slam_landmarks_dev(slam_ctx *ctx, const float *ranges, const double *cos_t, const double *sin_t, int S, int n,
                       double range_threshold, double radius_max_th, int lm_cap, int32_t *count_out,
                       int32_t *overflow_out, int32_t *ids_out, double *means_out, double *z_out, int32_t *labels_out);

/* Per-trajectory status of the filter and of the node replay below. */
enum {
    SLAM_NODE_OK = 0,
    SLAM_NODE_REF_RAISES = 1,   /* an observation matched the landmark appended in the same call: the reference
                                   raises ValueError from np.hstack (ekf_lm.py:37-38, its n1 is stale)          */
    SLAM_NODE_LM_CAP = 2,       /* the state would grow past max_lm landmarks                                   */
    SLAM_NODE_OBS_CAP = 3       /* node replay: a kept scan had more than lm_cap landmarks                      */
};
#define SLAM_EKF_MAX_LM 32
/* Replaces EKF.estimate(xEst, PEst, z, u) (W12m/ekf_lm.py:15-50) called once per step along B trajectories,
 * each from xEst = x0[b] (NULL: zeros), PEst = eye(3).  u [B][steps][3]; step_counts [B]: trajectory b runs
 * min(max(step_counts[b], 0), steps) steps; the observations of step (b, s) are the rows
 * z[z_off[b * steps + s] .. z_off[b * steps + s + 1]) of z [nz][2] (range, bearing); z_off has B * steps + 1
 * entries (the device form clamps them to [0, nz]).  The reference's stale n1 is reproduced, not fixed: a
 * second unmatched observation in one call ends the call before the yaw wrap (:40-42), and from the step at
 * which the reference raises (SLAM_NODE_REF_RAISES) or the state would pass max_lm (SLAM_NODE_LM_CAP) the
 * trajectory stops with the state it had BEFORE that step.
 * 0 <= max_lm <= SLAM_EKF_MAX_LM; N = 3 + 2 * max_lm.  x_out [B][N], P_out [B][N][N] (zero beyond the state),
 * nlm_out [B][steps] the landmark count after every step (-1: the step did not happen), status_out [B]. */
int slam_ekf_lm(slam_ctx *ctx, const double *x0, const double *u, const int32_t *step_counts, const int64_t *z_off,
                const double *z, int64_t nz, int B, int steps, int max_lm, double *x_out, double *P_out,
                int32_t *nlm_out, int32_t *status_out);
int slam_ekf_lm_dev(slam_ctx *ctx, const double *x0, const double *u, const int32_t *step_counts, const int64_t *z_off,
                    const double *z, int64_t nz, int B, int steps, int max_lm, double *x_out, double *P_out,
                    int32_t *nlm_out, int32_t *status_out);

/* Replaces SLAM_EKF.laserCallback (W12m/slam_ekf.py:63-95) in full - extraction (:79), the skip of a scan
 * without landmark (:80-82), calc_odometry (:109-113), T2u (:125-128), observation (:96-106), EKF.estimate
 * (:86) and the map cast from xEst (:88-90) - over L streams of n_scan already-decimated scans,
 * ranges [L][n_scan][n] float32.  Scan 0 of a stream is its first target whatever it shows; after it only
 * scans with at least one landmark are KEPT, and the scan matcher's target advances on kept scans only.
 * Step s of a trajectory matches kept scan s + 1 against kept scan s, filters, and casts kept scan s + 1 from
 * xEst into map grid_of_traj[l] (NULL: map 0) of `grid` (NULL: no map).  pose0 [L][3]; PEst starts as eye(3).
 * kept_out [L][n_scan] scan numbers (-1 behind the kept ones), kept_count_out [L]; per step s < kept_count - 1:
 * xest_out [L][n_scan-1][3] = xEst[:3] (NaN for steps that did not happen), nlm_out [L][n_scan-1] (-1 likewise),
 * T_out [L][n_scan-1][9] and iters_out [L][n_scan-1] (nullable; entries behind a trajectory's steps are void);
 * x_final_out [L][N], P_final_out [L][N][N], N = 3 + 2 * max_lm, zero beyond the state; status_out [L]
 * (SLAM_NODE_*): a trajectory that stops keeps the state, and casts the scans, of the steps before.
 * L <= 65535, n <= 4096; dtype, max_iter, tol as slam_replay.  The device form does not synchronise.
 * The scan matcher runs in ONE launch shape whatever L is (two queries per lane, or what "icp_qpt" / "icp_one_wave" = 1
 * name), so a trajectory's outputs are the same bits alone and in any batch. */
int slam_node_replay(slam_ctx *ctx, const float *ranges, const double *cos_t, const double *sin_t, int L, int n_scan,
                     int n, int dtype, int max_iter, double tol, double range_threshold, double radius_max_th,
                     int lm_cap, int max_lm, const double *pose0, slam_grid *grid, const int32_t *grid_of_traj,
                     int32_t *kept_out, int32_t *kept_count_out, double *xest_out, int32_t *nlm_out,
                     double *x_final_out, double *P_final_out, double *T_out, int32_t *iters_out, int32_t *status_out);
int slam_node_replay_dev(slam_ctx *ctx, const float *ranges, const double *cos_t, const double *sin_t, int L, int n_scan,
                         int n, int dtype, int max_iter, double tol, double range_threshold, double radius_max_th,
                         int lm_cap, int max_lm, const double *pose0, slam_grid *grid, const int32_t *grid_of_traj,
                         int32_t *kept_out, int32_t *kept_count_out, double *xest_out, int32_t *nlm_out,
                         double *x_final_out, double *P_final_out, double *T_out, int32_t *iters_out,
                         int32_t *status_out);

/* ---- fusion-localization node (W9), batched ---------------------------------------------- */
/* Per-trajectory status of slam_loc_replay. */
enum {
    SLAM_LOC_OK = 0,
    SLAM_LOC_NONFINITE = 1,     /* a transform of the step was not finite: the reference raises LinAlgError from
                                   numpy's svd (W12m/icp.py:161 as W9 runs it)                                   */
    SLAM_LOC_BAD_ROUTE = 2      /* device form: stream_of_traj / map_of_traj entry out of range                  */
};
/* Replaces Localization.laserCallback (W9/localization.py:66-126) in full - calc_odometry twice (:78, :100,
 * :159-168), calc_map_observation (:152-157) with laserEstimation (:128-150) and laserToNumpy (:170-176), the
 * pose algebra (:79-83, :113-118) and EKF.estimate (W9/ekf.py:17-87) - for L trajectories in lockstep over
 * streams of n_scan already-decimated scans, ranges [S][n_scan][n] float32 (every scan is one processed
 * message), n_scan >= 1.  Trajectory l replays stream stream_of_traj[l] (NULL: stream l, and S must equal L)
 * against the obstacles (ox, oy)[obs_off[m] .. obs_off[m + 1]) of map m = map_of_traj[l] (NULL: map 0);
 * obs_off has M + 1 ascending entries over one concatenated list of K = obs_off[M] points (K >= 0, a map may
 * be empty; the device form clamps the entries to [0, K]).  It starts from xEst = xOdom = pose0[l] (NULL:
 * zeros), PEst = eye(3).  Step s: T1 = ICP.process(previous scan, scan s) - for s = 0 the target is the
 * map's virtual scan at pose0 (:159-168) - and xOdom = compose(xOdom, T1); T2 = ICP.process(scan s, scan s)
 * (:100; solved, not assumed); t = the map observation at xEst, z = compose(xEst, t); xEst, PEst =
 * EKF.estimate(xEst, PEst, z, T2), its 3x3 inverse by elimination with partial pivoting as numpy's.  Points are
 * cos_t[i] * r, sin_t[i] * r without an inf clip.  T1 of s >= 1 and T2 are solved once per STREAM; T1 of step
 * 0 is the same pair as t of step 0 (same target, same source) and is solved once.
 * Outputs: xest_out, xodom_out [L][n_scan][3]; P_final_out [L][9]; status_out [L] (SLAM_LOC_*); nullable:
 * T_obs_out [L][n_scan][9] (t), iters_obs_out [L][n_scan], T_odom_out [L][n_scan][9] (T1), tar_pts_out
 * [L][n_scan][2][n] (the target points of every step's map observation, for inspection).  A trajectory one of
 * whose T1, T2, t is not finite at step s stops there (SLAM_LOC_NONFINITE): it keeps the state it had before
 * step s (P_final_out), its per-step outputs from s on are NaN, its iteration counts -1 and its tar_pts_out
 * entries void; the others are unaffected.
 * L <= 65535, n <= 4096, L * n_scan < 2^31; max_iter, tol as slam_icp_batch.  The host form rejects route
 * entries out of range; the device form does not synchronise, takes its workspaces from the context
 * (S (2 n_scan - 1) pairs of point sets, 32 n bytes each, and 32 n bytes per trajectory) and enqueues two
 * launches per step.  The scan matcher runs in ONE launch shape whatever L and S are (two queries per lane,
 * or what "icp_qpt" / "icp_one_wave" = 1 name), so a trajectory's outputs are the same bits alone and in any
 * batch. */
int slam_loc_replay(slam_ctx *ctx, const float *ranges, int S, int n_scan, int n, const int32_t *stream_of_traj,
                    const double *ox, const double *oy, const int64_t *obs_off, int M, const int32_t *map_of_traj,
                    const double *pose0, int L, const double *cos_t, const double *sin_t, double angle_min,
                    double angle_increment, int max_iter, double tol, double *xest_out, double *xodom_out,
                    double *P_final_out, int32_t *status_out, double *T_obs_out, int32_t *iters_obs_out,
                    double *T_odom_out, double *tar_pts_out);
/* Device form: K is the length of ox / oy (the host form reads it from obs_off[M]). */
int slam_loc_replay_dev(slam_ctx *ctx, const float *ranges, int S, int n_scan, int n, const int32_t *stream_of_traj,
                        const double *ox, const double *oy, const int64_t *obs_off, int M, int64_t K,
                        const int32_t *map_of_traj, const double *pose0, int L, const double *cos_t,
                        const double *sin_t, double angle_min, double angle_increment, int max_iter, double tol,
                        double *xest_out, double *xodom_out, double *P_final_out, int32_t *status_out,
                        double *T_obs_out, int32_t *iters_obs_out, double *T_odom_out, double *tar_pts_out);

#ifdef __cplusplus
}
#endif
#endif /* SLAM_HIP_H */
