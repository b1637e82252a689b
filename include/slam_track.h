/*
 * slam_track.h - the third header of libslamhip.so's C ABI: the scan-to-map tracker.
 * It includes slam_hip.h for the types, the error codes and the conventions (host form / *_dev form, return values,
 * slam_last_error); the two functions below live in the same library and take the same slam_ctx and slam_grid.
 */
#ifndef SLAM_TRACK_H
#define SLAM_TRACK_H

#include "slam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- scan-to-map tracker: match, refine, integrate per scan, batched over trajectories ---- */
/* One call runs S scans of L trajectories.  Trajectory l owns map map0 + l of the grid: every scan is matched against
 * that map as it stands after every earlier integration (slam_grid_match), refined below the cell (slam_grid_refine)
 * and, behind a keyframe gate, integrated into it (slam_grid_update_particles).  The reference has no counterpart.
 * The whole loop is enqueued on the context's stream; the device form never synchronises with the host.
 *
 * Inputs.  ranges float32 [L][S][n]; motion nullable float64 [L][S][3]: the odometry step (dx, dy, dtheta in the frame
 * of the previous pose) INTO scan s; cos_t, sin_t [n] as for slam_scan_to_points; rot_off [K] the heading offsets of
 * the matcher's rotations and rot_off_cs [K][2] their cosines and sines, both made by the caller, as every table of
 * this library is; nx, ny, step the matcher's window; iters, damping, step_cells, step_rad the refinement's
 * parameters; max_range, cap as for both; min_used, gate_dist, gate_turn below.
 *
 * State, in and out, float64 [L][8] = pose (x, y, theta), key pose (x, y, theta), keyed (0 or 1: anything but 0 reads
 * as 1), one spare (kept as it is).  pose is where the last scan was placed, key pose where the map was last
 * integrated.  A new trajectory is (its start pose, anything, 0, 0).  The state is everything the call keeps: S scans
 * in one call and the same scans over several calls give the same bits in every output and in the map.
 *
 * Everything is float64 with no fused multiply-add.  Per trajectory l and scan s, prev = the state's pose:
 *
 * 1 Predict.  With motion, (dx, dy, dth) = motion[l][s]:
 *     pred.x = (prev.x + cos(prev.th)*dx) - sin(prev.th)*dy
 *     pred.y = (prev.y + sin(prev.th)*dx) + cos(prev.th)*dy
 *     pred.th = prev.th + dth
 *   (slam_pose_compose's step).  With motion NULL pred = prev.  Then c0 = cos(pred.th), s0 = sin(pred.th): the only
 *   transcendental calls of the step outside the refinement (with motion, cos and sin of prev.th are two more).
 * 2 First scan (keyed == 0).  pose = pred; no match, no refinement; the scan is integrated (6).  The first scan needs
 *   a pose the map can take: when pred is not finite in all three components, or its x or y is 2^20 cells or more
 *   from the map's origin, nothing is integrated, LOST is set and keyed stays 0 - so every later scan of that
 *   trajectory is a first scan again, LOST again, and its map is never touched.
 * 3 Match (keyed != 0).  slam_grid_match's rule on the field (at `cap`) of map map0 + l as the counters stand now,
 *   centre (pred.x, pred.y), window nx, ny, step, and the rotation table
 *     rot_cs[k] = (c0*co_k - s0*so_k, s0*co_k + c0*so_k),  (co_k, so_k) = rot_off_cs[k]
 *   - two products and one subtraction or addition each, in that order.  The matched pose of the flat index
 *   best = (k, i, j) is (pred.x + (double)(i - nx)*step, pred.y + (double)(j - ny)*step, pred.th + rot_off[k]).
 *   Two outcomes leave pose = pred with nothing refined and nothing integrated: best == -1 (the centre is not finite
 *   or 2^20 cells or more away), which sets LOST; and used < min_used.
 * 4 Refine.  slam_grid_refine's rule from the matched pose on the same field.  The refined pose is kept iff its
 *   status is SLAM_REFINE_OK and cost_end <= cost_start; otherwise the matched pose stands.
 * 5 Gate.  With (dx, dy, dth) = pose - key pose, componentwise: integrate iff dx*dx + dy*dy >= gate_dist*gate_dist
 *   or fabs(dth) >= gate_turn.  Both comparisons are false for NaN; +inf for both never integrates (tracking in a
 *   given map: the caller passes keyed = 1); 0 and 0 integrate every placed scan.
 * 6 Integrate.  Exactly slam_grid_update_particles(ranges of this scan [L][n], poses [L][1][3], acc, F = L, P = 1,
 *   map0), where acc[l] is SLAM_MCL_DEAD for a trajectory that does not integrate: a range of +inf counts as 30 m, a
 *   pose or beam the index rule rejects raises the context's sticky status as it does there.  On integration
 *   key pose = pose and keyed = 1.
 * Then the state's pose = pose.
 *
 * Outputs.  poses_out [L][S][3] the pose of every scan.  info_out int32 [L][S][4] = (best, best cost, used, flags):
 * the matcher's three answers (-1, -1, 0 where no match ran or it was lost) and the bits below.  trace_out nullable
 * float64 [L][S][13] = pred (3), c0, s0, matched pose (3), refined pose (3), the refinement's cost at its start and
 * at its end; the matched pose is 0 unless MATCHED, and the refinement's five are 0 unless it ran (it runs iff
 * MATCHED) - then they are slam_grid_refine's own outputs, whatever its status.  With the trace every decision of the
 * call can be checked against the public calls bit for bit.
 *   SLAM_TRACK_MATCHED (1)      the match answered with used >= min_used: the matched pose was adopted
 *   SLAM_TRACK_REFINED (2)      the refined pose was kept
 *   SLAM_TRACK_INTEGRATED (4)   the scan was integrated and became the key
 *   SLAM_TRACK_LOST (8)         the match had no centre (3), or the first scan no pose (2)
 *
 * Batch rule.  A trajectory gets bit-identical outputs and map alone, in any batch, in any order, under any split of
 * S into calls, from the host and the device form: slam_grid_match and slam_grid_refine have that property and the
 * rest of the step has no sums.
 *
 * Side effects.  The call sees every update enqueued before it on the context's stream (it joins the context's
 * internal streams first).  It changes maps map0 .. map0 + L - 1 and nothing else of the grid.  The host form ends
 * with the status check slam_grid_update_particles ends with.  Under slam_timing_* the rebuilt fields count as
 * SLAM_K_FINALIZE and everything else as SLAM_K_GRID.  The field is rebuilt before every scan, whether or not the
 * scan before it integrated anything.
 *
 * Bounds.  Those of slam_grid_match (n * cap < 2^31, K >= 1, nx, ny >= 0, K * (2 nx + 1) * (2 ny + 1) <= 2^24,
 * L * K < 2^31, step finite and > 0, max_range > 0, 1 <= cap <= 32767) and of slam_grid_refine (0 <= iters <= 64,
 * damping finite and >= 0, step_cells > 0, step_rad > 0); L >= 1, S >= 1, 1 <= n <= 4096, L * S * n < 2^31,
 * map0 >= 0, map0 + L <= G, min_used >= 1, gate_dist and gate_turn >= 0 or +inf, not NaN.  Anything else is
 * SLAM_ERR_INVALID, enqueues nothing and leaves the context and the grid as they were. */
enum { SLAM_TRACK_MATCHED = 1, SLAM_TRACK_REFINED = 2, SLAM_TRACK_INTEGRATED = 4, SLAM_TRACK_LOST = 8 };
#define SLAM_TRACK_STATE_LEN 8
#define SLAM_TRACK_INFO_LEN 4
#define SLAM_TRACK_TRACE_LEN 13
int slam_track(slam_ctx *ctx, slam_grid *grid, const float *ranges, const double *motion, int L, int S,
               const double *cos_t, const double *sin_t, int n, const double *rot_off, const double *rot_off_cs, int K,
               int nx, int ny, double step, int iters, double damping, double step_cells, double step_rad,
               float max_range, int cap, int min_used, double gate_dist, double gate_turn, int map0, double *state,
               double *poses_out, int32_t *info_out, double *trace_out);
int slam_track_dev(slam_ctx *ctx, slam_grid *grid, const float *ranges, const double *motion, int L, int S,
                   const double *cos_t, const double *sin_t, int n, const double *rot_off, const double *rot_off_cs,
                   int K, int nx, int ny, double step, int iters, double damping, double step_cells, double step_rad,
                   float max_range, int cap, int min_used, double gate_dist, double gate_turn, int map0, double *state,
                   double *poses_out, int32_t *info_out, double *trace_out);

#ifdef __cplusplus
}
#endif
#endif /* SLAM_TRACK_H */
