/*
 * slam_refine.h - the second header of libslamhip.so's C ABI: the continuous refinement of a scan-to-map pose.
 * It includes slam_hip.h for the types, the error codes and the conventions (host form / *_dev form, return values,
 * slam_last_error); the two functions below live in the same library and take the same slam_ctx and slam_grid.
 */
#ifndef SLAM_REFINE_H
#define SLAM_REFINE_H

#include "slam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- scan-to-map refinement below the cell: damped Gauss-Newton on a smooth distance field ---- */
/* slam_grid_match and slam_grid_locate stop at the cell; this call moves a pose continuously from there.  The
 * reference has no counterpart.  The rule is free of decisions: no step is accepted or rejected and nothing tests for
 * convergence.  Only the cell a beam ends in, the used-beam test and the off-map test are discrete; everything else
 * is a continuous function of the inputs.
 *
 * Inputs.  ranges float32 [B][n], or one [n] for every hypothesis when shared != 0; poses [B][3] (x, y, theta);
 * grid_of_batch [B] (NULL: map 0, as for slam_grid_match); cos_t, sin_t [n] as for slam_scan_to_points; field
 * nullable int16 [G][xw][yw], made by slam_grid_distance_field(_dev) at the SAME cap: when given it is used and
 * nothing is built, when NULL the field of all G maps is rebuilt in the context's workspace at the start of the call,
 * as slam_mcl_weigh does.  In the host form field is a host array.
 *
 * Used beam.  As slam_grid_match: rr = (double)ranges[t]; used iff isfinite(rr) && ranges[t] < max_range (compared
 * as float32); lx = cos_t[t]*rr; ly = sin_t[t]*rr.
 *
 * Smooth field M of map gi.  d[i][j] = sqrt((double)field[gi][i][j]) inside the map - the distance in cells, at most
 * sqrt(cap) - and sqrt((double)cap) outside it.  For a point (x, y):
 *   u = scale*(x + off_x) - 0.5;  v = scale*(y + off_y) - 0.5       (cell centres are the integer points)
 *   i = floor(u);  a = u - i;  j = floor(v);  b = v - j
 *   M  = (1-b)*((1-a)*d[i][j] + a*d[i+1][j]) + b*((1-a)*d[i][j+1] + a*d[i+1][j+1])
 *   Mx = scale*((1-b)*(d[i+1][j]-d[i][j]) + b*(d[i+1][j+1]-d[i][j+1]))
 *   My = scale*((1-a)*(d[i][j+1]-d[i][j]) + a*(d[i+1][j+1]-d[i+1][j]))
 * A used beam whose u or v is not finite, or is 2^20 or more in magnitude, is "off": M = sqrt(cap), Mx = My = 0.
 *
 * One evaluation at pose (px, py, th).  c = cos(th), s = sin(th); per used beam, with no fused multiply-add:
 *   x = c*lx + (-s)*ly + px;  y = s*lx + c*ly + py;  r = M(x, y)
 *   J = (Mx, My, Mx*(-s*lx - c*ly) + My*(c*lx - s*ly))
 *   cost = sum r*r;  H = sum J^T J (6 distinct entries);  g = sum J*r
 * All sums are float64.  Their order is not part of the contract beyond the batch rule below.
 *
 * One step.  A = H + damping*diag(H) + 1e-9*I (each diagonal entry (Hkk + damping*Hkk) + 1e-9);
 * delta = -A^-1 g, by the adjugate of the symmetric A over its determinant; delta is clamped componentwise to
 * +-step_cells/scale in x and y and to +-step_rad in theta; pose += delta.  theta is not wrapped.
 * The call makes `iters` steps and iters + 1 evaluations.
 *
 * Outputs.  pose_out [B][3] the last pose; cost_out [B][2] the cost at the start and at the last pose; used_out
 * (nullable) [B] the number of used beams; normal_out (nullable) [B][9] = Hxx, Hxy, Hxt, Hyy, Hyt, Htt, gx, gy, gt of
 * the LAST evaluation, undamped: the information matrix of the fit and its gradient; status_out [B]:
 *   SLAM_REFINE_OK (0)        answered
 *   SLAM_REFINE_BAD_POSE (1)  the start pose is not finite, or its own u or v is not below 2^20 in magnitude
 *   SLAM_REFINE_NO_MAP (2)    the grid_of_batch entry is outside [0, G) (host and device form alike, as
 *                             slam_grid_match treats such an entry; it is looked at before the pose)
 * With status 1 or 2 pose_out is the input pose, both costs are -1, used is 0 and normal_out is 0; the others of the
 * batch are unaffected.  A scan with no used beam: the pose unchanged, costs 0, status 0.  The call does not choose
 * between start and end: cost_out lets the caller do that.
 *
 * Batch rule.  Every hypothesis gets bit-identical outputs alone, in any batch, in any order and under any chunking,
 * from the host and the device form, with field given or rebuilt: its sums are taken in an order that depends on n
 * alone (lane l of a wave of 64 adds beams l, l + 64, ... in ascending order, then the lanes are summed by a fixed
 * butterfly).
 *
 * Side effects.  The call sees every update enqueued before it on the context's stream, changes nothing in the grid,
 * keeps nothing between calls and leaves the context's sticky status untouched.  Under slam_timing_* a rebuilt field
 * counts as SLAM_K_FINALIZE, the refinement as SLAM_K_GRID.
 *
 * Bounds.  1 <= n <= 4096, B >= 1, B * n < 2^31, 0 <= iters <= 64, damping >= 0 and finite, step_cells > 0,
 * step_rad > 0 (+inf: that component is not clamped), 1 <= cap <= 32767, max_range > 0 (+inf: every finite range is
 * used); anything else is SLAM_ERR_INVALID, enqueues nothing and leaves the context as it was. */
enum { SLAM_REFINE_OK = 0, SLAM_REFINE_BAD_POSE = 1, SLAM_REFINE_NO_MAP = 2 };
#define SLAM_REFINE_NORMAL_LEN 9
int slam_grid_refine(slam_ctx *ctx, slam_grid *grid, const float *ranges, int shared, const double *poses, int B,
                     const int32_t *grid_of_batch, const double *cos_t, const double *sin_t, int n, int iters,
                     double damping, double step_cells, double step_rad, float max_range, int cap,
                     const int16_t *field, double *pose_out, double *cost_out, int32_t *used_out,
                     double *normal_out, int32_t *status_out);
int slam_grid_refine_dev(slam_ctx *ctx, slam_grid *grid, const float *ranges, int shared, const double *poses, int B,
                         const int32_t *grid_of_batch, const double *cos_t, const double *sin_t, int n, int iters,
                         double damping, double step_cells, double step_rad, float max_range, int cap,
                         const int16_t *field, double *pose_out, double *cost_out, int32_t *used_out,
                         double *normal_out, int32_t *status_out);

#ifdef __cplusplus
}
#endif
#endif /* SLAM_REFINE_H */
