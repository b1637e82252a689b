// A scan-to-map pose refined below the cell, for gfx950 (MI355X): damped Gauss-Newton on the bilinear interpolation of
// the distance field's square root (include/slam_refine.h).  The reference has no counterpart.
//
//   slam_grid_refine   per hypothesis iters steps  pose += clamp(-(H + damping diag H + 1e-9 I)^-1 g)  with
//                      cost = sum r^2, H = sum J^T J, g = sum J r over the used beams, r = M(beam end), J = dr/dpose
//
// The rule has no decisions - no accepted or rejected step, no convergence test - so a wave never diverges from the
// restatement except where a beam changes its cell.  One WAVE owns a hypothesis from its first evaluation to its last:
//   lanes      lane l takes beams l, l + 64, ... in ascending order and adds their ten terms to ten float64 registers;
//              unused beams add nothing.  ranges, cos_t and sin_t are read again in every evaluation (L1 / L2 hits after
//              the first): 4096 beams a wave, four waves a workgroup, do not fit LDS.
//   sums       an xor butterfly over the 64 lanes per sum: a + b is commutative, so both lanes of a pair hold the same
//              bits after every stage and all 64 hold the same ten sums at the end.  The order depends on n alone, which
//              is what makes a hypothesis's answer independent of its batch.  (Packing the used beams to the front
//              through an LDS counter, as the matcher does for its integer costs, would make the order depend on who
//              won the counter.)
//   solve      every lane solves the same 3 x 3 system from the same bits and keeps the pose in registers; lane 0 stores.
// Four waves share a workgroup and nothing else: no LDS, no barrier.  Workgroups beyond the launch cap go grid-stride
// (plan_refine, launch_shapes.h).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "slam_internal.h"

namespace slam {

constexpr int kRefineSums = 10;              // cost, Hxx, Hxy, Hxt, Hyy, Hyt, Htt, gx, gy, gt
constexpr double kRefineOff = 1048576.0;     // |u| or |v| of 2^20 or more (or not finite): the beam is off, the start pose bad

// d[i][j]: the distance in cells inside the map, sqrt(cap) outside it
__device__ __forceinline__ double refine_d(const int16_t *__restrict__ field, int xw, int yw, int i, int j, double sd)
{
    return ((unsigned)i < (unsigned)xw && (unsigned)j < (unsigned)yw) ? sqrt((double)field[(size_t)i * yw + j]) : sd;
}

// One evaluation at (px, py, th): S = the ten sums over the used beams, the same bits in every lane; used = their number.
__device__ __forceinline__ void refine_eval(const RefineArgs &a, const int16_t *__restrict__ field, const float *__restrict__ ranges,
                                            int lane, double px, double py, double th, double sd, double (&S)[kRefineSums], int &used)
{
    const GridDev &g = a.g;
    const double c = cos(th), s = sin(th);
#pragma unroll
    for (int k = 0; k < kRefineSums; ++k) S[k] = 0.0;
    int cnt = 0;
    for (int t = lane; t < a.n; t += kWave) {
        const float rf = ranges[t];
        const double rr = (double)rf;
        if (!(isfinite(rr) && rf < a.max_range)) continue;
        ++cnt;
        const double lx = a.cos_t[t] * rr, ly = a.sin_t[t] * rr;
        const double x = c * lx + (-s) * ly + px, y = s * lx + c * ly + py;
        const double u = g.scale * (x + g.off_x) - 0.5, v = g.scale * (y + g.off_y) - 0.5;
        double r = sd, mx = 0.0, my = 0.0;
        if (fabs(u) < kRefineOff && fabs(v) < kRefineOff) {              // (false for NaN)
            const double fu = floor(u), fv = floor(v);
            const int i = (int)fu, j = (int)fv;
            const double p = u - fu, q = v - fv;
            // two pairs adjacent in y: (i, j), (i, j + 1) and (i + 1, j), (i + 1, j + 1)
            const double d00 = refine_d(field, g.xw, g.yw, i, j, sd), d01 = refine_d(field, g.xw, g.yw, i, j + 1, sd);
            const double d10 = refine_d(field, g.xw, g.yw, i + 1, j, sd), d11 = refine_d(field, g.xw, g.yw, i + 1, j + 1, sd);
            r = (1.0 - q) * ((1.0 - p) * d00 + p * d10) + q * ((1.0 - p) * d01 + p * d11);
            mx = g.scale * ((1.0 - q) * (d10 - d00) + q * (d11 - d01));
            my = g.scale * ((1.0 - p) * (d01 - d00) + p * (d11 - d10));
        }
        const double jt = mx * (-s * lx - c * ly) + my * (c * lx - s * ly);
        S[0] += r * r;
        S[1] += mx * mx; S[2] += mx * my; S[3] += mx * jt;
        S[4] += my * my; S[5] += my * jt; S[6] += jt * jt;
        S[7] += mx * r;  S[8] += my * r;  S[9] += jt * r;
    }
#pragma unroll
    for (int off = kWave / 2; off; off >>= 1) {
#pragma unroll
        for (int k = 0; k < kRefineSums; ++k) S[k] = S[k] + shfl64(S[k], lane ^ off);
        cnt += __shfl_xor(cnt, off, kWave);
    }
    used = cnt;
}

__device__ __forceinline__ double refine_clamp(double v, double lim) { return v < -lim ? -lim : v > lim ? lim : v; }

// Wave w of workgroup k takes hypotheses k * kRefineWaves + w, then every gridDim.x * kRefineWaves-th after it.
__global__ void __launch_bounds__(kRefineThreads) k_refine(RefineArgs a)
{
    const GridDev &g = a.g;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const double sd = sqrt((double)a.cap);
    for (long b = (long)blockIdx.x * kRefineWaves + wave; b < a.B; b += (long)gridDim.x * kRefineWaves) {    // (wave-uniform)
        const int gi = a.maps ? a.maps[b] : 0;
        double px = a.poses[3 * (size_t)b], py = a.poses[3 * (size_t)b + 1], th = a.poses[3 * (size_t)b + 2];
        int status = SLAM_REFINE_OK;
        if ((unsigned)gi >= (unsigned)g.G) status = SLAM_REFINE_NO_MAP;
        else if (!(isfinite(px) && isfinite(py) && isfinite(th)) || !(fabs(g.scale * (px + g.off_x) - 0.5) < kRefineOff) ||
                 !(fabs(g.scale * (py + g.off_y) - 0.5) < kRefineOff))
            status = SLAM_REFINE_BAD_POSE;
        double S[kRefineSums];
        double cost0 = -1.0;
        int used = 0;
        if (status == SLAM_REFINE_OK) {
            const int16_t *field = a.field + (size_t)gi * g.xw * g.yw;
            const float *ranges = a.ranges + (size_t)b * a.range_stride;
            for (int it = 0;; ++it) {
                refine_eval(a, field, ranges, lane, px, py, th, sd, S, used);
                if (it == 0) cost0 = S[0];
                if (it == a.iters) break;
                // A = H + damping diag(H) + 1e-9 I, symmetric: [p q r; q u v; r v w]
                const double p = (S[1] + a.damping * S[1]) + 1e-9, q = S[2], r = S[3];
                const double u = (S[4] + a.damping * S[4]) + 1e-9, v = S[5], w = (S[6] + a.damping * S[6]) + 1e-9;
                const double c00 = u * w - v * v, c01 = r * v - q * w, c02 = q * v - r * u;
                const double c11 = p * w - r * r, c12 = q * r - p * v, c22 = p * u - q * q;
                const double det = p * c00 + q * c01 + r * c02;
                const double dx = -((c00 * S[7] + c01 * S[8] + c02 * S[9]) / det);
                const double dy = -((c01 * S[7] + c11 * S[8] + c12 * S[9]) / det);
                const double dt = -((c02 * S[7] + c12 * S[8] + c22 * S[9]) / det);
                px += refine_clamp(dx, a.step_xy);
                py += refine_clamp(dy, a.step_xy);
                th += refine_clamp(dt, a.step_rad);
            }
        } else {
#pragma unroll
            for (int k = 0; k < kRefineSums; ++k) S[k] = 0.0;
        }
        if (lane == 0) {
            a.pose_out[3 * (size_t)b] = px; a.pose_out[3 * (size_t)b + 1] = py; a.pose_out[3 * (size_t)b + 2] = th;
            a.cost_out[2 * (size_t)b] = cost0;
            a.cost_out[2 * (size_t)b + 1] = status == SLAM_REFINE_OK ? S[0] : -1.0;
            if (a.used_out) a.used_out[b] = used;
            a.status_out[b] = status;
        }
        if (a.normal_out && lane < SLAM_REFINE_NORMAL_LEN) {
            double val = 0.0;
#pragma unroll
            for (int k = 0; k < SLAM_REFINE_NORMAL_LEN; ++k) val = lane == k ? S[k + 1] : val;     // (selects: no indexed private array)
            a.normal_out[SLAM_REFINE_NORMAL_LEN * (size_t)b + lane] = val;
        }
    }
}

hipError_t launch_refine(const RefineArgs &a, hipStream_t s)
{
    const RefineShape p = plan_refine(a.B);
    SLAM_LAUNCH(k_refine, dim3((unsigned)p.grid), dim3(p.threads), 0, s, a);
    return hipGetLastError();
}

}  // namespace slam
