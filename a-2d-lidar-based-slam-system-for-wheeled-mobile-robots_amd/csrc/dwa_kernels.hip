// DWA local planner for gfx950: every (v, omega) sample of a control step scored at once,
// B planners per launch.
//
// Functional spec = NAV = "W12_LiDAR SLAM/w12-mapping/course_agv_nav/scripts" (under the
// reference checkout), as it executes:
//   calc_dynamic_window          dwa.py:65-83     planner prologue (every lane, uniform)
//   np.arange sample axes        dwa.py:95-96     arange_len / arange_at
//   predict_trajectory / motion  dwa.py:115-124, :57-63   lane rollout
//   calc_obstacle_cost           dwa.py:126-160   pair loop
//   calc_to_goal_cost            dwa.py:162-173
//   final cost, selection        dwa.py:101-111   lane cost, workgroup (cost, index) reduction
//   LocalPlanner.laserCallback   local_planner.py:57-68   scans form: obstacles formed in LDS
//
// Shape: one workgroup per planner (grid-stride over planners), one lane per sample.  The
// planner's obstacles sit in LDS as (x, y) pairs; a lane holds R rows of its trajectory in
// registers and walks the obstacle list - every lane reads the same LDS address (a broadcast)
// and tests it against its R rows: collision test and minimum squared distance in one pass.
// min(hypot) is taken as sqrt(min(dx^2 + dy^2)): the same pair up to rounding, and within
// a few ulps of the reference's value (a radius test can differ only at a margin of that size).
// Longer trajectories go through the obstacles once per chunk of R rows; obstacle lists longer
// than the LDS tile are staged tile by tile.
#include <hip/hip_runtime.h>

#include <math.h>

#include "slam_internal.h"

namespace slam {

namespace {

// Python's max(a, b) / min(a, b): the first argument unless the second compares greater / less.
__device__ __forceinline__ double py_max(double a, double b) { return b > a ? b : a; }
__device__ __forceinline__ double py_min(double a, double b) { return b < a ? b : a; }

// numpy's float arange: n = ceil((stop - start) / step), 0 when that is not positive; element 0
// is start, element 1 start + step, element i >= 2 start + i * ((start + step) - start).
__device__ __forceinline__ int arange_len(double start, double stop, double step, int cap)
{
    double q = (stop - start) / step;
    if (!(q > 0.0)) return 0;
    double n = ceil(q);
    return n < (double)cap ? (int)n : cap;
}
__device__ __forceinline__ double arange_at(double start, double step, int i)
{
    double a1 = start + step;
    if (i == 0) return start;
    if (i == 1) return a1;
    return start + (double)i * (a1 - start);
}

// motion() (dwa.py:57-63): yaw first, then x and y from the new yaw; products left to right.
__device__ __forceinline__ void dwa_step(double &px, double &py, double &yaw, double v, double w, double dt)
{
    yaw += w * dt;
    double s, c;
    sincos(yaw, &s, &c);
    px += v * c * dt;
    py += v * s * dt;
}

// (cost, index) order of the reference's `if min_cost >= final_cost` scan from inf: NaN never
// wins, lower cost wins, equal costs go to the larger index.  Index -1 = nothing yet.
__device__ __forceinline__ bool dwa_better(double c, int i, double bc, int bi)
{
    if (i < 0 || c != c) return false;
    if (bi < 0) return true;
    return c < bc || (c == bc && i > bi);
}

struct Window {
    double lo_v, lo_w;
    int nv, nw;
};

__device__ __forceinline__ Window dwa_window(const double *x, const DwaArgs &a)
{
    const DwaConfig &c = a.cfg;
    double vd0 = x[3] - c.max_accel * c.dt, vd1 = x[3] + c.max_accel * c.dt;
    double vd2 = x[4] - c.max_dyawrate * c.dt, vd3 = x[4] + c.max_dyawrate * c.dt;
    Window w;
    w.lo_v = py_max(c.min_speed, vd0);
    double hi_v = py_min(c.max_speed, vd1);
    w.lo_w = py_max(-c.max_yawrate, vd2);
    double hi_w = py_min(c.max_yawrate, vd3);
    w.nv = arange_len(w.lo_v, hi_v, c.v_reso, a.nv_cap);
    w.nw = arange_len(w.lo_w, hi_w, c.yawrate_reso, a.nw_cap);
    // a v or omega that is not finite: an empty window (the reference raises from np.arange for
    // inf; NaN drops out of max / min there and leaves the whole speed range, beyond nv_cap here)
    if (!isfinite(x[3]) || !isfinite(x[4])) w.nv = w.nw = 0;
    return w;
}

// Trajectory rows a lane holds at a time: the default 21 rows take two chunks (24 tested, three
// repeats of the last row).  With 24 rows in registers the compiler spills (make resource-usage).
constexpr int kDwaRows = 12;

}  // namespace

template <int R, bool RECT>
__global__ void __launch_bounds__(512) k_dwa(DwaArgs a)
{
    extern __shared__ double2 lds_ob[];                // tile_cap obstacles, then the guard bytes
    __shared__ int s_count, s_nan;
    __shared__ double s_red_c[kMaxWaves];
    __shared__ int s_red_i[kMaxWaves];
    char *guard = reinterpret_cast<char *>(lds_ob + a.tile_cap);
    lds_guard_fill(guard);
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const DwaConfig &c = a.cfg;
    const double hl = c.robot_length / 2, hw = c.robot_width / 2;

    for (long b = blockIdx.x; b < a.B; b += gridDim.x) {
        double x[5];
        for (int k = 0; k < 5; ++k) x[k] = a.states[b * 5 + k];
        const double gx = a.goals[b * 2], gy = a.goals[b * 2 + 1];
        const Window win = dwa_window(x, a);
        const int S = win.nv * win.nw;

        // ---- obstacles -> LDS ----------------------------------------------------------
        __syncthreads();                               // the previous planner is done with LDS
        int M;
        bool one_tile = true;
        const double *ob = nullptr;
        if (a.ranges) {
            // local_planner.py:61-68: sentinel (100, 100), then every beam with r < threshold
            if (tid == 0) { s_count = 1; s_nan = 0; lds_ob[0] = make_double2(100.0, 100.0); }
            __syncthreads();
            const float *rg = a.ranges + b * a.scan_stride;
            for (int i = tid; i < a.n; i += blockDim.x) {
                double r = (double)rg[i];
                if (r < a.threshold) {
                    double px = a.cos_t[i] * r, py = a.sin_t[i] * r;
                    lds_ob[atomicAdd(&s_count, 1)] = make_double2(px, py);
                    if (px != px || py != py) s_nan = 1;
                }
            }
            __syncthreads();
            M = s_count;
        } else {
            M = a.M;
            if (a.counts) M = min(M, (int)a.counts[a.count_stride * b]);
            ob = a.obs + b * a.ob_stride;
            if (tid == 0) s_nan = 0;
            one_tile = M <= a.tile_cap;
            if (one_tile) {
                __syncthreads();
                for (int j = tid; j < M; j += blockDim.x) {
                    double px = ob[j], py = ob[a.M + j];
                    lds_ob[j] = make_double2(px, py);
                    if (px != px || py != py) s_nan = 1;
                }
            }
            __syncthreads();
        }

        // ---- samples: one lane each ------------------------------------------------------
        double best_c = 0.0;
        int best_i = -1;
        for (int base = 0; base < S; base += blockDim.x) {   // uniform trip count: every lane syncs
            const int s = base + tid;
            const bool act = s < S && M > 0;
            const int iv = act ? s / win.nw : 0, iw = act ? s - iv * win.nw : 0;
            const double v = arange_at(win.lo_v, c.v_reso, iv), w = arange_at(win.lo_w, c.yawrate_reso, iw);
            double px = x[0], py = x[1], yaw = x[2];
            double dm0 = INFINITY, dm1 = INFINITY, dm2 = INFINITY, dm3 = INFINITY;
            bool hit = false, nanrow = false;
            for (int r0 = 0; r0 < a.rows; r0 += R) {
                double tx[R], ty[R];
#pragma unroll
                for (int k = 0; k < R; ++k) {
                    const int r = r0 + k;
                    if (r > 0 && r < a.rows) dwa_step(px, py, yaw, v, w, c.dt);
                    tx[k] = px;                          // rows past the end repeat the last row
                    ty[k] = py;
                    nanrow |= (px != px) | (py != py);
                }
                for (int t0 = 0; t0 < M; t0 += a.tile_cap) {
                    const int cnt = min(a.tile_cap, M - t0);
                    if (!one_tile) {
                        __syncthreads();
                        for (int j = tid; j < cnt; j += blockDim.x) {
                            double ox = ob[t0 + j], oy = ob[a.M + t0 + j];
                            lds_ob[j] = make_double2(ox, oy);
                            if (ox != ox || oy != oy) s_nan = 1;
                        }
                        __syncthreads();
                    }
#pragma unroll 1
                    for (int j = 0; j < cnt; ++j) {
                        const double2 o = lds_ob[j];
#pragma unroll
                        for (int k = 0; k < R; ++k) {
                            const double dx = tx[k] - o.x, dy = ty[k] - o.y;
                            const double d2 = fma(dx, dx, dy * dy);
                            if ((k & 3) == 0) dm0 = fmin(dm0, d2);
                            if ((k & 3) == 1) dm1 = fmin(dm1, d2);
                            if ((k & 3) == 2) dm2 = fmin(dm2, d2);
                            if ((k & 3) == 3) dm3 = fmin(dm3, d2);
                            // rectangle: |tx-ox| <= length/2 and |ty-oy| <= width/2, not rotated (dwa.py:134-152)
                            if (RECT) hit |= (int)(fabs(dx) <= hl) & (int)(fabs(dy) <= hw);
                        }
                    }
                }
            }
            if (!act) continue;
            const double rmin = sqrt(fmin(fmin(dm0, dm1), fmin(dm2, dm3)));
            if (!RECT) hit = rmin <= c.robot_radius;       // any(hypot <= robot_radius) (dwa.py:153-155)
            double obc;
            if (hit) obc = INFINITY;
            else if (nanrow || s_nan) obc = NAN;           // np.min propagates a NaN distance
            else obc = 1.0 / rmin;                         // dwa.py:157-158
            // dwa.py:101-105 and calc_to_goal_cost (:162-173) on the last row
            const double ang = atan2(gy - py, gx - px) - yaw;
            double sa, ca;
            sincos(ang, &sa, &ca);
            double f = c.to_goal_cost_gain * fabs(atan2(sa, ca));
            f = f + c.speed_cost_gain * (c.max_speed - v);
            f = f + c.obstacle_cost_gain * obc;
            if (a.costs_out && s < a.s_cap) a.costs_out[b * a.s_cap + s] = f;
            if (dwa_better(f, s, best_c, best_i)) { best_c = f; best_i = s; }
        }

        // ---- selection: workgroup (cost, index) reduction ----------------------------------
        for (int off = kWave / 2; off > 0; off >>= 1) {
            double oc = __shfl_xor(best_c, off);
            int oi = __shfl_xor(best_i, off);
            if (dwa_better(oc, oi, best_c, best_i)) { best_c = oc; best_i = oi; }
        }
        if (lane == 0) { s_red_c[wave] = best_c; s_red_i[wave] = best_i; }
        __syncthreads();
        if (tid == 0) {
            for (int k = 1; k < (int)(blockDim.x / kWave); ++k)
                if (dwa_better(s_red_c[k], s_red_i[k], best_c, best_i)) { best_c = s_red_c[k]; best_i = s_red_i[k]; }
            double u0 = 0.0, u1 = 0.0;
            if (best_i >= 0) {
                const int iv = best_i / win.nw, iw = best_i - iv * win.nw;
                u0 = arange_at(win.lo_v, c.v_reso, iv);
                u1 = arange_at(win.lo_w, c.yawrate_reso, iw);
            }
            a.u_out[b * 2] = u0;
            a.u_out[b * 2 + 1] = u1;
            a.cost_out[b] = best_i >= 0 ? best_c : INFINITY;
            a.index_out[b] = best_i;
            if (a.counts_out) { a.counts_out[b * 2] = M > 0 ? win.nv : 0; a.counts_out[b * 2 + 1] = M > 0 ? win.nw : 0; }
            if (a.traj_out) {
                // the winner's rollout again, by the same arithmetic as its lane; no winner: the state alone
                double *t = a.traj_out + b * (long)a.rows * 5;
                for (int k = 0; k < 5; ++k) t[k] = x[k];
                double px = x[0], py = x[1], yaw = x[2];
                for (int r = 1; r < a.rows; ++r) {
                    double *row = t + (long)r * 5;
                    if (best_i >= 0) {
                        dwa_step(px, py, yaw, u0, u1, c.dt);
                        row[0] = px; row[1] = py; row[2] = yaw; row[3] = u0; row[4] = u1;
                    } else {
                        for (int k = 0; k < 5; ++k) row[k] = NAN;
                    }
                }
            }
        }
    }
    lds_guard_check(guard, a.status);
}

hipError_t launch_dwa(const DwaArgs &a, hipStream_t s)
{
    // one lane per sample of the widest window the config admits, 64 .. 512 lanes
    long want = (long)a.nv_cap * a.nw_cap;
    int threads = (int)((want + kWave - 1) / kWave * kWave);
    if (threads < kWave) threads = kWave;
    if (threads > 512) threads = 512;
    const long groups = a.B < kDwaMaxGroups ? a.B : kDwaMaxGroups;
    const int lds = a.tile_cap * (int)sizeof(double2) + kLdsGuard;
    const bool rect = a.cfg.robot_type != 0;
    const void *fn = rect ? (const void *)k_dwa<kDwaRows, true> : (const void *)k_dwa<kDwaRows, false>;
    hipError_t e = allow_dynamic_lds(fn, lds);
    if (e != hipSuccess) return e;
    if (rect) SLAM_LAUNCH((k_dwa<kDwaRows, true>), dim3(groups), dim3(threads), lds, s, a);
    else SLAM_LAUNCH((k_dwa<kDwaRows, false>), dim3(groups), dim3(threads), lds, s, a);
    return hipGetLastError();
}

}  // namespace slam
