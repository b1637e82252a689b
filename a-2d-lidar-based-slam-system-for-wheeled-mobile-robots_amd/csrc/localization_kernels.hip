// Scan-to-map observation kernels for gfx950: the map's obstacle cells are
// projected into the LaserScan the robot would see from a pose hypothesis, which is then
// matched against the real scan by the ICP kernel.
//
// Functional spec = W9 = "W9_Fusion Localization (LiDAR Odometry)/course_agv_slam/scripts"
// (under /root/reference):
//   Localization.updateMap        localization.py:54-60    -> k_map_obstacles
//   Localization.laserEstimation  localization.py:128-150  -> k_virtual_scan
//   Localization.laserToNumpy     localization.py:168-174  -> k_ranges64_to_points
//   Localization.calc_map_observation :152-157            -> slam_map_observation (ABI layer)
//   Localization.laserCallback    localization.py:66-126   -> k_loc_step + the scan matcher (slam_loc_replay)
//   EKF.estimate                  W9/ekf.py:17-87          -> loc_filter (inside k_loc_step)
//
// The projection is a scatter-min: every obstacle drops its distance into one beam bin and
// the bin keeps the smallest.  Distances are non-negative float64, whose bit patterns order
// like the values, so the minimum is an integer atomicMin on the bits: order-free and
// reproducible.  One lane per (obstacle, pose hypothesis), bins privatised in LDS.
#include <hip/hip_runtime.h>

#include "slam_internal.h"

namespace slam {

// updateMap (localization.py:54-60): cells > 20 or < -0.5 are obstacles (occupied AND
// unknown: pmap's 50 counts).  `wire` selects the OccupancyGrid layout data[y*width + x]
// (what the reference receives); otherwise the map is [x][y] as Mapping.pmap.  The list
// order is arbitrary (atomic append); the consumers are order-free.
__global__ void __launch_bounds__(256) k_map_obstacles(const int8_t *__restrict__ map, int width, int height, int wire,
                                                       double resolution, double origin_x, double origin_y,
                                                       double *__restrict__ ox, double *__restrict__ oy, int cap,
                                                       int *__restrict__ count)
{
    const long cells = (long)width * height;
    for (long c = (long)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += (long)gridDim.x * blockDim.x) {
        int x, y;
        if (wire) { y = (int)(c / width); x = (int)(c - (long)y * width); }
        else      { x = (int)(c / height); y = (int)(c - (long)x * height); }
        int v = map[c];
        if (v > 20 || v < 0) {
            int k = atomicAdd(count, 1);
            if (k < cap) {
                ox[k] = (x * resolution + origin_x) * 1.0;           // :57
                oy[k] = (y * resolution + origin_y) * 1.0;           // :58
            }
        }
    }
}

__global__ void __launch_bounds__(256) k_fill_u64(unsigned long long *p, long n, unsigned long long v)
{
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) p[i] = v;
}

// One obstacle of laserEstimation (localization.py:137-146) dropped into the beam bins of a pose: the distance, the
// bin and its wrap, once for k_virtual_scan and k_loc_step - a step of the batched node fills the same bits
// slam_virtual_scan fills at that pose.
__device__ __forceinline__ void vscan_drop(unsigned long long *bins, int n, double px, double py, double pth, double x, double y,
                                           double angle_min, double angle_increment)
{
    double dist = hypot(px - x, py - y);                                          // :138
    double q = (atan2(y - py, x - px) - angle_min - pth) / angle_increment;       // :139
    if (!(fabs(q) < 2.0e9)) return;                  // NaN / absurd: the reference would raise or spin
    long index = (long)q;                            // int(): truncation toward zero
    index %= n;                                      // the two while-loops of :141-144
    if (index < 0) index += n;
    atomicMin(&bins[index], (unsigned long long)__double_as_longlong(dist));      // :145-146 (strict '<' = min)
}

// laserEstimation (localization.py:128-150).  blockIdx.y = pose hypothesis, blockIdx.x = slice
// of the obstacle list.  The beam bins of the hypothesis live in LDS (n x 8 B) and take the
// scatter-min there (ds_min_u64); a workgroup that owns the whole list stores its bins,
// otherwise the slices meet in global memory with one atomicMin per touched bin.
__global__ void __launch_bounds__(256) k_virtual_scan(const double *__restrict__ ox, const double *__restrict__ oy, int K,
                                                      const double *__restrict__ poses, double angle_min,
                                                      double angle_increment, int n, unsigned long long empty,
                                                      unsigned long long *__restrict__ ranges)
{
    extern __shared__ unsigned long long bins[];
    const int b = blockIdx.y;
    const double px = poses[3 * b], py = poses[3 * b + 1], pth = poses[3 * b + 2];
    unsigned long long *r = ranges + (long)b * n;
    for (int i = threadIdx.x; i < n; i += blockDim.x) bins[i] = empty;
    __syncthreads();
    const int per = (K + gridDim.x - 1) / gridDim.x;
    const int lo = blockIdx.x * per, hi = min(K, lo + per);
    for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        vscan_drop(bins, n, px, py, pth, ox[i], oy[i], angle_min, angle_increment);
    }
    __syncthreads();
    if (gridDim.x == 1) {
        for (int i = threadIdx.x; i < n; i += blockDim.x) r[i] = bins[i];
    } else {
        for (int i = threadIdx.x; i < n; i += blockDim.x)
            if (bins[i] < empty) atomicMin(&r[i], bins[i]);
    }
}

// laserToNumpy on float64 ranges (localization.py:168-174): [B][n] -> points [B][2][n].
__global__ void __launch_bounds__(256) k_ranges64_to_points(const double *__restrict__ ranges, const double *__restrict__ cos_t,
                                                            const double *__restrict__ sin_t, long total, int n,
                                                            double *__restrict__ pts)
{
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        long b = e / n;
        int i = (int)(e - b * n);
        double r = ranges[e];
        pts[b * 2 * n + i] = cos_t[i] * r;
        pts[b * 2 * n + n + i] = sin_t[i] * r;
    }
}

// ---- the batched node: Localization.laserCallback (localization.py:66-126) for L trajectories in lockstep ----------
//
// A step of a trajectory is three scan-matcher solves, two pose compositions and the 3x3 filter.  T1 of the steps
// after the first and every T2 depend on the stream alone and are solved up front (k_loc_stream_pairs + one scan-matcher
// launch); what is left per step is the map observation, whose target is the virtual scan at the xEst the step BEFORE
// left - a true recurrence.  So a step is two launches: k_loc_step, one workgroup per trajectory, finishes the step before
// from the transform the scan matcher left in memory (prologue, one lane) and prepares the pair of this step (body, every
// lane); then the scan matcher over the L pairs.  Nothing returns to the host in between.

// The pose algebra repeated at localization.py:79-83, 102-106, 113-118 and in ekf.py's odom_model, in the reference's
// evaluation order: x + cos*tx - sin*ty, y + sin*tx + cos*ty, theta + atan2(T10, T00).
__device__ __forceinline__ void loc_compose(const double s[3], const double T[9], double out[3])
{
    const double yaw = atan2(T[3], T[0]);
    const double c = cos(s[2]), sn = sin(s[2]);
    out[0] = s[0] + c * T[2] - sn * T[5];
    out[1] = s[1] + sn * T[2] + c * T[5];
    out[2] = s[2] + yaw;
}

// inv of a 3x3 matrix as numpy.linalg.inv does it (ekf.py:84): elimination with partial pivoting, then the three
// columns of the identity solved back.  Rows are exchanged value by value (constant indices: no scratch).
__device__ __forceinline__ void loc_inv3(const double A[9], double X[9])
{
    double a[3][6];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int j = 0; j < 6; ++j) a[r][j] = j < 3 ? A[3 * r + j] : (j - 3 == r ? 1.0 : 0.0);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int r = k + 1; r < 3; ++r) {
            const bool sw = fabs(a[r][k]) > fabs(a[k][k]);           // the largest of the column comes up; the first of equals stays
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const double u = a[k][j], v = a[r][j];
                a[k][j] = sw ? v : u;
                a[r][j] = sw ? u : v;
            }
        }
#pragma unroll
        for (int r = k + 1; r < 3; ++r) {
            const double f = a[r][k] / a[k][k];
#pragma unroll
            for (int j = k + 1; j < 6; ++j) a[r][j] = a[r][j] - f * a[k][j];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double x2 = a[2][3 + c] / a[2][2];
        const double x1 = (a[1][3 + c] - a[1][2] * x2) / a[1][1];
        const double x0 = (a[0][3 + c] - a[0][1] * x1 - a[0][2] * x2) / a[0][0];
        X[c] = x0; X[3 + c] = x1; X[6 + c] = x2;
    }
}

__device__ __forceinline__ void loc_mul3(const double A[9], const double B[9], double C[9])
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}

// EKF.estimate(xEst, PEst, z, T) of W9/ekf.py:17-87, operation by operation: odom_model and jacob_f predict,
// the absolute pose z corrects; the reference's R (prediction) and Q (innovation) are the same diagonal (:6-13).
__device__ __forceinline__ void loc_filter(double x[3], double P[9], const double z[3], const double T[9])
{
    const double third = (M_PI / 60.0) * (M_PI / 60.0);
    const double noise[3] = {0.2 * 0.2, 0.2 * 0.2, third};
    double xp[3];
    loc_compose(x, T, xp);                                            // odom_model
    double J[9] = {1.0, 0.0, -T[2] * T[3] - T[5] * T[0], 0.0, 1.0, T[2] * T[0] - T[5] * T[3], 0.0, 0.0, 1.0};   // jacob_f
    double Jt[9], JP[9], Pp[9], Sm[9], Si[9], K[9], IK[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Jt[3 * i + j] = J[3 * j + i];
    loc_mul3(J, P, JP);
    loc_mul3(JP, Jt, Pp);                                             // J P J^T + R
#pragma unroll
    for (int i = 0; i < 3; ++i) Pp[4 * i] = Pp[4 * i] + noise[i];
#pragma unroll
    for (int i = 0; i < 9; ++i) Sm[i] = Pp[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) Sm[4 * i] = Sm[4 * i] + noise[i];     // S = P_pred + Q
    loc_inv3(Sm, Si);
    loc_mul3(Pp, Si, K);                                              // K = P_pred S^-1
    const double y[3] = {z[0] - xp[0], z[1] - xp[1], z[2] - xp[2]};
#pragma unroll
    for (int i = 0; i < 3; ++i) x[i] = xp[i] + (K[3 * i] * y[0] + K[3 * i + 1] * y[1] + K[3 * i + 2] * y[2]);
#pragma unroll
    for (int i = 0; i < 9; ++i) IK[i] = ((i % 4 == 0) ? 1.0 : 0.0) - K[i];
    loc_mul3(IK, Pp, P);                                              // (I - K) P_pred
}

__device__ __forceinline__ bool loc_finite9(const double T[9])
{
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) ok = ok && isfinite(T[i]);
    return ok;
}

__global__ void __launch_bounds__(256) k_loc_step(LocArgs a)
{
    extern __shared__ unsigned long long loc_lds[];
    unsigned long long *bins = loc_lds;                               // [n] beam bins of the virtual scan
    double *hand = reinterpret_cast<double *>(bins + a.n);            // xEst and "this trajectory goes on"
    char *guard = reinterpret_cast<char *>(hand + 4);
    lds_guard_fill(guard);
    const int l = blockIdx.x, n = a.n, tid = threadIdx.x;
    const int st = a.stream_of_traj ? a.stream_of_traj[l] : l;
    const int m = a.map_of_traj ? a.map_of_traj[l] : 0;
    const bool routed = st >= 0 && st < a.S && m >= 0 && m < a.M;
    if (tid == 0) {
        double *sv = a.state + (long)l * kLocStateDoubles;
        double x[3], xo[3], P[9];
        int status;
        if (a.step == 0) {                                            // xEst = xOdom = pose0, PEst = eye(3) (localization.py:30-33)
#pragma unroll
            for (int i = 0; i < 3; ++i) x[i] = xo[i] = a.pose0 ? a.pose0[3 * (long)l + i] : 0.0;
#pragma unroll
            for (int i = 0; i < 9; ++i) P[i] = (i % 4 == 0) ? 1.0 : 0.0;
            status = routed ? SLAM_LOC_OK : SLAM_LOC_BAD_ROUTE;
        } else {
#pragma unroll
            for (int i = 0; i < 3; ++i) { x[i] = sv[i]; xo[i] = sv[3 + i]; }
#pragma unroll
            for (int i = 0; i < 9; ++i) P[i] = sv[6 + i];
            status = (int)sv[15];
            const int p = a.step - 1;                                 // the step the scan matcher has just solved
            const long o = (long)l * a.n_scan + p;
            double T1[9], T2[9], t[9];
            int it = -1;
            bool ok = status == SLAM_LOC_OK;
            if (ok) {
                const double *Ts = a.T_stream + (long)st * (2 * a.n_scan - 1) * 9;
#pragma unroll
                for (int i = 0; i < 9; ++i) {
                    t[i] = a.T_step[9 * (long)l + i];                 // calc_map_observation (:152-157)
                    T2[i] = Ts[9 * (long)p + i];                      // the second calc_odometry (:100): the scan against itself
                    // the first calc_odometry (:78): against the scan before; the very first target is the map's virtual
                    // scan at pose0 (:159-168) - the pair the map observation of step 0 has, solved once
                    T1[i] = p == 0 ? t[i] : Ts[9 * (long)(a.n_scan + p - 1) + i];
                }
                it = a.iters_step[l];
                ok = loc_finite9(T1) && loc_finite9(T2) && loc_finite9(t);   // numpy's svd raises LinAlgError in the reference
                if (!ok) status = SLAM_LOC_NONFINITE;                 // stops with the state it had before this step
            }
            if (ok) {
                double xo2[3], z[3];
                loc_compose(xo, T1, xo2);                             // :79-83
                loc_compose(x, t, z);                                 // :113-118
#pragma unroll
                for (int i = 0; i < 3; ++i) xo[i] = xo2[i];
                loc_filter(x, P, z, T2);                              // :120
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                a.xest_out[3 * o + i] = ok ? x[i] : NAN;
                a.xodom_out[3 * o + i] = ok ? xo[i] : NAN;
            }
            if (a.iters_obs_out) a.iters_obs_out[o] = ok ? it : -1;
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                if (a.T_obs_out) a.T_obs_out[9 * o + i] = ok ? t[i] : NAN;
                if (a.T_odom_out) a.T_odom_out[9 * o + i] = ok ? T1[i] : NAN;
            }
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) { sv[i] = x[i]; sv[3 + i] = xo[i]; hand[i] = x[i]; }
#pragma unroll
        for (int i = 0; i < 9; ++i) sv[6 + i] = P[i];
        sv[15] = (double)status;
        hand[3] = status == SLAM_LOC_OK ? 1.0 : 0.0;
        if (!a.body) {
#pragma unroll
            for (int i = 0; i < 9; ++i) a.P_final_out[9 * (long)l + i] = P[i];
            a.status_out[l] = status;
        }
    }
    __syncthreads();
    double *tar = a.tar_pts + (long)l * 2 * n, *src = a.src_pts + (long)l * 2 * n;
    if (a.body && hand[3] != 0.0) {
        // laserEstimation at xEst (:128-150): the scatter-min of k_virtual_scan over this trajectory's map
        const double px = hand[0], py = hand[1], pth = hand[2];
        const double hundred = 100.0;                                 // data.ranges = [100.0]*total_num (:135)
        const unsigned long long empty = (unsigned long long)__double_as_longlong(hundred);
        for (int i = tid; i < n; i += blockDim.x) bins[i] = empty;
        __syncthreads();
        long lo = a.obs_off[m], hi = a.obs_off[m + 1];
        lo = lo < 0 ? 0 : lo;
        hi = hi > a.K ? a.K : hi;
        for (long i = lo + tid; i < hi; i += blockDim.x) vscan_drop(bins, n, px, py, pth, a.ox[i], a.oy[i], a.angle_min, a.angle_increment);
        __syncthreads();
        const float *r32 = a.ranges + ((long)st * a.n_scan + a.step) * n;
        double *dbg = a.tar_pts_out ? a.tar_pts_out + ((long)l * a.n_scan + a.step) * 2 * n : nullptr;
        for (int i = tid; i < n; i += blockDim.x) {
            const double r = __longlong_as_double((long long)bins[i]);
            const double tx = a.cos_t[i] * r, ty = a.sin_t[i] * r;    // laserToNumpy on the virtual scan (:170-176)
            tar[i] = tx;
            tar[n + i] = ty;
            if (dbg) { dbg[i] = tx; dbg[n + i] = ty; }
            const double rs = (double)r32[i];                         // laserToNumpy on the message: no inf clip
            src[i] = a.cos_t[i] * rs;
            src[n + i] = a.sin_t[i] * rs;
        }
    } else if (a.body && a.step == 0) {
        // a trajectory that never starts: the scan matcher still reads its pair
        for (int i = tid; i < 2 * n; i += blockDim.x) tar[i] = src[i] = 0.0;
    }
    lds_guard_check(guard, a.status);
}

// laserToNumpy (:170-176) of both scans of every stream-only pair: pair j < n_scan of a stream is (scan j, scan j) -
// the second calc_odometry of step j (:100) - and pair n_scan + s - 1 is (scan s - 1, scan s), the first of step s >= 1.
__global__ void __launch_bounds__(256) k_loc_stream_pairs(const float *__restrict__ ranges, const double *__restrict__ cos_t,
                                                          const double *__restrict__ sin_t, int n_scan, int n,
                                                          double *__restrict__ pairs)
{
    const int per = 2 * n_scan - 1;
    const long pair = blockIdx.x;
    const long stream = pair / per;
    const int j = (int)(pair - stream * per);
    const int s_src = j < n_scan ? j : j - n_scan + 1, s_tar = j < n_scan ? j : j - n_scan;
    const float *rt = ranges + (stream * n_scan + s_tar) * n, *rs = ranges + (stream * n_scan + s_src) * n;
    double *o = pairs + pair * 4 * n;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const double a = (double)rt[i], b = (double)rs[i];
        o[i] = cos_t[i] * a;
        o[n + i] = sin_t[i] * a;
        o[2 * n + i] = cos_t[i] * b;
        o[3 * n + i] = sin_t[i] * b;
    }
}

hipError_t launch_loc_step(const LocArgs &a, hipStream_t s)
{
    const int lds = a.n * 8 + 32 + kLdsGuard;
    const int threads = a.n <= 64 && a.K <= 64 ? 64 : 256;
    SLAM_LAUNCH(k_loc_step, dim3(a.L), dim3(threads), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_loc_stream_pairs(const float *ranges, const double *cos_t, const double *sin_t, int S, int n_scan, int n,
                                   double *pairs, hipStream_t s)
{
    const long total = (long)S * (2 * n_scan - 1);
    SLAM_LAUNCH(k_loc_stream_pairs, dim3((unsigned)total), dim3(n <= 64 ? 64 : n <= 128 ? 128 : 256), 0, s, ranges, cos_t, sin_t,
                n_scan, n, pairs);
    return hipGetLastError();
}

hipError_t launch_map_obstacles(const int8_t *map, int width, int height, int wire, double resolution, double origin_x,
                                double origin_y, double *ox, double *oy, int cap, int *count, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(count, 0, sizeof(int), s);
    if (e != hipSuccess) return e;
    long cells = (long)width * height;
    long blocks = (cells + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    SLAM_LAUNCH(k_map_obstacles, dim3(blocks), dim3(256), 0, s, map, width, height, wire, resolution, origin_x,
                       origin_y, ox, oy, cap, count);
    return hipGetLastError();
}

hipError_t launch_virtual_scan(const double *ox, const double *oy, int K, const double *poses, int B, double angle_min,
                               double angle_increment, int n, double *ranges, hipStream_t s)
{
    const double hundred = 100.0;                                    // data.ranges = [100.0]*total_num (:135)
    unsigned long long bits;
    memcpy(&bits, &hundred, sizeof bits);
    // enough workgroups to fill 256 CUs a few times over; a slice is at least 1024 obstacles
    int slices = (2048 + B - 1) / B;
    int max_slices = (K + 1023) / 1024;
    if (slices > max_slices) slices = max_slices;
    if (slices < 1) slices = 1;
    long total = (long)B * n;
    if (slices > 1)
        SLAM_LAUNCH(k_fill_u64, dim3((total + 255) / 256 > 1024 ? 1024 : (total + 255) / 256), dim3(256), 0, s,
                           reinterpret_cast<unsigned long long *>(ranges), total, bits);
    SLAM_LAUNCH(k_virtual_scan, dim3(slices, B), dim3(256), (size_t)n * 8, s, ox, oy, K, poses, angle_min,
                       angle_increment, n, bits, reinterpret_cast<unsigned long long *>(ranges));
    return hipGetLastError();
}

hipError_t launch_ranges64_to_points(const double *ranges, const double *cos_t, const double *sin_t, int B, int n,
                                     double *pts, hipStream_t s)
{
    long total = (long)B * n;
    long blocks = (total + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    SLAM_LAUNCH(k_ranges64_to_points, dim3(blocks), dim3(256), 0, s, ranges, cos_t, sin_t, total, n, pts);
    return hipGetLastError();
}

}  // namespace slam
