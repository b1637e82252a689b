// The scan-to-map tracker's own kernels, for gfx950 (MI355X): the three small steps AROUND the matcher, the refinement
// and the ray cast of one scan (include/slam_track.h).  The matcher, the refinement, the field
// and the cast are the public calls' own launches (launch_match, launch_refine, launch_distance_field, launch_cast);
// nothing of their arithmetic is restated here.
//
//   k_track_predict   one workgroup per trajectory: lane 0 predicts (the pose step of k_pose_step), forms c0, s0 and
//                     names the map the matcher reads (none for a first scan); the lanes form the rotation table from
//                     c0, s0 and the caller's offsets and copy the scan's row of ranges [L][S][n] into the [L][n] block
//                     that the matcher, the refinement and the cast all read (the cast takes rows n apart)
//   k_track_seed      one lane per trajectory: the matcher's flat index becomes the refinement's start pose, or the
//                     refinement is told to skip the trajectory (no map)
//   k_track_decide    one lane per trajectory: keeps the refined pose or the matched one, gates, writes the skip mark
//                     and the pose the cast reads, the outputs and the state
// Every step is a handful of float64 operations per trajectory: the launches are there for the dependencies (the matcher
// needs the table, the refinement the matched pose, the cast the decision), not for the work.  Trajectories beyond a
// launch's workgroups are taken grid-stride (plan_track, launch_shapes.h).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "slam_internal.h"
#include "grid_walk.h"

namespace slam {

// state [L][8]: pose (3), key pose (3), keyed, spare
constexpr int kStPose = 0, kStKey = 3, kStKeyed = 6;

__global__ void __launch_bounds__(kTrackRowThreads) k_track_predict(TrackArgs a, int s)
{
    __shared__ double sh[2];                                         // c0, s0: all that the other lanes need of the prediction
    for (long l = blockIdx.x; l < a.L; l += gridDim.x) {
        const double *st = a.state + SLAM_TRACK_STATE_LEN * (size_t)l;
        __syncthreads();                                             // every lane is done with the last trajectory's sh
        if (threadIdx.x == 0) {
            double x = st[kStPose], y = st[kStPose + 1], th = st[kStPose + 2];
            if (a.motion) {
                const double *m = a.motion + 3 * ((size_t)l * a.S + s);
                const double c = cos(th), sn = sin(th);
                const double x1 = (x + c * m[0]) - sn * m[1];
                const double y1 = (y + sn * m[0]) + c * m[1];
                x = x1; y = y1; th = th + m[2];
            }
            const double c0 = cos(th), s0 = sin(th);
            sh[0] = c0; sh[1] = s0;
            double *p = a.pred + 5 * (size_t)l;
            p[0] = x; p[1] = y; p[2] = th; p[3] = c0; p[4] = s0;
            a.centres[2 * (size_t)l] = x; a.centres[2 * (size_t)l + 1] = y;
            a.match_maps[l] = st[kStKeyed] != 0.0 ? a.map0 + (int)l : -1;     // a first scan is not matched
            a.keys[l] = ~0ull;                                       // the matcher's "no candidate yet"
        }
        __syncthreads();
        const double c0 = sh[0], s0 = sh[1];
        for (int k = threadIdx.x; k < a.K; k += blockDim.x) {
            const double co = a.rot_off_cs[2 * (size_t)k], so = a.rot_off_cs[2 * (size_t)k + 1];
            double *r = a.rot_cs + 2 * ((size_t)l * a.K + k);
            r[0] = c0 * co - s0 * so;
            r[1] = s0 * co + c0 * so;
        }
        const float *src = a.ranges + ((size_t)l * a.S + s) * a.n;
        float *dst = a.scan + (size_t)l * a.n;
        for (int t = threadIdx.x; t < a.n; t += blockDim.x) dst[t] = src[t];
    }
}

// MATCHED: the match ran, answered and saw enough beams
__device__ __forceinline__ bool track_matched(const TrackArgs &a, long l, bool keyed)
{
    return keyed && a.best[l] >= 0 && a.used[l] >= a.min_used;
}

__global__ void __launch_bounds__(kTrackThreads) k_track_seed(TrackArgs a)
{
    for (long l = (long)blockIdx.x * blockDim.x + threadIdx.x; l < a.L; l += (long)gridDim.x * blockDim.x) {
        const double *p = a.pred + 5 * (size_t)l;
        double *q = a.start + 3 * (size_t)l;
        const bool keyed = a.state[SLAM_TRACK_STATE_LEN * (size_t)l + kStKeyed] != 0.0;
        if (!track_matched(a, l, keyed)) {
            q[0] = p[0]; q[1] = p[1]; q[2] = p[2];
            a.refine_maps[l] = -1;                                   // SLAM_REFINE_NO_MAP: nothing is evaluated
            continue;
        }
        const int wy = 2 * a.ny + 1, W = (2 * a.nx + 1) * wy;
        const int best = a.best[l], k = best / W, rem = best - k * W, i = rem / wy, j = rem - i * wy;
        q[0] = p[0] + (double)(i - a.nx) * a.step;
        q[1] = p[1] + (double)(j - a.ny) * a.step;
        q[2] = p[2] + a.rot_off[k];
        a.refine_maps[l] = a.map0 + (int)l;
    }
}

__global__ void __launch_bounds__(kTrackThreads) k_track_decide(TrackArgs a, int s)
{
    for (long l = (long)blockIdx.x * blockDim.x + threadIdx.x; l < a.L; l += (long)gridDim.x * blockDim.x) {
        double *st = a.state + SLAM_TRACK_STATE_LEN * (size_t)l;
        const double *p = a.pred + 5 * (size_t)l;
        const bool keyed = st[kStKeyed] != 0.0;
        double x = p[0], y = p[1], th = p[2];
        int flags = 0;
        bool integrate = false;
        const bool matched = track_matched(a, l, keyed);
        if (!keyed) {
            int bad = !(isfinite(x) && isfinite(y) && isfinite(th));
            (void)to_cell(x, a.scale, a.off_x, bad);
            (void)to_cell(y, a.scale, a.off_y, bad);
            if (bad) flags |= SLAM_TRACK_LOST;
            else integrate = true;
        } else if (a.best[l] < 0) {
            flags |= SLAM_TRACK_LOST;
        } else if (matched) {
            flags |= SLAM_TRACK_MATCHED;
            const double *q = a.start + 3 * (size_t)l, *r = a.refined + 3 * (size_t)l, *rc = a.refine_cost + 2 * (size_t)l;
            x = q[0]; y = q[1]; th = q[2];
            if (a.refine_status[l] == SLAM_REFINE_OK && rc[1] <= rc[0]) {
                flags |= SLAM_TRACK_REFINED;
                x = r[0]; y = r[1]; th = r[2];
            }
            const double dx = x - st[kStKey], dy = y - st[kStKey + 1], dth = th - st[kStKey + 2];
            integrate = dx * dx + dy * dy >= a.gate_dist * a.gate_dist || fabs(dth) >= a.gate_turn;
        }
        if (integrate) flags |= SLAM_TRACK_INTEGRATED;
        a.acc[l] = integrate ? 0 : SLAM_MCL_DEAD;
        double *cp = a.cast_pose + 3 * (size_t)l;
        cp[0] = x; cp[1] = y; cp[2] = th;
        const size_t row = (size_t)l * a.S + s;
        double *po = a.poses_out + 3 * row;
        po[0] = x; po[1] = y; po[2] = th;
        int32_t *io = a.info_out + SLAM_TRACK_INFO_LEN * row;
        io[0] = a.best[l]; io[1] = a.best_cost[l]; io[2] = a.used[l]; io[3] = flags;
        if (a.trace_out) {
            double *t = a.trace_out + SLAM_TRACK_TRACE_LEN * row;
            t[0] = p[0]; t[1] = p[1]; t[2] = p[2]; t[3] = p[3]; t[4] = p[4];
            const double *q = a.start + 3 * (size_t)l, *r = a.refined + 3 * (size_t)l, *rc = a.refine_cost + 2 * (size_t)l;
            for (int k = 0; k < 3; ++k) {
                t[5 + k] = matched ? q[k] : 0.0;
                t[8 + k] = matched ? r[k] : 0.0;
            }
            t[11] = matched ? rc[0] : 0.0;
            t[12] = matched ? rc[1] : 0.0;
        }
        st[kStPose] = x; st[kStPose + 1] = y; st[kStPose + 2] = th;
        if (integrate) { st[kStKey] = x; st[kStKey + 1] = y; st[kStKey + 2] = th; st[kStKeyed] = 1.0; }
    }
}

hipError_t launch_track_predict(const TrackArgs &a, int s, hipStream_t st)
{
    const TrackShape p = plan_track(a.L);
    SLAM_LAUNCH(k_track_predict, dim3((unsigned)p.row_grid), dim3(p.row_threads), 0, st, a, s);
    return hipGetLastError();
}

hipError_t launch_track_seed(const TrackArgs &a, hipStream_t st)
{
    const TrackShape p = plan_track(a.L);
    SLAM_LAUNCH(k_track_seed, dim3((unsigned)p.lane_grid), dim3(p.lane_threads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_track_decide(const TrackArgs &a, int s, hipStream_t st)
{
    const TrackShape p = plan_track(a.L);
    SLAM_LAUNCH(k_track_decide, dim3((unsigned)p.lane_grid), dim3(p.lane_threads), 0, st, a, s);
    return hipGetLastError();
}

}  // namespace slam
