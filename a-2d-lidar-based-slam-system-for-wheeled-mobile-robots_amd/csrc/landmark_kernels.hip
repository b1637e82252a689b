// Landmark half of the W12 node, batched:
//   Extraction.process        W12m/extraction.py:24-89  -> k_landmark_extract (one workgroup per scan)
//   SLAM_EKF.observation      W12m/slam_ekf.py:96-106   -> k_landmark_extract (the rows behind the means)
//   EKF.estimate              W12m/ekf_lm.py:15-50      -> k_ekf_lm (one wave per trajectory, state in LDS)
//   the kept-scan rule        W12m/slam_ekf.py:74-82    -> k_node_keep / k_node_gather
// One scan and one filter have no data parallelism; S scans and B trajectories do, and
// inside a filter step the association runs over the landmarks and the covariance update over the state.
// float64 throughout; the rules, quirks included, are those of extraction.py / ekf_lm.py of the package.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <math.h>

#include "slam_internal.h"

namespace slam {

namespace {

// Python's float % (floatobject.c float_rem, numpy npy_divmod): the result takes the sign of the divisor
__device__ __forceinline__ double py_mod(double a, double b)
{
    double m = fmod(a, b);
    if (m != 0.0) {
        if ((b < 0.0) != (m < 0.0)) m += b;
    } else {
        m = copysign(0.0, b);
    }
    return m;
}
__device__ __forceinline__ double pi_2_pi(double a) { return py_mod(a + M_PI, 2.0 * M_PI) - M_PI; }   // ekf_lm.py:141

// Exclusive prefix count of the 0 / 1 flags f[0 .. m) into out[0 .. m); returns the total.  Whole workgroup
// (a multiple of 64 threads, at most kMaxWaves waves); wsum: kMaxWaves ints of LDS.
__device__ int block_prefix(const int *f, int *out, int m, int *wsum)
{
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave, nw = blockDim.x / kWave;
    int base = 0;
    for (int c0 = 0; c0 < m; c0 += blockDim.x) {
        const int i = c0 + threadIdx.x;
        const bool on = i < m && f[i] != 0;
        const unsigned long long mask = __ballot(on);
        if (lane == 0) wsum[w] = __popcll(mask);
        __syncthreads();
        int pre = base, tot = 0;
        for (int k = 0; k < nw; ++k) {
            if (k < w) pre += wsum[k];
            tot += wsum[k];
        }
        if (i < m) out[i] = pre + __popcll(mask & ((1ull << lane) - 1ull));
        base += tot;
        __syncthreads();
    }
    return base;
}

}  // namespace

// ---- extraction ------------------------------------------------------------------------
// One workgroup per scan.  The sequential labelling of extraction.py:36-61 has a closed form: the gaps that
// are NOT below the threshold ("breaks") cut the first n-1 points into runs; the cluster number of point i is
// the number of breaks before it; break i closes cluster pre[i] = points first .. i where first follows the
// previous break, and needs i - first >= 2.  So: break flags in parallel, one prefix count, then the closed
// clusters are tested for their extent wave by wave - pairs taken farthest apart in index first, so a wall
// (100-150 beams) is out on its (first, last) pair - and the landmarks are ranked by a second prefix count.
__global__ void __launch_bounds__(256) k_landmark_extract(LandmarkArgs a)
{
    extern __shared__ double lm_lds[];
    __shared__ int wsum[kMaxWaves];
    const int n = a.n, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave, nw = blockDim.x / kWave;
    double *px = lm_lds, *py = px + n;
    int *brk = reinterpret_cast<int *>(py + n);       // break flags, later the landmark flag of every closed cluster
    int *pre = brk + n;                               // breaks before point i, later the rank of a landmark
    int *cfirst = pre + n;                            // [n + 1] first point of cluster id
    int *clast = cfirst + n + 1;                      // the break that closes cluster id
    char *guard = reinterpret_cast<char *>(clast + n + 1);
    lds_guard_fill(guard);
    for (long s = blockIdx.x; s < a.S; s += gridDim.x) {
        const float *r = a.ranges + s * n;
        for (int i = tid; i < n; i += blockDim.x) {
            double rr = (double)r[i];
            if (rr == INFINITY) rr = 30.0;                               // slam_ekf.py:119
            px[i] = a.cos_t[i] * rr;                                     // :122
            py[i] = a.sin_t[i] * rr;
        }
        __syncthreads();
        const int m = n - 1;                                             // gaps = labelled points (extraction.py:36)
        for (int i = tid; i < m; i += blockDim.x) {
            const double dx = px[i] - px[i + 1], dy = py[i] - py[i + 1];
            brk[i] = !(sqrt(dx * dx + dy * dy) < a.range_threshold);     // :37-38
        }
        if (tid == 0) cfirst[0] = 0;
        __syncthreads();
        const int nb = m > 0 ? block_prefix(brk, pre, m, wsum) : 0;     // closed clusters: ids 0 .. nb-1
        for (int i = tid; i < m; i += blockDim.x)
            if (brk[i]) {
                clast[pre[i]] = i;
                cfirst[pre[i] + 1] = i + 1;
            }
        __syncthreads();
        if (a.labels)
            for (int i = tid; i < m; i += blockDim.x) {
                int lab = pre[i];
                if (brk[i] && i - cfirst[lab] < 2) lab = -1;             // :56-61
                a.labels[s * m + i] = lab;
            }
        __syncthreads();
        // extent of every closed cluster with two earlier members (:41-49); brk[] becomes the landmark flag
        for (int id = wave; id < nb; id += nw) {
            const int f = cfirst[id], mp = clast[id] - f + 1;
            bool fail = mp < 3;
            for (int d = mp - 1; d >= 0 && !fail; --d) {
                bool far = false;
                for (int p = lane; p < mp - d; p += kWave) {
                    const double dx = px[f + p] - px[f + p + d], dy = py[f + p] - py[f + p + d];
                    far |= !(sqrt(dx * dx + dy * dy) < a.radius_max_th);
                }
                fail = __any(far);
            }
            if (lane == 0) brk[id] = !fail;
        }
        __syncthreads();
        const int found = nb > 0 ? block_prefix(brk, pre, nb, wsum) : 0;
        for (int id = tid; id < nb; id += blockDim.x) {
            const int k = pre[id];
            if (!brk[id] || k >= a.lm_cap) continue;
            const int f = cfirst[id], l = clast[id];
            double sx = 0.0, sy = 0.0;
            for (int p = f; p <= l; ++p) {                               // running sums in index order (:81-83)
                sx += px[p];
                sy += py[p];
            }
            const double cnt = (double)(l - f + 1), mx = sx / cnt, my = sy / cnt;
            const long o = s * a.lm_cap + k;
            a.ids[o] = id;
            a.means[2 * o] = mx;
            a.means[2 * o + 1] = my;
            a.z[2 * o] = hypot(mx, my);                                  // slam_ekf.py:96-106
            a.z[2 * o + 1] = pi_2_pi(atan2(my, mx));
        }
        const int kept = found < a.lm_cap ? found : a.lm_cap;
        for (int k = kept + tid; k < a.lm_cap; k += blockDim.x) {        // unused slots read the same on every run
            const long o = s * a.lm_cap + k;
            a.ids[o] = -1;
            a.means[2 * o] = a.means[2 * o + 1] = a.z[2 * o] = a.z[2 * o + 1] = 0.0;
        }
        if (tid == 0) {
            a.count[s] = kept;
            a.overflow[s] = found > a.lm_cap;
        }
        __syncthreads();
    }
    lds_guard_check(guard, a.status);
}

size_t landmark_lds_bytes(int n) { return (size_t)n * 16 + ((size_t)4 * n + 2) * 4 + 8; }

hipError_t launch_landmarks(const LandmarkArgs &a, hipStream_t s)
{
    const int lds = (int)landmark_lds_bytes(a.n) + kLdsGuard;
    hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(&k_landmark_extract), lds);
    if (e != hipSuccess) return e;
    const int threads = a.n <= 64 ? 64 : a.n <= 128 ? 128 : 256;
    const long groups = a.S < kLandmarkMaxGroups ? a.S : kLandmarkMaxGroups;
    SLAM_LAUNCH(k_landmark_extract, dim3((unsigned)groups), dim3(threads), lds, s, a);
    return hipGetLastError();
}

// ---- filter ----------------------------------------------------------------------------
// One wave per trajectory: a filter step is a chain of dependent scalar work (sqrt, atan2, a 2x2 inverse)
// between three short parallel pieces, so more lanes would only wait at barriers.  x and P live in LDS with
// the row stride of the largest state, 3 + 2 max_lm, so appending a landmark moves nothing.
// H has five non-zero columns (the pose and the landmark): S, K and the update P -= K (H P) touch only them;
// (I - K H) P of ekf_lm.py:48 is the same product without the zeros.
namespace {

constexpr double kMDistTh = 0.6;                       // ekf_lm.py:8
struct Corr {                                          // laser_correction (:110-122) without the dense H
    double y0, y1, g[2][5];
    int col[5];
};

__device__ __forceinline__ void correction(const double *x, int id, double zr, double zb, Corr &c)
{
    const int L = 3 + 2 * id;
    const double dx = x[L] - x[0], dy = x[L + 1] - x[1];
    const double q = dx * dx + dy * dy;
    const double za = atan2(dy, dx) - x[2];
    const double sq = sqrt(q);
    c.y0 = zr - sq;
    c.y1 = pi_2_pi(zb - pi_2_pi(za));
    c.g[0][0] = -sq * dx / q; c.g[0][1] = -sq * dy / q; c.g[0][2] = 0.0 / q; c.g[0][3] = sq * dx / q; c.g[0][4] = sq * dy / q;
    c.g[1][0] = dy / q; c.g[1][1] = -dx / q; c.g[1][2] = -q / q; c.g[1][3] = -dy / q; c.g[1][4] = dx / q;   // :124-138
    c.col[0] = 0; c.col[1] = 1; c.col[2] = 2; c.col[3] = L; c.col[4] = L + 1;
}

}  // namespace

__global__ void __launch_bounds__(64) k_ekf_lm(EkfArgs a)
{
    extern __shared__ double ekf_lds[];
    const int N = 3 + 2 * a.max_lm, lane = threadIdx.x;
    double *x = ekf_lds, *P = x + N, *xb = P + N * N, *Pb = xb + N, *HP = Pb + N * N, *K = HP + 2 * N, *dist = K + 2 * N;
    char *guard = reinterpret_cast<char *>(dist + a.max_lm + 1);
    lds_guard_fill(guard);
    const double cx0 = 0.35 * 0.35, cx2 = (15.0 * (M_PI / 180.0)) * (15.0 * (M_PI / 180.0));   // ekf_lm.py:5
    for (long b = blockIdx.x; b < a.B; b += gridDim.x) {
        for (int i = lane; i < N * N; i += kWave) P[i] = (i / N == i % N && i / N < 3) ? 1.0 : 0.0;
        for (int i = lane; i < N; i += kWave) x[i] = (i < 3 && a.x0) ? a.x0[3 * b + i] : 0.0;
        __syncthreads();
        int nlm = 0, status = SLAM_NODE_OK;
        int steps = a.steps[b] - a.steps_bias;
        steps = steps < 0 ? 0 : steps > a.steps_max ? a.steps_max : steps;
        int s = 0;
        for (; s < steps; ++s) {
            const long step = b * a.steps_max + s;
            // this step's observation rows
            long zs;
            int zc;
            if (a.kept) {
                const long scan = b * (a.steps_max + 1) + a.kept[b * (a.steps_max + 1) + s + 1];
                if (a.lm_overflow[scan]) { status = SLAM_NODE_OBS_CAP; break; }
                zs = scan * a.lm_cap;
                zc = a.lm_count[scan];
            } else {
                long z0 = a.z_off[step], z1 = a.z_off[step + 1];
                z0 = z0 < 0 ? 0 : z0 > a.nz ? a.nz : z0;
                z1 = z1 < z0 ? z0 : z1 > a.nz ? a.nz : z1;
                zs = z0;
                zc = (int)(z1 - z0 > INT_MAX ? INT_MAX : z1 - z0);
            }
            const int Nc0 = 3 + 2 * nlm;
            for (int i = lane; i < Nc0 * Nc0; i += kWave) Pb[(i / Nc0) * N + i % Nc0] = P[(i / Nc0) * N + i % Nc0];
            for (int i = lane; i < Nc0; i += kWave) xb[i] = x[i];
            double ux, uy, uw;
            if (a.u) {
                ux = a.u[3 * step]; uy = a.u[3 * step + 1]; uw = a.u[3 * step + 2];
            } else {                                                     // T2u, slam_ekf.py:125-128
                const double *T = a.T + 9 * step;
                ux = T[2]; uy = T[5]; uw = atan2(T[3], T[0]);
            }
            // predict (:19-22): every lane computes it, lane 0 stores
            {
                const double yaw = x[2], cy = cos(yaw), sy = sin(yaw);
                double G[3][3] = {{1.0, 0.0, -sy * ux - cy * uy}, {0.0, 1.0, cy * ux - sy * uy}, {0.0, 0.0, 1.0}};
                double P3[3][3], A[3][3], R[3][3];
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) P3[i][j] = P[i * N + j];
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        double v = 0.0;
#pragma unroll
                        for (int k = 0; k < 3; ++k) v += G[k][i] * P3[k][j];     // G.transpose() . P
                        A[i][j] = v;
                    }
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        double v = 0.0;
#pragma unroll
                        for (int k = 0; k < 3; ++k) v += A[i][k] * G[k][j];
                        R[i][j] = v + (i == j ? (i < 2 ? cx0 : cx2) : 0.0);
                    }
                const double nx = x[0] + cy * ux - sy * uy, ny = x[1] + sy * ux + cy * uy, nyaw = yaw + uw;   // :52-63
                __syncthreads();
                if (lane == 0) {
                    x[0] = nx; x[1] = ny; x[2] = nyaw;
#pragma unroll
                    for (int i = 0; i < 3; ++i)
#pragma unroll
                        for (int j = 0; j < 3; ++j) P[i * N + j] = R[i][j];
                }
                __syncthreads();
            }
            const int num_lm = nlm;                                      // (n1 - 3) / 2 of :16, never refreshed
            bool early = false;
            for (int o = 0; o < zc && status == SLAM_NODE_OK; ++o) {
                const double zr = a.z[2 * (zs + o)], zb = a.z[2 * (zs + o) + 1];
                // association (:90-108): one lane per known landmark
                for (int j = lane; j < nlm; j += kWave) {
                    Corr c;
                    correction(x, j, zr, zb, c);
                    double hp[2][5], S[2][2];
#pragma unroll
                    for (int r = 0; r < 2; ++r)
#pragma unroll
                        for (int k2 = 0; k2 < 5; ++k2) {
                            double v = 0.0;
#pragma unroll
                            for (int k = 0; k < 5; ++k) v += c.g[r][k] * P[c.col[k] * N + c.col[k2]];
                            hp[r][k2] = v;
                        }
#pragma unroll
                    for (int r = 0; r < 2; ++r)
#pragma unroll
                        for (int r2 = 0; r2 < 2; ++r2) {
                            double v = 0.0;
#pragma unroll
                            for (int k = 0; k < 5; ++k) v += hp[r][k] * c.g[r2][k];
                            S[r][r2] = v + (r == r2 ? cx0 : 0.0);
                        }
                    const double det = S[0][0] * S[1][1] - S[0][1] * S[1][0];
                    const double i00 = S[1][1] / det, i01 = -S[0][1] / det, i10 = -S[1][0] / det, i11 = S[0][0] / det;
                    const double t0 = c.y0 * i00 + c.y1 * i10, t1 = c.y0 * i01 + c.y1 * i11;
                    dist[j] = t0 * c.y0 + t1 * c.y1;
                }
                __syncthreads();
                int best = nlm;
                double best_d = kMDistTh;                                // the threshold is the list's last entry
                for (int j = 0; j < nlm; ++j) {                          // min_dist.index(min(min_dist)): first minimum
                    const double d = dist[j];
                    if (d < best_d || (d == best_d && best == nlm)) { best = j; best_d = d; }
                }
                if (best == num_lm) {                                    // :36-38
                    if (nlm != num_lm) { status = SLAM_NODE_REF_RAISES; break; }   // np.hstack of n1 + 2 and n1 rows raises
                    if (nlm == a.max_lm) { status = SLAM_NODE_LM_CAP; break; }
                    const int Nc = 3 + 2 * nlm;
                    const double ang = x[2] + zb;
                    const double lx = x[0] + zr * cos(ang), ly = x[1] + zr * sin(ang);   // :77-83
                    __syncthreads();
                    for (int i = lane; i < 2 * (Nc + 2); i += kWave) {
                        const int r = Nc + i / (Nc + 2), cc = i % (Nc + 2);
                        P[r * N + cc] = (r == cc) ? 1.0 : 0.0;
                        if (cc < Nc) P[cc * N + r] = 0.0;
                    }
                    if (lane == 0) { x[Nc] = lx; x[Nc + 1] = ly; }
                    ++nlm;
                    __syncthreads();
                } else if (best == nlm) {                                // no slot for it: `if len(lm) == 0: return` (:40-42)
                    early = true;
                    break;
                }
                const int Nc = 3 + 2 * nlm;
                Corr c;
                correction(x, best, zr, zb, c);
                for (int i = lane; i < 2 * Nc; i += kWave) {             // H P (2 x Nc) and P H^T (Nc x 2)
                    const int r = i / Nc, cc = i % Nc;
                    double v = 0.0, w = 0.0;
#pragma unroll
                    for (int k = 0; k < 5; ++k) {
                        const double g = r ? c.g[1][k] : c.g[0][k];      // (a select: indexing by r would put c in scratch)
                        v += g * P[c.col[k] * N + cc];
                        w += P[cc * N + c.col[k]] * g;
                    }
                    HP[r * N + cc] = v;
                    K[r * N + cc] = w;                                   // P H^T for now
                }
                __syncthreads();
                double S[2][2];
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int r2 = 0; r2 < 2; ++r2) {
                        double v = 0.0;
#pragma unroll
                        for (int k = 0; k < 5; ++k) v += HP[r * N + c.col[k]] * c.g[r2][k];
                        S[r][r2] = v + (r == r2 ? cx0 : 0.0);
                    }
                const double det = S[0][0] * S[1][1] - S[0][1] * S[1][0];
                const double i00 = S[1][1] / det, i01 = -S[0][1] / det, i10 = -S[1][0] / det, i11 = S[0][0] / det;
                __syncthreads();
                for (int i = lane; i < Nc; i += kWave) {                 // K = P H^T S^-1 (:46), x += K y (:47)
                    const double p0 = K[i], p1 = K[N + i];
                    const double k0 = p0 * i00 + p1 * i10, k1 = p0 * i01 + p1 * i11;
                    K[i] = k0;
                    K[N + i] = k1;
                    x[i] = x[i] + (k0 * c.y0 + k1 * c.y1);
                }
                __syncthreads();
                for (int i = lane; i < Nc * Nc; i += kWave) {            // P = (I - K H) P (:48)
                    const int r = i / Nc, cc = i % Nc;
                    P[r * N + cc] = P[r * N + cc] - (K[r] * HP[cc] + K[N + r] * HP[N + cc]);
                }
                __syncthreads();
            }
            if (status != SLAM_NODE_OK) {                                // the step did not happen
                __syncthreads();
                nlm = num_lm;
                for (int i = lane; i < Nc0 * Nc0; i += kWave) P[(i / Nc0) * N + i % Nc0] = Pb[(i / Nc0) * N + i % Nc0];
                for (int i = lane; i < Nc0; i += kWave) x[i] = xb[i];
                __syncthreads();
                break;
            }
            if (!early) {
                const double yaw = pi_2_pi(x[2]);                        // :49
                __syncthreads();
                if (lane == 0) x[2] = yaw;
                __syncthreads();
            }
            if (lane == 0) a.nlm_hist[step] = nlm;
            if (lane < 3) {
                if (a.x_hist) a.x_hist[3 * step + lane] = x[lane];
                if (a.cast_poses) a.cast_poses[3 * step + lane] = x[lane];
            }
        }
        for (int k = s; k < a.steps_max; ++k) {                          // steps that did not happen
            const long step = b * a.steps_max + k;
            if (lane == 0) a.nlm_hist[step] = -1;
            if (lane < 3) {
                if (a.x_hist) a.x_hist[3 * step + lane] = NAN;
                // a scan cast from an infinite pose has no finite beam: Mapping.update skips every one (mapping.py:30)
                if (a.cast_poses) a.cast_poses[3 * step + lane] = lane == 0 ? INFINITY : 0.0;
            }
        }
        const int Nc = 3 + 2 * nlm;
        for (int i = lane; i < N; i += kWave) a.x_out[b * N + i] = i < Nc ? x[i] : 0.0;
        for (int i = lane; i < N * N; i += kWave) a.P_out[b * N * N + i] = (i / N < Nc && i % N < Nc) ? P[i] : 0.0;
        if (lane == 0) {
            a.status_out[b] = status;
            if (a.nlm_out) a.nlm_out[b] = nlm;
        }
        __syncthreads();
    }
    lds_guard_check(guard, a.status);
}

size_t ekf_lds_bytes(int max_lm)
{
    const size_t N = 3 + 2 * (size_t)max_lm;
    return (2 * (N + N * N) + 4 * N + (size_t)max_lm + 1) * 8;
}

hipError_t launch_ekf_lm(const EkfArgs &a, hipStream_t s)
{
    const int lds = (int)ekf_lds_bytes(a.max_lm) + kLdsGuard;
    hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(&k_ekf_lm), lds);
    if (e != hipSuccess) return e;
    const long groups = a.B < kLandmarkMaxGroups ? a.B : kLandmarkMaxGroups;
    SLAM_LAUNCH(k_ekf_lm, dim3((unsigned)groups), dim3(kWave), lds, s, a);
    return hipGetLastError();
}

// ---- the node's kept scans -----------------------------------------------------------------
// slam_ekf.py:74-82: the first scan is the first target whatever it shows; after it a scan without a landmark
// is dropped before the odometry, so the target does not move.  One wave per trajectory.
__global__ void __launch_bounds__(64) k_node_keep(const int32_t *__restrict__ lm_count, int L, int n_scan,
                                                  int32_t *__restrict__ kept, int32_t *__restrict__ kept_count)
{
    const int lane = threadIdx.x;
    for (long l = blockIdx.x; l < L; l += gridDim.x) {
        int base = 0;
        for (int c0 = 0; c0 < n_scan; c0 += kWave) {
            const int k = c0 + lane;
            const bool keep = k < n_scan && (k == 0 || lm_count[l * n_scan + k] >= 1);
            const unsigned long long mask = __ballot(keep);
            if (keep) kept[l * n_scan + base + __popcll(mask & ((1ull << lane) - 1ull))] = k;
            base += __popcll(mask);
        }
        for (int j = base + lane; j < n_scan; j += kWave) kept[l * n_scan + j] = -1;
        if (lane == 0) kept_count[l] = base;
    }
}

// The kept scans of every trajectory moved to the front of its block, so that the scan matcher and the ray
// cast address (previous kept, current kept) as (k, k + 1) like any replay.  The places behind them repeat the
// last kept scan: a pair of equal scans is matched at once, and k_ekf_lm leaves their poses infinite.
__global__ void __launch_bounds__(256) k_node_gather(const float *__restrict__ ranges, const int32_t *__restrict__ kept,
                                                     const int32_t *__restrict__ kept_count, int n_scan, int n,
                                                     float *__restrict__ out)
{
    const long l = blockIdx.y;
    for (int j = blockIdx.x; j < n_scan; j += gridDim.x) {
        const int cnt = kept_count[l];
        const int k = kept[l * n_scan + (j < cnt ? j : cnt - 1)];
        const float *src = ranges + (l * n_scan + k) * n;
        float *dst = out + (l * n_scan + j) * n;
        for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
    }
}

hipError_t launch_node_keep(const int32_t *lm_count, int L, int n_scan, int32_t *kept, int32_t *kept_count, hipStream_t s)
{
    const long groups = L < kLandmarkMaxGroups ? L : kLandmarkMaxGroups;
    SLAM_LAUNCH(k_node_keep, dim3((unsigned)groups), dim3(kWave), 0, s, lm_count, L, n_scan, kept, kept_count);
    return hipGetLastError();
}

hipError_t launch_node_gather(const float *ranges, const int32_t *kept, const int32_t *kept_count, int L, int n_scan, int n,
                              float *out, hipStream_t s)
{
    if (L > 65535) return hipErrorInvalidValue;
    SLAM_LAUNCH(k_node_gather, dim3((unsigned)(n_scan < 4096 ? n_scan : 4096), (unsigned)L), dim3(n <= 64 ? 64 : n <= 128 ? 128 : 256),
                0, s, ranges, kept, kept_count, n_scan, n, out);
    return hipGetLastError();
}

}  // namespace slam
