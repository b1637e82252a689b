// Where a scan fits a map best, for gfx950 (MI355X): the distance field of the occupancy grid and a correlative
// window matcher on it.  The reference has no counterpart: it only writes its map.
//
//   slam_grid_distance_field   field[g][x][y] = min(cap, min over cells (u, v) with pmap == 100 of (x-u)^2 + (y-v)^2),
//                              int16, exact for every 1 <= cap <= 32767; cap everywhere on a map with no occupied cell
//   slam_grid_match            every pose of a window (K rotations x (2 nx + 1) x (2 ny + 1) translations) around a
//                              centre: one field lookup per used beam, int32 costs, the smallest wins, ties to the
//                              lowest flat index
//
// "Occupied" is what the ray cast reads: OccRule on the live integer counters, packed by launch_raycast_pack into
// mask[g][lx][ly / 32].  Like that mask the field is REBUILT on the context's stream at the start of every call
// that needs it, for all G maps, into arena scratch; nothing is cached between calls.
//
// The field is a separable transform.  With R = ceil(sqrt(cap)), a cell further than R - 1 rows or columns from every
// occupied cell is at cap, so both passes are bounded by R <= 182:
//   k_field_rows   per cell the distance ALONG ITS ROW to the nearest set bit, by bit scans on the mask words,
//                  min'ed with R (one byte per cell)
//   k_field_cols   per cell min over rows x - d .. x + d of d^2 + rowd^2, walking outwards until d^2 reaches the best
// Integer throughout, so exact.
//
// The matcher forms a beam's end as the ray cast does (one_ray of raycast_kernels.hip):
//   x = c*lx + (-s)*ly + px*1.0,  y = s*lx + c*ly + py*1.0,  both through to_cell.
// c*lx + (-s)*ly does not depend on the translation: a workgroup takes one hypothesis and a run of its rotations,
// puts that sum for every USED beam of every rotation of the run into LDS (used beams packed to the front: the cost
// is an integer sum, its order is free), and then its lanes run over the candidates (rotation, i, j) with j fastest -
// neighbouring lanes read neighbouring int16 of one field row when step = 1 / scale - each lane looping over the
// beams.  Adding px afterwards is the same left-to-right sum (the library is built with -ffp-contract=off).
// The argmin is a minimum of (cost << 32 | flat index) keys: per lane, per wave by shuffles, per workgroup through
// LDS, per hypothesis by one 64-bit atomic minimum per workgroup; k_match_finish unpacks the keys.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "slam_internal.h"
#include "grid_walk.h"

namespace slam {

// Distance along the row to the nearest set bit, min'ed with R.  Block x = (map, row), lanes stride along the row
// as in k_raycast_pack.  A neighbouring word is looked at only while its nearest bit would be closer than R.
__global__ void __launch_bounds__(256) k_field_rows(const uint32_t *__restrict__ mask, long rows, int yw, int wpr, int R,
                                                    uint8_t *__restrict__ rowd)
{
    for (long row = blockIdx.x; row < rows; row += gridDim.x) {
        const uint32_t *m = mask + (size_t)row * wpr;
        for (int ly = threadIdx.x; ly < yw; ly += blockDim.x) {
            const int w = ly >> 5, bit = ly & 31;
            const uint32_t own = m[w];
            int d = R;
            uint32_t lo = own & (0xffffffffu >> (31 - bit));             // bits at or below ly
            int ww = w;
            while (!lo && ww > 0 && ly - (ww * 32 - 1) < R) lo = m[--ww];
            if (lo) d = std::min(d, ly - (ww * 32 + 31 - __clz((int)lo)));
            uint32_t hi = own & (0xffffffffu << bit);                    // bits at or above ly
            ww = w;
            while (!hi && ww + 1 < wpr && (ww + 1) * 32 - ly < R) hi = m[++ww];
            if (hi) d = std::min(d, ww * 32 + __ffs((int)hi) - 1 - ly);
            rowd[(size_t)row * yw + ly] = (uint8_t)d;
        }
    }
}

// The lower envelope across rows, bounded: rows further than d with d^2 >= the best so far cannot improve it.
__global__ void __launch_bounds__(256) k_field_cols(const uint8_t *__restrict__ rowd, long rows, int xw, int yw, int R, int cap,
                                                    int16_t *__restrict__ field)
{
    for (long row = blockIdx.x; row < rows; row += gridDim.x) {
        const int lx = (int)(row % xw);
        const uint8_t *map = rowd + (size_t)(row - lx) * yw;
        for (int ly = threadIdx.x; ly < yw; ly += blockDim.x) {
            int best = cap;
            for (int d = 0; d < R && d * d < best; ++d) {
                if (lx - d >= 0) {
                    const int v = map[(size_t)(lx - d) * yw + ly];
                    best = std::min(best, d * d + v * v);
                }
                if (d && lx + d < xw) {
                    const int v = map[(size_t)(lx + d) * yw + ly];
                    best = std::min(best, d * d + v * v);
                }
            }
            field[(size_t)row * yw + ly] = (int16_t)best;
        }
    }
}

constexpr unsigned long long kNoKey = ~0ull;           // no candidate yet / a hypothesis that has none

__device__ __forceinline__ unsigned long long key_min_wave(unsigned long long key)
{
#pragma unroll
    for (int off = kWave / 2; off; off >>= 1) {
        const unsigned hi = __shfl_xor((unsigned)(key >> 32), off, kWave), lo = __shfl_xor((unsigned)key, off, kWave);
        const unsigned long long other = ((unsigned long long)hi << 32) | lo;
        key = other < key ? other : key;
    }
    return key;
}

// Group = (hypothesis b, rotations [k0, k0 + kc) of it), taken grid-stride.  Dynamic LDS: rx[kc][n], ry[kc][n].
__global__ void __launch_bounds__(256) k_match(MatchArgs a)
{
    extern __shared__ double lds_beams[];
    __shared__ int s_used;
    __shared__ unsigned long long s_key[256 / kWave];
    const GridDev &g = a.g;
    const int n = a.n, wy = 2 * a.ny + 1, W = (2 * a.nx + 1) * wy;
    double *rx = lds_beams, *ry = lds_beams + (size_t)a.kc * n;
    char *guard = reinterpret_cast<char *>(lds_beams + 2 * (size_t)a.kc * n);
    lds_guard_fill(guard);
    const long groups = (long)a.B * a.chunks;
    for (long grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int b = (int)(grp / a.chunks), k0 = (int)(grp % a.chunks) * a.kc, kn = std::min(a.kc, a.K - k0);
        const int gi = a.maps ? a.maps[b] : 0;
        const double cx = a.centres[2 * (size_t)b], cy = a.centres[2 * (size_t)b + 1];
        int bad = (unsigned)gi >= (unsigned)g.G || !isfinite(cx) || !isfinite(cy);
        (void)to_cell(cx, g.scale, g.off_x, bad);
        (void)to_cell(cy, g.scale, g.off_y, bad);
        const int cands = kn * W;
        int32_t *costs = a.cost_out ? a.cost_out + ((size_t)b * a.K + k0) * W : nullptr;
        if (bad) {                                                    // (block-uniform) the key of b stays kNoKey
            if (costs)
                for (int c = threadIdx.x; c < cands; c += blockDim.x) costs[c] = -1;
            if (k0 == 0 && threadIdx.x == 0 && a.used_out) a.used_out[b] = 0;
            continue;
        }
        __syncthreads();                                              // every lane is done with the beams staged before
        if (threadIdx.x == 0) s_used = 0;
        __syncthreads();
        const float *ranges = a.ranges + (size_t)b * a.range_stride;
        const double *rot = a.rot_cs + 2 * ((size_t)b * a.K + k0);
        for (int t = threadIdx.x; t < n; t += blockDim.x) {
            const float rf = ranges[t];
            const double rr = (double)rf;
            if (isfinite(rr) && rf < a.max_range) {
                const int pos = atomicAdd(&s_used, 1);
                const double lx = a.cos_t[t] * rr, ly = a.sin_t[t] * rr;
                for (int kk = 0; kk < kn; ++kk) {
                    const double c = rot[2 * kk], s = rot[2 * kk + 1];
                    rx[(size_t)kk * n + pos] = c * lx + (-s) * ly;
                    ry[(size_t)kk * n + pos] = s * lx + c * ly;
                }
            }
        }
        __syncthreads();
        const int m = s_used;
        const int16_t *field = a.field + (size_t)gi * g.xw * g.yw;
        unsigned long long best = kNoKey;
        for (int c = threadIdx.x; c < cands; c += blockDim.x) {
            const int kk = c / W, rem = c - kk * W, i = rem / wy, j = rem - i * wy;
            const double px = cx + (double)(i - a.nx) * a.step, py = cy + (double)(j - a.ny) * a.step;
            const double *qx = rx + (size_t)kk * n, *qy = ry + (size_t)kk * n;
            int cost = 0;
            for (int t = 0; t < m; ++t) {
                const double x = qx[t] + px * 1.0, y = qy[t] + py * 1.0;
                int off = 0;
                const int ex = to_cell(x, g.scale, g.off_x, off), ey = to_cell(y, g.scale, g.off_y, off);
                const bool in = !off && (unsigned)ex < (unsigned)g.xw && (unsigned)ey < (unsigned)g.yw;
                cost += in ? (int)field[(size_t)ex * g.yw + ey] : a.cap;
            }
            if (costs) costs[c] = cost;
            const unsigned long long key = ((unsigned long long)(unsigned)cost << 32) | (unsigned)(k0 * W + c);
            best = key < best ? key : best;
        }
        best = key_min_wave(best);
        if ((threadIdx.x & (kWave - 1)) == 0) s_key[threadIdx.x / kWave] = best;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < (int)(blockDim.x / kWave); ++w) best = s_key[w] < best ? s_key[w] : best;
            atomicMin(&a.keys[b], best);
            if (k0 == 0 && a.used_out) a.used_out[b] = m;
        }
    }
    lds_guard_check(guard, g.status);
}

__global__ void __launch_bounds__(256) k_match_finish(const unsigned long long *__restrict__ keys, int B,
                                                      int32_t *__restrict__ best_out, int32_t *__restrict__ best_cost_out)
{
    for (long b = (long)blockIdx.x * blockDim.x + threadIdx.x; b < B; b += (long)gridDim.x * blockDim.x) {
        const unsigned long long key = keys[b];
        best_out[b] = key == kNoKey ? -1 : (int32_t)(unsigned)key;
        best_cost_out[b] = key == kNoKey ? -1 : (int32_t)(key >> 32);
    }
}

constexpr long kMatchMaxBlocks = 1L << 20;             // workgroups per launch; more groups are taken grid-stride
constexpr int kMatchLdsBytes = 32 * 1024;              // staged beams of one workgroup, unless one rotation alone needs more

size_t field_rowd_bytes(const GridDev &g) { return (size_t)g.G * g.xw * g.yw; }

int field_radius(int cap)
{
    int R = 1;
    while (R * R < cap) ++R;
    return R;
}

hipError_t launch_distance_field(const GridDev &g, const uint32_t *mask, int cap, uint8_t *rowd, int16_t *field, hipStream_t s)
{
    const long rows = (long)g.G * g.xw;
    const int R = field_radius(cap);
    const dim3 grid((unsigned)std::min(rows, kMatchMaxBlocks));
    SLAM_LAUNCH(k_field_rows, grid, dim3(256), 0, s, mask, rows, g.yw, (g.yw + 31) / 32, R, rowd);
    SLAM_LAUNCH(k_field_cols, grid, dim3(256), 0, s, rowd, rows, g.xw, g.yw, R, cap, field);
    return hipGetLastError();
}

// Launch shape: as many lanes as one hypothesis has candidates, up to 256; as many rotations per workgroup as fill
// those lanes and fit kMatchLdsBytes of beams (one at least).
hipError_t launch_match(MatchArgs a, hipStream_t s)
{
    const long W = (long)(2 * a.nx + 1) * (2 * a.ny + 1), all = W * a.K;
    const int threads = (int)std::min(256L, (all + kWave - 1) / kWave * kWave);
    long kc = std::max(1L, std::min((long)a.K, threads / W));
    kc = std::max(1L, std::min(kc, (long)kMatchLdsBytes / (16L * a.n)));
    a.kc = (int)kc;
    a.chunks = (int)((a.K + kc - 1) / kc);
    const int lds = (int)(16 * kc * a.n) + kLdsGuard;
    hipError_t e = allow_dynamic_lds((const void *)k_match, lds);
    if (e != hipSuccess) return e;
    const long groups = (long)a.B * a.chunks;
    SLAM_LAUNCH(k_match, dim3((unsigned)std::min(groups, kMatchMaxBlocks)), dim3(threads), lds, s, a);
    SLAM_LAUNCH(k_match_finish, dim3((unsigned)std::min(((long)a.B + 255) / 256, kMatchMaxBlocks)), dim3(256), 0, s, a.keys, a.B,
                a.best_out, a.best_cost_out);
    return hipGetLastError();
}

}  // namespace slam
