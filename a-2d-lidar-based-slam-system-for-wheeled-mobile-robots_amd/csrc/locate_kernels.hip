// Where in a map a scan was taken, for gfx950 (MI355X): an exact branch and bound over a min-pooled pyramid of the
// distance field (include/slam_hip.h, slam_grid_locate).  The reference has no counterpart.
//
// The scan is discretised once per rotation into cell offsets (ax, ay); candidate (k, i, j) costs the sum of
// E(i + ax, j + ay) over the used beams, E the field inside the map and cap outside.  A whole-cell shift of the robot
// shifts every end cell alike, so with P_h[x][y] = min over 0 <= a, b < 2^h of E(x + a, y + b) the sum of
// P_h[x0 + ax][y0 + ay] bounds every candidate of the 2^h x 2^h block at (x0, y0) from below, exactly.
//
//   k_locate_pyramid   level h from level h - 1: the min of four cells at offsets 0 and 2^(h-1); block = a row of one
//                      map, lanes along y (rows are read coalesced); stored from -(2^h - 1) in both axes
//   k_locate_dense     the level-H nodes of every (hypothesis, rotation) pair: offsets of the used beams packed into
//                      LDS (the cost is an integer sum, its order is free), lanes over the nodes of a tile.  <false>:
//                      the minimum of (LB << 32 | node index) per hypothesis.  <true> (per chunk of pairs):
//                      nodes with LB <= U are appended to the level-H list, one atomic per wave, and the pair's
//                      packed offsets are copied to the chunk's table
//   k_locate_descend   a workgroup per hypothesis walks from the best level-H node to a leaf, a wave per child, and
//                      leaves the leaf's cost U: the incumbent, fixed before the sweep and never tightened
//   k_locate_sweep     a lane per child of a listed survivor, each looping over its pair's row of the chunk's offset
//                      table (written by k_locate_dense<true>); grid-stride over a list whose length is read on the
//                      device; survivors go to the next list, at level 0 into the key minimum, one atomic per wave
//   k_locate_finish    unpacks the keys (k_match_finish's idea) and writes the statistics
// Every result is a minimum of integer keys or a count, so list order, batch, order and chunking change nothing.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>

#include "slam_internal.h"

namespace slam {

namespace {

constexpr unsigned long long kNoKey = ~0ull;           // no node yet / a hypothesis that has none

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

__device__ __forceinline__ int sum_wave(int v)
{
#pragma unroll
    for (int off = kWave / 2; off; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

// the map and the region of hypothesis b; false: it names no map or no region inside it
struct Hyp {
    int gi, i0, j0, ni, nj;
};
__device__ __forceinline__ bool hyp_of(const LocateArgs &a, int b, Hyp &h)
{
    h.gi = a.maps ? a.maps[b] : 0;
    h.i0 = h.j0 = 0;
    h.ni = a.g.xw;
    h.nj = a.g.yw;
    if (a.region) {
        const int32_t *r = a.region + 4 * (size_t)b;
        h.i0 = r[0]; h.j0 = r[1]; h.ni = r[2]; h.nj = r[3];
    }
    return (unsigned)h.gi < (unsigned)a.g.G && h.i0 >= 0 && h.j0 >= 0 && h.ni >= 1 && h.nj >= 1 && h.ni <= a.max_ni &&
           h.nj <= a.max_nj && (long)h.i0 + h.ni <= a.g.xw && (long)h.j0 + h.nj <= a.g.yw;
}

__device__ __forceinline__ int ceil_shift(int v, int h) { return (int)(((long)v + (1L << h) - 1) >> h); }

// children of node (I, J) of level h + 1 that intersect the region: those with an index below the level-h node counts
__device__ __forceinline__ int children(int I, int J, int nIc, int nJc)
{
    return (2 * I + 1 < nIc ? 2 : 1) * (2 * J + 1 < nJc ? 2 : 1);
}

// 0: the beam is not used; 1: (ax, ay) is its end cell relative to the robot's; 2: used, but off every map
__device__ __forceinline__ int beam_offset(const LocateArgs &a, const float *ranges, int t, double c, double s, int &ax, int &ay)
{
    const float rf = ranges[t];
    const double rr = (double)rf;
    if (!(isfinite(rr) && rf < a.max_range)) return 0;
    const double lx = a.cos_t[t] * rr, ly = a.sin_t[t] * rr;
    const double vx = a.g.scale * (c * lx + (-s) * ly), vy = a.g.scale * (s * lx + c * ly);
    if (!(fabs(vx) < 1048576.0) || !(fabs(vy) < 1048576.0)) return 2;      // (NaN compares false)
    ax = (int)floor(vx + 0.5);
    ay = (int)floor(vy + 0.5);
    return 1;
}

__device__ __forceinline__ int level_at(const LocateLevel &L, const int16_t *map, int x, int y, int cap)
{
    const int u = x + L.pad, v = y + L.pad;
    return ((unsigned)u < (unsigned)L.X && (unsigned)v < (unsigned)L.Y) ? (int)map[(size_t)u * L.Y + v] : cap;
}

// LB of node (I, J) of level h by one wave: lanes over the beams
__device__ __forceinline__ int node_bound_wave(const LocateArgs &a, int h, const Hyp &hy, const float *ranges, double c, double s,
                                               int I, int J)
{
    const LocateLevel L = a.lvl[h];
    const int16_t *map = L.base + (size_t)hy.gi * L.X * L.Y;
    const int x0 = hy.i0 + (I << h), y0 = hy.j0 + (J << h);
    int v = 0;
    for (int t = threadIdx.x & (kWave - 1); t < a.n; t += kWave) {
        int ax = 0, ay = 0;
        const int kind = beam_offset(a, ranges, t, c, s, ax, ay);
        if (kind == 1) v += level_at(L, map, x0 + ax, y0 + ay, a.cap);
        else if (kind == 2) v += a.cap;
    }
    return sum_wave(v);
}

}  // namespace

// Block = row x + pad of one map of level `dst`; rows = G * dst.X.
__global__ void __launch_bounds__(256) k_locate_pyramid(LocateLevel src, LocateLevel dst, long rows, int step, int cap,
                                                        int16_t *__restrict__ out)
{
    for (long row = blockIdx.x; row < rows; row += gridDim.x) {
        const int gi = (int)(row / dst.X), x = (int)(row % dst.X) - dst.pad;
        const int16_t *m = src.base + (size_t)gi * src.X * src.Y;
        for (int v = threadIdx.x; v < dst.Y; v += blockDim.x) {
            const int y = v - dst.pad;
            const int lo = std::min(level_at(src, m, x, y, cap), level_at(src, m, x, y + step, cap));
            const int hi = std::min(level_at(src, m, x + step, y, cap), level_at(src, m, x + step, y + step, cap));
            out[(size_t)row * dst.Y + v] = (int16_t)std::min(lo, hi);
        }
    }
}

// Group = (pair p0 + q, tile of level-H nodes), taken grid-stride.  Dynamic LDS: (ax, ay)[n].
template <bool append>
__global__ void __launch_bounds__(kLocateThreads) k_locate_dense(LocateArgs a, long p0, long pairs, long tile, long tiles)
{
    extern __shared__ int lds_offsets[];
    __shared__ int s_used, s_off;
    __shared__ unsigned long long s_key[kLocateThreads / kWave];
    __shared__ int s_kids[kLocateThreads / kWave];
    char *guard = reinterpret_cast<char *>(lds_offsets + 2 * (size_t)a.n);
    lds_guard_fill(guard);
    const int sh = a.H, lane = threadIdx.x & (kWave - 1);
    const LocateLevel L = a.lvl[sh];
    const long groups = pairs * tiles;
    for (long grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const long p = p0 + grp / tiles, tl = grp % tiles;
        const int b = (int)(p / a.K), k = (int)(p % a.K);
        const bool first = !append && k == 0 && tl == 0 && threadIdx.x == 0;
        Hyp hy;
        if (!hyp_of(a, b, hy)) {                                      // (block-uniform, as every `continue` below)
            if (first) a.used[b] = -1;
            continue;
        }
        if (append && a.used[b] == 0) continue;                       // no used beam: no search
        __syncthreads();                                              // every lane is done with the offsets staged before
        if (threadIdx.x == 0) s_used = s_off = 0;
        __syncthreads();
        const float *ranges = a.ranges + (size_t)b * a.range_stride;
        const double c = a.rot_cs[2 * (size_t)k], s = a.rot_cs[2 * (size_t)k + 1];
        for (int t = threadIdx.x; t < a.n; t += blockDim.x) {
            int ax = 0, ay = 0;
            const int kind = beam_offset(a, ranges, t, c, s, ax, ay);
            if (kind == 1) {
                const int pos = atomicAdd(&s_used, 1);
                lds_offsets[2 * pos] = ax;
                lds_offsets[2 * pos + 1] = ay;
            } else if (kind == 2) {
                atomicAdd(&s_off, 1);
            }
        }
        __syncthreads();
        const int m = s_used, off = s_off;
        if (first) a.used[b] = m + off;
        if (m + off == 0) continue;
        if (append && tl == 0) {                                      // the pair's row of the chunk's table, for the sweep
            const long q = grp / tiles;
            for (int t = threadIdx.x; t < 2 * m; t += blockDim.x) a.table[2 * q * a.n + t] = lds_offsets[t];
            if (threadIdx.x == 0) {
                a.table_cnt[2 * q] = m;
                a.table_cnt[2 * q + 1] = off;
            }
        }
        const int nI = ceil_shift(hy.ni, sh), nJ = ceil_shift(hy.nj, sh);
        const int nIc = sh ? ceil_shift(hy.ni, sh - 1) : 0, nJc = sh ? ceil_shift(hy.nj, sh - 1) : 0;
        const long nodes = (long)nI * nJ, c0 = tl * tile, c1 = std::min(nodes, c0 + tile);
        const int16_t *map = L.base + (size_t)hy.gi * L.X * L.Y;
        const int U = append ? a.bound[b] : 0;
        unsigned long long best = kNoKey;
        int kids = 0;
        for (long cb = c0; cb < c1; cb += blockDim.x) {               // the same trips for every lane: a ballot inside
            const long cn = cb + threadIdx.x;
            const bool live = cn < c1;
            const int I = live ? (int)(cn / nJ) : 0, J = live ? (int)(cn - (long)I * nJ) : 0;
            int lb = off * a.cap;
            if (live) {
                const int x0 = hy.i0 + (I << sh), y0 = hy.j0 + (J << sh);
                for (int t = 0; t < m; ++t) lb += level_at(L, map, x0 + lds_offsets[2 * t], y0 + lds_offsets[2 * t + 1], a.cap);
            }
            if (!append) {
                const unsigned long long key = ((unsigned long long)(unsigned)lb << 32) | (unsigned)(k * nodes + cn);
                best = live && key < best ? key : best;
                continue;
            }
            const bool keep = live && lb <= U;
            const unsigned long long mask = __ballot(keep);
            if (!mask) continue;                                      // (wave-uniform)
            const int leader = __ffsll((long long)mask) - 1;
            unsigned base = 0;
            if (lane == leader) base = atomicAdd(&a.list_len[sh], (unsigned)__popcll(mask));
            base = __shfl(base, leader, kWave);
            if (keep) {
                const long slot = (long)base + __popcll(mask & ((1ull << lane) - 1));
                if (slot < a.list_cap[sh]) {
                    a.list[sh][2 * slot] = (int32_t)p;
                    a.list[sh][2 * slot + 1] = (int32_t)cn;
                }
                kids += children(I, J, nIc, nJc);
            }
        }
        const int w = threadIdx.x / kWave;
        if (!append) {
            best = key_min_wave(best);
            if (lane == 0) s_key[w] = best;
        } else {
            kids = sum_wave(kids);
            if (lane == 0) s_kids[w] = kids;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int waves = (int)(blockDim.x / kWave);
            if (!append) {
                for (int q = 1; q < waves; ++q) best = s_key[q] < best ? s_key[q] : best;
                atomicMin(&a.key_top[b], best);
            } else {
                for (int q = 1; q < waves; ++q) kids += s_kids[q];
                if (kids) atomicAdd(&a.evaluated[(size_t)b * (a.H + 1) + sh - 1], (unsigned long long)kids);
            }
        }
    }
    lds_guard_check(guard, a.g.status);
}

// Workgroup (four waves) = hypothesis: from its best level-H node down to a leaf, a wave per child.
__global__ void __launch_bounds__(kLocateThreads) k_locate_descend(LocateArgs a)
{
    __shared__ int s_lb[4];
    const int w = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        Hyp hy;
        if (!hyp_of(a, b, hy)) continue;
        const unsigned long long key = a.key_top[b];
        if (key == kNoKey) {                                          // no used beam
            if (threadIdx.x == 0) a.bound[b] = 0;
            continue;
        }
        const long nJ = ceil_shift(hy.nj, a.H), nodes = (long)ceil_shift(hy.ni, a.H) * nJ, idx = (long)(unsigned)key;
        const int k = (int)(idx / nodes);
        int I = (int)(idx % nodes / nJ), J = (int)(idx % nodes % nJ), lb = (int)(key >> 32);
        const float *ranges = a.ranges + (size_t)b * a.range_stride;
        const double c = a.rot_cs[2 * (size_t)k], s = a.rot_cs[2 * (size_t)k + 1];
        for (int h = a.H - 1; h >= 0; --h) {
            const int cI = 2 * I + (w >> 1), cJ = 2 * J + (w & 1);
            int v = INT_MAX;                                          // (a bound is at most n * cap < INT_MAX)
            if (cI < ceil_shift(hy.ni, h) && cJ < ceil_shift(hy.nj, h)) v = node_bound_wave(a, h, hy, ranges, c, s, cI, cJ);
            __syncthreads();                                          // the round before has been read
            if (lane == 0) s_lb[w] = v;
            __syncthreads();
            int bw = 0;
            lb = s_lb[0];
            for (int q = 1; q < 4; ++q)                               // smallest (LB, I, J): q runs in (I, J) order
                if (s_lb[q] < lb) { lb = s_lb[q]; bw = q; }
            I = 2 * I + (bw >> 1);
            J = 2 * J + (bw & 1);
        }
        if (threadIdx.x == 0) a.bound[b] = lb;
    }
}

// Lane = one child (level hp - 1) of one listed survivor of level hp, grid-stride over a list whose length is read here.
// The offsets are the chunk's table (k_locate_dense<true> wrote each pair's row): neighbouring lanes are children of one
// parent or of its list neighbours, mostly of one pair, so a row is read as a broadcast.  Survivors are appended with one
// atomic per wave; counts and keys go through one atomic per wave too while the wave's survivors share a hypothesis.
__global__ void __launch_bounds__(kLocateThreads) k_locate_sweep(LocateArgs a, long p0, int hp)
{
    const int h = hp - 1, lane = threadIdx.x & (kWave - 1);
    const LocateLevel L = a.lvl[h];
    const long listed = std::min((long)a.list_len[hp], a.list_cap[hp]), items = 4 * listed;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long base = (long)blockIdx.x * blockDim.x + threadIdx.x - lane; base < items; base += stride) {   // (wave-uniform)
        const long it = base + lane;
        bool live = it < items;
        long p = 0;
        int b = 0, k = 0, I = 0, J = 0, nJc = 0, lb = 0;
        Hyp hy = {0, 0, 0, 1, 1};
        if (live) {
            const int32_t *e = a.list[hp] + 2 * (it >> 2);
            p = e[0];
            const int cn = e[1];
            b = (int)(p / a.K);
            k = (int)(p % a.K);
            (void)hyp_of(a, b, hy);                                   // (a listed node's hypothesis is a good one)
            const int nJp = ceil_shift(hy.nj, hp);
            nJc = ceil_shift(hy.nj, h);
            I = 2 * (cn / nJp) + (int)((it >> 1) & 1);
            J = 2 * (cn % nJp) + (int)(it & 1);
            live = I < ceil_shift(hy.ni, h) && J < nJc;               // else: outside the region
        }
        if (live) {
            const long q = p - p0;
            const int m = a.table_cnt[2 * q];
            const int32_t *o = a.table + 2 * q * a.n;
            const int16_t *map = L.base + (size_t)hy.gi * L.X * L.Y;
            const int x0 = hy.i0 + (I << h), y0 = hy.j0 + (J << h);
            lb = a.table_cnt[2 * q + 1] * a.cap;
            for (int t = 0; t < m; ++t) lb += level_at(L, map, x0 + o[2 * t], y0 + o[2 * t + 1], a.cap);
        }
        const bool keep = live && lb <= a.bound[b];
        const unsigned long long mask = __ballot(keep);
        if (!mask) continue;                                          // (wave-uniform)
        const int leader = __ffsll((long long)mask) - 1;
        const int b0 = __shfl(b, leader, kWave);
        const bool one = __ballot(keep && b != b0) == 0;              // every survivor of the wave is of hypothesis b0
        if (h > 0) {
            unsigned at = 0;
            if (lane == leader) at = atomicAdd(&a.list_len[h], (unsigned)__popcll(mask));
            at = __shfl(at, leader, kWave);
            int kids = 0;
            if (keep) {
                const long slot = (long)at + __popcll(mask & ((1ull << lane) - 1));
                if (slot < a.list_cap[h]) {
                    a.list[h][2 * slot] = (int32_t)p;
                    a.list[h][2 * slot + 1] = I * nJc + J;
                }
                kids = children(I, J, ceil_shift(hy.ni, h - 1), ceil_shift(hy.nj, h - 1));
            }
            unsigned long long *cnt = a.evaluated + (size_t)(one ? b0 : b) * (a.H + 1) + h - 1;
            if (one) {
                kids = sum_wave(kids);
                if (lane == leader) atomicAdd(cnt, (unsigned long long)kids);
            } else if (keep) {
                atomicAdd(cnt, (unsigned long long)kids);
            }
        } else {
            const long flat = ((long)k * hy.ni + I) * hy.nj + J;
            unsigned long long key = keep ? ((unsigned long long)(unsigned)lb << 32) | (unsigned)flat : kNoKey;
            if (one) {
                key = key_min_wave(key);
                if (lane == leader) atomicMin(&a.key_leaf[b0], key);
            } else if (keep) {
                atomicMin(&a.key_leaf[b], key);
            }
        }
    }
}

__global__ void __launch_bounds__(256) k_locate_finish(LocateArgs a)
{
    for (long b = (long)blockIdx.x * blockDim.x + threadIdx.x; b < a.B; b += (long)gridDim.x * blockDim.x) {
        Hyp hy;
        const bool ok = hyp_of(a, (int)b, hy);
        const int used = ok ? a.used[b] : 0;
        int32_t *best = a.best_out + 3 * (size_t)b;
        int64_t *st = a.stats_out ? a.stats_out + (size_t)b * (a.H + 2) : nullptr;
        if (a.used_out) a.used_out[b] = used;
        if (!ok || used == 0) {
            best[0] = ok ? 0 : -1;
            best[1] = ok ? hy.i0 : -1;
            best[2] = ok ? hy.j0 : -1;
            a.best_cost_out[b] = ok ? 0 : -1;
            if (st)
                for (int h = 0; h < a.H + 2; ++h) st[h] = 0;
            continue;
        }
        const unsigned long long key = a.H ? a.key_leaf[b] : a.key_top[b];
        const long flat = (long)(unsigned)key, cells = (long)hy.ni * hy.nj;
        best[0] = (int32_t)(flat / cells);
        best[1] = hy.i0 + (int32_t)(flat % cells / hy.nj);
        best[2] = hy.j0 + (int32_t)(flat % cells % hy.nj);
        a.best_cost_out[b] = (int32_t)(key >> 32);
        if (st) {
            for (int h = 0; h < a.H; ++h) st[h] = (int64_t)a.evaluated[(size_t)b * (a.H + 1) + h];
            st[a.H] = (int64_t)a.K * ceil_shift(hy.ni, a.H) * ceil_shift(hy.nj, a.H);
            st[a.H + 1] = a.H ? a.bound[b] : (int32_t)(key >> 32);
        }
    }
}

size_t locate_pyramid_cells(const GridDev &g, int H)
{
    size_t cells = 0;
    for (int h = 1; h <= H; ++h) cells += (size_t)g.G * (g.xw + (1 << h) - 1) * (g.yw + (1 << h) - 1);
    return cells;
}

hipError_t launch_locate_pyramid(LocateArgs &a, const int16_t *field, int16_t *pyr, hipStream_t s)
{
    const GridDev &g = a.g;
    a.lvl[0].base = field; a.lvl[0].pad = 0; a.lvl[0].X = g.xw; a.lvl[0].Y = g.yw;
    for (int h = 1; h <= a.H; ++h) {
        LocateLevel &d = a.lvl[h];
        d.base = pyr; d.pad = (1 << h) - 1; d.X = g.xw + d.pad; d.Y = g.yw + d.pad;
        const long rows = (long)g.G * d.X;
        SLAM_LAUNCH(k_locate_pyramid, dim3((unsigned)std::min(rows, kLocateMaxBlocks)), dim3(256), 0, s, a.lvl[h - 1], d, rows,
                    1 << (h - 1), a.cap, pyr);
        pyr += (size_t)rows * d.Y;
    }
    return hipGetLastError();
}

hipError_t launch_locate(const LocateArgs &a, const LocateShape &p, hipStream_t s)
{
    hipError_t e = allow_dynamic_lds((const void *)k_locate_dense<false>, p.dense_lds);
    if (e == hipSuccess) e = allow_dynamic_lds((const void *)k_locate_dense<true>, p.dense_lds);
    if (e != hipSuccess) return e;
    const long pairs = (long)a.B * a.K;
    const dim3 threads(p.dense_threads);
    SLAM_LAUNCH(k_locate_dense<false>, dim3((unsigned)std::min(pairs * p.tiles, kLocateMaxBlocks)), threads, p.dense_lds, s, a, 0L,
                pairs, p.tile, p.tiles);
    if (a.H > 0) {
        SLAM_LAUNCH(k_locate_descend, dim3((unsigned)std::min((long)a.B, kLocateMaxBlocks)), dim3(kLocateThreads), 0, s, a);
        for (long p0 = 0; p0 < pairs; p0 += p.chunk_pairs) {
            const long np = std::min(p.chunk_pairs, pairs - p0);
            e = hipMemsetAsync(a.list_len, 0, sizeof(unsigned) * (kLocateMaxLevels + 1), s);
            if (e != hipSuccess) return e;
            SLAM_LAUNCH(k_locate_dense<true>, dim3((unsigned)std::min(np * p.tiles, kLocateMaxBlocks)), threads, p.dense_lds, s, a, p0,
                        np, p.tile, p.tiles);
            for (int hp = a.H; hp >= 1; --hp) {
                const long worst = 4 * np * p.level_nodes[hp];            // children a full list has
                SLAM_LAUNCH(k_locate_sweep, dim3((unsigned)std::min((worst + p.sweep_threads - 1) / p.sweep_threads, (long)kLocateSweepBlocks)),
                            dim3(p.sweep_threads), 0, s, a, p0, hp);
            }
        }
    }
    SLAM_LAUNCH(k_locate_finish, dim3((unsigned)std::min(((long)a.B + 255) / 256, kLocateMaxBlocks)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace slam
