// Map frontiers for gfx950 (MI355X): the free cells that border unexplored space, grouped into 8-connected clusters, one
// reachable cell per cluster (include/slam_hip.h, slam_grid_frontiers).  The reference has no
// counterpart.  Integer end to end: every output is a count, a sum, a minimum or a maximum, so no order of arrival shows.
//
//   k_frontier_tile     a workgroup per (query, tile of 32 x 64 cells): the cell classes of the tile and a halo from the
//                       counters (OccRule, what k_grid_finalize would write) into LDS, the window's unknown count as row
//                       sums then column sums, the frontier bits (counted per segment of 1 024 cells of the query, one
//                       atomic per row of the tile), a union-find over the tile's frontier cells in LDS (atomicMin on the
//                       larger root), and one int32 label per cell: the flat index of the tile's root
//   k_frontier_border   a lane per cell of a tile's first row or column: unions with the frontier cells across the
//                       border, lock-free through global memory - find both roots, atomicMin on the larger, go on from
//                       the value returned when the root has moved.  Labels only decrease; every loop is bounded by the
//                       number of cells anyway.  Labels of other workgroups are read with agent-scope atomic loads only.
// then a workgroup per (query, segment), each pass leaving a segment without a frontier cell alone:
//   k_frontier_flatten  every frontier cell takes its root; a root takes -(1 + 1), its size of one
//   k_frontier_sizes    every other frontier cell adds one to its root's size, one atomic per (wave, root)
//   k_frontier_segs     kept roots (size >= min_size) per segment
//   k_frontier_rank     the ordered table: a kept root's row is the number of kept roots before it - the segments before
//                       its own summed, the segment scanned - so the rows are in ascending label order whatever ran
//                       first; writes the counts, starts the rows and leaves the row number in the root's label word
//   k_frontier_stats    sums and boxes of the clusters that have a row, one atomic per (wave, cluster); labels_out
//   k_frontier_rep      the member nearest to the rounded centroid: the minimum of (d2 << 32 | flat), kept in the row's
//                       two representative words
//   k_frontier_finish   unpacks that key into (rep_x, rep_y)
// Cross-workgroup steps are separate launches, or the lock-free unions above: nothing waits for another workgroup.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>

#include "slam_internal.h"
#include "grid_walk.h"

namespace slam {

namespace {

constexpr int kTX = kFrontierTileX, kTY = kFrontierTileY, kTileCells = kTX * kTY;
constexpr int kCellsPerLane = kTileCells / kFrontierThreads;
static_assert(kTY == kWave && kTileCells % kFrontierThreads == 0, "a wave takes a row of the tile");
static_assert(kFrontierSeg == 4 * kFrontierThreads, "k_frontier_segs and k_frontier_rank take four rounds per segment");

enum : unsigned char { kFree = 0, kUnknown = 1, kOccupied = 2, kOutside = 3 };

__device__ __forceinline__ int ld_agent(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int ld_group(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// ---- union-find on the tile's labels in LDS: L[i] <= i, a root has L[i] == i -----------------------------------------
__device__ __forceinline__ int tile_find(const int *L, int i)
{
    for (int t = 0; t < kTileCells; ++t) {
        const int v = ld_group(L + i);
        if (v == i) break;
        i = v;
    }
    return i;
}
__device__ __forceinline__ void tile_union(int *L, int a, int b)
{
    for (int t = 0; t < kTileCells; ++t) {
        a = tile_find(L, a);
        b = tile_find(L, b);
        if (a == b) return;
        if (a < b) { const int s = a; a = b; b = s; }
        const int old = atomicMin(L + a, b);
        if (old == a) return;
        a = old;            // a was no root any more: what it pointed to still has to meet b
    }
}

// ---- the same on a query's labels in global memory; from k_frontier_flatten on a root is negative --------------------
__device__ __forceinline__ int cell_find(const int32_t *L, int i, int cells)
{
    for (int t = 0; t < cells; ++t) {
        const int v = ld_agent(L + i);
        if (v < 0 || v == i) break;
        i = v;
    }
    return i;
}
__device__ __forceinline__ void cell_union(int32_t *L, int a, int b, int cells)
{
    for (int t = 0; t < cells; ++t) {
        a = cell_find(L, a, cells);
        b = cell_find(L, b, cells);
        if (a == b) return;
        if (a < b) { const int s = a; a = b; b = s; }
        const int old = atomicMin(L + a, b);
        if (old == a) return;
        a = old;
    }
}

__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int off = kWave / 2; off; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}
__device__ __forceinline__ int wave_min(int v)
{
#pragma unroll
    for (int off = kWave / 2; off; off >>= 1) v = std::min(v, __shfl_xor(v, off, kWave));
    return v;
}
__device__ __forceinline__ int wave_max(int v)
{
#pragma unroll
    for (int off = kWave / 2; off; off >>= 1) v = std::max(v, __shfl_xor(v, off, kWave));
    return v;
}
__device__ __forceinline__ unsigned long long wave_min_key(unsigned long long key)
{
#pragma unroll
    for (int off = kWave / 2; off; off >>= 1) {
        const unsigned hi = __shfl_xor((unsigned)(key >> 32), off, kWave), lo = __shfl_xor((unsigned)key, off, kWave);
        const unsigned long long other = ((unsigned long long)hi << 32) | lo;
        key = other < key ? other : key;
    }
    return key;
}

// the map of query b, -1: it names none
__device__ __forceinline__ int map_of(const FrontierArgs &a, long b)
{
    const int gi = a.maps ? a.maps[b] : (int)b;
    return (unsigned)gi < (unsigned)a.g.G ? gi : -1;
}

// sum over the workgroup's kFrontierThreads lanes, the same in every lane; s_part: one int per wave
__device__ __forceinline__ int block_sum(int v, int *s_part)
{
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & (kWave - 1)) == 0) s_part[threadIdx.x / kWave] = v;
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int w = 0; w < kFrontierThreads / kWave; ++w) total += s_part[w];
    return total;
}

}  // namespace

// Group = (query b0 + q, tile), taken grid-stride.  Dynamic LDS: frontier_lds_bytes(radius).  Adds the tile's frontier
// cells to seg[q][s][1] (zero on entry), s the segment of kFrontierSeg cells they lie in.
__global__ void __launch_bounds__(kFrontierThreads) k_frontier_tile(FrontierArgs a, int tiles_x, int tiles_y, long segs, long b0, long groups)
{
    extern __shared__ int lds_frontier[];
    const int h = frontier_halo(a.radius), W = kTY + 2 * h, HX = kTX + 2 * h, r = a.radius;
    int *L = lds_frontier;
    unsigned char *code = reinterpret_cast<unsigned char *>(L + kTileCells);
    unsigned char *rows = code + HX * W;
    char *guard = reinterpret_cast<char *>(lds_frontier) + (frontier_lds_bytes(a.radius, 0));
    lds_guard_fill(guard);
    const OccRule rule = OccRule::of(a.g);
    const int xw = a.g.xw, yw = a.g.yw, tid = threadIdx.x;
    const size_t cells = (size_t)xw * yw;
    const long tiles = (long)tiles_x * tiles_y;
    for (long grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const long q = grp / tiles;
        const int t = (int)(grp % tiles), x0 = (t / tiles_y) * kTX, y0 = (t % tiles_y) * kTY;
        const int gi = map_of(a, b0 + q);
        const uint32_t *pass = a.g.pass + (size_t)(gi < 0 ? 0 : gi) * cells, *hit = a.g.hit + (size_t)(gi < 0 ? 0 : gi) * cells;
#pragma unroll 2
        for (int i = tid; i < HX * W; i += kFrontierThreads) {
            const int x = x0 + i / W - h, y = y0 + i % W - h;
            unsigned char c = kOutside;
            if (gi >= 0 && (unsigned)x < (unsigned)xw && (unsigned)y < (unsigned)yw) {
                const size_t at = (size_t)x * yw + y;
                const uint32_t v = rule.value(pass[at], hit[at]);
                c = v == 0u ? kFree : v == 50u ? kUnknown : kOccupied;
            }
            code[i] = c;
        }
        __syncthreads();
        if (a.min_unknown > 0) {
            for (int i = tid; i < HX * kTY; i += kFrontierThreads) {
                const unsigned char *row = code + (i / kTY) * W + (i % kTY) + h;
                int n = 0;
                for (int d = -r; d <= r; ++d) n += row[d] == kUnknown;
                rows[i] = (unsigned char)n;
            }
            __syncthreads();
        }
        int32_t *out = a.lab + (size_t)q * cells;
        int32_t *seg = a.seg + q * segs * 2;
        int any = 0;
#pragma unroll 1
        for (int k = 0; k < kCellsPerLane; ++k) {
            const int lx = tid / kTY + k * (kFrontierThreads / kTY), ly = tid % kTY, x = x0 + lx, y = y0 + ly;
            const unsigned char *c = code + (lx + h) * W + ly + h;
            bool f = x < xw && y < yw && c[0] == kFree && (c[-1] == kUnknown || c[1] == kUnknown || c[-W] == kUnknown || c[W] == kUnknown);
            if (f && a.min_unknown > 0) {
                int n = 0;
                for (int d = -r; d <= r; ++d) n += rows[(lx + h + d) * kTY + ly];
                f = n >= a.min_unknown;
            }
            if (f && a.min_clear2 > 0) f = (int)a.field[(size_t)gi * cells + (size_t)x * yw + y] >= a.min_clear2;
            L[lx * kTY + ly] = f ? lx * kTY + ly : -1;
            // the frontier cells of this row of the tile, by segment of the query's cells: a row of 64 meets two at most
            const unsigned long long bits = __ballot(f);
            any |= bits != 0;
            if (bits && ly == 0) {
                const long c0 = (long)x * yw + y0, s0 = c0 / kFrontierSeg, first = (s0 + 1) * kFrontierSeg - c0;
                const unsigned long long lo = first >= kWave ? bits : bits & ((1ull << first) - 1);
                if (lo) atomicAdd(seg + s0 * 2 + 1, (int)__popcll(lo));
                if (bits != lo) atomicAdd(seg + (s0 + 1) * 2 + 1, (int)__popcll(bits ^ lo));
            }
        }
        if (!__syncthreads_or(any)) {           // no frontier cell in this tile: its labels are -1, nothing to join
#pragma unroll 1
            for (int k = 0; k < kCellsPerLane; ++k) {
                const int x = x0 + tid / kTY + k * (kFrontierThreads / kTY), y = y0 + tid % kTY;
                if (x < xw && y < yw) out[(size_t)x * yw + y] = -1;
            }
            continue;
        }
        // the neighbours before a cell in flat order: W, NW, N, NE; the other four meet it from their side
        // (a frontier cell's word is never negative, whatever its unions have made of it)
#pragma unroll 1
        for (int k = 0; k < kCellsPerLane; ++k) {
            const int lx = tid / kTY + k * (kFrontierThreads / kTY), ly = tid % kTY, li = lx * kTY + ly;
            if (ld_group(L + li) < 0) continue;
            if (ly > 0 && ld_group(L + li - 1) >= 0) tile_union(L, li, li - 1);
            if (lx > 0) {
                if (ld_group(L + li - kTY) >= 0) tile_union(L, li, li - kTY);
                if (ly > 0 && ld_group(L + li - kTY - 1) >= 0) tile_union(L, li, li - kTY - 1);
                if (ly < kTY - 1 && ld_group(L + li - kTY + 1) >= 0) tile_union(L, li, li - kTY + 1);
            }
        }
        __syncthreads();
#pragma unroll 1
        for (int k = 0; k < kCellsPerLane; ++k) {
            const int lx = tid / kTY + k * (kFrontierThreads / kTY), ly = tid % kTY, x = x0 + lx, y = y0 + ly;
            if (x >= xw || y >= yw) continue;
            int label = -1;
            if (ld_group(L + lx * kTY + ly) >= 0) {
                const int root = tile_find(L, lx * kTY + ly);
                label = (x0 + root / kTY) * yw + y0 + root % kTY;
            }
            out[(size_t)x * yw + y] = label;
        }
        __syncthreads();
    }
    lds_guard_check(guard, a.g.status);
}

// Item = a cell of row x = k * TileX (it meets row x - 1) or of column y = k * TileY (it meets column y - 1) of one
// query: every pair of 8-neighbours in two tiles is met by one of them.  items = queries * border.
__global__ void __launch_bounds__(kFrontierThreads) k_frontier_border(FrontierArgs a, int tiles_x, long border, long items)
{
    const int xw = a.g.xw, yw = a.g.yw, cells = xw * yw;
    const long across = (long)(tiles_x - 1) * yw;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (long)gridDim.x * blockDim.x) {
        int32_t *L = a.lab + (size_t)(i / border) * cells;
        long j = i % border;
        int x, y, dx, dy;       // the three cells met: (x - 1, y + d) or (x + d, y - 1), d = -1, 0, 1
        if (j < across) { x = (int)(j / yw + 1) * kTX; y = (int)(j % yw); dx = 0; dy = 1; }
        else { j -= across; y = (int)(j / xw + 1) * kTY; x = (int)(j % xw); dx = 1; dy = 0; }
        const int c = x * yw + y;
        if (ld_agent(L + c) < 0) continue;
        for (int d = -1; d <= 1; ++d) {
            const int nx = dx ? x + d : x - 1, ny = dy ? y + d : y - 1;
            if ((unsigned)nx >= (unsigned)xw || (unsigned)ny >= (unsigned)yw) continue;
            const int n = nx * yw + ny;
            if (ld_agent(L + n) >= 0) cell_union(L, c, n, cells);
        }
    }
}

// Every pass from here on is a workgroup per (query, segment of kFrontierSeg cells), four cells a lane, and leaves a
// segment without a frontier cell alone: the explored part of a map has few.

// Every frontier cell takes its root; a root takes -2 = -(size 1 + 1).  A lane that walks through a cell rewritten here
// reads its old parent or its root, and both lead to the root.
__global__ void __launch_bounds__(kFrontierThreads) k_frontier_flatten(FrontierArgs a, int cells, long segs, long groups)
{
    for (long grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        if (a.seg[grp * 2 + 1] == 0) continue;
        int32_t *L = a.lab + (size_t)(grp / segs) * cells;
        const long c0 = grp % segs * kFrontierSeg;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long c = c0 + k * kFrontierThreads + threadIdx.x;
            if (c >= cells || ld_agent(L + c) == -1) continue;
            const int root = cell_find(L, (int)c, cells);
            __hip_atomic_store(L + c, root == c ? -2 : root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// A root's word counts its cells: -(size + 1).  One atomic per (wave, root).
__global__ void __launch_bounds__(kFrontierThreads) k_frontier_sizes(FrontierArgs a, int cells, long segs, long groups)
{
    const int lane = threadIdx.x & (kWave - 1);
    for (long grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        if (a.seg[grp * 2 + 1] == 0) continue;
        int32_t *L = a.lab + (size_t)(grp / segs) * cells;
        const long c0 = grp % segs * kFrontierSeg;
        for (int k = 0; k < 4; ++k) {
            const long c = c0 + k * kFrontierThreads + threadIdx.x;
            const int at = c < cells ? L[c] : -1;           // the root's cell: other frontier cells only
            unsigned long long todo = __ballot(at >= 0);
            while (todo) {
                const int leader = __ffsll((long long)todo) - 1;
                const int root = __shfl(at, leader, kWave);
                const unsigned long long same = __ballot(at == root);
                if (lane == leader) atomicAdd(L + root, -(int)__popcll(same));
                todo &= ~same;
            }
        }
    }
}

// seg[group][0] = the kept roots of the segment (zero on entry; [1], its frontier cells, is k_frontier_tile's).
__global__ void __launch_bounds__(kFrontierThreads) k_frontier_segs(FrontierArgs a, int cells, long segs, long groups)
{
    __shared__ int s_part[kFrontierThreads / kWave];
    for (long grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        if (a.seg[grp * 2 + 1] == 0) continue;
        int32_t *L = a.lab + (size_t)(grp / segs) * cells;
        const long c0 = grp % segs * kFrontierSeg;
        int kept = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long c = c0 + k * kFrontierThreads + threadIdx.x;
            if (c >= cells) continue;
            const int v = L[c];
            kept += v <= -2 && -(v + 1) >= a.min_size;
        }
        kept = block_sum(kept, s_part);
        if (threadIdx.x == 0) a.seg[grp * 2] = kept;
    }
}

// Group = (query, segment).  The row of a kept root is the number of kept roots with a smaller flat index.
__global__ void __launch_bounds__(kFrontierThreads) k_frontier_rank(FrontierArgs a, int cells, long segs, long b0, long groups)
{
    __shared__ int s_part[kFrontierThreads / kWave];
    __shared__ int s_wave[4][kFrontierThreads / kWave];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    for (long grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const long q = grp / segs, s = grp % segs, b = b0 + q;
        int32_t *L = a.lab + (size_t)q * cells;
        const int32_t *seg = a.seg + q * segs * 2;
        int before = 0, kept_all = 0, frontier_all = 0;
        for (long t = threadIdx.x; t < segs; t += kFrontierThreads) {
            const int n = seg[t * 2];
            kept_all += n;
            before += t < s ? n : 0;
            if (s == 0) frontier_all += seg[t * 2 + 1];
        }
        before = block_sum(before, s_part);
        if (s == 0) {
            kept_all = block_sum(kept_all, s_part);
            frontier_all = block_sum(frontier_all, s_part);
            if (threadIdx.x == 0) {
                const bool valid = map_of(a, b) >= 0;
                a.count_out[b * 2] = valid ? kept_all : -1;
                a.count_out[b * 2 + 1] = valid ? frontier_all : -1;
            }
        }
        if (seg[s * 2 + 1] == 0) continue;      // (block-uniform)
        int v[4];
        unsigned long long ahead[4];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long c = s * kFrontierSeg + k * kFrontierThreads + threadIdx.x;
            v[k] = c < cells ? L[c] : -1;
            const unsigned long long m = __ballot(v[k] <= -2 && -(v[k] + 1) >= a.min_size);
            ahead[k] = m & ((1ull << lane) - 1);
            if (lane == 0) s_wave[k][wave] = (int)__popcll(m);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long c = s * kFrontierSeg + k * kFrontierThreads + threadIdx.x;
            if (v[k] > -2) continue;
            const int size = -(v[k] + 1);
            int word = kFrontierNoRow;
            if (size >= a.min_size) {
                int row = before + (int)__popcll(ahead[k]);
                for (int kk = 0; kk < 4; ++kk)
                    for (int w = 0; w < kFrontierThreads / kWave; ++w)
                        if (kk < k || (kk == k && w < wave)) row += s_wave[kk][w];
                if (row < a.M) {
                    int32_t *out = a.clusters_out + ((size_t)b * a.M + row) * 8;
                    out[0] = (int32_t)c; out[1] = size; out[2] = -1; out[3] = -1;     // (2, 3): the key of k_frontier_rep
                    out[4] = INT_MAX; out[5] = INT_MAX; out[6] = -1; out[7] = -1;
                    a.sums_out[((size_t)b * a.M + row) * 2] = 0;
                    a.sums_out[((size_t)b * a.M + row) * 2 + 1] = 0;
                    word = -(row + 2);
                }
            }
            L[c] = word;
        }
        __syncthreads();
    }
}

// which row of its query's table a cell adds to (-1: none), and its label
__device__ __forceinline__ int row_of(const int32_t *L, int c, int &label)
{
    const int v = L[c];
    label = v == -1 ? -1 : v >= 0 ? v : c;
    if (v == -1) return -1;
    const int word = v >= 0 ? L[v] : v;
    return word == kFrontierNoRow ? -1 : -(word + 2);
}

// Sums and boxes, one atomic of each kind per (wave, cluster); the labels of the frontier cells when they are asked for
// (labels_out is -1 on entry).
__global__ void __launch_bounds__(kFrontierThreads) k_frontier_stats(FrontierArgs a, int cells, long segs, long b0, long groups)
{
    const int lane = threadIdx.x & (kWave - 1), yw = a.g.yw;
    for (long grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        if (a.seg[grp * 2 + 1] == 0) continue;
        int32_t *L = a.lab + (size_t)(grp / segs) * cells;
        const long c0 = grp % segs * kFrontierSeg;
        const long b = b0 + grp / segs;
        for (int k = 0; k < 4; ++k) {
            const long c = c0 + k * kFrontierThreads + threadIdx.x;
            int row = -1, x = 0, y = 0;
            if (c < cells) {
                int label;
                row = row_of(L, (int)c, label);
                if (a.labels_out && label >= 0) a.labels_out[(size_t)b * cells + c] = label;
                x = (int)(c / yw);
                y = (int)(c % yw);
            }
            unsigned long long todo = __ballot(row >= 0);
            while (todo) {
                const int leader = __ffsll((long long)todo) - 1;
                const int r = __shfl(row, leader, kWave);
                const bool in = row == r;
                const unsigned long long same = __ballot(in);
                const int sx = wave_sum(in ? x : 0), sy = wave_sum(in ? y : 0);
                const int x0 = wave_min(in ? x : INT_MAX), y0 = wave_min(in ? y : INT_MAX);
                const int x1 = wave_max(in ? x : -1), y1 = wave_max(in ? y : -1);
                if (lane == leader) {
                    unsigned long long *sums = reinterpret_cast<unsigned long long *>(a.sums_out) + ((size_t)b * a.M + r) * 2;
                    atomicAdd(sums, (unsigned long long)sx);
                    atomicAdd(sums + 1, (unsigned long long)sy);
                    int32_t *out = a.clusters_out + ((size_t)b * a.M + r) * 8;
                    atomicMin(out + 4, x0); atomicMin(out + 5, y0); atomicMax(out + 6, x1); atomicMax(out + 7, y1);
                }
                todo &= ~same;
            }
        }
    }
}

// The member nearest to the rounded centroid, ties to the lowest flat index: min of (d2 << 32 | flat).
__global__ void __launch_bounds__(kFrontierThreads) k_frontier_rep(FrontierArgs a, int cells, long segs, long b0, long groups)
{
    const int lane = threadIdx.x & (kWave - 1), yw = a.g.yw;
    for (long grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        if (a.seg[grp * 2 + 1] == 0) continue;
        int32_t *L = a.lab + (size_t)(grp / segs) * cells;
        const long c0 = grp % segs * kFrontierSeg;
        const long b = b0 + grp / segs;
        for (int k = 0; k < 4; ++k) {
            const long c = c0 + k * kFrontierThreads + threadIdx.x;
            int row = -1;
            unsigned long long key = ~0ull;
            if (c < cells) {
                int label;
                row = row_of(L, (int)c, label);
                if (row >= 0) {
                    const size_t at = (size_t)b * a.M + row;
                    const long size = a.clusters_out[at * 8 + 1];
                    const long cx = (2 * a.sums_out[at * 2] + size) / (2 * size), cy = (2 * a.sums_out[at * 2 + 1] + size) / (2 * size);
                    const long dx = c / yw - cx, dy = c % yw - cy;
                    key = (unsigned long long)(dx * dx + dy * dy) << 32 | (unsigned)c;
                }
            }
            unsigned long long todo = __ballot(row >= 0);
            while (todo) {
                const int leader = __ffsll((long long)todo) - 1;
                const int r = __shfl(row, leader, kWave);
                const bool in = row == r;
                const unsigned long long same = __ballot(in);
                const unsigned long long best = wave_min_key(in ? key : ~0ull);
                if (lane == leader) atomicMin(reinterpret_cast<unsigned long long *>(a.clusters_out + ((size_t)b * a.M + r) * 8 + 2), best);
                todo &= ~same;
            }
        }
    }
}

// Row = (query, m): the key's low word, the representative's flat index, becomes (rep_x, rep_y).
__global__ void __launch_bounds__(kFrontierThreads) k_frontier_finish(FrontierArgs a, long row0, long rows)
{
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += (long)gridDim.x * blockDim.x) {
        int32_t *out = a.clusters_out + (size_t)(row0 + i) * 8;
        if (out[0] < 0) continue;
        const int flat = out[2];
        out[2] = flat / a.g.yw;
        out[3] = flat % a.g.yw;
    }
}

hipError_t launch_frontiers(const FrontierArgs &a, const FrontierShape &p, long b0, long nb, hipStream_t s)
{
    const int cells = a.g.xw * a.g.yw;
    auto blocks_for = [](long n, long per) { return (unsigned)std::max(1L, std::min(kFrontierMaxBlocks, (n + per - 1) / per)); };
    const dim3 block(kFrontierThreads);
    hipError_t e = hipMemsetAsync(a.seg, 0, (size_t)nb * p.segs * 8, s);
    if (e == hipSuccess && a.M > 0) {       // rows of -1 wherever k_frontier_rank writes none
        e = hipMemsetAsync(a.clusters_out + (size_t)b0 * a.M * 8, 0xff, (size_t)nb * a.M * 32, s);
        if (e == hipSuccess) e = hipMemsetAsync(a.sums_out + (size_t)b0 * a.M * 2, 0xff, (size_t)nb * a.M * 16, s);
    }
    if (e == hipSuccess && a.labels_out) e = hipMemsetAsync(a.labels_out + (size_t)b0 * cells, 0xff, (size_t)nb * cells * 4, s);
    if (e == hipSuccess) e = allow_dynamic_lds(reinterpret_cast<const void *>(&k_frontier_tile), p.lds);
    if (e != hipSuccess) return e;
    SLAM_LAUNCH(k_frontier_tile, dim3(blocks_for(nb * p.tiles, 1)), block, (size_t)p.lds, s, a, p.tiles_x, p.tiles_y, p.segs, b0, nb * p.tiles);
    if (p.border > 0)
        SLAM_LAUNCH(k_frontier_border, dim3(blocks_for(nb * p.border, kFrontierThreads)), block, 0, s, a, p.tiles_x, p.border, nb * p.border);
    const long groups = nb * p.segs;
    const dim3 by_seg(blocks_for(groups, 1));
    SLAM_LAUNCH(k_frontier_flatten, by_seg, block, 0, s, a, cells, p.segs, groups);
    SLAM_LAUNCH(k_frontier_sizes, by_seg, block, 0, s, a, cells, p.segs, groups);
    SLAM_LAUNCH(k_frontier_segs, by_seg, block, 0, s, a, cells, p.segs, groups);
    SLAM_LAUNCH(k_frontier_rank, by_seg, block, 0, s, a, cells, p.segs, b0, groups);
    if (a.M > 0 || a.labels_out) SLAM_LAUNCH(k_frontier_stats, by_seg, block, 0, s, a, cells, p.segs, b0, groups);
    if (a.M > 0) {
        SLAM_LAUNCH(k_frontier_rep, by_seg, block, 0, s, a, cells, p.segs, b0, groups);
        SLAM_LAUNCH(k_frontier_finish, dim3(blocks_for(nb * a.M, kFrontierThreads)), block, 0, s, a, b0 * a.M, nb * a.M);
    }
    return hipGetLastError();
}

}  // namespace slam
