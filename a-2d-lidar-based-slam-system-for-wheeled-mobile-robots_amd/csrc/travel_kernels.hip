// Travel-cost field for gfx950 (MI355X): the least cost of driving from the robot's cell to every traversable cell of a
// map, eight moves at 10 / 14 with no corner cutting, the move to take back from every cell and the paths to a list of
// goals (include/slam_hip.h, slam_grid_travel).  The reference has no counterpart.  Integer end to
// end and defined from the final costs alone, so no order of arrival shows.
//
//   k_travel_classes  a workgroup per (query, tile of 64 x 64 cells): the bits of the traversable set T from the counters
//                     (OccRule, what k_grid_finalize would write), the optional field and the foot squares of the
//                     sources, one ballot per row of the tile; every cost word to "unreached", 0 in the source cells; the
//                     tile's pending key: 0 when a source lies in the tile or next to it, clean otherwise
//   k_travel_relax    ONE workgroup per query owns its whole relaxation, so __syncthreads() is all that orders it: while
//                     a tile is dirty it takes the one with the lowest pending key, loads its costs and T bytes with a
//                     one-cell halo into LDS, forms every cell's allowed moves, lowers every cell to the minimum over
//                     them until a pass changes nothing (in place: a cost read is an upper bound whichever pass wrote it),
//                     writes back what went down and gives each of the eight neighbouring tiles whose facing border row,
//                     column or corner went down the lowest such cost as its key.  Keys only rise from one activation to
//                     the next, which bounds the activations (launch_shapes.h); both loops carry a hard trip bound.
//   k_travel_finish   a lane per cell: "unreached" becomes -1; dir_out from the final costs
//   k_travel_paths    a lane per (query, goal): the goal's cost, one walk along dir to count and one to write
// Nothing waits for another workgroup.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>

#include "slam_internal.h"
#include "grid_walk.h"

namespace slam {

namespace {

constexpr int kT = kTravelTile, kTileCells = kT * kT, kH = kT + 2, kHaloCells = kH * kH;
constexpr int kWaves = kTravelThreads / kWave;          // rows of the tile taken at once
constexpr int kCellsPerLane = kTileCells / kTravelThreads;
static_assert(kT == kWave, "a wave takes a row of the tile and its ballot is the row's word of T");
static_assert(kTileCells % kTravelThreads == 0 && kCellsPerLane * 8 <= 32, "a lane's allowed moves fit one word");
static_assert(kTravelMaxSources <= kTravelThreads, "a lane per source");

// direction codes 0..7, two bits each of (step + 1)
constexpr int kDx[8] = {1, 0, -1, 0, 1, -1, -1, 1}, kDy[8] = {0, 1, 0, -1, 1, 1, -1, -1};
constexpr unsigned pack_steps(const int (&v)[8])
{
    unsigned p = 0;
    for (int d = 0; d < 8; ++d) p |= (unsigned)(v[d] + 1) << (2 * d);
    return p;
}
constexpr unsigned kDxPack = pack_steps(kDx), kDyPack = pack_steps(kDy);
__device__ __forceinline__ int dx_of(int d) { return (int)(kDxPack >> (2 * d) & 3u) - 1; }
__device__ __forceinline__ int dy_of(int d) { return (int)(kDyPack >> (2 * d) & 3u) - 1; }
__device__ __forceinline__ int weight_of(int d) { return d < 4 ? kTravelStraight : kTravelDiagonal; }
// the code of a step (sx, sy), each in -1..1, not both 0
__device__ __forceinline__ int code_of(int sx, int sy)
{
    if (sy == 0) return sx > 0 ? 0 : 2;
    if (sx == 0) return sy > 0 ? 1 : 3;
    return sy > 0 ? (sx > 0 ? 4 : 5) : (sx > 0 ? 7 : 6);
}

__device__ __forceinline__ int ld_group(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void st_group(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

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
__device__ __forceinline__ int map_of(const TravelArgs &a, long b)
{
    const int gi = a.maps ? a.maps[b] : (int)b;
    return (unsigned)gi < (unsigned)a.g.G ? gi : -1;
}
// where the costs of query b = b0 + q live
__device__ __forceinline__ int32_t *cost_of(const TravelArgs &a, long b0, long q, size_t cells)
{
    return a.cost_out ? a.cost_out + (size_t)(b0 + q) * cells : a.ws_cost + (size_t)q * cells;
}

// a query's view of T and its costs, for the passes behind the relaxation
struct Field {
    const unsigned long long *mask;
    const int32_t *cost;
    int xw, yw, tiles_y;
    __device__ __forceinline__ bool in(int x, int y) const
    {
        if ((unsigned)x >= (unsigned)xw || (unsigned)y >= (unsigned)yw) return false;
        return mask[(size_t)x * tiles_y + (y >> 6)] >> (y & 63) & 1ull;
    }
    // the move from a cell of T in direction d: both cells in T, and for a diagonal the two cells it passes between
    __device__ __forceinline__ bool move(int x, int y, int d) const
    {
        const int dx = dx_of(d), dy = dy_of(d);
        if (!in(x + dx, y + dy)) return false;
        return d < 4 || (in(x + dx, y) && in(x, y + dy));
    }
    // the lowest code whose move is allowed and whose neighbour's cost + weight is the cell's; -1 for a source and for
    // a cell without a cost
    __device__ __forceinline__ int dir(int x, int y) const
    {
        const int c = cost[(size_t)x * yw + y];
        if (c <= 0 || c >= kTravelUnreached) return -1;
#pragma unroll 1
        for (int d = 0; d < 8; ++d) {
            if (!move(x, y, d)) continue;
            const int n = cost[(size_t)(x + dx_of(d)) * yw + y + dy_of(d)];
            if (n >= 0 && n < kTravelUnreached && n + weight_of(d) == c) return d;
        }
        return -1;
    }
};
__device__ __forceinline__ Field field_of(const TravelArgs &a, int tiles_y, long b0, long q)
{
    const size_t cells = (size_t)a.g.xw * a.g.yw;
    return Field{a.mask + (size_t)q * a.g.xw * tiles_y, cost_of(a, b0, q, cells), a.g.xw, a.g.yw, tiles_y};
}

}  // namespace

// Group = (query b0 + q, tile), taken grid-stride.  A wave takes rows wave, wave + kWaves, ... of the tile, a lane the
// cell y0 + lane of the row.
__global__ void __launch_bounds__(kTravelThreads) k_travel_classes(TravelArgs a, int tiles_x, int tiles_y, long b0, long groups)
{
    const OccRule rule = OccRule::of(a.g);
    const int xw = a.g.xw, yw = a.g.yw, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const size_t cells = (size_t)xw * yw;
    const long tiles = (long)tiles_x * tiles_y;
    for (long grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const long q = grp / tiles;
        const int t = (int)(grp % tiles), x0 = (t / tiles_y) * kT, y0 = (t % tiles_y) * kT;
        const int gi = map_of(a, b0 + q);
        const int32_t *src = a.sources + (size_t)(b0 + q) * a.S * 2;
        const uint32_t *pass = a.g.pass + (size_t)(gi < 0 ? 0 : gi) * cells, *hit = a.g.hit + (size_t)(gi < 0 ? 0 : gi) * cells;
        int32_t *cost = cost_of(a, b0, q, cells);
        unsigned long long *mask = a.mask + (size_t)q * xw * tiles_y;
#pragma unroll 1
        for (int k = 0; k < kCellsPerLane; ++k) {
            const int x = x0 + wave + k * kWaves, y = y0 + lane;
            if (x >= xw) break;                     // the same for the whole wave
            const size_t at = (size_t)x * yw + y;
            bool in = false, source = false;
            if (gi >= 0 && y < yw) {
                const uint32_t v = rule.value(pass[at], hit[at]);
                in = v == 0u || (a.through_unknown && v == 50u);
                if (in && a.min_clear2 > 0) in = (int)a.field[(size_t)gi * cells + at] >= a.min_clear2;
                for (int s = 0; s < a.S; ++s) {
                    const int sx = src[2 * s], sy = src[2 * s + 1];
                    if ((unsigned)sx >= (unsigned)xw || (unsigned)sy >= (unsigned)yw) continue;
                    const int cheb = std::max(abs(x - sx), abs(y - sy));
                    in |= cheb <= a.foot;
                    source |= cheb == 0;
                }
            }
            const unsigned long long bits = __ballot(in);
            if (lane == 0) mask[(size_t)x * tiles_y + t % tiles_y] = bits;
            if (y < yw) cost[at] = source ? 0 : kTravelUnreached;
        }
        // dirty from the start: a tile with a source in it or in the ring of cells around it
        int near = 0;
        if (gi >= 0 && tid < a.S) {
            const int sx = src[2 * tid], sy = src[2 * tid + 1];
            near = (unsigned)sx < (unsigned)xw && (unsigned)sy < (unsigned)yw && sx >= x0 - 1 && sx <= x0 + kT && sy >= y0 - 1 && sy <= y0 + kT;
        }
        near = __syncthreads_or(near);
        if (tid == 0) a.dirty[q * tiles + t] = near ? 0 : kTravelClean;
    }
}

// Workgroup = query b0 + q, taken grid-stride.  Dynamic LDS: travel_lds_bytes().
__global__ void __launch_bounds__(kTravelThreads) k_travel_relax(TravelArgs a, int tiles_x, int tiles_y, long trips, long b0, long nb)
{
    extern __shared__ __attribute__((aligned(16))) int lds_travel[];
    int *C = lds_travel;                                                            // [kH][kH] costs, halo included
    unsigned char *Tb = reinterpret_cast<unsigned char *>(C + kHaloCells);          // [kH][kH] 1: in T
    unsigned long long *sel = reinterpret_cast<unsigned long long *>(Tb + (kHaloCells + 15) / 16 * 16);   // [kWaves] selection keys
    int *mark = reinterpret_cast<int *>(sel + kWaves);                              // [8] keys for the neighbouring tiles
    static_assert(kWaves * 8 + 8 * 4 <= 64 * 4, "the control words fit what travel_lds_bytes leaves them");
    char *guard = reinterpret_cast<char *>(lds_travel) + travel_lds_bytes(0);
    lds_guard_fill(guard);
    const int xw = a.g.xw, yw = a.g.yw, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const size_t cells = (size_t)xw * yw;
    const long tiles = (long)tiles_x * tiles_y;
    for (long q = blockIdx.x; q < nb; q += gridDim.x) {
        const int gi = map_of(a, b0 + q);
        int32_t *cost = cost_of(a, b0, q, cells);
        const unsigned long long *mask = a.mask + (size_t)q * xw * tiles_y;
        int32_t *dirty = a.dirty + q * tiles;
        int tripped = 0;
        for (long act = 0; gi >= 0; ++act) {
            // the dirty tile with the lowest pending key, ties to the lowest tile
            unsigned long long key = ~0ull;
            for (long t = tid; t < tiles; t += kTravelThreads) {
                const int k = dirty[t];
                if (k != kTravelClean) key = std::min(key, ((unsigned long long)(unsigned)k << 32) | (unsigned)t);
            }
            key = wave_min_key(key);
            if (lane == 0) sel[wave] = key;
            __syncthreads();
            key = sel[0];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) key = std::min(key, sel[w]);
            if (key == ~0ull) break;
            if (act >= trips) { tripped = 1; break; }
            const int t = (int)(unsigned)key, tx = t / tiles_y, ty = t % tiles_y, x0 = tx * kT, y0 = ty * kT;
            if (tid == 0) dirty[t] = kTravelClean;
            if (tid < 8) mark[tid] = kTravelUnreached;
            for (int i = tid; i < kHaloCells; i += kTravelThreads) {
                const int x = x0 + i / kH - 1, y = y0 + i % kH - 1;
                int c = kTravelUnreached;
                unsigned char in = 0;
                if ((unsigned)x < (unsigned)xw && (unsigned)y < (unsigned)yw) {
                    in = (unsigned char)(mask[(size_t)x * tiles_y + (y >> 6)] >> (y & 63) & 1ull);
                    if (in) c = cost[(size_t)x * yw + y];
                }
                C[i] = c;
                Tb[i] = in;
            }
            __syncthreads();
            // a lane's cells: rows wave + k * kWaves, column lane; their allowed moves, a byte each, and their costs on entry
            unsigned moves = 0;
            int entry[kCellsPerLane];
#pragma unroll
            for (int k = 0; k < kCellsPerLane; ++k) {
                const int h = (wave + k * kWaves + 1) * kH + lane + 1;
                entry[k] = C[h];
                if (!Tb[h]) continue;
                unsigned m = 0;
#pragma unroll
                for (int d = 0; d < 8; ++d) {
                    bool ok = Tb[h + kDx[d] * kH + kDy[d]];
                    if (d >= 4) ok = ok && Tb[h + kDx[d] * kH] && Tb[h + kDy[d]];
                    m |= (unsigned)ok << d;
                }
                moves |= m << (8 * k);
            }
            for (int it = 0;; ++it) {
                int changed = 0;
#pragma unroll
                for (int k = 0; k < kCellsPerLane; ++k) {
                    const unsigned m = moves >> (8 * k) & 0xffu;
                    if (!m) continue;
                    const int h = (wave + k * kWaves + 1) * kH + lane + 1;
                    const int c = ld_group(C + h);
                    int best = c;
#pragma unroll
                    for (int d = 0; d < 8; ++d) {
                        const int v = ld_group(C + h + kDx[d] * kH + kDy[d]) + (d < 4 ? kTravelStraight : kTravelDiagonal);
                        if (m >> d & 1u) best = std::min(best, v);
                    }
                    if (best < c) { st_group(C + h, best); changed = 1; }
                }
                if (!__syncthreads_or(changed)) break;
                if (it >= kTileCells) { tripped = 1; break; }       // every pass that changes a cost settles a cell for good
            }
            if (tripped) break;
            // what went down goes back; a border cell that went down is news for the tiles it faces
#pragma unroll
            for (int k = 0; k < kCellsPerLane; ++k) {
                const int lx = wave + k * kWaves, h = (lx + 1) * kH + lane + 1;
                const int c = C[h];
                if (c >= entry[k]) continue;
                cost[(size_t)(x0 + lx) * yw + y0 + lane] = c;           // a cell of T, so inside the map
                const int sx = lx == 0 ? -1 : lx == kT - 1 ? 1 : 0, sy = lane == 0 ? -1 : lane == kT - 1 ? 1 : 0;
                if (sx) atomicMin(mark + code_of(sx, 0), c);
                if (sy) atomicMin(mark + code_of(0, sy), c);
                if (sx && sy) atomicMin(mark + code_of(sx, sy), c);
            }
            __syncthreads();
            if (tid < 8 && mark[tid] < kTravelUnreached) {
                const int nx = tx + dx_of(tid), ny = ty + dy_of(tid);
                if ((unsigned)nx < (unsigned)tiles_x && (unsigned)ny < (unsigned)tiles_y) {
                    int32_t *word = dirty + (long)nx * tiles_y + ny;
                    if (mark[tid] < *word) *word = mark[tid];
                }
            }
            __syncthreads();                        // the next selection reads these keys
        }
        if (tid == 0) a.status_out[b0 + q] = gi < 0 ? -1 : tripped ? 1 : 0;
        __syncthreads();
    }
    lds_guard_check(guard, a.g.status);
}

// Item = a cell of a query.
__global__ void __launch_bounds__(256) k_travel_finish(TravelArgs a, int tiles_y, long b0, long items)
{
    const long cells = (long)a.g.xw * a.g.yw;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (long)gridDim.x * blockDim.x) {
        const long q = i / cells, c = i % cells;
        const Field f = field_of(a, tiles_y, b0, q);
        // (a neighbour's word may turn from "unreached" into -1 meanwhile: dir takes neither for a cost)
        if (a.dir_out) a.dir_out[(size_t)(b0 + q) * cells + c] = (int8_t)f.dir((int)(c / a.g.yw), (int)(c % a.g.yw));
        if (f.cost[c] >= kTravelUnreached) cost_of(a, b0, q, (size_t)cells)[c] = -1;
    }
}

// Item = (query, goal).  path_out is all -1 on entry.
__global__ void __launch_bounds__(256) k_travel_paths(TravelArgs a, int tiles_y, long b0, long items)
{
    const int xw = a.g.xw, yw = a.g.yw;
    const long cells = (long)xw * yw;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (long)gridDim.x * blockDim.x) {
        const long q = i / a.Q;
        const size_t row = (size_t)(b0 + q) * a.Q + (size_t)(i % a.Q);
        const Field f = field_of(a, tiles_y, b0, q);
        const int gx = a.goals[row * 2], gy = a.goals[row * 2 + 1];
        int c = -1;
        if (map_of(a, b0 + q) >= 0 && (unsigned)gx < (unsigned)xw && (unsigned)gy < (unsigned)yw) c = f.cost[(size_t)gx * yw + gy];
        int len = 0;
        if (c >= 0) {
            int x = gx, y = gy;
            len = 1;
            for (long step = 0; step < cells; ++step) {
                const int d = f.dir(x, y);
                if (d < 0) break;
                x += dx_of(d); y += dy_of(d); ++len;
            }
        }
        a.goal_cost_out[row] = c < 0 ? -1 : c;
        a.path_len_out[row] = len;
        if (a.path_cap > 0 && len > 0) {
            int32_t *out = a.path_out + row * a.path_cap * 2;
            int x = gx, y = gy;
            for (int at = len - 1; at >= 0; --at) {         // source first: the goal is cell len - 1
                if (at < a.path_cap) { out[2 * (size_t)at] = x; out[2 * (size_t)at + 1] = y; }
                const int d = f.dir(x, y);
                if (d < 0) break;
                x += dx_of(d); y += dy_of(d);
            }
        }
    }
}

hipError_t launch_travel(const TravelArgs &a, const TravelShape &p, long b0, long nb, hipStream_t s)
{
    const long cells = (long)a.g.xw * a.g.yw;
    auto blocks_for = [](long n, long per) { return (unsigned)std::max(1L, std::min(kTravelMaxBlocks, (n + per - 1) / per)); };
    hipError_t e = hipSuccess;
    if (a.goals && a.path_cap > 0)
        e = hipMemsetAsync(a.path_out + (size_t)b0 * a.Q * a.path_cap * 2, 0xff, (size_t)nb * a.Q * a.path_cap * 8, s);
    if (e == hipSuccess) e = allow_dynamic_lds(reinterpret_cast<const void *>(&k_travel_relax), p.lds);
    if (e != hipSuccess) return e;
    SLAM_LAUNCH(k_travel_classes, dim3(blocks_for(nb * p.tiles, 1)), dim3(kTravelThreads), 0, s, a, p.tiles_x, p.tiles_y, b0, nb * p.tiles);
    SLAM_LAUNCH(k_travel_relax, dim3(blocks_for(nb, 1)), dim3(kTravelThreads), (size_t)p.lds, s, a, p.tiles_x, p.tiles_y, p.trips, b0, nb);
    SLAM_LAUNCH(k_travel_finish, dim3(blocks_for(nb * cells, 256)), dim3(256), 0, s, a, p.tiles_y, b0, nb * cells);
    if (a.goals && a.Q > 0)
        SLAM_LAUNCH(k_travel_paths, dim3(blocks_for(nb * a.Q, 256)), dim3(256), 0, s, a, p.tiles_y, b0, nb * (long)a.Q);
    return hipGetLastError();
}

}  // namespace slam
