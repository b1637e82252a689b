// A* global planner on gfx950 (wave64), after course_agv_nav/scripts/global_planner.py:
//   find_path.start_find obstacle inflation  :148-155  -> k_astar_inflate (trigger rows) + k_astar_inflate_apply
//   start_find search :157-179, append_around_open :181-204, find_min_cost_f :216-223,
//   append_path :206-213, append_close :235-237         -> k_astar
//
// Inflation.  The reference's loop writes 99 in place, so a cell in rows / columns [r, span - r) that
// holds 100 or -1 triggers only if no earlier trigger (scan order) has its (2r+1)^2 window over it.
// Row i depends on the triggers of rows i - r .. i - 1 and on those to its left, so one wave per map
// walks the rows: the row's candidates as 64-bit column masks (one word per lane, by ballot), minus
// the horizontally dilated triggers of the r rows above (kept in an LDS ring), then the greedy pass
// along the row on the uniform word masks (a trigger blocks the next r columns).  A second kernel
// writes 99 over the windows of every trigger, in parallel over cells.
//
// Search.  One wave per query in a persistent grid; each wave owns a workspace slot of H x W cells
// (state byte = open / closed + the direction to the parent, the open-list position) and an open
// list of (key, cell, g) entries.  find_min_cost_f's pop - the first index of the smallest f below
// 100 000, else index 0 - is the smallest key (min(f, 100000) << 32 | seq), seq numbering cells in
// the order they were first appended (a replacement keeps its list position, a removal keeps the
// order); the list itself is unordered (swap-remove) and the argmin is a wave reduction.  The 8
// neighbours of an expansion are 8 lanes in the reference's order: new cells take consecutive seq
// by ballot rank, an open cell is replaced only if its g (f less the cell's own h) is strictly
// larger.  A slot resets the cells its last query touched before it moves on: its open and closed
// cells, and the popped cell an EDGE stop leaves in neither list; the caller zeroes the state bytes
// once per call.
//
// Lanes of one wave hand data to each other through plain global loads and stores (one lane swaps
// an entry out, another reads it on the next step).  Under the language's per-lane memory model
// these are data races; the kernel relies on the gfx9 backend and hardware instead: a wave's vector
// memory instructions execute in order and the L1 is write-through, so it suffices that the
// compiler does not move the accesses across wave_fence() (a wavefront-scope fence plus a wave
// barrier: ordering points for the compiler, not synchronisation the language defines for them).
#include <hip/hip_runtime.h>

#include "slam_internal.h"

namespace slam {

namespace {

constexpr int kStOpen = 1, kStClosed = 2;  // low two bits of a state byte; 0: never appended
constexpr int kFClamp = 100000;        // find_min_cost_f's initial min_cost (:217)
constexpr int kInflateLdsMax = 32768;  // LDS ring of dilated trigger rows; larger rings stay in global memory

__device__ __forceinline__ void wave_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// neighbour k of append_around_open (:182-185): row offset outer, column offset inner, (0, 0) skipped
__device__ __forceinline__ int nb_di(int k) { return k < 3 ? -1 : (k < 5 ? 0 : 1); }
__device__ __forceinline__ int nb_dj(int k) { return (k == 0 || k == 3 || k == 5) ? -1 : ((k == 1 || k == 6) ? 0 : 1); }

// bits [o, o + 64) of a row whose word q is held by lane q (words < 64); bits outside the row are 0
__device__ __forceinline__ unsigned long long row_bits(unsigned long long s, int words, int o)
{
    const int q = o >= 0 ? o / 64 : -((63 - o) / 64);
    const int sh = o - q * 64;
    const unsigned long long a = __shfl(s, q & 63, kWave), b = __shfl(s, (q + 1) & 63, kWave);
    const unsigned long long lo = (q >= 0 && q < words) ? a : 0ull;
    const unsigned long long hi = (q + 1 >= 0 && q + 1 < words) ? b : 0ull;
    return sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
}

// One wave per map: the trigger set of start_find's in-place loop (:149-155), each row stored
// dilated by r columns (bit j set iff a trigger lies in columns [j - r, j + r]) to dil[G][span][words].
template <bool kLdsRing>
__global__ void __launch_bounds__(64) k_astar_inflate(const int8_t *__restrict__ maps, int G, int H, int W, int wire,
                                                      int span, int r, int words, unsigned long long *__restrict__ dil,
                                                      int *status)
{
    extern __shared__ unsigned long long ring[];   // [r][words] when kLdsRing
    const int lane = threadIdx.x;
    if (kLdsRing) lds_guard_fill(reinterpret_cast<char *>(ring + (size_t)r * words));
    const long cells = (long)H * W;
    const int lo = r, hi = span - r;
    for (int g = blockIdx.x; g < G; g += gridDim.x) {
        const int8_t *m = maps + (size_t)g * cells;
        unsigned long long *out = dil + (size_t)g * span * words;
        for (int i = lo; i < hi; ++i) {
            unsigned long long cand = 0;
            for (int k = 0; k < words; ++k) {
                const int j = k * 64 + lane;
                bool t = false;
                if (j >= lo && j < hi) {
                    const int v = wire ? m[(long)i * W + j] : m[(long)j * H + i];
                    t = v == 100 || v == -1;                       // :152
                }
                const unsigned long long b = __ballot(t);
                if (lane == k) cand = b;
            }
            if (lane < words)                                      // windows of the triggers above
                for (int t = 1; t <= r && i - t >= lo; ++t)
                    cand &= ~(kLdsRing ? ring[((i - t) % r) * words + lane] : out[(size_t)(i - t) * words + lane]);
            // left to right along the row: a candidate triggers unless the last trigger lies within r columns
            unsigned long long s = 0;
            long last = -(1L << 40);
            for (int w = 0; w < words; ++w) {
                unsigned long long c = __shfl(cand, w, kWave), sw = 0;
                for (;;) {
                    const long lim = last + r - (long)w * 64;      // bits 0 .. lim are within reach
                    if (lim >= 63) c = 0;
                    else if (lim >= 0) c &= ~((2ull << lim) - 1ull);
                    if (!c) break;
                    const int p = __ffsll((long long)c) - 1;
                    sw |= 1ull << p;
                    last = (long)w * 64 + p;
                }
                if (lane == w) s = sw;
            }
            unsigned long long d = 0;
            for (int t = -r; t <= r; ++t) d |= row_bits(s, words, lane * 64 + t);
            if (lane < words) {
                out[(size_t)i * words + lane] = d;
                if (kLdsRing && r > 0) ring[(i % r) * words + lane] = d;
            }
        }
    }
    if (kLdsRing) lds_guard_check(reinterpret_cast<const char *>(ring + (size_t)r * words), status);
}

// 99 over the window of every trigger (:153-155), the rest as it was; out is row-major [G][H][W].
__global__ void __launch_bounds__(256) k_astar_inflate_apply(const int8_t *__restrict__ maps, int G, int H, int W,
                                                             int wire, int span, int r, int words,
                                                             const unsigned long long *__restrict__ dil,
                                                             int8_t *__restrict__ out)
{
    const long cells = (long)H * W, total = cells * G;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long g = e / cells, c = e - g * cells;
        const int y = (int)(c / W), x = (int)(c - (long)y * W);
        int v = wire ? maps[e] : maps[g * cells + (long)x * H + y];
        if (y < span && x < span) {
            const unsigned long long *d = dil + (size_t)g * span * words + (x >> 6);
            const unsigned long long bit = 1ull << (x & 63);
            const int t0 = y - r > r ? y - r : r, t1 = y + r < span - r - 1 ? y + r : span - r - 1;
            for (int t = t0; t <= t1; ++t)
                if (d[(size_t)t * words] & bit) { v = 99; break; }
        }
        out[e] = (int8_t)v;
    }
}

__global__ void __launch_bounds__(64) k_astar(AstarArgs a)
{
    const int lane = threadIdx.x;
    const int H = a.H, W = a.W;
    const long cells = (long)H * W;
    const size_t so = (size_t)blockIdx.x * cells;
    uint8_t *st = a.state + so;
    int32_t *pos = a.pos + so, *ocell = a.ocell + so, *og = a.og + so, *closed = a.closed + so;
    unsigned long long *okey = a.okey + so;
    const int di = nb_di(lane & 7), dj = nb_dj(lane & 7);

    for (long q = blockIdx.x; q < a.B; q += gridDim.x) {
        int status = SLAM_ASTAR_OK, len = 0, nclosed = 0, n_open = 0;
        const int mi = a.map_of_query ? a.map_of_query[q] : (a.G == 1 ? 0 : (int)q);
        const int sr = a.starts[2 * q] - 1, sc = a.starts[2 * q + 1] - 1;    // find_path's in-place -1 (:137-142)
        const int gr = a.goals[2 * q] - 1, gc = a.goals[2 * q + 1] - 1;
        if (mi < 0 || mi >= a.G) {
            status = SLAM_ASTAR_BAD_MAP;
        } else {
            const int8_t *m = a.imaps + (size_t)mi * cells;
            if (sr < 0 || sr >= H || sc < 0 || sc >= W) status = SLAM_ASTAR_EDGE;
            else if (m[sr * W + sc] != 0) status = SLAM_ASTAR_INVALID_START;      // :157-159
            else if (gr < 0 || gr >= H || gc < 0 || gc >= W) status = SLAM_ASTAR_EDGE;
            else if (m[gr * W + gc] != 0) status = SLAM_ASTAR_INVALID_GOAL;       // :160-162
        }
        if (status == SLAM_ASTAR_OK) {
            const int8_t *m = a.imaps + (size_t)mi * cells;
            const int s = sr * W + sc, goal = gr * W + gc;
            int cur = s, g = 0, nseq = 0;
            for (;;) {
                // append_around_open(cur, g) (:181-204)
                const int cr = cur / W, cc = cur - cr * W;
                if (cr == 0 || cr == H - 1 || cc == 0 || cc == W - 1) {
                    // a popped cell is off the open list and not closed: the resets below walk the lists only
                    if (lane == 0) st[cur] = 0;
                    status = SLAM_ASTAR_EDGE;
                    break;
                }
                const int ng = g + 10;
                bool add = false;
                int n = 0;
                unsigned long long key = 0;
                if (lane < 8) {
                    n = cur + di * W + dj;
                    const int sn = st[n];
                    if (m[n] == 0 && (sn & 3) != kStClosed) {
                        const int f = ng + 10 * (abs(gr - (cr + di)) + abs(gc - (cc + dj)));
                        key = (unsigned long long)(f < kFClamp ? f : kFClamp) << 32;
                        if ((sn & 3) == kStOpen) {
                            const int e = pos[n];
                            if (og[e] > ng) {                                // cost_f > new cost_f, same h (:200)
                                og[e] = ng;
                                okey[e] = key | (okey[e] & 0xffffffffull);
                                st[n] = (uint8_t)(kStOpen | (lane << 2));
                            }
                        } else {
                            add = true;
                        }
                    }
                }
                const unsigned long long am = __ballot(add);
                if (add) {
                    const int rank = __popcll(am & ((1ull << lane) - 1ull));
                    const int e = n_open + rank;
                    okey[e] = key | (unsigned)(nseq + rank);
                    ocell[e] = n;
                    og[e] = ng;
                    pos[n] = e;
                    st[n] = (uint8_t)(kStOpen | (lane << 2));
                }
                n_open += __popcll(am);
                nseq += __popcll(am);
                if (lane == 0) {                                         // append_close (:235-237)
                    st[cur] = (uint8_t)((st[cur] & ~3) | kStClosed);
                    closed[nclosed] = cur;
                }
                ++nclosed;
                wave_fence();
                if (n_open == 0) { status = SLAM_ASTAR_NO_PATH; break; }  // open_list[0] of an empty list
                // find_min_cost_f (:216-223) as the smallest key
                unsigned long long best = ~0ull;
                int bi = 0;
                for (int e = lane; e < n_open; e += kWave) {
                    const unsigned long long k = okey[e];
                    if (k < best) { best = k; bi = e; }
                }
                unsigned long long wb = best;
                for (int off = 32; off > 0; off >>= 1) {
                    const unsigned long long o = __shfl_xor(wb, off, kWave);
                    wb = o < wb ? o : wb;
                }
                const int src = __ffsll((long long)__ballot(best == wb)) - 1;
                const int e = __shfl(bi, src, kWave);
                cur = ocell[e];
                g = og[e];
                if (cur == goal) break;                                  // :173-175; the goal is never closed
                --n_open;                                                // open_list.remove (:178)
                if (lane == 0 && e != n_open) {
                    const int lc = ocell[n_open];
                    okey[e] = okey[n_open];
                    ocell[e] = lc;
                    og[e] = og[n_open];
                    pos[lc] = e;
                }
                wave_fence();
            }
            if (status == SLAM_ASTAR_OK) {
                // append_path (:206-213): parents from the goal back to the start, written start -> goal
                len = 1;
                for (int c = goal; c != s; ++len) {
                    const int k = st[c] >> 2;
                    c -= nb_di(k) * W + nb_dj(k);
                }
                if (len > a.path_cap) status = SLAM_ASTAR_TRUNCATED;
                if (lane == 0) {
                    int32_t *p = a.path + (size_t)q * a.path_cap * 2;
                    int c = goal;
                    for (int k = len - 1; k >= 0; --k) {
                        if (k < a.path_cap) {
                            p[2 * k] = c / W;
                            p[2 * k + 1] = c % W;
                        }
                        if (k) {
                            const int d = st[c] >> 2;
                            c -= nb_di(d) * W + nb_dj(d);
                        }
                    }
                }
                wave_fence();
            }
            // the slot's next query starts from clean state bytes: every touched cell is open or closed
            for (int e = lane; e < n_open; e += kWave) st[ocell[e]] = 0;
            for (int e = lane; e < nclosed; e += kWave) st[closed[e]] = 0;
            wave_fence();
        }
        if (lane == 0) {
            a.status[q] = status;
            a.path_len[q] = len;
            a.expansions[q] = nclosed;                                   // len(close_list)
        }
    }
}

}  // namespace

hipError_t launch_astar_inflate(const int8_t *maps, int G, int H, int W, int wire, int span, int r,
                                unsigned long long *dil, int8_t *out, int *status, hipStream_t s)
{
    const int words = (span + 63) / 64;
    const int groups = G < 65535 ? G : 65535;
    if (span - r > r) {                                      // some row can trigger
        const size_t ring = (size_t)r * words * sizeof(unsigned long long);
        if (ring <= (size_t)kInflateLdsMax)
            SLAM_LAUNCH(k_astar_inflate<true>, dim3(groups), dim3(64), (unsigned)(ring + kLdsGuard), s, maps, G, H, W,
                        wire, span, r, words, dil, status);
        else
            SLAM_LAUNCH(k_astar_inflate<false>, dim3(groups), dim3(64), 0, s, maps, G, H, W, wire, span, r, words, dil,
                        status);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const long total = (long)G * H * W;
    const long blocks = (total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384;
    SLAM_LAUNCH(k_astar_inflate_apply, dim3((unsigned)blocks), dim3(256), 0, s, maps, G, H, W, wire, span, r, words, dil,
                out);
    return hipGetLastError();
}

hipError_t launch_astar(const AstarArgs &a, hipStream_t s)
{
    SLAM_LAUNCH(k_astar, dim3((unsigned)a.slots), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace slam
