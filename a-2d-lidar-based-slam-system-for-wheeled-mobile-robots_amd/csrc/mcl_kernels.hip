// Monte Carlo localisation on the distance field, for gfx950 (MI355X): F filters of P particles each are weighed
// against their filter's scan and resampled without leaving the device.  The reference has no
// counterpart: it only writes its map.
//
//   slam_mcl_weigh      moves every particle by its filter's odometry step (plus the caller's noise) with the pose
//                       step's formula, then costs the filter's scan from the NEW pose on the field: the matcher's
//                       expression for one candidate whose rotation is the particle's own.  int32 costs, added to the
//                       particle's accumulated cost `acc` (the integer log-weight), saturating at 2^30.
//   slam_mcl_resample   weights from a table indexed by (acc - min acc) >> shift, the weighted estimate, the effective
//                       sample size and systematic resampling; every index is decided in integers.
//
// The weigh has two launch shapes with the same bits, chosen by beam count in launch_mcl_weigh (context option
// "mcl_shape").  Both stage the filter's USED beams (lx, ly) once per workgroup in LDS, packed to the front through an LDS
// counter as k_match packs them (the cost is an integer sum: its order is free).
//   k_mcl_weigh       a workgroup takes a run of ONE filter's particles, one per lane; each lane computes cos / sin of its
//                     particle's heading and the motion once and loops over the beams: one 16-byte LDS broadcast read,
//                     four multiplies and four adds in float64, to_cell twice, one int16 load
//   k_mcl_weigh_wave  a wave per particle, lanes over the beams, a wave sum; faster from about a hundred beams up
//
// Resampling is four launches:
//   k_mcl_reduce      per filter min of (acc, index) keys over the live particles and their number
//   k_mcl_scan_block  per 1024 particles: the weights, their inclusive prefix sums WITHIN the block (uint64, into
//                     cum), the block's sum, its sum of squares and its partial sums of the estimate
//   k_mcl_scan_sums   one wave per filter: exclusive scan of the block sums (any number of blocks, 64 at a time with a
//                     running carry), S, Q, the estimate, the gate and the offset o
//   k_mcl_select      per slot j the smallest i with cum[i] * P > o + j * S by a binary search over
//                     cum[i] = (offset of i's block) + (prefix within the block), then the gather
// The block size of the scan is fixed, so the partial sums of the float64 estimate are added in an order that depends
// on P alone: a filter gets the same bits alone, in any batch and in any order, and from call to call.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "slam_internal.h"
#include "grid_walk.h"

namespace slam {

constexpr long kMclMaxBlocks = 1L << 20;               // workgroups per launch; more groups are taken grid-stride
constexpr uint32_t kMclWeightMax = 1u << 20;           // a table entry above it counts as this
constexpr int kMclAccMax = 1 << 30;                    // accumulated cost saturates here
constexpr int kMclScanThreads = 256;
constexpr int kMclPerLane = kMclScanBlock / kMclScanThreads;   // consecutive particles of one lane of the scan
constexpr int kMclReduceRun = 4096;                    // particles per workgroup of k_mcl_reduce
constexpr unsigned long long kMclNoKey = ~0ull;

// The filter's USED beams (lx, ly) into LDS, packed to the front; returns their number (after a barrier).
__device__ __forceinline__ int mcl_stage_beams(const MclWeighArgs &a, int f, double *lds, int *s_used)
{
    __syncthreads();                                                  // every lane is done with the beams staged before
    if (threadIdx.x == 0) *s_used = 0;
    __syncthreads();
    const float *ranges = a.ranges + (size_t)f * a.n;
    for (int t = threadIdx.x; t < a.n; t += blockDim.x) {
        const float rf = ranges[t];
        const double rr = (double)rf;
        if (isfinite(rr) && rf < a.max_range) {
            const int pos = atomicAdd(s_used, 1);
            lds[2 * pos] = a.cos_t[t] * rr;
            lds[2 * pos + 1] = a.sin_t[t] * rr;
        }
    }
    __syncthreads();
    return *s_used;
}

// Particle i of filter f: the motion (written back by `writer` lanes), then whether it is dead (reported by `writer` lanes).
// Returns true for a live particle, with its pose and its accumulated cost so far.
__device__ __forceinline__ bool mcl_move(const MclWeighArgs &a, int f, size_t i, bool nomap, bool writer, double &px, double &py,
                                         double &th, int &before)
{
    const GridDev &g = a.g;
    px = a.poses[3 * i]; py = a.poses[3 * i + 1]; th = a.poses[3 * i + 2];
    if (a.motion) {
        double dx = a.motion[3 * (size_t)f], dy = a.motion[3 * (size_t)f + 1], dth = a.motion[3 * (size_t)f + 2];
        if (a.noise) {
            dx = dx + a.noise[3 * i];
            dy = dy + a.noise[3 * i + 1];
            dth = dth + a.noise[3 * i + 2];
        }
        const double c0 = cos(th), s0 = sin(th);
        px = (px + c0 * dx) - s0 * dy;
        py = (py + s0 * dx) + c0 * dy;
        th = th + dth;
        if (writer) {
            a.poses[3 * i] = px;
            a.poses[3 * i + 1] = py;
            a.poses[3 * i + 2] = th;
        }
    }
    int bad = nomap || !isfinite(px) || !isfinite(py) || !isfinite(th);
    (void)to_cell(px, g.scale, g.off_x, bad);
    (void)to_cell(py, g.scale, g.off_y, bad);
    before = a.acc ? a.acc[i] : 0;
    if (!bad && before != SLAM_MCL_DEAD) return true;
    if (writer) {
        if (a.cost_out) a.cost_out[i] = -1;
        if (a.acc) a.acc[i] = SLAM_MCL_DEAD;
    }
    return false;
}

// One beam's term of the cost: the matcher's expression (k_match) with the particle's own rotation.
__device__ __forceinline__ int mcl_beam(const MclWeighArgs &a, const int16_t *field, double c, double s, double px, double py,
                                        double lx, double ly)
{
    const GridDev &g = a.g;
    const double x = c * lx + (-s) * ly + px * 1.0, y = s * lx + c * ly + py * 1.0;
    int off = 0;
    const int ex = to_cell(x, g.scale, g.off_x, off), ey = to_cell(y, g.scale, g.off_y, off);
    const bool in = !off && (unsigned)ex < (unsigned)g.xw && (unsigned)ey < (unsigned)g.yw;
    return in ? (int)field[(size_t)ex * g.yw + ey] : a.cap;
}

// The map of particle i = f * P + p: its filter's (slam_mcl_weigh), or its own (slam_mcl_weigh_maps).
__device__ __forceinline__ int mcl_map_of(const MclWeighArgs &a, int f, size_t i)
{
    if (a.own_maps) return a.pmaps ? a.pmaps[i] : (int)i;
    return a.maps ? a.maps[f] : 0;
}

__device__ __forceinline__ void mcl_store(const MclWeighArgs &a, size_t i, int before, int cost)
{
    if (a.cost_out) a.cost_out[i] = cost;
    if (a.acc) a.acc[i] = (int)std::min((long long)before + cost, (long long)kMclAccMax);
}

// Lanes over particles.  Group = (filter f, particles [ch * blockDim.x, (ch + 1) * blockDim.x) of it), taken grid-stride.
// Dynamic LDS: (lx, ly) of the used beams, [n][2].
__global__ void __launch_bounds__(256) k_mcl_weigh(MclWeighArgs a)
{
    extern __shared__ double lds_mcl[];
    __shared__ int s_used;
    const GridDev &g = a.g;
    char *guard = reinterpret_cast<char *>(lds_mcl + 2 * (size_t)a.n);
    lds_guard_fill(guard);
    const long groups = (long)a.F * a.chunks;
    for (long grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int f = (int)(grp / a.chunks), ch = (int)(grp % a.chunks);
        const int m = mcl_stage_beams(a, f, lds_mcl, &s_used);
        if (ch == 0 && threadIdx.x == 0 && a.used_out) a.used_out[f] = m;
        const int p = ch * (int)blockDim.x + (int)threadIdx.x;
        const size_t i = (size_t)f * a.P + p;
        const int gi = p < a.P ? mcl_map_of(a, f, i) : 0;             // the lane's own particle's map
        const bool nomap = (unsigned)gi >= (unsigned)g.G;
        double px, py, th;
        int before;
        if (p < a.P && mcl_move(a, f, i, nomap, true, px, py, th, before)) {   // (no lane leaves the loop body early: the barriers above)
            const double c = cos(th), s = sin(th);
            const int16_t *field = a.field + (size_t)gi * g.xw * g.yw;
            int cost = 0;
            for (int t = 0; t < m; ++t) cost += mcl_beam(a, field, c, s, px, py, lds_mcl[2 * t], lds_mcl[2 * t + 1]);
            mcl_store(a, i, before, cost);
        }
    }
    lds_guard_check(guard, g.status);
}

// (shfl64, a 64-bit value across a wave: slam_internal.h)
// The other shape: a wave per particle, lanes over the beams, the cost summed across the wave.  Group = (filter f,
// kMclWaveRun particles of it), a quarter of them per wave.  First the lanes of a wave each move ONE of its particles and
// take the cosine and sine of its heading (so that work is not repeated by 64 lanes); then the wave goes through its
// particles, their values broadcast from the lane that holds them, and the sum lands in that lane, which stores it.
constexpr int kMclWaveRun = 64;
__global__ void __launch_bounds__(256) k_mcl_weigh_wave(MclWeighArgs a)
{
    extern __shared__ double lds_mcl[];
    __shared__ int s_used;
    const GridDev &g = a.g;
    char *guard = reinterpret_cast<char *>(lds_mcl + 2 * (size_t)a.n);
    lds_guard_fill(guard);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, per = kMclWaveRun / (int)(blockDim.x / kWave);
    const long groups = (long)a.F * a.chunks;
    for (long grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int f = (int)(grp / a.chunks), ch = (int)(grp % a.chunks);
        const int m = mcl_stage_beams(a, f, lds_mcl, &s_used);
        if (ch == 0 && threadIdx.x == 0 && a.used_out) a.used_out[f] = m;
        const int p = ch * kMclWaveRun + wave * per + lane;
        const size_t i = (size_t)f * a.P + p;
        const int gi = lane < per && p < a.P ? mcl_map_of(a, f, i) : 0;   // broadcast below with the particle's other values
        const bool nomap = (unsigned)gi >= (unsigned)g.G;
        double px = 0.0, py = 0.0, th = 0.0, c = 0.0, s = 0.0;
        int before = 0, mine = 0;
        if (lane < per && p < a.P && mcl_move(a, f, i, nomap, true, px, py, th, before)) {
            c = cos(th);
            s = sin(th);
            mine = 1;
        }
        int cost = 0;
        for (int q = 0; q < per; ++q) {
            if (!__shfl(mine, q, kWave)) continue;                    // (wave-uniform) no such particle, or a dead one
            const double qx = shfl64(px, q), qy = shfl64(py, q), qc = shfl64(c, q), qs = shfl64(s, q);
            const int16_t *field = a.field + (size_t)__shfl(gi, q, kWave) * g.xw * g.yw;   // (a live particle: its map exists)
            int part = 0;
            for (int t = lane; t < m; t += kWave) part += mcl_beam(a, field, qc, qs, qx, qy, lds_mcl[2 * t], lds_mcl[2 * t + 1]);
#pragma unroll
            for (int off = kWave / 2; off; off >>= 1) part += __shfl_xor(part, off, kWave);
            if (lane == q) cost = part;
        }
        if (mine) mcl_store(a, i, before, cost);
    }
    lds_guard_check(guard, g.status);
}

// inclusive prefix sum over the lanes of a wave
__device__ __forceinline__ unsigned long long wave_scan(unsigned long long v)
{
    const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const unsigned long long o = shfl64(v, lane >= off ? lane - off : lane);
        if (lane >= off) v += o;
    }
    return v;
}

// sum over the lanes of a wave by a fixed butterfly: every lane ends with the same bits
template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
    const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
    for (int off = kWave / 2; off; off >>= 1) {
        const T o = shfl64(v, lane ^ off);
        v = v + o;                                                    // (commutative: both lanes of a pair get the same bits)
    }
    return v;
}

__device__ __forceinline__ unsigned long long mcl_key(int acc, int p)
{
    return ((unsigned long long)((unsigned)acc + 0x80000000u) << 32) | (unsigned)p;   // signed order of acc, then the index
}

// Group = (filter f, particles [ch * kMclReduceRun, ...)): one 64-bit atomic minimum and one add per workgroup.
__global__ void __launch_bounds__(256) k_mcl_reduce(const int32_t *__restrict__ acc, int F, int P, int chunks,
                                                    unsigned long long *__restrict__ keys, int32_t *__restrict__ live)
{
    __shared__ unsigned long long s_key[256 / kWave];
    __shared__ int s_live[256 / kWave];
    const long groups = (long)F * chunks;
    for (long grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int f = (int)(grp / chunks), p0 = (int)(grp % chunks) * kMclReduceRun, p1 = std::min(P, p0 + kMclReduceRun);
        const int32_t *af = acc + (size_t)f * P;
        unsigned long long best = kMclNoKey;
        int cnt = 0;
        for (int p = p0 + threadIdx.x; p < p1; p += blockDim.x) {
            const int v = af[p];
            if (v != SLAM_MCL_DEAD) {
                const unsigned long long key = mcl_key(v, p);
                best = key < best ? key : best;
                ++cnt;
            }
        }
#pragma unroll
        for (int off = kWave / 2; off; off >>= 1) {
            const unsigned long long o = shfl64(best, (int)(threadIdx.x & (kWave - 1)) ^ off);
            best = o < best ? o : best;
            cnt += __shfl_xor(cnt, off, kWave);
        }
        __syncthreads();                                              // the words of the group before have been read
        if ((threadIdx.x & (kWave - 1)) == 0) {
            s_key[threadIdx.x / kWave] = best;
            s_live[threadIdx.x / kWave] = cnt;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < (int)(blockDim.x / kWave); ++w) {
                best = s_key[w] < best ? s_key[w] : best;
                cnt += s_live[w];
            }
            if (best != kMclNoKey) atomicMin(&keys[f], best);
            if (cnt) atomicAdd(&live[f], cnt);
        }
    }
}

// Group = (filter f, scan block ch of it): kMclScanBlock particles, kMclPerLane consecutive ones per lane.
__global__ void __launch_bounds__(kMclScanThreads) k_mcl_scan_block(MclResampleArgs a)
{
    __shared__ unsigned long long s_sum[kMclScanThreads / kWave], s_q[kMclScanThreads / kWave];
    __shared__ double s_est[4][kMclScanThreads / kWave];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const long groups = (long)a.F * a.nblk;
    for (long grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int f = (int)(grp / a.nblk), ch = (int)(grp % a.nblk);
        const unsigned long long key = a.keys[f];
        const int amin = key == kMclNoKey ? 0 : (int)((unsigned)(key >> 32) - 0x80000000u);
        const size_t base = (size_t)f * a.P;
        const int p0 = ch * kMclScanBlock + (int)threadIdx.x * kMclPerLane;
        unsigned long long w[kMclPerLane], sum = 0, q = 0;
        double ex = 0.0, ey = 0.0, es = 0.0, ec = 0.0;
#pragma unroll
        for (int k = 0; k < kMclPerLane; ++k) {
            const int p = p0 + k;
            w[k] = 0;
            if (p < a.P) {
                const int v = a.acc[base + p];
                if (v != SLAM_MCL_DEAD) {
                    const int d = (int)std::min((long long)(((long long)v - amin) >> a.shift), (long long)(a.T - 1));
                    w[k] = std::min(a.table[d], kMclWeightMax);
                }
                if (w[k]) {                                           // (a dead particle's pose may hold NaN)
                    const double wd = (double)w[k], th = a.poses[3 * (base + p) + 2];
                    ex = ex + wd * a.poses[3 * (base + p)];
                    ey = ey + wd * a.poses[3 * (base + p) + 1];
                    es = es + wd * sin(th);
                    ec = ec + wd * cos(th);
                }
            }
            sum += w[k];
            q += w[k] * w[k];
        }
        const unsigned long long incl = wave_scan(sum);
        q = wave_sum(q);
        ex = wave_sum(ex); ey = wave_sum(ey); es = wave_sum(es); ec = wave_sum(ec);
        __syncthreads();                                              // the words of the group before have been read
        if (lane == kWave - 1) s_sum[wave] = incl;
        if (lane == 0) {
            s_q[wave] = q;
            s_est[0][wave] = ex; s_est[1][wave] = ey; s_est[2][wave] = es; s_est[3][wave] = ec;
        }
        __syncthreads();
        unsigned long long run = incl - sum;                          // exclusive within the block
        for (int v = 0; v < wave; ++v) run += s_sum[v];
#pragma unroll
        for (int k = 0; k < kMclPerLane; ++k) {
            run += w[k];
            if (p0 + k < a.P) a.cum[base + p0 + k] = run;
        }
        if (threadIdx.x == 0) {
            const size_t b = (size_t)f * a.nblk + ch;
            unsigned long long S = 0, Q = 0;
            double e[4] = {0.0, 0.0, 0.0, 0.0};
            for (int v = 0; v < kMclScanThreads / kWave; ++v) {
                S += s_sum[v];
                Q += s_q[v];
                for (int k = 0; k < 4; ++k) e[k] = e[k] + s_est[k][v];
            }
            a.bsum[b] = S;
            a.bq[b] = Q;
            for (int k = 0; k < 4; ++k) a.bpart[4 * b + k] = e[k];
        }
    }
}

// One wave per filter, taken grid-stride: bsum becomes the exclusive offsets of the scan blocks.
__global__ void __launch_bounds__(kWave) k_mcl_scan_sums(MclResampleArgs a)
{
    const int lane = threadIdx.x;
    for (long f = blockIdx.x; f < a.F; f += gridDim.x) {
        unsigned long long carry = 0, q = 0;
        double e[4] = {0.0, 0.0, 0.0, 0.0};
        for (int c0 = 0; c0 < a.nblk; c0 += kWave) {
            const int c = c0 + lane;
            const size_t b = (size_t)f * a.nblk + c;
            const unsigned long long v = c < a.nblk ? a.bsum[b] : 0;
            const unsigned long long incl = wave_scan(v);
            if (c < a.nblk) {
                a.bsum[b] = carry + incl - v;
                q += a.bq[b];
                for (int k = 0; k < 4; ++k) e[k] = e[k] + a.bpart[4 * b + k];
            }
            carry += shfl64(incl, kWave - 1);
        }
        q = wave_sum(q);
        for (int k = 0; k < 4; ++k) e[k] = wave_sum(e[k]);
        if (lane == 0) {                                              // (the shuffles of the next filter need every lane)
            const unsigned long long S = carry, key = a.keys[f];
            const double Sd = (double)S, nan = __longlong_as_double(0x7ff8000000000000ll);
            const double ess = S ? Sd * Sd / (double)q : 0.0;
            double *est = a.est_out + 4 * (size_t)f;
            est[0] = S ? e[0] / Sd : nan;
            est[1] = S ? e[1] / Sd : nan;
            est[2] = S ? atan2(e[2], e[3]) : nan;
            est[3] = ess;
            const bool go = S > 0 && ess < a.ess_frac * (double)a.P;
            unsigned long long o = 0;
            if (go) {
                const double u = a.u0[f], prod = (u >= 0.0 ? u : 0.0) * Sd;   // (u0 outside [0, 1) is the caller's error: clamped)
                o = prod >= Sd ? S - 1 : (unsigned long long)prod;
                o = std::min(o, S - 1);
            }
            int32_t *info = a.info_out + 4 * (size_t)f;
            info[0] = key == kMclNoKey ? -1 : (int32_t)(unsigned)key;
            info[1] = a.live[f];
            info[2] = go ? 1 : 0;
            info[3] = key == kMclNoKey ? 0 : (int32_t)((unsigned)(key >> 32) - 0x80000000u);
            a.fpar[2 * (size_t)f] = go ? S : 0;                           // S == 0: the filter does not resample
            a.fpar[2 * (size_t)f + 1] = o;
        }
    }
}

// One lane per slot (f, j) over the flat index, grid-stride.
__global__ void __launch_bounds__(256) k_mcl_select(MclResampleArgs a)
{
    const long total = (long)a.F * a.P;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int f = (int)(idx / a.P), j = (int)(idx - (long)f * a.P);
        const unsigned long long S = a.fpar[2 * (size_t)f];
        int anc = j;
        if (S) {
            const unsigned long long t = a.fpar[2 * (size_t)f + 1] + (unsigned long long)j * S, Pu = (unsigned long long)a.P;
            const unsigned long long *cum = a.cum + (size_t)f * a.P, *boff = a.bsum + (size_t)f * a.nblk;
            int lo = 0, hi = a.P - 1;                                 // the answer lies in [lo, hi]: cum[P - 1] * P = S * P > t
            while (lo < hi) {
                const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
                if ((boff[mid / kMclScanBlock] + cum[mid]) * Pu > t) hi = mid;
                else lo = mid + 1;
            }
            anc = lo;
            a.acc[idx] = 0;
        }
        const double *src = a.poses + 3 * ((size_t)f * a.P + anc);
        double *dst = a.poses_out + 3 * (size_t)idx;
        dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
        if (a.ancestors_out) a.ancestors_out[idx] = anc;
    }
}

// slam_mcl_settle: the resampled set rearranged so that every surviving particle keeps its own slot.  One workgroup per
// filter, taken grid-stride.  Dynamic LDS, three int arrays of P: cnt (how often each slot is an ancestor), the exclusive
// rank of every slot among the free ones (cnt == 0) and the inclusive sum of the surplus max(cnt - 1, 0).  The free slot
// of rank r takes the smallest i whose surplus sum exceeds r (a binary search): free slots and surplus copies are paired
// in ascending order, and the two lists are equally long because the counts add up to P.
constexpr int kMclSettleThreads = 256;
__global__ void __launch_bounds__(kMclSettleThreads) k_mcl_settle(MclSettleArgs a)
{
    extern __shared__ int lds_settle[];
    __shared__ int s_wave[2][kMclSettleThreads / kWave], s_moved;
    const int P = a.P, lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    int *cnt = lds_settle, *frank = lds_settle + P, *sur = lds_settle + 2 * (size_t)P;
    char *guard = reinterpret_cast<char *>(lds_settle + 3 * (size_t)P);
    lds_guard_fill(guard);
    const int per = (P + kMclSettleThreads - 1) / kMclSettleThreads;   // consecutive slots of one lane of the scans
    for (long f = blockIdx.x; f < a.F; f += gridDim.x) {
        const size_t base = (size_t)f * P;
        __syncthreads();                                              // every lane is done with the filter before
        for (int j = threadIdx.x; j < P; j += blockDim.x) cnt[j] = 0;
        if (threadIdx.x == 0) s_moved = 0;
        __syncthreads();
        for (int j = threadIdx.x; j < P; j += blockDim.x) atomicAdd(&cnt[std::min(std::max(a.ancestors[base + j], 0), P - 1)], 1);
        __syncthreads();
        const int j0 = (int)threadIdx.x * per, j1 = std::min(P, j0 + per);
        int nfree = 0, nsur = 0;
        for (int j = j0; j < j1; ++j) {
            nfree += cnt[j] == 0;
            nsur += std::max(cnt[j] - 1, 0);
        }
        int ifree = nfree, isur = nsur;                               // inclusive over the lanes of the wave
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const int of = __shfl_up(ifree, off, kWave), os = __shfl_up(isur, off, kWave);
            if (lane >= off) { ifree += of; isur += os; }
        }
        if (lane == kWave - 1) { s_wave[0][wave] = ifree; s_wave[1][wave] = isur; }
        __syncthreads();
        int rfree = ifree - nfree, rsur = isur - nsur;                // exclusive within the workgroup
        for (int v = 0; v < wave; ++v) { rfree += s_wave[0][v]; rsur += s_wave[1][v]; }
        for (int j = j0; j < j1; ++j) {
            frank[j] = rfree;
            rfree += cnt[j] == 0;
            rsur += std::max(cnt[j] - 1, 0);
            sur[j] = rsur;
        }
        __syncthreads();
        int moved = 0;
        for (int j = threadIdx.x; j < P; j += blockDim.x) {
            int from = j;
            if (cnt[j] == 0) {
                const int r = frank[j];
                int lo = 0, hi = P - 1;                               // the answer lies in [lo, hi]: sur[P - 1] = the free slots > r
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (sur[mid] > r) hi = mid;
                    else lo = mid + 1;
                }
                from = lo;
                ++moved;
            }
            a.settled[base + j] = from;
            if (a.map_src) a.map_src[base + j] = a.map0 + (int)base + from;
            if (a.poses_out) {
                const double *src = a.poses_src + 3 * (base + from);
                double *dst = a.poses_out + 3 * (base + j);
                dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
            }
        }
        if (a.moved) {
#pragma unroll
            for (int off = kWave / 2; off; off >>= 1) moved += __shfl_xor(moved, off, kWave);
            if (lane == 0 && moved) atomicAdd(&s_moved, moved);
            __syncthreads();
            if (threadIdx.x == 0) a.moved[f] = s_moved;
        }
    }
    lds_guard_check(guard, a.status);
}

hipError_t launch_mcl_settle(const MclSettleArgs &a, hipStream_t s)
{
    const int lds = 3 * 4 * a.P + kLdsGuard;                          // P <= kMclSettleMaxP: 48 KiB, within what a kernel gets unasked
    SLAM_LAUNCH(k_mcl_settle, dim3((unsigned)std::min((long)a.F, kMclMaxBlocks)), dim3(kMclSettleThreads), lds, s, a);
    return hipGetLastError();
}

// Launch shape of the weigh (context option "mcl_shape"; DESIGN.md section 15 has the measurements).
//   0, lanes over particles: one particle per lane; 256 lanes per workgroup, halved (down to one wave) while the launch has
//      fewer than 1024 workgroups, so that one filter of 65 536 particles still puts two workgroups on every CU and 4 096
//      filters of 16 particles do not carry 240 idle lanes each.
//   1, a wave per particle: 256 lanes, kMclWaveRun particles per group.  Its lanes idle where a scan has few beams.
//  -1: by the beam count, kMclWaveMinBeams and more take the wave shape.
constexpr int kMclWaveMinBeams = 112;
hipError_t launch_mcl_weigh(MclWeighArgs a, int shape, hipStream_t s)
{
    if (shape < 0) shape = a.n >= kMclWaveMinBeams ? 1 : 0;
    const int lds = 16 * a.n + kLdsGuard;
    if (shape == 1) {
        a.chunks = (a.P + kMclWaveRun - 1) / kMclWaveRun;
        hipError_t e = allow_dynamic_lds((const void *)k_mcl_weigh_wave, lds);
        if (e != hipSuccess) return e;
        SLAM_LAUNCH(k_mcl_weigh_wave, dim3((unsigned)std::min((long)a.F * a.chunks, kMclMaxBlocks)), dim3(256), lds, s, a);
        return hipGetLastError();
    }
    int threads = (int)std::min(256L, ((long)a.P + kWave - 1) / kWave * kWave);
    while (threads > kWave && (long)a.F * ((a.P + threads - 1) / threads) < 1024) threads /= 2;
    a.chunks = (a.P + threads - 1) / threads;
    hipError_t e = allow_dynamic_lds((const void *)k_mcl_weigh, lds);
    if (e != hipSuccess) return e;
    const long groups = (long)a.F * a.chunks;
    SLAM_LAUNCH(k_mcl_weigh, dim3((unsigned)std::min(groups, kMclMaxBlocks)), dim3(threads), lds, s, a);
    return hipGetLastError();
}

// keys: every byte 0xff on entry; live: zero on entry.
hipError_t launch_mcl_resample(MclResampleArgs a, hipStream_t s)
{
    a.nblk = mcl_scan_blocks(a.P);
    const int rchunks = (a.P + kMclReduceRun - 1) / kMclReduceRun;
    const int rthreads = (int)std::min(256L, ((long)a.P + kWave - 1) / kWave * kWave);
    SLAM_LAUNCH(k_mcl_reduce, dim3((unsigned)std::min((long)a.F * rchunks, kMclMaxBlocks)), dim3(rthreads), 0, s, a.acc, a.F, a.P,
                rchunks, a.keys, a.live);
    SLAM_LAUNCH(k_mcl_scan_block, dim3((unsigned)std::min((long)a.F * a.nblk, kMclMaxBlocks)), dim3(kMclScanThreads), 0, s, a);
    SLAM_LAUNCH(k_mcl_scan_sums, dim3((unsigned)std::min((long)a.F, kMclMaxBlocks)), dim3(kWave), 0, s, a);
    const long total = (long)a.F * a.P;
    SLAM_LAUNCH(k_mcl_select, dim3((unsigned)std::min((total + 255) / 256, kMclMaxBlocks)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace slam
