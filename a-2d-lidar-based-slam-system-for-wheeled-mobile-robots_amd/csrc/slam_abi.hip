// C-ABI layer of libslamhip.so (include/slam_hip.h): contexts, workspaces, error
// reporting, host<->device staging and the launch sequences.  No compute happens on the
// host; without a gfx950 device every entry point fails.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <initializer_list>
#include <mutex>
#include <utility>
#include <vector>

#include "slam_internal.h"
#include "slam_stamps.h"
#include "workspace.h"

using namespace slam;

namespace {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return fail(SLAM_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_));       \
    } while (0)

// REQUIRE_IN: a check written once for an entry point and its host / device twin reports the name it was called by
#define REQUIRE_IN(fn, cond, msg)                                                                      \
    do {                                                                                               \
        if (!(cond)) return fail(SLAM_ERR_INVALID, "%s: %s", fn, msg);                                 \
    } while (0)
#define REQUIRE(cond, msg) REQUIRE_IN(__func__, cond, msg)

#define TRY(expr)                                                                                      \
    do {                                                                                               \
        int rc_ = (expr);                                                                              \
        if (rc_ != SLAM_OK) return rc_;                                                                \
    } while (0)

size_t dtype_size(int dtype)
{
    switch (dtype) {
    case SLAM_F64: return 8;
    case SLAM_F32: return 4;
    case SLAM_F16: return 2;
    }
    return 0;
}

size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

// a grid object's state, one allocation [pass | hit | visit counter]: the two counter planes of all its cells, then the slots
size_t grid_plane_bytes(size_t cells) { return align_up(cells * 4); }
size_t grid_state_bytes(size_t cells)
{
    return grid_plane_bytes(cells) * 2 + align_up((size_t)kVisitSlots * kVisitStride * sizeof(unsigned long long));
}

struct Arena {
    char *base = nullptr;
    size_t cap = 0;
};

struct Pending {
    int kind;
    hipEvent_t e0, e1;
    bool first;      // first launch of its timing bracket: the family's launch count goes by brackets
};

}  // namespace

struct slam_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    Arena staging;   // device copies of host arguments (host-pointer entry points)
    Arena scratch;   // temporaries of *_dev sequences
    Arena tiles;     // recorded walks of the tiled ray cast
    char *pinned = nullptr;   // page-locked host block: small calls go through it in one copy each way
    size_t pinned_cap = 0;
    int *status = nullptr;
    bool timing = false;
    unsigned timing_mask = ~0u;   // families (bit SLAM_K_*) whose launches carry events while timing is on
    std::vector<hipEvent_t> pool;
    std::vector<Pending> pending;
    double ms[SLAM_K_COUNT] = {0};
    int64_t launches[SLAM_K_COUNT] = {0};
    int grid_mode = 1;    // 0: direct global atomics, 1: automatic, 2: tiles, 3: LDS window, 4: wedges
    int grid_group = 0;   // scans per workgroup in window mode (0: automatic)
    int grid_split = -1;  // window mode: two workgroups per group, one per direction half (-1: when the launch cannot fill the chip)
    int icp_qpt = 0;      // queries per lane of batched scan matching (0: by batch size)
    int replay_reset = 0; // 1: slam_replay_dev clears its map's counters itself (inside the scan-matching launch)
    int icp_f32_filter = -1; // float32 pre-filter of the one-wave shape's beam windows: -1 = the library's choice (on), 0 = off, 1 = on; changes no result
    int win_lds_hits = -1; // shared-map window ray cast: hits of sorted rays counted in the LDS window, one global add per end cell: -1 = the library's choice (chip-filling launches), 0 = off, 1 = on; changes no result
    int icp_one_wave = -1; // scan matching with one wave per pair: -1 = where a full-chip launch allows it, 0 = never, 1 = wherever a pair fits
    int raycast_lds = -1; // rays traced through a map: -1 = automatic, 0 = mask words from global memory, 1 = from LDS wherever the mask fits
    int mcl_shape = -1;   // slam_mcl_weigh: -1 = the library's choice by beam count, 0 = lanes over particles, 1 = a wave per particle, lanes over beams; changes no result
    long locate_ws_bytes = 64L << 20; // slam_grid_locate: bytes its node lists may take ("locate_ws_mb"); pairs are cut into chunks that fit; changes no result
    long frontier_ws_bytes = 256L << 20; // slam_grid_frontiers: bytes its labels may take ("frontier_ws_mb"); queries are cut into chunks that fit; changes no result
    long travel_ws_bytes = 256L << 20; // slam_grid_travel: bytes its costs, traversable bits and tile keys may take ("travel_ws_mb"); queries are cut into chunks that fit; changes no result
    int gain_lds = -1;    // slam_grid_view_gain: -1 = automatic, 0 = every bit window in the workspace, 1 = in LDS wherever a view's window fits; changes no result
    long gain_ws_bytes = 256L << 20; // slam_grid_view_gain: bytes the window slots of its global engine may take ("gain_ws_mb"); changes no result
    int icp_team = 0;     // first-iteration queries without a beam window: 0 = listed and searched apart from their lanes (nn_listed), 1 = box search
    // "pipeline" option: the map stage of slam_replay_dev (reset -> ray cast -> finalize) runs on
    // a second stream, so the map stage of one replay overlaps the scan matching of the next.
    int pipeline = 0;
    hipStream_t gstream = nullptr;                   // map stage
    hipStream_t cstream = nullptr;                   // pose composition (a serial chain in one workgroup)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_icp = nullptr, ev_pose = nullptr;
    hipEvent_t ev_cast[2] = {nullptr, nullptr};     // "compose + ray cast of that replay have read T / poses"
    const void *cast_poses[2] = {nullptr, nullptr};
    const void *cast_T[2] = {nullptr, nullptr};
    double *pipe_T[2] = {nullptr, nullptr};          // T buffers when the caller passes none
    size_t pipe_T_bytes = 0;
    int cast_pos = 0;
    bool gdirty = false;                             // work on gstream the main stream has not waited for
    bool mgrid = false;                              // map work on the main stream gstream has not waited for
    // Particle batches in chunks (option "particle_chunks"): scan matching and pose steps of chunk k on the main stream,
    // its ray cast on pstream behind an event - the vector-issue-bound matcher of chunk k + 1 shares the chip with the
    // memory-bound ray cast of chunk k (slam_particles_dev).
    int particle_chunks = 0;                         // 0 / 1: off, else the number of chunks
    hipStream_t pstream = nullptr;
    std::vector<hipEvent_t> pev_pose, pev_cast;      // per chunk: "poses written" (main -> pstream), "ray cast done" (pstream -> main)
    hipEvent_t pev_join = nullptr;
    bool pdirty = false;                             // ray casts on pstream the main stream has not waited for
    hipEvent_t ev_order = nullptr;                   // slam_stream_order: ordering with a caller's stream
};

struct slam_grid {
    GridDev d;
    unsigned long long *visits = nullptr;
    size_t state_bytes = 0;        // pass[] + hit[] + visit counter, one allocation
    int8_t *pmap_one = nullptr;    // [xw][yw] read-back staging
    double *datamap_one = nullptr;
    int8_t *pmap_live = nullptr;   // [G][xw][yw], slam_grid_live_pmap
    bool live_dirty = false;       // pmap_live is behind the counters
    bool pristine = true;          // nothing has been cast since creation / the last reset: every cell is 50
};

namespace slam {
thread_local LaunchTimer g_launch_timer = {nullptr, nullptr};

hipError_t allow_dynamic_lds(const void *kernel, int bytes)
{
    struct Entry { int dev; const void *kernel; int bytes; };
    static std::mutex mu;
    static std::vector<Entry> done;       // largest size the attribute has been set to, per (device, kernel)
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    Entry *hit = nullptr;
    for (auto &d : done)
        if (d.dev == dev && d.kernel == kernel) hit = &d;
    if (hit && hit->bytes >= bytes) return hipSuccess;
    // (a kernel whose LDS need depends on the launch - k_wedge_sort: beams x scans per group - asks again with more)
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return e;
    if (hit) hit->bytes = bytes;
    else done.push_back(Entry{dev, kernel, bytes});
    return hipSuccess;
}
}  // namespace slam

namespace {

int arena_reserve(slam_ctx *c, Arena &a, size_t bytes)
{
    if (bytes <= a.cap) return SLAM_OK;
    HIPCHK(hipStreamSynchronize(c->stream));
    if (a.base) HIPCHK(hipFree(a.base));
    a.base = nullptr;
    a.cap = 0;
    size_t want = align_up(bytes + bytes / 4, 1 << 20);
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&a.base), want);
    if (e != hipSuccess) return fail(SLAM_ERR_NOMEM, "hipMalloc(%zu bytes): %s", want, hipGetErrorString(e));
    a.cap = want;
    return SLAM_OK;
}

// The arena sized for a call's layout and the layout placed in it: every pointer bound to a piece is set.  A layout that
// does not fit is an error code here, before the entry point has enqueued anything.
int reserve(slam_ctx *c, Arena &a, const Layout &ws)
{
    TRY(arena_reserve(c, a, ws.bytes()));
    if (ws.place(a.base, a.cap)) return SLAM_OK;
    return fail(SLAM_ERR_NOMEM, "internal: a workspace of %zu bytes (more than %d pieces?) in an arena of %zu", ws.bytes(), Layout::kMaxPieces, a.cap);
}

// RAII bracket around the kernel launch(es) of a family: every SLAM_LAUNCH inside it draws a
// fresh pair of events from it (slam_internal.h), and the family's time is the sum of its launches.
struct Timed {
    slam_ctx *c;
    int kind;
    LaunchTimer saved;
    bool used = false;
    // counts: the bracket's first launch counts as a launch of its family (false: one more piece of a family whose
    // launches are counted elsewhere - the later chunks of a particle batch)
    Timed(slam_ctx *ctx, int k, hipStream_t = nullptr, bool counts = true) : c(ctx), kind(k), saved(g_launch_timer), used(!counts)
    {
        if (c->timing && (c->timing_mask >> k & 1u)) g_launch_timer = {this, &Timed::next};
    }
    ~Timed() { g_launch_timer = saved; }
    static bool next(void *self, hipEvent_t *e0, hipEvent_t *e1)
    {
        Timed *t = static_cast<Timed *>(self);
        *e0 = t->get();
        *e1 = t->get();
        if (!*e0 || !*e1) {
            if (*e0) t->c->pool.push_back(*e0);
            if (*e1) t->c->pool.push_back(*e1);
            return false;
        }
        t->c->pending.push_back({t->kind, *e0, *e1, !t->used});
        t->used = true;
        return true;
    }
    hipEvent_t get()
    {
        if (!c->pool.empty()) {
            hipEvent_t e = c->pool.back();
            c->pool.pop_back();
            return e;
        }
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        return e;
    }
};

int use(slam_ctx *c)
{
    if (!c) return fail(SLAM_ERR_INVALID, "null context");
    HIPCHK(hipSetDevice(c->device));
    return SLAM_OK;
}

// stream of the pipelined map stage
hipStream_t gs(slam_ctx *c) { return c->pipeline ? c->gstream : c->stream; }

// the map stream must see everything enqueued on the main stream so far
int fork_to_grid(slam_ctx *c)
{
    if (!c->pipeline) return SLAM_OK;
    HIPCHK(hipEventRecord(c->ev_fork, c->stream));
    HIPCHK(hipStreamWaitEvent(c->gstream, c->ev_fork, 0));
    c->gdirty = true;
    return SLAM_OK;
}

// the main stream must see the ray casts of chunked particle batches (pstream) enqueued so far
int join_particles(slam_ctx *c)
{
    if (!c->pdirty) return SLAM_OK;
    HIPCHK(hipEventRecord(c->pev_join, c->pstream));
    HIPCHK(hipStreamWaitEvent(c->stream, c->pev_join, 0));
    c->pdirty = false;
    return SLAM_OK;
}

// the main stream must see everything enqueued on the map stream so far
int join_from_grid(slam_ctx *c)
{
    if (int rc = join_particles(c)) return rc;
    if (!c->pipeline || !c->gdirty) return SLAM_OK;
    HIPCHK(hipEventRecord(c->ev_join, c->gstream));
    HIPCHK(hipStreamWaitEvent(c->stream, c->ev_join, 0));
    c->gdirty = false;
    return SLAM_OK;
}

constexpr size_t kPinnedBytes = 256 * 1024;

bool ensure_pinned(slam_ctx *c)
{
    if (c->pinned) return true;
    if (hipHostMalloc(reinterpret_cast<void **>(&c->pinned), kPinnedBytes, hipHostMallocDefault) != hipSuccess) {
        c->pinned = nullptr;
        (void)hipGetLastError();
        return false;
    }
    c->pinned_cap = kPinnedBytes;
    return true;
}

// Device copies of the arguments of a host-pointer entry point.  The entry point declares its
// pieces once, in order (a Layout, workspace.h); upload() reserves exactly their aligned sum in the staging
// arena, sets every device pointer and copies the inputs in; download() copies the outputs back and ends with
// a stream synchronise (so the page-locked block is free at the next call).  The pieces lie in
// ONE arena in ascending order, so when those of one direction are small (a drop-in call: one
// scan pair, one scan) they cross the bus in one copy through the page-locked block, laid out
// like the device pieces; otherwise one copy per piece.
class Staging {
public:
    explicit Staging(slam_ctx *c) : c_(c) {}
    // an input copied from `host`; absent (null device pointer) when `host` is null
    template <typename T> Staging &in(T *&dev, const T *host, size_t n) { return add(dev, n, host, nullptr, !host); }
    // copied from `host` and back to it; absent when `host` is null
    template <typename T> Staging &inout(T *&dev, T *host, size_t n) { return add(dev, n, host, host, !host); }
    // an output copied back to `host`; absent when `host` is null
    template <typename T> Staging &out(T *&dev, T *host, size_t n) { return add(dev, n, nullptr, host, !host); }
    // an output the device form always needs: copied back only when `host` is non-null
    template <typename T> Staging &out_always(T *&dev, T *host, size_t n) { return add(dev, n, nullptr, host, false); }
    // device-only workspace
    template <typename T> Staging &work(T *&dev, size_t n) { return add(dev, n, nullptr, nullptr, false); }

    int upload()
    {
        TRY(reserve(c_, c_->staging, ws_));
        char *d = c_->staging.base;
        size_t lo, hi;
        if (!span(true, lo, hi)) return SLAM_OK;
        if (hi - lo <= kPinnedBytes / 2 && ensure_pinned(c_)) {
            for (int i = 0; i < ws_.count(); ++i)
                if (h_[i].src) memcpy(c_->pinned + (ws_.offset(i) - lo), h_[i].src, ws_.size(i));
            HIPCHK(hipMemcpyAsync(d + lo, c_->pinned, hi - lo, hipMemcpyHostToDevice, c_->stream));
            return SLAM_OK;
        }
        for (int i = 0; i < ws_.count(); ++i)
            if (h_[i].src) HIPCHK(hipMemcpyAsync(d + ws_.offset(i), h_[i].src, ws_.size(i), hipMemcpyHostToDevice, c_->stream));
        return SLAM_OK;
    }

    int download()
    {
        char *d = c_->staging.base;
        size_t lo, hi;
        if (span(false, lo, hi) && hi - lo <= kPinnedBytes / 2 && ensure_pinned(c_)) {
            char *h = c_->pinned + kPinnedBytes / 2;
            HIPCHK(hipMemcpyAsync(h, d + lo, hi - lo, hipMemcpyDeviceToHost, c_->stream));
            HIPCHK(hipStreamSynchronize(c_->stream));
            for (int i = 0; i < ws_.count(); ++i)
                if (h_[i].dst) memcpy(h_[i].dst, h + (ws_.offset(i) - lo), ws_.size(i));
            return SLAM_OK;
        }
        for (int i = 0; i < ws_.count(); ++i)
            if (h_[i].dst) HIPCHK(hipMemcpyAsync(h_[i].dst, d + ws_.offset(i), ws_.size(i), hipMemcpyDeviceToHost, c_->stream));
        HIPCHK(hipStreamSynchronize(c_->stream));
        return SLAM_OK;
    }

private:
    struct Host {
        const void *src;                      // host source of an input (null: nothing to copy in)
        void *dst;                            // host destination of an output (null: nothing to copy back)
    };

    template <typename T> Staging &add(T *&dev, size_t n, const void *src, void *dst, bool absent)
    {
        dev = nullptr;
        if (absent) return *this;
        const int i = ws_.count();
        ws_.add(dev, n);
        if (ws_.count() > i) h_[i] = Host{n ? src : nullptr, n ? dst : nullptr};
        return *this;
    }
    // byte range [lo, hi) of the arena that the copies of one direction cover; false: nothing to copy
    bool span(bool in, size_t &lo, size_t &hi) const
    {
        lo = ws_.bytes();
        hi = 0;
        for (int i = 0; i < ws_.count(); ++i)
            if (in ? h_[i].src != nullptr : h_[i].dst != nullptr) {
                lo = std::min(lo, ws_.offset(i));
                hi = std::max(hi, ws_.offset(i) + ws_.size(i));
            }
        return lo < hi;
    }

    slam_ctx *c_;
    Layout ws_;                               // the device pieces, in the order they were declared
    Host h_[Layout::kMaxPieces];              // piece i of ws_: where its bytes come from and go to
};

// entry points that touch a map on the MAIN stream call this first
int grid_on_main(slam_ctx *c)
{
    if (int rc = join_particles(c)) return rc;
    if (!c->pipeline) return SLAM_OK;
    c->mgrid = true;
    return join_from_grid(c);
}

// entry points that take NO map and enqueue on the MAIN stream call this first: their device arguments may be results of
// the pipelined stages (poses_out, pmap_dev) or buffers those stages still read.  The map stream waits for the pose
// stream, so joining it joins both; no map work is marked (the map stream need not fork again).  Pipeline off, no chunked
// particle batch in flight: two flag tests.
int streams_on_main(slam_ctx *c) { return join_from_grid(c); }

int status_to_code(int st)
{
    if (st & kStatusGuard) return fail(SLAM_ERR_HIP, "internal: a kernel wrote past its LDS regions (SLAM_LDS_GUARD build)");
    if (st & kStatusNaN) return fail(SLAM_ERR_NAN, "cannot convert float NaN to integer (mapping.py:33-36)");
    if (st & kStatusOverflow)
        return fail(SLAM_ERR_OVERFLOW, "cannot convert float infinity to integer / cell index beyond 2^20 (mapping.py:33-36)");
    return SLAM_OK;
}

int check_status_sync(slam_ctx *c)
{
    int st = 0;
    if (int rc = join_from_grid(c)) return rc;
    HIPCHK(hipMemcpyAsync(&st, c->status, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (st) {
        HIPCHK(hipMemsetAsync(c->status, 0, sizeof(int), c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return status_to_code(st);
}

#define D2H(dst, src, bytes) HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream))

// ---- DWA local planner -------------------------------------------------------------------
// Config checks and launch shape shared by the DWA entry points (slam_dwa_shape documents them).
constexpr int kDwaMaxRows = 65536;
constexpr long kDwaMaxSamples = 1L << 20;

// Bound of np.arange(lo, hi, reso) over every state: lo >= spec_lo, hi <= spec_hi and
// hi - lo <= 2 * accel * dt up to rounding (calc_dynamic_window, dwa.py:65-83).
long dwa_axis_cap(double spec_lo, double spec_hi, double accel_dt, double reso)
{
    double width = std::fmin(spec_hi - spec_lo, 2.0 * accel_dt);
    if (!(width > 0.0)) return 0;
    double n = std::ceil(width / reso) + 2.0;
    return n > (double)kDwaMaxSamples ? kDwaMaxSamples + 1 : (long)n;
}

int dwa_config(const double *config, DwaConfig *cfg, int *rows, int *nv_cap, int *nw_cap)
{
    if (!config) return fail(SLAM_ERR_INVALID, "slam_dwa: config is null");
    for (int i = 0; i < SLAM_DWA_CONFIG_LEN; ++i)
        if (!std::isfinite(config[i])) return fail(SLAM_ERR_INVALID, "slam_dwa: config[%d] is not finite", i);
    DwaConfig c;
    static_assert(sizeof(DwaConfig) == SLAM_DWA_CONFIG_LEN * sizeof(double), "config layout");
    memcpy(&c, config, sizeof c);
    if (!(c.dt > 0.0) || !(c.v_reso > 0.0) || !(c.yawrate_reso > 0.0))
        return fail(SLAM_ERR_INVALID, "slam_dwa: dt, v_reso and yawrate_reso must be > 0");
    if (c.robot_type != 0.0 && c.robot_type != 1.0) return fail(SLAM_ERR_INVALID, "slam_dwa: robot_type must be 0 or 1");
    // predict_trajectory's loop (dwa.py:118-122), time accumulated in float64
    int steps = 0;
    for (double t = 0.0; t <= c.predict_time; t += c.dt)
        if (++steps >= kDwaMaxRows) return fail(SLAM_ERR_INVALID, "slam_dwa: more than %d trajectory rows", kDwaMaxRows);
    if (steps == 0) return fail(SLAM_ERR_INVALID, "slam_dwa: predict_time < 0 leaves no trajectory step");
    long nv = dwa_axis_cap(c.min_speed, c.max_speed, c.max_accel * c.dt, c.v_reso);
    long nw = dwa_axis_cap(-c.max_yawrate, c.max_yawrate, c.max_dyawrate * c.dt, c.yawrate_reso);
    if (nv * nw > kDwaMaxSamples) return fail(SLAM_ERR_INVALID, "slam_dwa: window of up to %ld x %ld samples (> 2^20)", nv, nw);
    if (cfg) *cfg = c;
    *rows = steps + 1;
    *nv_cap = (int)nv;
    *nw_cap = (int)nw;
    return SLAM_OK;
}

struct DwaOut {
    double *u, *cost;
    int32_t *index, *counts;
    double *costs;
    int s_cap;
    double *traj;
};

// Checks of every DWA entry point; fills the config and launch shape of `a`.
int check_dwa(const char *fn, const double *states, const double *goals, const double *config, int B, const DwaOut &o, DwaArgs &a)
{
    REQUIRE_IN(fn, states && goals && o.u && o.cost && o.index, "null pointer");
    REQUIRE_IN(fn, B > 0, "B must be > 0");
    REQUIRE_IN(fn, !o.costs || o.s_cap > 0, "costs_out needs s_cap > 0");
    return dwa_config(config, &a.cfg, &a.rows, &a.nv_cap, &a.nw_cap);
}

int dwa_launch(slam_ctx *c, DwaArgs &a, const DwaOut &o)
{
    a.u_out = o.u;
    a.cost_out = o.cost;
    a.index_out = o.index;
    a.counts_out = o.counts;
    a.costs_out = o.costs;
    a.s_cap = o.s_cap;
    a.traj_out = o.traj;
    a.status = c->status;
    HIPCHK(launch_dwa(a, c->stream));
    return SLAM_OK;
}

// ---- A* global planner -------------------------------------------------------------------
// Checks shared by the A* entry points (include/slam_hip.h documents them).
int check_astar_maps(const char *fn, const int8_t *maps, int G, int H, int W, int span, int r)
{
    REQUIRE_IN(fn, maps, "null pointer");
    REQUIRE_IN(fn, G > 0 && H > 0 && W > 0, "G, H and W must be > 0");
    REQUIRE_IN(fn, (long)H * W < (1L << 31), "H * W must be < 2^31");
    REQUIRE_IN(fn, H <= W, "H > W (find_path's state_map is W x W, global_planner.py:136)");
    REQUIRE_IN(fn, r >= 0, "r must be >= 0");
    REQUIRE_IN(fn, span >= 0 && span <= H, "span must be in [0, min(H, W)] (the inflation loop indexes past the map, global_planner.py:150-155)");
    REQUIRE_IN(fn, span <= kAstarMaxSpan, "span must be <= 4096");
    return SLAM_OK;
}

int check_astar(const char *fn, const int8_t *maps, int G, int H, int W, int span, int r, const int32_t *starts,
                const int32_t *goals, const int32_t *map_of_query, int B, int path_cap, const int32_t *status,
                const int32_t *path_len, const int32_t *path, const int32_t *expansions)
{
    TRY(check_astar_maps(fn, maps, G, H, W, span, r));
    REQUIRE_IN(fn, starts && goals && status && path_len && expansions, "null pointer");
    REQUIRE_IN(fn, B > 0, "B must be > 0");
    REQUIRE_IN(fn, path_cap >= 0 && (path_cap == 0 || path), "path_cap must be >= 0, path_out non-null when it is > 0");
    REQUIRE_IN(fn, map_of_query || G == 1 || G == B, "map_of_query is NULL but G is neither 1 nor B");
    return SLAM_OK;
}

// Inflation of G maps into `inflated` and, when `a` is non-null, the search of its queries over them.  The
// workspace (trigger rows, the inflated maps when the caller keeps none, the search slots) is the scratch arena.
int astar_run(slam_ctx *c, const int8_t *maps, int G, int H, int W, int wire, int span, int r, int8_t *inflated,
              AstarArgs *a)
{
    TRY(grid_on_main(c));
    const size_t cells = (size_t)H * W;
    const size_t dil_words = (size_t)G * span * ((span + 63) / 64);     // trigger rows: G x span rows of 64-column words
    long slots = 0;
    if (a) {
        slots = a->B < kAstarMaxSlots ? a->B : kAstarMaxSlots;
        const long fit = (long)(kAstarSlotBudget / (cells * kAstarSlotBytesPerCell));
        if (slots > fit) slots = fit > 0 ? fit : 1;
    }
    const size_t sc = (size_t)slots * cells;
    unsigned long long *d_dil;
    Layout ws;
    ws.add(d_dil, dil_words);
    if (!inflated) ws.add(inflated, (size_t)G * cells);
    if (a) ws.add(a->state, sc).add(a->pos, sc).add(a->ocell, sc).add(a->og, sc).add(a->closed, sc).add(a->okey, sc);
    TRY(reserve(c, c->scratch, ws));
    HIPCHK(launch_astar_inflate(maps, G, H, W, wire, span, r, d_dil, inflated, c->status, c->stream));
    if (!a) return SLAM_OK;
    a->imaps = inflated;
    a->slots = (int)slots;
    HIPCHK(hipMemsetAsync(a->state, 0, sc, c->stream));
    HIPCHK(launch_astar(*a, c->stream));
    return SLAM_OK;
}

}  // namespace

extern "C" {

int slam_abi_version(void) { return SLAM_ABI_VERSION; }

const char *slam_last_error(void) { return g_err.c_str(); }

int slam_create(int device, void *stream, slam_ctx **out)
{
    if (!out) return fail(SLAM_ERR_INVALID, "slam_create: out is null");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(SLAM_ERR_NODEVICE, "no HIP device visible (%s); this library has no CPU path",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device < 0 || device >= ndev) return fail(SLAM_ERR_INVALID, "device %d out of range [0,%d)", device, ndev);
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(SLAM_ERR_NODEVICE, "device %d is %s; libslamhip is built for gfx950 (MI355X) only", device,
                    prop.gcnArchName);
    slam_ctx *c = new slam_ctx();
    c->device = device;
    if (stream) {
        c->stream = static_cast<hipStream_t>(stream);
    } else {
        e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            delete c;
            return fail(SLAM_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
        }
        c->own_stream = true;
    }
#ifdef SLAM_STAMPS
    const size_t status_bytes = 256 + (size_t)kStampRecords * 32;   // diagnostic build: per-workgroup phase records behind the status block
#else
    const size_t status_bytes = 256;
#endif
    e = hipMalloc(reinterpret_cast<void **>(&c->status), status_bytes);
    if (e == hipSuccess) e = hipMemsetAsync(c->status, 0, status_bytes, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        delete c;
        return fail(SLAM_ERR_HIP, "context init: %s", hipGetErrorString(e));
    }
    *out = c;
    return SLAM_OK;
}

int slam_destroy(slam_ctx *c)
{
    if (!c) return SLAM_OK;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->pstream) {
        (void)hipStreamSynchronize(c->pstream);
        (void)hipStreamDestroy(c->pstream);
        for (hipEvent_t e : c->pev_pose) (void)hipEventDestroy(e);
        for (hipEvent_t e : c->pev_cast) (void)hipEventDestroy(e);
        if (c->pev_join) (void)hipEventDestroy(c->pev_join);
    }
    if (c->gstream) {
        (void)hipStreamSynchronize(c->cstream);
        (void)hipStreamSynchronize(c->gstream);
        (void)hipStreamDestroy(c->cstream);
        (void)hipStreamDestroy(c->gstream);
        for (hipEvent_t e : {c->ev_fork, c->ev_join, c->ev_icp, c->ev_pose, c->ev_cast[0], c->ev_cast[1]})
            if (e) (void)hipEventDestroy(e);
        for (double *t : c->pipe_T)
            if (t) (void)hipFree(t);
    }
    if (c->ev_order) (void)hipEventDestroy(c->ev_order);
    for (auto &p : c->pending) { (void)hipEventDestroy(p.e0); (void)hipEventDestroy(p.e1); }
    for (auto e : c->pool) (void)hipEventDestroy(e);
    if (c->staging.base) (void)hipFree(c->staging.base);
    if (c->scratch.base) (void)hipFree(c->scratch.base);
    if (c->tiles.base) (void)hipFree(c->tiles.base);
    if (c->pinned) (void)hipHostFree(c->pinned);
    if (c->status) (void)hipFree(c->status);
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return SLAM_OK;
}

int slam_synchronize(slam_ctx *c)
{
    TRY(use(c));
    TRY(join_from_grid(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SLAM_OK;
}

int slam_stream_order(slam_ctx *c, void *stream, int direction)
{
    TRY(use(c));
    REQUIRE(direction == 0 || direction == 1, "direction is 0 (the stream waits for the context) or 1 (the context waits for the stream)");
    hipStream_t other = static_cast<hipStream_t>(stream);
    if (!c->ev_order) HIPCHK(hipEventCreateWithFlags(&c->ev_order, hipEventDisableTiming));
    if (direction == 0) {
        TRY(join_from_grid(c));                    // the map / pose / particle streams into the context's stream first
        if (other == c->stream) return SLAM_OK;
        HIPCHK(hipEventRecord(c->ev_order, c->stream));
        HIPCHK(hipStreamWaitEvent(other, c->ev_order, 0));
        return SLAM_OK;
    }
    if (other != c->stream) {
        HIPCHK(hipEventRecord(c->ev_order, other));
        HIPCHK(hipStreamWaitEvent(c->stream, c->ev_order, 0));
    }
    // with the "pipeline" option the map stage runs on a stream of its own: it forks from the context's stream again before
    // its next piece of work (as after any map work on the context's stream)
    if (c->pipeline) {
        TRY(join_from_grid(c));
        c->mgrid = true;
    }
    return SLAM_OK;
}

int slam_check_status(slam_ctx *c)
{
    TRY(use(c));
    return check_status_sync(c);
}

// The options' names, the values each takes and the words that say so.  slam_set_option checks name and value against
// this table before it touches the context: a caller's mistake is named as such whatever the state of the device.
struct OptionRange {
    const char *name;
    bool (*ok)(double);
    const char *msg;
};
static const OptionRange kOptionRanges[] = {
    {"grid_mode", [](double v) { return v == 0 || v == 1 || v == 2 || v == 3 || v == 4; }, "grid_mode is 0..4"},
    {"grid_group", [](double v) { return v >= 0 && v <= 64; }, "grid_group in [0, 64]"},
    {"grid_split", [](double v) { return v == -1 || v == 0 || v == 1; }, "grid_split is -1, 0 or 1"},
    {"replay_reset", [](double v) { return v == 0 || v == 1; }, "replay_reset is 0 or 1"},
    {"icp_team", [](double v) { return v == 0 || v == 1; }, "icp_team is 0 or 1"},
    {"icp_one_wave", [](double v) { return v == -1 || v == 0 || v == 1; }, "icp_one_wave is -1, 0 or 1"},
    {"icp_f32_filter", [](double v) { return v == -1 || v == 0 || v == 1; }, "icp_f32_filter is -1, 0 or 1"},
    {"win_lds_hits", [](double v) { return v == -1 || v == 0 || v == 1; }, "win_lds_hits is -1, 0 or 1"},
    {"particle_chunks", [](double v) { return v >= 0 && v <= 64 && v == (int)v; }, "particle_chunks in [0, 64]"},
    {"icp_qpt", [](double v) { return v >= 0 && v <= 3; }, "icp_qpt in [0, 3]"},
    {"pipeline", [](double v) { return v == 0 || v == 1; }, "pipeline is 0 or 1"},
    {"raycast_lds", [](double v) { return v == -1 || v == 0 || v == 1; }, "raycast_lds is -1, 0 or 1"},
    {"mcl_shape", [](double v) { return v == -1 || v == 0 || v == 1; }, "mcl_shape is -1, 0 or 1"},
    {"locate_ws_mb", [](double v) { return v > 0 && v <= 1048576; }, "locate_ws_mb in (0, 1048576]"},
    {"frontier_ws_mb", [](double v) { return v > 0 && v <= 1048576; }, "frontier_ws_mb in (0, 1048576]"},
    {"travel_ws_mb", [](double v) { return v > 0 && v <= 1048576; }, "travel_ws_mb in (0, 1048576]"},
    {"gain_lds", [](double v) { return v == -1 || v == 0 || v == 1; }, "gain_lds is -1, 0 or 1"},
    {"gain_ws_mb", [](double v) { return v > 0 && v <= 1048576; }, "gain_ws_mb in (0, 1048576]"},
};

int slam_set_option(slam_ctx *c, const char *name, double value)
{
    REQUIRE(name, "null name");
    const OptionRange *opt = nullptr;
    for (const OptionRange &o : kOptionRanges)
        if (!strcmp(name, o.name)) opt = &o;
    if (!opt) return fail(SLAM_ERR_INVALID, "unknown option %s", name);
    REQUIRE(opt->ok(value), opt->msg);
    TRY(use(c));
    if (!strcmp(name, "grid_mode")) c->grid_mode = (int)value;
    else if (!strcmp(name, "grid_group")) c->grid_group = (int)value;
    else if (!strcmp(name, "grid_split")) c->grid_split = (int)value;
    else if (!strcmp(name, "replay_reset")) c->replay_reset = (int)value;
    else if (!strcmp(name, "icp_team")) c->icp_team = (int)value;
    else if (!strcmp(name, "icp_one_wave")) c->icp_one_wave = (int)value;
    else if (!strcmp(name, "icp_f32_filter")) c->icp_f32_filter = (int)value;
    else if (!strcmp(name, "win_lds_hits")) c->win_lds_hits = (int)value;
    else if (!strcmp(name, "particle_chunks")) { TRY(join_particles(c)); c->particle_chunks = (int)value; }
    else if (!strcmp(name, "icp_qpt")) c->icp_qpt = (int)value;
    else if (!strcmp(name, "raycast_lds")) c->raycast_lds = (int)value;
    else if (!strcmp(name, "mcl_shape")) c->mcl_shape = (int)value;
    else if (!strcmp(name, "locate_ws_mb")) c->locate_ws_bytes = (long)(value * 1048576.0);
    else if (!strcmp(name, "frontier_ws_mb")) c->frontier_ws_bytes = (long)(value * 1048576.0);
    else if (!strcmp(name, "travel_ws_mb")) c->travel_ws_bytes = (long)(value * 1048576.0);
    else if (!strcmp(name, "gain_lds")) c->gain_lds = (int)value;
    else if (!strcmp(name, "gain_ws_mb")) c->gain_ws_bytes = (long)(value * 1048576.0);
    else if (!strcmp(name, "pipeline")) {
        TRY(join_from_grid(c));
        if (value == 1 && !c->gstream) {
            HIPCHK(hipStreamCreateWithFlags(&c->gstream, hipStreamNonBlocking));
            HIPCHK(hipStreamCreateWithFlags(&c->cstream, hipStreamNonBlocking));
            for (hipEvent_t *e : {&c->ev_fork, &c->ev_join, &c->ev_icp, &c->ev_pose, &c->ev_cast[0], &c->ev_cast[1]})
                HIPCHK(hipEventCreateWithFlags(e, hipEventDisableTiming));
        }
        if (value == 0 && c->pipeline) HIPCHK(hipStreamSynchronize(c->gstream));
        c->pipeline = (int)value;
        c->cast_poses[0] = c->cast_poses[1] = nullptr;
        c->cast_T[0] = c->cast_T[1] = nullptr;
    }
    return SLAM_OK;
}

int slam_timing_enable(slam_ctx *c, int on)
{
    TRY(use(c));
    TRY(join_from_grid(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (auto &p : c->pending) { c->pool.push_back(p.e0); c->pool.push_back(p.e1); }
    c->pending.clear();
    for (int k = 0; k < SLAM_K_COUNT; ++k) { c->ms[k] = 0; c->launches[k] = 0; }
    c->timing = on != 0;
    c->timing_mask = on > 1 ? (unsigned)on >> 1 : ~0u;   // on = 1: every family; on = 2 * mask: the families in mask (bit SLAM_K_*)
    return SLAM_OK;
}

int slam_timing_read(slam_ctx *c, double ms_out[SLAM_K_COUNT], int64_t launches_out[SLAM_K_COUNT])
{
    TRY(use(c));
    TRY(join_from_grid(c));                 // (timed launches on the map / particle streams)
    HIPCHK(hipStreamSynchronize(c->stream));
    for (auto &p : c->pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.e0, p.e1) == hipSuccess) {
            c->ms[p.kind] += ms;
            c->launches[p.kind] += p.first ? 1 : 0;
        }
        c->pool.push_back(p.e0);
        c->pool.push_back(p.e1);
    }
    c->pending.clear();
    for (int k = 0; k < SLAM_K_COUNT; ++k) {
        if (ms_out) ms_out[k] = c->ms[k];
        if (launches_out) launches_out[k] = c->launches[k];
        c->ms[k] = 0;
        c->launches[k] = 0;
    }
    return SLAM_OK;
}

/* ---- introspection of the launch decisions (launch_shapes.h): no context, no device call ---- */

static int sat_int(long v) { return v > INT_MAX ? INT_MAX : (int)v; }

int slam_plan_win(int L, int scans, int n, int group, int has_got, int pmap_live, int maps_are_private, int hit_levels, int xw,
                  int yw, int has_redo, int split_pref, int hits_pref, int cus, int lds_per_cu, int guard, slam_win_plan *out)
{
    if (!out) return fail(SLAM_ERR_INVALID, "slam_plan_win: out is null");
    if (L < 1 || scans < 1 || n < 1 || group < 1 || xw < 1 || yw < 1 || cus < 1 || lds_per_cu < 1)
        return fail(SLAM_ERR_INVALID, "slam_plan_win: L, scans, n, group, xw, yw, cus and lds_per_cu must be positive");
    WinRequest r{L, scans, n, group, has_got != 0, pmap_live != 0, maps_are_private != 0, hit_levels, xw, yw, has_redo != 0,
                 split_pref, hits_pref, cus, (long)lds_per_cu, guard < 0 ? kLdsGuard : guard};
    const WinShape p = plan_win(r);
    *out = slam_win_plan{p.form, p.grid_x, p.grid_y, p.threads, (int)p.lds, (int)p.lds_attr, p.exclusive, p.sort_cap, p.win_cells,
                         p.split, p.lds_hits, p.two_per_cu, sat_int(p.wgs), p.own8_lds, p.own8_win, p.redo_grid, p.live_dirty ? 1 : 0};
    return SLAM_OK;
}

int slam_plan_icp(int B, int n_src, int n_tar, int is_scan, int qpt_pref, int batch_invariant, int one_wave, int f32_filter,
                  int team_mode, int guard, slam_icp_plan *out)
{
    if (!out) return fail(SLAM_ERR_INVALID, "slam_plan_icp: out is null");
    if (B < 1 || n_src < 1 || n_tar < 1) return fail(SLAM_ERR_INVALID, "slam_plan_icp: B, n_src and n_tar must be positive");
    IcpRequest r{B, n_src, n_tar, is_scan != 0, qpt_pref, batch_invariant, one_wave, f32_filter, team_mode, guard < 0 ? kLdsGuard : guard};
    const IcpShape p = plan_icp(r);
    *out = slam_icp_plan{p.form, p.pref, p.preferred, p.qpt, p.unroll, p.block, sat_int((long)p.lds), p.polar_copy, p.team_cap,
                         p.cap_wanted, p.raise_attr ? 1 : 0, sat_int((long)p.nn_bytes)};
    return SLAM_OK;
}

int slam_plan_win_phases(const int32_t bbox[4], const int32_t origins[4], int xw, int yw, int ymask, int win_cells, int sorted,
                         int half, slam_win_phases *out)
{
    if (!bbox || !origins || !out) return fail(SLAM_ERR_INVALID, "slam_plan_win_phases: null pointer");
    if (xw < 1 || yw < 1 || half < -1 || half > 1) return fail(SLAM_ERR_INVALID, "slam_plan_win_phases: xw, yw must be positive, half -1, 0 or 1");
    int qbox[4][4];
    for (auto &q : qbox) { q[0] = q[1] = INT_MAX; q[2] = q[3] = INT_MIN; }
    if (bbox[0] <= bbox[2]) quadrant_boxes(bbox, origins[0], origins[1], origins[2], origins[3], qbox);
    auto fits = [&](unsigned mask) -> bool { int o[4]; return !box_of(qbox, mask, xw, yw, ymask, o) || box_fits(o, win_cells); };
    unsigned part[4] = {0u, 0u, 0u, 0u};
    slam_win_phases p{};
    p.nph = 1;
    pick_parts(half >= 0, half, sorted != 0, fits, part, p.nph, p.parity);
    for (int ph = 0; ph < p.nph; ++ph) {
        p.part[ph] = (int)part[ph];
        p.any[ph] = box_of(qbox, part[ph], xw, yw, ymask, p.box[ph]) ? 1 : 0;
        p.fits[ph] = fits(part[ph]) ? 1 : 0;
    }
    *out = p;
    return SLAM_OK;
}

static LocateShape locate_plan_for(int ni, int nj, int H, long pairs, long ws_bytes, int guard)
{
    LocateRequest r;
    r.pairs = pairs; r.n = 1; r.ni = ni; r.nj = nj; r.H = H; r.ws_bytes = ws_bytes; r.guard = guard;
    return plan_locate(r);
}

// pairs per chunk for a budget and a pair's worst-case bytes, as plan_locate cuts them (0: one pair does not fit)
static int64_t locate_plan_chunk(long ws_bytes, long pair_bytes, long pairs)
{
    if (pairs < 1 || pair_bytes < 0) return 0;
    return pair_bytes ? std::min(pairs, ws_bytes / pair_bytes) : pairs;
}

static FrontierShape frontier_plan_for(int xw, int yw, int radius, long B, long ws_bytes, int guard)
{
    FrontierRequest r;
    r.B = B; r.xw = xw; r.yw = yw; r.radius = radius; r.ws_bytes = ws_bytes; r.guard = guard;
    return plan_frontiers(r);
}

static TravelShape travel_plan_for(int xw, int yw, bool own_costs, long B, long ws_bytes, int guard)
{
    TravelRequest r;
    r.B = B; r.xw = xw; r.yw = yw; r.own_costs = own_costs; r.ws_bytes = ws_bytes; r.guard = guard;
    return plan_travel(r);
}
// a budget of `kib` KiB, queries of `bytes` bytes, B of them, as plan_travel cuts them: the queries of a chunk (chunks:
// their number); 0 when one query does not fit
static int64_t travel_plan_chunk(long kib, long bytes, long B, bool chunks)
{
    if (bytes <= 0 || B < 1) return 0;
    const long per = std::min(B, kib * 1024 / bytes);
    if (per < 1) return 0;
    return chunks ? (B + per - 1) / per : per;
}

// the view gain's plan for a map of xw x yw, B views and a box of `rows` rows of `words` words (0: the whole map)
static ViewShape view_plan_for(int xw, int yw, int rows, int words, int lds_mode, long B, long ws_bytes, int guard)
{
    ViewRequest r;
    r.B = B; r.xw = xw; r.yw = yw; r.box_rows = rows; r.box_words = words; r.lds_mode = lds_mode; r.ws_bytes = ws_bytes; r.guard = guard;
    return plan_view(r);
}
// a box of a rows x b words on a map large enough to hold it
static ViewShape view_box_plan(int a, int b, int mode, int guard)
{
    return view_plan_for(std::max(a, 1), 32 * std::max(b, 1), a, b, mode, 1, 1L << 40, guard);
}
// a budget of `kib` KiB, slots of `bytes` bytes (a multiple of 4), B views, as plan_view cuts them (global engine)
static int64_t view_plan_chunk(long kib, long bytes, long B, bool chunks)
{
    if (bytes < 4 || B < 1) return 0;
    const ViewShape p = view_plan_for((int)(bytes / 4), 1, 0, 0, 0, B, kib * 1024, 0);
    return !p.ok ? 0 : chunks ? p.chunks : p.chunk_views;
}

int slam_plan_query(const char *name, int a, int b, int c, int guard, int64_t *out)
{
    if (!name || !out) return fail(SLAM_ERR_INVALID, "slam_plan_query: null pointer");
    const int g = guard < 0 ? kLdsGuard : guard;
    struct Entry { const char *name; int64_t value; };
    const Entry table[] = {
        {"kLdsGuard", kLdsGuard}, {"kLdsPerCu", (int64_t)kLdsPerCu}, {"kLdsDefault", (int64_t)kLdsDefault}, {"kChipCus", kChipCus},
        {"kWave", kWave}, {"kMaxWaves", kMaxWaves}, {"kScanConstBytes", (int64_t)kScanConstBytes}, {"kDouble2Bytes", (int64_t)kDouble2Bytes},
        {"kBoxBytes", (int64_t)kBoxBytes}, {"kListSlotBytes", (int64_t)kListSlotBytes},
        {"kWinCells", kWinCells}, {"kWinMaxGroup", kWinMaxGroup}, {"kSortBins", kSortBins}, {"kMaxSortRays", kMaxSortRays},
        {"kRaysPerLane", kRaysPerLane}, {"kWinBoxInts", kWinBoxInts}, {"kWinHalfSlack", kWinHalfSlack}, {"kWinTwoFloor", kWinTwoFloor},
        {"kWinMinThreads", kWinMinThreads}, {"kOwnerThreads", kOwnerThreads}, {"kOwnerMaxRays", kOwnerMaxRays}, {"kOwn8Threads", kOwn8Threads},
        {"kOwn8LdsBytes", kOwn8LdsBytes},
        {"kNNBlock", kNNBlock}, {"kNNStride", kNNStride}, {"kPolarTail", kPolarTail}, {"kRedStride", kRedStride},
        {"kIcpExtraLds", kIcpExtraLds}, {"kWaveQpt", kWaveQpt}, {"kWaveRound", kWaveRound}, {"kIcpFullChipWaves", kIcpFullChipWaves},
        {"win_sc_bytes", (int64_t)win_sc_bytes(a)}, {"win_sort_cap", win_sort_cap(a)}, {"win_lds_bytes", (int64_t)win_lds_bytes(a, b, c, g)},
        {"win_cells_for", win_cells_for(a, b, c != 0, (long)kLdsPerCu, g)}, {"win_lds_max", (int64_t)win_lds_max(g)},
        {"own8_fixed_bytes", (int64_t)own8_fixed_bytes(a)},
        {"nn_blocks", nn_blocks(a)}, {"nn_boxes_padded", nn_boxes_padded(a)}, {"nn_boxes4", nn_boxes4(a)}, {"nn_lds_bytes", (int64_t)nn_lds_bytes(a)},
        {"icp_polar_bytes", (int64_t)icp_polar_bytes(a)}, {"icp_red_bytes", (int64_t)icp_red_bytes(a)},
        {"icp_wave_lds_bytes", (int64_t)icp_wave_lds_bytes(a, b, c != 0)}, {"icp_block", b > 0 ? icp_block(a, b) : 0},
        // slam_grid_copy_maps: a = xw, b = yw, c = count
        {"kCopyThreads", kCopyThreads}, {"kCopyChunkCells", kCopyChunkCells}, {"kCopyMaxGroups", (int64_t)kCopyMaxGroups},
        {"copy_chunks", (int64_t)plan_copy_maps((long)a * b, c).chunks}, {"copy_groups", (int64_t)plan_copy_maps((long)a * b, c).groups},
        {"copy_grid", (int64_t)plan_copy_maps((long)a * b, c).grid}, {"copy_threads", plan_copy_maps((long)a * b, c).threads},
        // slam_grid_locate: a = ni, b = nj, c = level (locate_level_nodes) or levels (locate_pair_bytes, locate_tile*: the top level's
        // nodes per workgroup and workgroups per pair); locate_dense_lds: a = n; locate_dense_threads: a = nodes;
        // locate_table_bytes: a = n; locate_chunk_pairs: a = the budget in KiB, b = locate_pair_bytes + locate_table_bytes, c = pairs
        {"kLocateMaxLevels", kLocateMaxLevels}, {"kLocateMaxBeams", kLocateMaxBeams}, {"kLocateThreads", kLocateThreads},
        {"kLocateTileRounds", kLocateTileRounds}, {"kLocateNodeBytes", (int64_t)kLocateNodeBytes}, {"kLocateSweepBlocks", kLocateSweepBlocks},
        {"locate_level_nodes", (c >= 0 && c <= kLocateMaxLevels) ? locate_level_nodes(a, b, c) : 0},
        {"locate_pair_bytes", (c >= 0 && c <= kLocateMaxLevels) ? locate_pair_bytes(a, b, c) : 0},
        {"locate_table_bytes", locate_table_bytes(a)}, {"locate_dense_lds", (int64_t)locate_dense_lds(a, g)}, {"locate_dense_threads", locate_dense_threads(a)},
        {"locate_tile", locate_plan_for(a, b, c, 1, 1L << 40, g).tile}, {"locate_tiles", locate_plan_for(a, b, c, 1, 1L << 40, g).tiles},
        {"locate_chunk_pairs", locate_plan_chunk((long)a * 1024, b, c)},
        // slam_grid_frontiers: a = xw, b = yw (frontier_tiles*, frontier_border, frontier_segs, frontier_query_bytes); frontier_lds:
        // a = radius; frontier_chunk_queries: a = the budget in KiB, b = frontier_query_bytes, c = B, as plan_frontiers cuts them
        {"kFrontierTileX", kFrontierTileX}, {"kFrontierTileY", kFrontierTileY}, {"kFrontierThreads", kFrontierThreads},
        {"kFrontierSeg", kFrontierSeg}, {"kFrontierMaxRadius", kFrontierMaxRadius}, {"kFrontierMaxClusters", kFrontierMaxClusters},
        {"frontier_tiles_x", frontier_plan_for(a, b, 0, 1, 1L << 40, g).tiles_x}, {"frontier_tiles_y", frontier_plan_for(a, b, 0, 1, 1L << 40, g).tiles_y},
        {"frontier_tiles", frontier_plan_for(a, b, 0, 1, 1L << 40, g).tiles}, {"frontier_border", frontier_plan_for(a, b, 0, 1, 1L << 40, g).border},
        {"frontier_segs", frontier_plan_for(a, b, 0, 1, 1L << 40, g).segs}, {"frontier_query_bytes", frontier_plan_for(a, b, 0, 1, 1L << 40, g).query_bytes},
        {"frontier_lds", (a >= 0 && a <= kFrontierMaxRadius) ? (int64_t)frontier_lds_bytes(a, g) : 0},
        {"frontier_chunk_queries", (b > 0 && c >= 1) ? std::min((int64_t)c, (int64_t)a * 1024 / b) : 0},
        // slam_grid_travel: a = xw, b = yw (travel_tiles*, travel_mask_words, travel_trips; travel_query_bytes: c != 0 = the costs
        // live in the workspace); travel_chunk_queries / travel_chunks: a = the budget in KiB, b = travel_query_bytes, c = B
        {"kTravelTile", kTravelTile}, {"kTravelMaxBlocks", (int64_t)kTravelMaxBlocks}, {"kTravelThreads", kTravelThreads}, {"kTravelTripsPerTile", kTravelTripsPerTile},
        {"kTravelMaxSources", kTravelMaxSources}, {"kTravelMaxFoot", kTravelMaxFoot}, {"kTravelMaxGoals", kTravelMaxGoals},
        {"travel_tiles_x", travel_plan_for(a, b, true, 1, 1L << 40, g).tiles_x}, {"travel_tiles_y", travel_plan_for(a, b, true, 1, 1L << 40, g).tiles_y},
        {"travel_tiles", travel_plan_for(a, b, true, 1, 1L << 40, g).tiles}, {"travel_mask_words", travel_plan_for(a, b, true, 1, 1L << 40, g).mask_words},
        {"travel_trips", travel_plan_for(a, b, true, 1, 1L << 40, g).trips},
        {"travel_query_bytes", travel_plan_for(a, b, c != 0, 1, 1L << 40, g).query_bytes}, {"travel_lds", (int64_t)travel_lds_bytes(g)},
        {"travel_chunk_queries", travel_plan_chunk(a, b, c, false)}, {"travel_chunks", travel_plan_chunk(a, b, c, true)},
        // slam_grid_view_gain: view_row_words: a = yw; view_bytes: a = xw, b = yw (a global slot, and seen_out, of one view);
        // view_window_words, view_lds_bytes, view_engine (1 = LDS, 0 = global): a box of a rows x b words, c = "gain_lds";
        // view_chunk_views / view_chunks: a = the budget in KiB, b = view_bytes, c = B, as plan_view cuts them
        {"kViewLdsBytes", (int64_t)kViewLdsBytes}, {"kViewThreads", kViewThreads}, {"kViewMaxBlocks", (int64_t)kViewMaxBlocks},
        {"view_row_words", view_plan_for(1, std::max(a, 1), 0, 0, -1, 1, 1L << 40, g).row_words},
        {"view_bytes", view_plan_for(std::max(a, 1), std::max(b, 1), 0, 0, -1, 1, 1L << 40, g).view_bytes},
        {"view_window_words", view_box_plan(a, b, c, g).window_words}, {"view_lds_bytes", view_box_plan(a, b, c, g).lds_bytes},
        {"view_engine", view_box_plan(a, b, c, g).engine_lds ? 1 : 0},
        {"view_chunk_views", view_plan_chunk(a, b, c, false)}, {"view_chunks", view_plan_chunk(a, b, c, true)},
        // slam_grid_refine: a = B.  "refine": the workgroups of its launch; refine_blocks: those the batch needs; refine_pass:
        // the hypotheses one sweep of the launch takes; refine_cap: the most a launch takes in one sweep, whatever B
        {"kRefineWaves", kRefineWaves}, {"kRefineThreads", kRefineThreads}, {"kRefineMaxBlocks", (int64_t)kRefineMaxBlocks},
        {"refine", (int64_t)plan_refine(a).grid}, {"refine_blocks", (int64_t)plan_refine(a).blocks},
        {"refine_pass", (int64_t)plan_refine(a).pass}, {"refine_cap", (int64_t)(kRefineMaxBlocks * kRefineWaves)},
        // slam_track: a = L.  track_rows: the workgroups of its predict step (one per trajectory); track_lanes: those of its seed
        // and decide steps (one lane per trajectory)
        {"kTrackRowThreads", kTrackRowThreads}, {"kTrackThreads", kTrackThreads}, {"kTrackMaxBlocks", (int64_t)kTrackMaxBlocks},
        {"track_rows", (int64_t)plan_track(a).row_grid}, {"track_lanes", (int64_t)plan_track(a).lane_grid},
        // the ray casts of large maps: a = scans of the cast (L * scans), b = beams, c = groups: where the engine's layout ends
        {"wedge_ws_bytes", (int64_t)cast_layout_bytes(CastPath::Wedges, (long)a * b, a, c)},
        {"tile_ws_bytes", (int64_t)cast_layout_bytes(CastPath::Tiles, (long)a * b, a, c)},
        // slam_grid_create: a = G, b = xw, c = yw: the bytes of the grid object's state, which a reset (slam_grid_reset, option
        // "replay_reset") clears - pass and hit counters of every map and the visit slots
        {"grid_state_bytes", (a > 0 && b > 0 && c > 0) ? (int64_t)grid_state_bytes((size_t)a * b * c) : 0},
    };
    for (const Entry &e : table)
        if (!strcmp(e.name, name)) { *out = e.value; return SLAM_OK; }
    return fail(SLAM_ERR_INVALID, "slam_plan_query: unknown name");
}

#if defined(SLAM_STAMPS) || defined(SLAM_STAMPS_ICP)
/* diagnostic builds only: the 256-byte status block (word 0: status bits; from word 8: phase counters) */
int slam_debug_read(slam_ctx *c, void *out256, int clear)
{
    TRY(use(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(out256, c->status, 256, hipMemcpyDeviceToHost));
    if (clear) HIPCHK(hipMemset(reinterpret_cast<char *>(c->status) + 32, 0, 224));
    return SLAM_OK;
}
#endif
#ifdef SLAM_STAMPS_ICP
/* diagnostic build: lane efficiency counters of the beam-window search (slam_stamps.h, ISTAMP_SCAN): own candidates and
   candidate slots of the first iteration, of the later ones */
int slam_debug_lanes(slam_ctx *c, unsigned long long *out6, int clear)
{
    TRY(use(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(slam::debug_polar_lanes(out6, clear != 0));
    return SLAM_OK;
}
#endif
#ifdef SLAM_STAMPS
/* diagnostic build: the per-workgroup records (8 dwords each, slam_stamps.h) of the launches since the last clear */
int slam_debug_records(slam_ctx *c, void *out, int max_records)
{
    TRY(use(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    const int n = max_records < kStampRecords ? max_records : kStampRecords;
    HIPCHK(hipMemcpy(out, reinterpret_cast<char *>(c->status) + 256, (size_t)n * 32, hipMemcpyDeviceToHost));
    return SLAM_OK;
}
#endif

/* ---- ICP ------------------------------------------------------------------------ */

static int check_scan_to_points(const char *fn, const float *ranges, const double *cos_t, const double *sin_t, int B, int n,
                                int dtype, const void *pts_out)
{
    REQUIRE_IN(fn, ranges && cos_t && sin_t && pts_out, "null pointer");
    REQUIRE_IN(fn, B > 0 && n > 0, "B and n must be positive");
    REQUIRE_IN(fn, dtype_size(dtype), "unknown dtype");
    return SLAM_OK;
}

int slam_scan_to_points_dev(slam_ctx *c, const float *ranges, const double *cos_t, const double *sin_t, int B, int n,
                            int clip_inf, int dtype, void *pts_out)
{
    TRY(use(c));
    TRY(streams_on_main(c));
    TRY(check_scan_to_points(__func__, ranges, cos_t, sin_t, B, n, dtype, pts_out));
    Timed t(c, SLAM_K_POINTS);
    HIPCHK(launch_scan_to_points(ranges, cos_t, sin_t, (long)B * n, n, clip_inf, dtype, pts_out, c->stream));
    return SLAM_OK;
}

int slam_scan_to_points(slam_ctx *c, const float *ranges, const double *cos_t, const double *sin_t, int B, int n,
                        int clip_inf, int dtype, void *pts_out)
{
    TRY(use(c));
    TRY(check_scan_to_points(__func__, ranges, cos_t, sin_t, B, n, dtype, pts_out));
    const size_t nr = (size_t)B * n;
    float *d_r; double *d_c, *d_s; char *d_p;
    Staging s(c);
    s.in(d_r, ranges, nr).in(d_c, cos_t, n).in(d_s, sin_t, n).out(d_p, static_cast<char *>(pts_out), 2 * nr * dtype_size(dtype));
    TRY(s.upload());
    TRY(slam_scan_to_points_dev(c, d_r, d_c, d_s, B, n, clip_inf, dtype, d_p));
    return s.download();
}

static int check_nn(const char *fn, const void *src, const void *tar, int B, int n_src, int n_tar, int dtype,
                    const double *dist, const int32_t *idx)
{
    REQUIRE_IN(fn, src && tar && dist && idx, "null pointer");
    REQUIRE_IN(fn, B > 0 && n_src > 0 && n_tar > 0, "sizes must be positive");
    REQUIRE_IN(fn, dtype_size(dtype), "unknown dtype");
    REQUIRE_IN(fn, n_tar <= 8192, "n_tar too large for the LDS-resident target (max 8192 points)");
    return SLAM_OK;
}

int slam_nn_dev(slam_ctx *c, const void *src, const void *tar, int B, int n_src, int n_tar, int dtype, double *dist,
                int32_t *idx)
{
    TRY(use(c));
    TRY(streams_on_main(c));
    TRY(check_nn(__func__, src, tar, B, n_src, n_tar, dtype, dist, idx));
    Timed t(c, SLAM_K_NN);
    HIPCHK(launch_nn(src, tar, B, n_src, n_tar, dtype, dist, idx, c->stream));
    return SLAM_OK;
}

int slam_nn(slam_ctx *c, const void *src, const void *tar, int B, int n_src, int n_tar, int dtype, double *dist,
            int32_t *idx)
{
    TRY(use(c));
    TRY(check_nn(__func__, src, tar, B, n_src, n_tar, dtype, dist, idx));
    const size_t ds = dtype_size(dtype), q = (size_t)B * n_src;
    char *d_s, *d_t; double *d_d; int32_t *d_i;
    Staging s(c);
    s.in(d_s, static_cast<const char *>(src), q * 2 * ds).in(d_t, static_cast<const char *>(tar), (size_t)B * 2 * n_tar * ds);
    s.out(d_d, dist, q).out(d_i, idx, q);
    TRY(s.upload());
    TRY(slam_nn_dev(c, d_s, d_t, B, n_src, n_tar, dtype, d_d, d_i));
    return s.download();
}

static int check_kabsch2d(const char *fn, const double *src, const double *tar, int B, int n, const double *T_out)
{
    REQUIRE_IN(fn, src && tar && T_out, "null pointer");
    REQUIRE_IN(fn, B > 0 && n > 0, "sizes must be positive");
    return SLAM_OK;
}

int slam_kabsch2d_dev(slam_ctx *c, const double *src, const double *tar, int B, int n, double *T_out)
{
    TRY(use(c));
    TRY(streams_on_main(c));
    TRY(check_kabsch2d(__func__, src, tar, B, n, T_out));
    Timed t(c, SLAM_K_KABSCH);
    HIPCHK(launch_kabsch(src, tar, B, n, T_out, c->stream));
    return SLAM_OK;
}

int slam_kabsch2d(slam_ctx *c, const double *src, const double *tar, int B, int n, double *T_out)
{
    TRY(use(c));
    TRY(check_kabsch2d(__func__, src, tar, B, n, T_out));
    double *d_s, *d_t, *d_T;
    Staging s(c);
    s.in(d_s, src, (size_t)B * 2 * n).in(d_t, tar, (size_t)B * 2 * n).out(d_T, T_out, (size_t)B * 9);
    TRY(s.upload());
    TRY(slam_kabsch2d_dev(c, d_s, d_t, B, n, d_T));
    return s.download();
}

static int check_icp_batch(const char *fn, const void *tar, const void *src, int B, int n_tar, int n_src, int dtype,
                           int max_iter, const double *T_out)
{
    REQUIRE_IN(fn, tar && src && T_out, "null pointer");
    REQUIRE_IN(fn, B > 0 && n_src > 0 && n_tar > 0, "sizes must be positive");
    REQUIRE_IN(fn, max_iter >= 0, "max_iter must be >= 0");
    REQUIRE_IN(fn, dtype_size(dtype), "unknown dtype");
    REQUIRE_IN(fn, n_src <= 8192, "n_src > 8192 not supported");
    REQUIRE_IN(fn, n_tar <= 8192, "n_tar too large for the LDS-resident target (max 8192 points)");
    return SLAM_OK;
}

int slam_icp_batch_dev(slam_ctx *c, const void *tar, const void *src, int B, int n_tar, int n_src, int dtype,
                       int tar_shared, int src_shared, const double *prior, int max_iter, double tol, double *T_out,
                       int32_t *iters_out, double *mean_err_out)
{
    TRY(use(c));
    TRY(streams_on_main(c));
    TRY(check_icp_batch(__func__, tar, src, B, n_tar, n_src, dtype, max_iter, T_out));
    IcpArgs a;
    a.tar = tar; a.src = src; a.prior = prior;
    a.ranges = nullptr; a.cos_t = a.sin_t = nullptr; a.tar_scan_stride = a.src_scan_stride = 0;
    a.tar_stride = tar_shared ? 0 : 2L * n_tar;
    a.src_stride = src_shared ? 0 : 2L * n_src;
    a.ppt = 0;
    a.B = B; a.n_tar = n_tar; a.n_src = n_src; a.max_iter = max_iter; a.tol = tol;
    a.T_out = T_out; a.iters_out = iters_out; a.err_out = mean_err_out;
    a.status = c->status; a.qpt_pref = c->icp_qpt; a.team_mode = c->icp_team; a.one_wave = c->icp_one_wave; a.f32_filter = c->icp_f32_filter;
    Timed t(c, SLAM_K_ICP);
    HIPCHK(launch_icp(a, dtype, c->stream));
    return SLAM_OK;
}

int slam_icp_batch(slam_ctx *c, const void *tar, const void *src, int B, int n_tar, int n_src, int dtype, int tar_shared,
                   int src_shared, const double *prior, int max_iter, double tol, double *T_out, int32_t *iters_out,
                   double *mean_err_out)
{
    TRY(use(c));
    TRY(check_icp_batch(__func__, tar, src, B, n_tar, n_src, dtype, max_iter, T_out));
    const size_t ds = dtype_size(dtype);
    char *d_t, *d_s; double *d_p, *d_T, *d_e; int32_t *d_i;
    Staging s(c);
    s.in(d_t, static_cast<const char *>(tar), (size_t)(tar_shared ? 1 : B) * 2 * n_tar * ds)
        .in(d_s, static_cast<const char *>(src), (size_t)(src_shared ? 1 : B) * 2 * n_src * ds)
        .in(d_p, prior, (size_t)B * 6);
    s.out(d_T, T_out, (size_t)B * 9).out_always(d_i, iters_out, B).out_always(d_e, mean_err_out, B);
    TRY(s.upload());
    TRY(slam_icp_batch_dev(c, d_t, d_s, B, n_tar, n_src, dtype, tar_shared, src_shared, d_p, max_iter, tol, d_T, d_i, d_e));
    return s.download();
}

static int check_pose_compose(const char *fn, const double *T, const double *pose0, int L, int n, const double *poses_out)
{
    REQUIRE_IN(fn, T && pose0 && poses_out, "null pointer");
    REQUIRE_IN(fn, L > 0 && n > 0, "sizes must be positive");
    return SLAM_OK;
}

int slam_pose_compose_dev(slam_ctx *c, const double *T, const double *pose0, int L, int n, double *poses_out)
{
    TRY(use(c));
    TRY(streams_on_main(c));
    TRY(check_pose_compose(__func__, T, pose0, L, n, poses_out));
    Timed t(c, SLAM_K_COMPOSE);
    HIPCHK(launch_pose_compose(T, pose0, L, n, poses_out, c->stream));
    return SLAM_OK;
}

int slam_pose_compose(slam_ctx *c, const double *T, const double *pose0, int L, int n, double *poses_out)
{
    TRY(use(c));
    TRY(check_pose_compose(__func__, T, pose0, L, n, poses_out));
    const size_t nt = (size_t)L * n;
    double *d_T, *d_0, *d_P;
    Staging s(c);
    s.in(d_T, T, nt * 9).in(d_0, pose0, (size_t)L * 3).out(d_P, poses_out, nt * 3);
    TRY(s.upload());
    TRY(slam_pose_compose_dev(c, d_T, d_0, L, n, d_P));
    return s.download();
}

/* ---- occupancy grid --------------------------------------------------------------- */

int slam_grid_create(slam_ctx *c, int G, int xw, int yw, double scale, double off_x, double off_y, double free_inc,
                     double hit_inc, double thresh, slam_grid **out)
{
    TRY(use(c));
    REQUIRE(out, "out is null");
    *out = nullptr;
    REQUIRE(G > 0 && xw > 0 && yw > 0, "G, xw, yw must be positive");
    REQUIRE(scale > 0 && std::isfinite(scale) && std::isfinite(off_x) && std::isfinite(off_y), "bad index rule");
    REQUIRE(free_inc > 0 && hit_inc > 0 && std::isfinite(thresh), "increments must be positive");
    // Occupied rule on the integer counters.  The reference keeps a float64 running sum per
    // cell (mapping.py:43,45) and tests it against thresh (:47).  With h hits and p passes the
    // sum is evaluated here in ONE canonical order, hits first, with the same sequential IEEE
    // adds: hit_levels = fewest hits that exceed thresh on their own (1 for +20; 3 for the +4
    // of w12-mapping-online), pass_thresh[h] = fewest passes that exceed it after h hits
    // (1001 for (0.01, 10), because 1000 sequential adds of 0.01 give 9.99999999999983).
    // For +20 the rule is exactly the reference's in any order.  For +4 the reference's own
    // answer depends on the order in which a cell's +4 and +0.01 arrived when p is exactly on
    // a threshold (p = pass_thresh[h] - 1 or pass_thresh[h]; the rounding of <= 1001 adds is
    // ~1e-13 << 0.01, so no other p is affected): those cells follow the canonical order.
    uint32_t levels = 0, table[kMaxHitLevels];
    {
        volatile double base = 0.0;
        while (levels < (uint32_t)kMaxHitLevels && !(base > thresh)) {
            volatile double acc = base;
            uint32_t k = 0;
            while (!(acc > thresh) && k < 0xfffffff0u) { acc = acc + free_inc; ++k; }
            table[levels++] = k;
            base = base + hit_inc;
        }
        REQUIRE(base > thresh, "hit_inc is too small: more than 8 hits would be needed to exceed thresh");
    }
    slam_grid *g = new slam_grid();
    size_t cells = (size_t)G * xw * yw;
    g->d.G = G; g->d.xw = xw; g->d.yw = yw;
    g->d.scale = scale; g->d.off_x = off_x; g->d.off_y = off_y;
    g->d.free_inc = free_inc; g->d.hit_inc = hit_inc;
    g->d.hit_levels = (int)levels;
    for (uint32_t k = 0; k < (uint32_t)kMaxHitLevels; ++k) g->d.pass_thresh[k] = k < levels ? table[k] : 0;
    g->d.status = c->status;
    // one allocation [pass | hit | visit counter] so that a reset is a single memset
    g->state_bytes = grid_state_bytes(cells);
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&g->d.pass), g->state_bytes);
    if (e == hipSuccess) {
        g->d.hit = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(g->d.pass) + grid_plane_bytes(cells));
        g->visits = reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(g->d.pass) + 2 * grid_plane_bytes(cells));
    }
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&g->pmap_one), align_up((size_t)xw * yw));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&g->datamap_one), (size_t)xw * yw * 8);
    if (e != hipSuccess) {
        slam_grid_destroy(c, g);
        return fail(SLAM_ERR_NOMEM, "grid allocation (%zu cells): %s", cells, hipGetErrorString(e));
    }
    g->d.visits = g->visits;
    g->d.pmap_live = nullptr;
    g->d.redo = nullptr;
    g->d.live_dirty = &g->live_dirty;
    *out = g;
    return slam_grid_reset(c, g);
}

int slam_grid_destroy(slam_ctx *c, slam_grid *g)
{
    if (!g) return SLAM_OK;
    if (c) {
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
        if (c->gstream) { (void)hipStreamSynchronize(c->cstream); (void)hipStreamSynchronize(c->gstream); }
        if (c->pstream) (void)hipStreamSynchronize(c->pstream);
    }
    if (g->pmap_live) (void)hipFree(g->pmap_live);
    if (g->d.redo) (void)hipFree(g->d.redo);
    if (g->d.pass) (void)hipFree(g->d.pass);   // also holds hit[] and the visit counter
    if (g->pmap_one) (void)hipFree(g->pmap_one);
    if (g->datamap_one) (void)hipFree(g->datamap_one);
    delete g;
    return SLAM_OK;
}

int slam_grid_reset(slam_ctx *c, slam_grid *g)
{
    TRY(use(c));
    REQUIRE(g, "null grid");
    TRY(join_particles(c));
    if (c->pipeline && c->mgrid) {
        TRY(fork_to_grid(c));
        c->mgrid = false;
    }
    HIPCHK(hipMemsetAsync(g->d.pass, 0, g->state_bytes, gs(c)));
    g->pristine = true;
    if (g->pmap_live) {
        HIPCHK(hipMemsetAsync(g->pmap_live, 50, (size_t)g->d.G * g->d.xw * g->d.yw, gs(c)));
        g->live_dirty = false;
    }
    if (c->pipeline) c->gdirty = true;
    return SLAM_OK;
}

static int check_grid_update(const char *fn, const slam_grid *g, const double *ox, const double *oy, const double *cx,
                             const double *cy, int B, int n)
{
    REQUIRE_IN(fn, g && ox && oy && cx && cy, "null pointer");
    REQUIRE_IN(fn, B > 0 && n > 0, "sizes must be positive");
    return SLAM_OK;
}

int slam_grid_update_dev(slam_ctx *c, slam_grid *g, const double *ox, const double *oy, const double *cx, const double *cy,
                         int B, int n, const int32_t *grid_of_batch)
{
    TRY(use(c));
    TRY(grid_on_main(c));
    TRY(check_grid_update(__func__, g, ox, oy, cx, cy, B, n));
    g->pristine = false;
    Timed t(c, SLAM_K_GRID);
    CastRequest r;
    r.ox = ox; r.oy = oy; r.cx = cx; r.cy = cy; r.scans = B; r.n = n; r.maps = grid_of_batch;
    r.group = c->grid_group; r.split = c->grid_split; r.lds_hits = c->win_lds_hits;
    const CastPath path = plan_cast(g->d, c->grid_mode, r);
    const size_t need = cast_scratch_bytes(path, r);
    if (need > c->tiles.cap) TRY(arena_reserve(c, c->tiles, need));
    HIPCHK(launch_cast(g->d, path, r, c->tiles.base, c->tiles.cap, c->stream));
    return SLAM_OK;
}

int slam_grid_update(slam_ctx *c, slam_grid *g, const double *ox, const double *oy, const double *cx, const double *cy,
                     int B, int n, const int32_t *grid_of_batch)
{
    TRY(use(c));
    TRY(check_grid_update(__func__, g, ox, oy, cx, cy, B, n));
    if (grid_of_batch)
        for (int b = 0; b < B; ++b) REQUIRE(grid_of_batch[b] >= 0 && grid_of_batch[b] < g->d.G, "grid_of_batch out of range");
    const size_t np = (size_t)B * n;
    double *d_x, *d_y, *d_cx, *d_cy; int32_t *d_g;
    Staging s(c);
    s.in(d_x, ox, np).in(d_y, oy, np).in(d_cx, cx, B).in(d_cy, cy, B).in(d_g, grid_of_batch, B);
    TRY(s.upload());
    TRY(slam_grid_update_dev(c, g, d_x, d_y, d_cx, d_cy, B, n, d_g));
    return check_status_sync(c);
}

// Ray cast of L streams x (n_scan - 1) scans into `g` on stream st, along the path plan_cast picks for grid_mode
// (0 direct atomics, 1 automatic, 2 recorded walks + tiles, 3 LDS window, 4 direction wedges).
static int cast_replay(slam_ctx *c, slam_grid *g, const float *ranges, const double *cos_t, const double *sin_t,
                       const double *poses, const double *centres, int L, int n_scan, int n, const int32_t *got,
                       hipStream_t st)
{
    g->pristine = false;
    CastRequest r;
    r.ranges = ranges; r.cos_t = cos_t; r.sin_t = sin_t; r.poses = poses; r.centres = centres;
    r.L = L; r.scans = n_scan - 1; r.n = n; r.maps = got;
    r.group = c->grid_group; r.split = c->grid_split; r.lds_hits = c->win_lds_hits;
    const CastPath path = plan_cast(g->d, c->grid_mode, r);
    REQUIRE(path != CastPath::Direct || !centres, "grid_mode 0 has no separate ray origins");
    const size_t need = cast_scratch_bytes(path, r);
    if (need > c->tiles.cap) {
        if (c->gstream) HIPCHK(hipStreamSynchronize(c->gstream));
        TRY(arena_reserve(c, c->tiles, need));
    }
    HIPCHK(launch_cast(g->d, path, r, c->tiles.base, c->tiles.cap, st));
    return SLAM_OK;
}

static int check_grid_update_scans(const char *fn, const slam_grid *g, const float *ranges, const double *cos_t,
                                   const double *sin_t, const double *poses, int S, int n)
{
    REQUIRE_IN(fn, g && ranges && cos_t && sin_t && poses, "null pointer");
    REQUIRE_IN(fn, S > 0 && n > 0 && n <= 65535, "bad sizes");
    return SLAM_OK;
}

int slam_grid_update_scans_dev(slam_ctx *c, slam_grid *g, const float *ranges, const double *cos_t, const double *sin_t,
                               const double *poses, const double *centres, int S, int n)
{
    TRY(use(c));
    TRY(grid_on_main(c));
    TRY(check_grid_update_scans(__func__, g, ranges, cos_t, sin_t, poses, S, n));
    Timed t(c, SLAM_K_GRID);
    // scan k of cast_replay's stream is ranges[k + 1]: shift the base by one scan
    return cast_replay(c, g, ranges - n, cos_t, sin_t, poses, centres, 1, S + 1, n, nullptr, c->stream);
}

int slam_grid_update_scans(slam_ctx *c, slam_grid *g, const float *ranges, const double *cos_t, const double *sin_t,
                           const double *poses, const double *centres, int S, int n)
{
    TRY(use(c));
    TRY(check_grid_update_scans(__func__, g, ranges, cos_t, sin_t, poses, S, n));
    float *d_r; double *d_c, *d_s, *d_p, *d_o;
    Staging s(c);
    s.in(d_r, ranges, (size_t)S * n).in(d_c, cos_t, n).in(d_s, sin_t, n).in(d_p, poses, (size_t)S * 3).in(d_o, centres, (size_t)S * 2);
    TRY(s.upload());
    TRY(slam_grid_update_scans_dev(c, g, d_r, d_c, d_s, d_p, d_o, S, n));
    return check_status_sync(c);
}

static int refresh_live(slam_ctx *c, slam_grid *g, hipStream_t st)
{
    if (!g->pmap_live || !g->live_dirty) return SLAM_OK;
    Timed t(c, SLAM_K_FINALIZE, st);
    HIPCHK(launch_grid_finalize(g->d, 0, g->d.G, g->pmap_live, st));
    g->live_dirty = false;
    return SLAM_OK;
}

int slam_grid_live_pmap(slam_ctx *c, slam_grid *g, int8_t **pmap_dev_out)
{
    TRY(use(c));
    REQUIRE(g && pmap_dev_out, "null pointer");
    TRY(grid_on_main(c));
    if (!g->pmap_live) {
        size_t bytes = (size_t)g->d.G * g->d.xw * g->d.yw;
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&g->pmap_live), align_up(bytes));
        if (e != hipSuccess) {
            g->pmap_live = nullptr;
            return fail(SLAM_ERR_NOMEM, "live pmap (%zu bytes): %s", bytes, hipGetErrorString(e));
        }
        g->d.pmap_live = g->pmap_live;
        if (hipMalloc(reinterpret_cast<void **>(&g->d.redo), ((size_t)g->d.G + 2) * sizeof(int32_t)) != hipSuccess) {
            g->d.redo = nullptr;                  // (the owner kernels then run without the byte-window fast path)
            (void)hipGetLastError();
        } else {
            HIPCHK(hipMemsetAsync(g->d.redo, 0, ((size_t)g->d.G + 2) * sizeof(int32_t), c->stream));
        }
        if (g->pristine) {                    // untouched maps: every cell is 50 (no finalize pass over G maps of zeros)
            HIPCHK(hipMemsetAsync(g->pmap_live, 50, bytes, c->stream));
            g->live_dirty = false;
        } else {
            g->live_dirty = true;
            TRY(refresh_live(c, g, c->stream));
        }
    }
    *pmap_dev_out = g->pmap_live;
    return SLAM_OK;
}

int slam_grid_finalize_dev(slam_ctx *c, slam_grid *g, int8_t *pmap_dev)
{
    TRY(use(c));
    REQUIRE(g && pmap_dev, "null pointer");
    TRY(join_particles(c));        // (a chunked particle batch casts on a stream of its own)
    TRY(fork_to_grid(c));          // pmap_dev may still be in use by work on the main stream
    if (g->pmap_live) {            // kept current by the ray casts; refresh only if something bypassed that
        TRY(refresh_live(c, g, gs(c)));
        if (pmap_dev != g->pmap_live)
            HIPCHK(hipMemcpyAsync(pmap_dev, g->pmap_live, (size_t)g->d.G * g->d.xw * g->d.yw, hipMemcpyDeviceToDevice, gs(c)));
        return SLAM_OK;
    }
    Timed t(c, SLAM_K_FINALIZE, gs(c));
    HIPCHK(launch_grid_finalize(g->d, 0, g->d.G, pmap_dev, gs(c)));
    return SLAM_OK;
}

int slam_grid_read(slam_ctx *c, slam_grid *g, int gi, int8_t *pmap, double *datamap, uint32_t *pass, uint32_t *hit)
{
    TRY(use(c));
    TRY(grid_on_main(c));
    REQUIRE(g, "null grid");
    REQUIRE(gi >= 0 && gi < g->d.G, "grid index out of range");
    size_t per = (size_t)g->d.xw * g->d.yw;
    if (pmap && g->pmap_live) {
        TRY(refresh_live(c, g, c->stream));
        D2H(pmap, g->pmap_live + per * gi, per);
    } else if (pmap) {
        {
            Timed t(c, SLAM_K_FINALIZE);
            HIPCHK(launch_grid_finalize(g->d, gi, 1, g->pmap_one, c->stream));
        }
        D2H(pmap, g->pmap_one, per);
    }
    if (datamap) {
        HIPCHK(launch_grid_datamap(g->d, gi, g->datamap_one, c->stream));
        D2H(datamap, g->datamap_one, per * 8);
    }
    if (pass) D2H(pass, g->d.pass + per * gi, per * 4);
    if (hit) D2H(hit, g->d.hit + per * gi, per * 4);
    HIPCHK(hipStreamSynchronize(c->stream));
    return SLAM_OK;
}

int slam_grid_counters_dev(slam_ctx *c, slam_grid *g, uint32_t **pass_dev, uint32_t **hit_dev)
{
    TRY(use(c));
    REQUIRE(g && pass_dev && hit_dev, "null pointer");
    TRY(grid_on_main(c));                 // later work on the context's stream sees every update so far
    if (g->pmap_live) g->live_dirty = true;   // the caller may change the counters behind the library's back
    g->pristine = false;
    *pass_dev = g->d.pass;
    *hit_dev = g->d.hit;
    return SLAM_OK;
}

int slam_grid_occupancy_data(slam_ctx *c, slam_grid *g, int gi, int8_t *data)
{
    TRY(use(c));
    TRY(grid_on_main(c));
    REQUIRE(g && data, "null pointer");
    REQUIRE(gi >= 0 && gi < g->d.G, "grid index out of range");
    size_t per = (size_t)g->d.xw * g->d.yw;
    int8_t *d_data;
    TRY(reserve(c, c->scratch, Layout().add(d_data, per)));
    const int8_t *pm = g->pmap_one;
    if (g->pmap_live) {                       // kept current by the ray casts: no finalize pass
        TRY(refresh_live(c, g, c->stream));
        pm = g->pmap_live + per * gi;
    } else {
        HIPCHK(launch_grid_finalize(g->d, gi, 1, g->pmap_one, c->stream));
    }
    HIPCHK(launch_grid_transpose(pm, g->d.xw, g->d.yw, d_data, c->stream));
    D2H(data, d_data, per);
    HIPCHK(hipStreamSynchronize(c->stream));
    return SLAM_OK;
}

int slam_grid_visits(slam_ctx *c, slam_grid *g, uint64_t *visits_out)
{
    TRY(use(c));
    TRY(grid_on_main(c));
    REQUIRE(g && visits_out, "null pointer");
    static thread_local unsigned long long slots[kVisitSlots * kVisitStride];
    D2H(slots, g->visits, sizeof slots);
    HIPCHK(hipStreamSynchronize(c->stream));
    unsigned long long v = 0;
    for (int k = 0; k < kVisitSlots; ++k) v += slots[(size_t)k * kVisitStride];
    *visits_out = v;
    return SLAM_OK;
}

// ---- rays traced through a map (raycast_kernels.hip) ------------------------------------------------------------
static int check_raycast(const char *fn, const slam_grid *g, const double *poses, int B, const double *cos_t,
                         const double *sin_t, int n, int skip, const void *out)
{
    REQUIRE_IN(fn, g && poses && cos_t && sin_t && out, "null pointer");
    REQUIRE_IN(fn, n >= 1 && n <= 4096, "n outside [1, 4096]");
    REQUIRE_IN(fn, B >= 1 && (long)B * n < (1L << 31), "B < 1 or B * n >= 2^31");
    REQUIRE_IN(fn, skip >= 0 && skip <= kMaxRayCells, "skip outside [0, 2^20]");
    return SLAM_OK;
}

static int check_grid_of_batch(const char *fn, const slam_grid *g, const int32_t *grid_of_batch, int B)
{
    if (grid_of_batch)
        for (int b = 0; b < B; ++b)
            if (grid_of_batch[b] < 0 || grid_of_batch[b] >= g->d.G)
                return fail(SLAM_ERR_INVALID, "%s: grid_of_batch[%d] = %d outside [0, G = %d)", fn, b, grid_of_batch[b], g->d.G);
    return SLAM_OK;
}

// pack the occupied bits of every map as the counters stand on the stream now (what k_grid_finalize would call 100),
// then trace.  The counters are only read: a live pmap stays as current or as stale as it was.
static int run_raycast(slam_ctx *c, slam_grid *g, RaycastArgs &a)
{
    TRY(grid_on_main(c));
    const size_t words = raycast_mask_words(g->d);
    uint32_t *mask;
    TRY(reserve(c, c->scratch, Layout().add(mask, words)));
    a.g = g->d;
    a.mask = mask;
    {
        Timed t(c, SLAM_K_FINALIZE);      // the threshold rule over every cell, as a finalize pass is
        HIPCHK(launch_raycast_pack(g->d, mask, c->stream));
    }
    Timed t(c, SLAM_K_GRID);
    HIPCHK(launch_raycast(a, choose_raycast_path(g->d, c->raycast_lds, a.B, a.n), c->stream));
    return SLAM_OK;
}

int slam_grid_raycast_dev(slam_ctx *c, slam_grid *g, const double *poses, int B, const int32_t *grid_of_batch,
                          const double *cos_t, const double *sin_t, int n, float max_range, int skip, float *ranges_out,
                          int32_t *cells_out)
{
    TRY(use(c));
    TRY(check_raycast(__func__, g, poses, B, cos_t, sin_t, n, skip, ranges_out));
    REQUIRE(std::isfinite(max_range) && max_range > 0, "max_range must be finite and > 0");
    RaycastArgs a;
    a.poses = poses; a.maps = grid_of_batch; a.cos_t = cos_t; a.sin_t = sin_t;
    a.B = B; a.n = n; a.skip = skip; a.max_range = max_range;
    a.ranges_out = ranges_out; a.cells_out = cells_out;
    return run_raycast(c, g, a);
}

int slam_grid_raycast(slam_ctx *c, slam_grid *g, const double *poses, int B, const int32_t *grid_of_batch, const double *cos_t,
                      const double *sin_t, int n, float max_range, int skip, float *ranges_out, int32_t *cells_out)
{
    TRY(use(c));
    TRY(check_raycast(__func__, g, poses, B, cos_t, sin_t, n, skip, ranges_out));
    REQUIRE(std::isfinite(max_range) && max_range > 0, "max_range must be finite and > 0");
    TRY(check_grid_of_batch(__func__, g, grid_of_batch, B));
    const size_t rays = (size_t)B * n;
    double *d_p, *d_c, *d_s; int32_t *d_g, *d_cells; float *d_r;
    Staging s(c);
    s.in(d_p, poses, (size_t)B * 3).in(d_g, grid_of_batch, B).in(d_c, cos_t, n).in(d_s, sin_t, n)
        .out(d_r, ranges_out, rays).out(d_cells, cells_out, 2 * rays);
    TRY(s.upload());
    TRY(slam_grid_raycast_dev(c, g, d_p, B, d_g, d_c, d_s, n, max_range, skip, d_r, d_cells));
    return s.download();
}

int slam_grid_scan_score_dev(slam_ctx *c, slam_grid *g, const float *ranges, int shared, const double *poses, int B,
                             const int32_t *grid_of_batch, const double *cos_t, const double *sin_t, int n, int skip,
                             int32_t *counts_out, int8_t *class_out)
{
    TRY(use(c));
    TRY(check_raycast(__func__, g, poses, B, cos_t, sin_t, n, skip, counts_out));
    REQUIRE(ranges, "null pointer");
    RaycastArgs a;
    a.poses = poses; a.maps = grid_of_batch; a.cos_t = cos_t; a.sin_t = sin_t;
    a.B = B; a.n = n; a.skip = skip;
    a.ranges = ranges; a.range_stride = shared ? 0 : n;
    a.counts_out = counts_out; a.class_out = class_out;
    HIPCHK(hipMemsetAsync(counts_out, 0, (size_t)B * SLAM_RAY_CLASSES * sizeof(int32_t), c->stream));
    return run_raycast(c, g, a);
}

int slam_grid_scan_score(slam_ctx *c, slam_grid *g, const float *ranges, int shared, const double *poses, int B,
                         const int32_t *grid_of_batch, const double *cos_t, const double *sin_t, int n, int skip,
                         int32_t *counts_out, int8_t *class_out)
{
    TRY(use(c));
    TRY(check_raycast(__func__, g, poses, B, cos_t, sin_t, n, skip, counts_out));
    REQUIRE(ranges, "null pointer");
    TRY(check_grid_of_batch(__func__, g, grid_of_batch, B));
    const size_t rays = (size_t)B * n;
    float *d_r; double *d_p, *d_c, *d_s; int32_t *d_g, *d_cnt; int8_t *d_cls;
    Staging s(c);
    s.in(d_r, ranges, shared ? (size_t)n : rays).in(d_p, poses, (size_t)B * 3).in(d_g, grid_of_batch, B).in(d_c, cos_t, n)
        .in(d_s, sin_t, n).out(d_cnt, counts_out, (size_t)B * SLAM_RAY_CLASSES).out(d_cls, class_out, rays);
    TRY(s.upload());
    TRY(slam_grid_scan_score_dev(c, g, d_r, shared, d_p, B, d_g, d_c, d_s, n, skip, d_cnt, d_cls));
    return s.download();
}

// ---- view gain (view_kernels.hip) -----------------------------------------------------------------------------------
static int check_view(const char *fn, const slam_ctx *c, const slam_grid *g, const double *poses, int B, const double *cos_t,
                      const double *sin_t, int n, float max_range, int skip, const int32_t *counts_out, const uint32_t *seen_out,
                      ViewShape &plan)
{
    TRY(check_raycast(fn, g, poses, B, cos_t, sin_t, n, skip, counts_out));
    REQUIRE_IN(fn, std::isfinite(max_range) && max_range > 0, "max_range must be finite and > 0");
    const long map_words = (long)g->d.xw * ((g->d.yw + 31) / 32);
    REQUIRE_IN(fn, map_words < (1L << 31), "xw * ceil(yw / 32) >= 2^31");
    REQUIRE_IN(fn, !seen_out || (long)B * map_words < (1L << 31), "B * xw * ceil(yw / 32) >= 2^31 with seen_out");
    plan = view_plan_for(g->d.xw, g->d.yw, 0, 0, c->gain_lds, B, c->gain_ws_bytes, kLdsGuard);
    if (!plan.ok)
        return fail(SLAM_ERR_INVALID, "%s: the bit window of one view (%ld bytes) does not fit the context option gain_ws_mb (%ld bytes)",
                    fn, plan.view_bytes, c->gain_ws_bytes);
    return SLAM_OK;
}

// pack the two class planes of every map as the counters stand on the stream now, then the views.  The counters are
// only read.
static int view_dev(const char *fn, slam_ctx *c, slam_grid *g, const double *poses, int B, const int32_t *grid_of_batch,
                    const double *cos_t, const double *sin_t, int n, float max_range, int skip, int32_t *counts_out, uint32_t *seen_out)
{
    ViewShape plan;
    TRY(check_view(fn, c, g, poses, B, cos_t, sin_t, n, max_range, skip, counts_out, seen_out, plan));
    TRY(grid_on_main(c));
    const size_t plane = raycast_mask_words(g->d);
    uint32_t *occ, *unk, *slots;
    TRY(reserve(c, c->scratch, Layout().add(occ, plane).add(unk, plane).add(slots, (size_t)plan.grid_global * plan.map_words)));
    ViewArgs a;
    a.g = g->d; a.occ = occ; a.unk = unk; a.wpr = plan.row_words;
    a.poses = poses; a.maps = grid_of_batch; a.cos_t = cos_t; a.sin_t = sin_t;
    a.B = B; a.n = n; a.skip = skip; a.max_range = max_range; a.lds_mode = c->gain_lds;
    a.slots = slots; a.counts_out = counts_out; a.seen_out = seen_out;
    {
        Timed t(c, SLAM_K_FINALIZE);      // the threshold rule over every cell, as a finalize pass is
        HIPCHK(launch_view_pack(g->d, occ, unk, c->stream));
    }
    Timed t(c, SLAM_K_GRID);
    HIPCHK(launch_view(a, plan, c->stream));
    return SLAM_OK;
}

int slam_grid_view_gain_dev(slam_ctx *c, slam_grid *g, const double *poses, int B, const int32_t *grid_of_batch, const double *cos_t,
                            const double *sin_t, int n, float max_range, int skip, int32_t *counts_out, uint32_t *seen_out)
{
    TRY(use(c));
    return view_dev(__func__, c, g, poses, B, grid_of_batch, cos_t, sin_t, n, max_range, skip, counts_out, seen_out);
}

int slam_grid_view_gain(slam_ctx *c, slam_grid *g, const double *poses, int B, const int32_t *grid_of_batch, const double *cos_t,
                        const double *sin_t, int n, float max_range, int skip, int32_t *counts_out, uint32_t *seen_out)
{
    TRY(use(c));
    ViewShape plan;
    TRY(check_view(__func__, c, g, poses, B, cos_t, sin_t, n, max_range, skip, counts_out, seen_out, plan));
    TRY(check_grid_of_batch(__func__, g, grid_of_batch, B));
    double *d_p, *d_c, *d_s; int32_t *d_g, *d_cnt; uint32_t *d_seen;
    Staging s(c);
    s.in(d_p, poses, (size_t)B * 3).in(d_g, grid_of_batch, B).in(d_c, cos_t, n).in(d_s, sin_t, n)
        .out(d_cnt, counts_out, (size_t)B * SLAM_VIEW_COUNTS).out(d_seen, seen_out, (size_t)B * plan.map_words);
    TRY(s.upload());
    TRY(view_dev(__func__, c, g, d_p, B, d_g, d_c, d_s, n, max_range, skip, d_cnt, d_seen));
    return s.download();
}

// ---- distance field and window matcher (match_kernels.hip) --------------------------------------------------------
// The occupied bits packed as the counters stand on the stream now, then the field of all G maps.  `ws` holds the caller's
// own pieces of the scratch arena (a copy: the pointers they are bound to are the caller's); the mask, the row distances
// and, with `field` null, the field (the matcher's own copy) join them, and the arena is reserved for all of them at once.
// The field's own pieces (field_layout) and its launches in pieces already placed (enqueue_field) are apart for the call
// that builds the field many times in one workspace (slam_track_dev).
struct FieldPieces {
    uint32_t *mask = nullptr;
    uint8_t *rowd = nullptr;
};

static void field_layout(const slam_grid *g, Layout &ws, FieldPieces &p, int16_t *&field)
{
    ws.add(p.mask, raycast_mask_words(g->d)).add(p.rowd, field_rowd_bytes(g->d));
    if (!field) ws.add(field, (size_t)g->d.G * g->d.xw * g->d.yw);
}

static int enqueue_field(slam_ctx *c, slam_grid *g, int cap, const FieldPieces &p, int16_t *field)
{
    Timed t(c, SLAM_K_FINALIZE);          // the threshold rule over every cell, as a finalize pass is
    HIPCHK(launch_raycast_pack(g->d, p.mask, c->stream));
    HIPCHK(launch_distance_field(g->d, p.mask, cap, p.rowd, field, c->stream));
    return SLAM_OK;
}

static int build_field(slam_ctx *c, slam_grid *g, int cap, Layout ws, int16_t *&field)
{
    TRY(grid_on_main(c));
    FieldPieces p;
    field_layout(g, ws, p, field);
    TRY(reserve(c, c->scratch, ws));
    return enqueue_field(c, g, cap, p, field);
}

static int check_field(const char *fn, const slam_grid *g, int cap, const void *out)
{
    REQUIRE_IN(fn, g && out, "null pointer");
    REQUIRE_IN(fn, cap >= 1 && cap <= 32767, "cap outside [1, 32767]");
    return SLAM_OK;
}

int slam_grid_distance_field_dev(slam_ctx *c, slam_grid *g, int cap, int16_t *field_out)
{
    TRY(use(c));
    TRY(check_field(__func__, g, cap, field_out));
    return build_field(c, g, cap, Layout(), field_out);
}

int slam_grid_distance_field(slam_ctx *c, slam_grid *g, int cap, int16_t *field_out)
{
    TRY(use(c));
    TRY(check_field(__func__, g, cap, field_out));
    int16_t *d_f;
    Staging s(c);
    s.out(d_f, field_out, (size_t)g->d.G * g->d.xw * g->d.yw);
    TRY(s.upload());
    TRY(slam_grid_distance_field_dev(c, g, cap, d_f));
    return s.download();
}

static int check_match(const char *fn, const slam_grid *g, const float *ranges, const double *centres, int B, const double *cos_t,
                       const double *sin_t, int n, const double *rot_cs, int K, int nx, int ny, double step, float max_range,
                       int cap, const int32_t *best_out, const int32_t *best_cost_out)
{
    REQUIRE_IN(fn, g && ranges && centres && cos_t && sin_t && rot_cs && best_out && best_cost_out, "null pointer");
    REQUIRE_IN(fn, cap >= 1 && cap <= 32767, "cap outside [1, 32767]");
    REQUIRE_IN(fn, n >= 1 && (long)n * cap < (1L << 31), "n < 1 or n * cap >= 2^31");
    REQUIRE_IN(fn, n <= 4096, "n outside [1, 4096]");
    REQUIRE_IN(fn, B >= 1 && (long)B * n < (1L << 31), "B < 1 or B * n >= 2^31");
    REQUIRE_IN(fn, K >= 1 && nx >= 0 && ny >= 0, "K < 1, nx < 0 or ny < 0");
    const long lim = 1L << 24;
    REQUIRE_IN(fn, K <= lim && nx < lim && ny < lim && (2L * nx + 1) * (2L * ny + 1) <= lim &&
                       (long)K * ((2L * nx + 1) * (2L * ny + 1)) <= lim, "K * (2 nx + 1) * (2 ny + 1) > 2^24");
    REQUIRE_IN(fn, (long)B * K < (1L << 31), "B * K >= 2^31");
    REQUIRE_IN(fn, std::isfinite(step) && step > 0, "step must be finite and > 0");
    REQUIRE_IN(fn, max_range > 0, "max_range must be > 0");
    return SLAM_OK;
}

int slam_grid_match_dev(slam_ctx *c, slam_grid *g, const float *ranges, int shared, const double *centres, int B,
                        const int32_t *grid_of_batch, const double *cos_t, const double *sin_t, int n, const double *rot_cs,
                        int K, int nx, int ny, double step, float max_range, int cap, int32_t *best_out,
                        int32_t *best_cost_out, int32_t *used_out, int32_t *cost_out)
{
    TRY(use(c));
    TRY(check_match(__func__, g, ranges, centres, B, cos_t, sin_t, n, rot_cs, K, nx, ny, step, max_range, cap, best_out,
                    best_cost_out));
    int16_t *field = nullptr;
    MatchArgs a;
    TRY(build_field(c, g, cap, Layout().add(a.keys, B), field));
    a.g = g->d; a.field = field;
    a.ranges = ranges; a.range_stride = shared ? 0 : n;
    a.centres = centres; a.maps = grid_of_batch; a.cos_t = cos_t; a.sin_t = sin_t; a.rot_cs = rot_cs;
    a.B = B; a.n = n; a.K = K; a.nx = nx; a.ny = ny; a.step = step; a.max_range = max_range; a.cap = cap;
    a.best_out = best_out; a.best_cost_out = best_cost_out; a.used_out = used_out; a.cost_out = cost_out;
    HIPCHK(hipMemsetAsync(a.keys, 0xff, (size_t)B * 8, c->stream));
    Timed t(c, SLAM_K_GRID);
    HIPCHK(launch_match(a, c->stream));
    return SLAM_OK;
}

int slam_grid_match(slam_ctx *c, slam_grid *g, const float *ranges, int shared, const double *centres, int B,
                    const int32_t *grid_of_batch, const double *cos_t, const double *sin_t, int n, const double *rot_cs, int K,
                    int nx, int ny, double step, float max_range, int cap, int32_t *best_out, int32_t *best_cost_out,
                    int32_t *used_out, int32_t *cost_out)
{
    TRY(use(c));
    TRY(check_match(__func__, g, ranges, centres, B, cos_t, sin_t, n, rot_cs, K, nx, ny, step, max_range, cap, best_out,
                    best_cost_out));
    const size_t cands = (size_t)K * (2 * (size_t)nx + 1) * (2 * (size_t)ny + 1);
    float *d_r; double *d_ctr, *d_c, *d_s, *d_rot; int32_t *d_g, *d_best, *d_cost, *d_used, *d_vol;
    Staging s(c);
    s.in(d_r, ranges, shared ? (size_t)n : (size_t)B * n).in(d_ctr, centres, (size_t)B * 2).in(d_g, grid_of_batch, B)
        .in(d_c, cos_t, n).in(d_s, sin_t, n).in(d_rot, rot_cs, (size_t)B * K * 2)
        .out(d_best, best_out, B).out(d_cost, best_cost_out, B).out(d_used, used_out, B).out(d_vol, cost_out, (size_t)B * cands);
    TRY(s.upload());
    TRY(slam_grid_match_dev(c, g, d_r, shared, d_ctr, B, d_g, d_c, d_s, n, d_rot, K, nx, ny, step, max_range, cap, d_best,
                            d_cost, d_used, d_vol));
    return s.download();
}

// ---- refinement of a scan-to-map pose below the cell (refine_kernels.hip, include/slam_refine.h) ---------------------
static int check_refine(const char *fn, const slam_grid *g, const float *ranges, const double *poses, int B, const double *cos_t,
                        const double *sin_t, int n, int iters, double damping, double step_cells, double step_rad, float max_range,
                        int cap, const double *pose_out, const double *cost_out, const int32_t *status_out)
{
    REQUIRE_IN(fn, g && ranges && poses && cos_t && sin_t && pose_out && cost_out && status_out, "null pointer");
    REQUIRE_IN(fn, cap >= 1 && cap <= 32767, "cap outside [1, 32767]");
    REQUIRE_IN(fn, n >= 1 && n <= 4096, "n outside [1, 4096]");
    REQUIRE_IN(fn, B >= 1 && (long)B * n < (1L << 31), "B < 1 or B * n >= 2^31");
    REQUIRE_IN(fn, iters >= 0 && iters <= 64, "iters outside [0, 64]");
    REQUIRE_IN(fn, std::isfinite(damping) && damping >= 0, "damping must be finite and >= 0");
    REQUIRE_IN(fn, step_cells > 0 && step_rad > 0, "step_cells and step_rad must be > 0");
    REQUIRE_IN(fn, max_range > 0, "max_range must be > 0");
    return SLAM_OK;
}

int slam_grid_refine_dev(slam_ctx *c, slam_grid *g, const float *ranges, int shared, const double *poses, int B,
                         const int32_t *grid_of_batch, const double *cos_t, const double *sin_t, int n, int iters, double damping,
                         double step_cells, double step_rad, float max_range, int cap, const int16_t *field, double *pose_out,
                         double *cost_out, int32_t *used_out, double *normal_out, int32_t *status_out)
{
    TRY(use(c));
    TRY(check_refine(__func__, g, ranges, poses, B, cos_t, sin_t, n, iters, damping, step_cells, step_rad, max_range, cap, pose_out,
                     cost_out, status_out));
    int16_t *built = nullptr;
    if (!field) TRY(build_field(c, g, cap, Layout(), built));      // (joins the internal streams first, as grid_on_main does)
    else TRY(grid_on_main(c));
    RefineArgs a;
    a.g = g->d; a.field = field ? field : built;
    a.ranges = ranges; a.range_stride = shared ? 0 : n;
    a.poses = poses; a.maps = grid_of_batch; a.cos_t = cos_t; a.sin_t = sin_t;
    a.B = B; a.n = n; a.iters = iters; a.damping = damping; a.step_xy = step_cells / g->d.scale; a.step_rad = step_rad;
    a.max_range = max_range; a.cap = cap;
    a.pose_out = pose_out; a.cost_out = cost_out; a.used_out = used_out; a.normal_out = normal_out; a.status_out = status_out;
    Timed t(c, SLAM_K_GRID);
    HIPCHK(launch_refine(a, c->stream));
    return SLAM_OK;
}

int slam_grid_refine(slam_ctx *c, slam_grid *g, const float *ranges, int shared, const double *poses, int B,
                     const int32_t *grid_of_batch, const double *cos_t, const double *sin_t, int n, int iters, double damping,
                     double step_cells, double step_rad, float max_range, int cap, const int16_t *field, double *pose_out,
                     double *cost_out, int32_t *used_out, double *normal_out, int32_t *status_out)
{
    TRY(use(c));
    TRY(check_refine(__func__, g, ranges, poses, B, cos_t, sin_t, n, iters, damping, step_cells, step_rad, max_range, cap, pose_out,
                     cost_out, status_out));
    float *d_r; double *d_p, *d_c, *d_s, *d_po, *d_co, *d_no; int32_t *d_g, *d_used, *d_st; int16_t *d_f;
    Staging s(c);
    s.in(d_r, ranges, shared ? (size_t)n : (size_t)B * n).in(d_p, poses, (size_t)B * 3).in(d_g, grid_of_batch, B).in(d_c, cos_t, n)
        .in(d_s, sin_t, n).in(d_f, field, (size_t)g->d.G * g->d.xw * g->d.yw).out(d_po, pose_out, (size_t)B * 3)
        .out(d_co, cost_out, (size_t)B * 2).out(d_used, used_out, B).out(d_no, normal_out, (size_t)B * SLAM_REFINE_NORMAL_LEN)
        .out(d_st, status_out, B);
    TRY(s.upload());
    TRY(slam_grid_refine_dev(c, g, d_r, shared, d_p, B, d_g, d_c, d_s, n, iters, damping, step_cells, step_rad, max_range, cap, d_f,
                             d_po, d_co, d_used, d_no, d_st));
    return s.download();
}

// ---- global scan localisation (locate_kernels.hip) ------------------------------------------------------------------
// Everything the host can check, and the plan.  max_ni, max_nj: the largest region of the batch where the host knows the
// regions (the host form), else the map (the device form: a region the device finds outside the map costs its hypothesis
// its answer, as a map entry outside [0, G) does).
static int check_locate(const char *fn, const slam_ctx *c, const slam_grid *g, const float *ranges, int B, const double *cos_t,
                        const double *sin_t, int n, const double *rot_cs, int K, int max_ni, int max_nj, int levels,
                        float max_range, int cap, const int32_t *best_out, const int32_t *best_cost_out, LocateShape &plan)
{
    REQUIRE_IN(fn, g && ranges && cos_t && sin_t && rot_cs && best_out && best_cost_out, "null pointer");
    REQUIRE_IN(fn, cap >= 1 && cap <= 32767, "cap outside [1, 32767]");
    REQUIRE_IN(fn, n >= 1 && n <= kLocateMaxBeams, "n outside [1, 4096]");
    REQUIRE_IN(fn, (long)n * cap < (1L << 31), "n * cap >= 2^31");
    REQUIRE_IN(fn, B >= 1 && K >= 1, "B < 1 or K < 1");
    REQUIRE_IN(fn, (long)B * K < (1L << 31), "B * K >= 2^31");
    REQUIRE_IN(fn, levels >= 0 && levels <= kLocateMaxLevels, "levels outside [0, 8]");
    REQUIRE_IN(fn, max_range > 0, "max_range must be > 0");
    REQUIRE_IN(fn, (long)K * ((long)max_ni * max_nj) < (1L << 31), "K * ni * nj >= 2^31");
    LocateRequest r;
    r.pairs = (long)B * K; r.n = n; r.ni = max_ni; r.nj = max_nj; r.H = levels; r.ws_bytes = c->locate_ws_bytes;
    plan = plan_locate(r);
    if (!plan.ok)
        return fail(SLAM_ERR_INVALID, "%s: the node lists and offsets of one rotation (%ld bytes at worst) do not fit the context option "
                    "locate_ws_mb (%ld bytes)", fn, plan.pair_bytes, c->locate_ws_bytes);
    return SLAM_OK;
}

static int locate_dev(const char *fn, slam_ctx *c, slam_grid *g, const float *ranges, int shared, int B,
                      const int32_t *grid_of_batch, const double *cos_t, const double *sin_t, int n, const double *rot_cs, int K,
                      const int32_t *region, int max_ni, int max_nj, int levels, float max_range, int cap, int32_t *best_out,
                      int32_t *best_cost_out, int32_t *used_out, int64_t *stats_out)
{
    LocateShape plan;
    TRY(check_locate(fn, c, g, ranges, B, cos_t, sin_t, n, rot_cs, K, max_ni, max_nj, levels, max_range, cap, best_out,
                     best_cost_out, plan));
    const int H = levels;
    const size_t pyr_cells = locate_pyramid_cells(g->d, H), keys = 2 * (size_t)B, evals = (size_t)B * (H + 1);
    const size_t rows = H ? (size_t)plan.chunk_pairs : 0;
    LocateArgs a;
    int16_t *pyr, *field = nullptr;
    unsigned long long *words;
    Layout ws;
    ws.add(pyr, pyr_cells).add(words, keys + evals).add(a.bound, B).add(a.used, B).add(a.list_len, kLocateMaxLevels + 1);
    for (int h = 1; h <= H; ++h) {
        a.list_cap[h] = plan.chunk_pairs * plan.level_nodes[h];
        ws.add(a.list[h], (size_t)a.list_cap[h] * 2);
    }
    ws.add(a.table, rows * n * 2).add(a.table_cnt, rows * 2);
    TRY(build_field(c, g, cap, ws, field));
    a.key_top = words; a.key_leaf = words + B; a.evaluated = words + keys;
    a.g = g->d;
    a.ranges = ranges; a.range_stride = shared ? 0 : n;
    a.maps = grid_of_batch; a.cos_t = cos_t; a.sin_t = sin_t; a.rot_cs = rot_cs; a.region = region;
    a.B = B; a.n = n; a.K = K; a.H = H; a.max_ni = max_ni; a.max_nj = max_nj; a.max_range = max_range; a.cap = cap;
    a.best_out = best_out; a.best_cost_out = best_cost_out; a.used_out = used_out; a.stats_out = stats_out;
    HIPCHK(hipMemsetAsync(words, 0xff, keys * 8, c->stream));
    HIPCHK(hipMemsetAsync(words + keys, 0, evals * 8, c->stream));
    {
        Timed t(c, SLAM_K_FINALIZE);      // the pyramid is part of the field: a pass over every cell of every map
        HIPCHK(launch_locate_pyramid(a, field, pyr, c->stream));
    }
    Timed t(c, SLAM_K_GRID);
    HIPCHK(launch_locate(a, plan, c->stream));
    return SLAM_OK;
}

int slam_grid_locate_dev(slam_ctx *c, slam_grid *g, const float *ranges, int shared, int B, const int32_t *grid_of_batch,
                         const double *cos_t, const double *sin_t, int n, const double *rot_cs, int K, const int32_t *region,
                         int levels, float max_range, int cap, int32_t *best_out, int32_t *best_cost_out, int32_t *used_out,
                         int64_t *stats_out)
{
    TRY(use(c));
    REQUIRE(g, "null pointer");
    return locate_dev(__func__, c, g, ranges, shared, B, grid_of_batch, cos_t, sin_t, n, rot_cs, K, region, g->d.xw, g->d.yw, levels,
                      max_range, cap, best_out, best_cost_out, used_out, stats_out);
}

int slam_grid_locate(slam_ctx *c, slam_grid *g, const float *ranges, int shared, int B, const int32_t *grid_of_batch,
                     const double *cos_t, const double *sin_t, int n, const double *rot_cs, int K, const int32_t *region, int levels,
                     float max_range, int cap, int32_t *best_out, int32_t *best_cost_out, int32_t *used_out, int64_t *stats_out)
{
    TRY(use(c));
    REQUIRE(g && B >= 1, "null pointer or B < 1");
    int max_ni = g->d.xw, max_nj = g->d.yw;
    if (region) {
        max_ni = max_nj = 1;
        for (int b = 0; b < B; ++b) {
            const int32_t *r = region + 4 * (size_t)b;
            if (r[0] < 0 || r[1] < 0 || r[2] < 1 || r[3] < 1 || (long)r[0] + r[2] > g->d.xw || (long)r[1] + r[3] > g->d.yw)
                return fail(SLAM_ERR_INVALID, "%s: region[%d] = (%d, %d, %d, %d) is empty or not inside the map of %d x %d cells",
                            __func__, b, r[0], r[1], r[2], r[3], g->d.xw, g->d.yw);
            max_ni = std::max(max_ni, r[2]);
            max_nj = std::max(max_nj, r[3]);
        }
    }
    LocateShape plan;
    TRY(check_locate(__func__, c, g, ranges, B, cos_t, sin_t, n, rot_cs, K, max_ni, max_nj, levels, max_range, cap, best_out,
                     best_cost_out, plan));
    float *d_r; double *d_c, *d_s, *d_rot; int32_t *d_g, *d_reg, *d_best, *d_cost, *d_used; int64_t *d_st;
    Staging s(c);
    s.in(d_r, ranges, shared ? (size_t)n : (size_t)B * n).in(d_g, grid_of_batch, B).in(d_c, cos_t, n).in(d_s, sin_t, n)
        .in(d_rot, rot_cs, (size_t)K * 2).in(d_reg, region, (size_t)B * 4).out(d_best, best_out, (size_t)B * 3)
        .out(d_cost, best_cost_out, B).out(d_used, used_out, B).out(d_st, stats_out, (size_t)B * (levels + 2));
    TRY(s.upload());
    TRY(locate_dev(__func__, c, g, d_r, shared, B, d_g, d_c, d_s, n, d_rot, K, d_reg, max_ni, max_nj, levels, max_range, cap, d_best,
                   d_cost, d_used, d_st));
    return s.download();
}

// ---- map frontiers (frontier_kernels.hip) -----------------------------------------------------------------------------
static int check_frontiers(const char *fn, const slam_ctx *c, const slam_grid *g, int B, const int32_t *grid_of_batch, int radius,
                           int min_unknown, int min_clear2, int cap, int min_size, int max_clusters, const int32_t *count_out,
                           const int32_t *clusters_out, const int64_t *sums_out, FrontierShape &plan)
{
    REQUIRE_IN(fn, g && count_out, "null pointer");
    REQUIRE_IN(fn, B >= 1, "B < 1");
    REQUIRE_IN(fn, grid_of_batch || B <= g->d.G, "B > G without grid_of_batch (query b reads map b)");
    REQUIRE_IN(fn, radius >= 0 && radius <= kFrontierMaxRadius, "radius outside [0, 8]");
    REQUIRE_IN(fn, min_unknown >= 0 && min_unknown <= (2 * radius + 1) * (2 * radius + 1), "min_unknown outside [0, (2 radius + 1)^2]");
    REQUIRE_IN(fn, min_clear2 >= 0, "min_clear2 < 0");
    if (min_clear2 > 0) {
        REQUIRE_IN(fn, cap >= 1 && cap <= 32767, "cap outside [1, 32767]");
        REQUIRE_IN(fn, min_clear2 <= cap, "min_clear2 > cap");
    }
    REQUIRE_IN(fn, min_size >= 1, "min_size < 1");
    REQUIRE_IN(fn, max_clusters >= 0 && max_clusters <= kFrontierMaxClusters, "max_clusters outside [0, 65536]");
    REQUIRE_IN(fn, (long)B * std::max(max_clusters, 1) < (1L << 31), "B * max(max_clusters, 1) >= 2^31");
    REQUIRE_IN(fn, max_clusters == 0 || (clusters_out && sums_out), "null table with max_clusters > 0");
    REQUIRE_IN(fn, g->d.xw <= 32768 && g->d.yw <= 32768, "a map of more than 32768 cells in an axis");
    plan = frontier_plan_for(g->d.xw, g->d.yw, radius, B, c->frontier_ws_bytes, kLdsGuard);
    if (!plan.ok)
        return fail(SLAM_ERR_INVALID, "%s: the labels of one query (%ld bytes) do not fit the context option frontier_ws_mb (%ld bytes)",
                    fn, plan.query_bytes, c->frontier_ws_bytes);
    return SLAM_OK;
}

static int frontiers_dev(const char *fn, slam_ctx *c, slam_grid *g, int B, const int32_t *grid_of_batch, int radius, int min_unknown,
                         int min_clear2, int cap, int min_size, int max_clusters, int32_t *count_out, int32_t *clusters_out,
                         int64_t *sums_out, int32_t *labels_out)
{
    FrontierShape plan;
    TRY(check_frontiers(fn, c, g, B, grid_of_batch, radius, min_unknown, min_clear2, cap, min_size, max_clusters, count_out,
                        clusters_out, sums_out, plan));
    const size_t cells = (size_t)g->d.xw * g->d.yw;
    const size_t lab_words = (size_t)plan.chunk_queries * cells, seg_words = (size_t)plan.chunk_queries * plan.segs * 2;
    FrontierArgs a;
    Layout ws;
    ws.add(a.lab, lab_words).add(a.seg, seg_words);
    if (min_clear2 > 0) {       // the field of all G maps, as slam_grid_match builds it
        int16_t *field = nullptr;
        TRY(build_field(c, g, cap, ws, field));
        a.field = field;
    } else {
        TRY(grid_on_main(c));
        TRY(reserve(c, c->scratch, ws));
    }
    a.g = g->d;
    a.maps = grid_of_batch;
    a.B = B; a.radius = radius; a.min_unknown = min_unknown; a.min_clear2 = min_clear2; a.min_size = min_size; a.M = max_clusters;
    a.count_out = count_out; a.clusters_out = clusters_out; a.sums_out = sums_out; a.labels_out = labels_out;
    Timed t(c, SLAM_K_GRID);
    for (long b0 = 0; b0 < B; b0 += plan.chunk_queries)
        HIPCHK(launch_frontiers(a, plan, b0, std::min(plan.chunk_queries, (long)B - b0), c->stream));
    return SLAM_OK;
}

int slam_grid_frontiers_dev(slam_ctx *c, slam_grid *g, int B, const int32_t *grid_of_batch, int radius, int min_unknown, int min_clear2,
                            int cap, int min_size, int max_clusters, int32_t *count_out, int32_t *clusters_out, int64_t *sums_out,
                            int32_t *labels_out)
{
    TRY(use(c));
    return frontiers_dev(__func__, c, g, B, grid_of_batch, radius, min_unknown, min_clear2, cap, min_size, max_clusters, count_out,
                         clusters_out, sums_out, labels_out);
}

int slam_grid_frontiers(slam_ctx *c, slam_grid *g, int B, const int32_t *grid_of_batch, int radius, int min_unknown, int min_clear2,
                        int cap, int min_size, int max_clusters, int32_t *count_out, int32_t *clusters_out, int64_t *sums_out,
                        int32_t *labels_out)
{
    TRY(use(c));
    FrontierShape plan;
    TRY(check_frontiers(__func__, c, g, B, grid_of_batch, radius, min_unknown, min_clear2, cap, min_size, max_clusters, count_out,
                        clusters_out, sums_out, plan));
    const size_t rows = (size_t)B * max_clusters;
    int32_t *d_g, *d_cnt, *d_cl, *d_lab; int64_t *d_sums;
    Staging s(c);
    s.in(d_g, grid_of_batch, B).out(d_cnt, count_out, (size_t)B * 2).out(d_cl, clusters_out, rows * 8).out(d_sums, sums_out, rows * 2)
        .out(d_lab, labels_out, (size_t)B * g->d.xw * g->d.yw);
    TRY(s.upload());
    TRY(frontiers_dev(__func__, c, g, B, d_g, radius, min_unknown, min_clear2, cap, min_size, max_clusters, d_cnt, d_cl, d_sums, d_lab));
    return s.download();
}

// ---- travel-cost field (travel_kernels.hip) ---------------------------------------------------------------------------
static int check_travel(const char *fn, const slam_ctx *c, const slam_grid *g, int B, const int32_t *grid_of_batch, const int32_t *sources,
                        int S, int foot, int min_clear2, int cap, const int32_t *goals, int Q, int path_cap, const int32_t *status_out,
                        const int32_t *cost_out, const int8_t *dir_out, const int32_t *goal_cost_out, const int32_t *path_len_out,
                        const int32_t *path_out, TravelShape &plan)
{
    REQUIRE_IN(fn, g && sources && status_out, "null pointer");
    REQUIRE_IN(fn, B >= 1, "B < 1");
    REQUIRE_IN(fn, grid_of_batch || B <= g->d.G, "B > G without grid_of_batch (query b reads map b)");
    REQUIRE_IN(fn, S >= 1 && S <= kTravelMaxSources, "S outside [1, 64]");
    REQUIRE_IN(fn, foot >= 0 && foot <= kTravelMaxFoot, "foot outside [0, 8]");
    REQUIRE_IN(fn, min_clear2 >= 0, "min_clear2 < 0");
    if (min_clear2 > 0) {
        REQUIRE_IN(fn, cap >= 1 && cap <= 32767, "cap outside [1, 32767]");
        REQUIRE_IN(fn, min_clear2 <= cap, "min_clear2 > cap");
    }
    const long cells = (long)g->d.xw * g->d.yw;
    REQUIRE_IN(fn, Q >= 0 && Q <= kTravelMaxGoals, "Q outside [0, 65536]");
    REQUIRE_IN(fn, path_cap >= 0 && path_cap <= cells, "path_cap outside [0, xw * yw]");
    REQUIRE_IN(fn, (long)B * std::max(Q, 1) * std::max(path_cap, 1) < (1L << 31), "B * max(Q, 1) * max(path_cap, 1) >= 2^31");
    REQUIRE_IN(fn, (long)kTravelDiagonal * cells < (1L << 31), "a map of 2^31 / 14 cells or more: a cost may overflow");
    const bool with_goals = goals && Q > 0;
    REQUIRE_IN(fn, !with_goals || (goal_cost_out && path_len_out && (path_cap == 0 || path_out)), "goals without their outputs");
    REQUIRE_IN(fn, cost_out || dir_out || with_goals, "no output asked for");
    plan = travel_plan_for(g->d.xw, g->d.yw, cost_out == nullptr, B, c->travel_ws_bytes, kLdsGuard);
    if (!plan.ok)
        return fail(SLAM_ERR_INVALID, "%s: the workspace of one query (%ld bytes) does not fit the context option travel_ws_mb (%ld bytes)",
                    fn, plan.query_bytes, c->travel_ws_bytes);
    return SLAM_OK;
}

static int travel_dev(const char *fn, slam_ctx *c, slam_grid *g, int B, const int32_t *grid_of_batch, const int32_t *sources, int S,
                      int foot, int through_unknown, int min_clear2, int cap, const int32_t *goals, int Q, int path_cap,
                      int32_t *status_out, int32_t *cost_out, int8_t *dir_out, int32_t *goal_cost_out, int32_t *path_len_out,
                      int32_t *path_out)
{
    TravelShape plan;
    TRY(check_travel(fn, c, g, B, grid_of_batch, sources, S, foot, min_clear2, cap, goals, Q, path_cap, status_out, cost_out, dir_out,
                     goal_cost_out, path_len_out, path_out, plan));
    const size_t cells = (size_t)g->d.xw * g->d.yw;
    const size_t mask_words = (size_t)plan.chunk_queries * plan.mask_words;
    const size_t dirty_words = (size_t)plan.chunk_queries * plan.tiles;
    TravelArgs a;
    Layout ws;
    ws.add(a.mask, mask_words).add(a.dirty, dirty_words);
    if (!cost_out) ws.add(a.ws_cost, (size_t)plan.chunk_queries * cells);
    if (min_clear2 > 0) {       // the field of all G maps, as slam_grid_match builds it
        int16_t *field = nullptr;
        TRY(build_field(c, g, cap, ws, field));
        a.field = field;
    } else {
        TRY(grid_on_main(c));
        TRY(reserve(c, c->scratch, ws));
    }
    a.g = g->d;
    a.maps = grid_of_batch;
    a.sources = sources;
    a.goals = Q > 0 ? goals : nullptr;
    a.B = B; a.S = S; a.foot = foot; a.through_unknown = through_unknown != 0; a.min_clear2 = min_clear2; a.Q = Q; a.path_cap = path_cap;
    a.status_out = status_out; a.cost_out = cost_out; a.dir_out = dir_out;
    a.goal_cost_out = goal_cost_out; a.path_len_out = path_len_out; a.path_out = path_out;
    Timed t(c, SLAM_K_GRID);
    for (long b0 = 0; b0 < B; b0 += plan.chunk_queries)
        HIPCHK(launch_travel(a, plan, b0, std::min(plan.chunk_queries, (long)B - b0), c->stream));
    return SLAM_OK;
}

int slam_grid_travel_dev(slam_ctx *c, slam_grid *g, int B, const int32_t *grid_of_batch, const int32_t *sources, int S, int foot,
                         int through_unknown, int min_clear2, int cap, const int32_t *goals, int Q, int path_cap, int32_t *status_out,
                         int32_t *cost_out, int8_t *dir_out, int32_t *goal_cost_out, int32_t *path_len_out, int32_t *path_out)
{
    TRY(use(c));
    return travel_dev(__func__, c, g, B, grid_of_batch, sources, S, foot, through_unknown, min_clear2, cap, goals, Q, path_cap, status_out,
                      cost_out, dir_out, goal_cost_out, path_len_out, path_out);
}

int slam_grid_travel(slam_ctx *c, slam_grid *g, int B, const int32_t *grid_of_batch, const int32_t *sources, int S, int foot,
                     int through_unknown, int min_clear2, int cap, const int32_t *goals, int Q, int path_cap, int32_t *status_out,
                     int32_t *cost_out, int8_t *dir_out, int32_t *goal_cost_out, int32_t *path_len_out, int32_t *path_out)
{
    TRY(use(c));
    TravelShape plan;
    TRY(check_travel(__func__, c, g, B, grid_of_batch, sources, S, foot, min_clear2, cap, goals, Q, path_cap, status_out, cost_out,
                     dir_out, goal_cost_out, path_len_out, path_out, plan));
    const size_t cells = (size_t)B * g->d.xw * g->d.yw, rows = (size_t)B * Q;
    const bool with_goals = goals && Q > 0;
    int32_t *d_g, *d_src, *d_goals, *d_status, *d_cost, *d_gc, *d_len, *d_path; int8_t *d_dir;
    Staging s(c);
    s.in(d_g, grid_of_batch, B).in(d_src, sources, (size_t)B * S * 2).in(d_goals, with_goals ? goals : nullptr, rows * 2)
        .out(d_status, status_out, B).out(d_cost, cost_out, cells).out(d_dir, dir_out, cells)
        .out(d_gc, with_goals ? goal_cost_out : nullptr, rows).out(d_len, with_goals ? path_len_out : nullptr, rows)
        .out(d_path, with_goals ? path_out : nullptr, rows * path_cap * 2);
    TRY(s.upload());
    TRY(travel_dev(__func__, c, g, B, d_g, d_src, S, foot, through_unknown, min_clear2, cap, d_goals, Q, path_cap, d_status, d_cost, d_dir,
                   d_gc, d_len, d_path));
    return s.download();
}

// ---- Monte Carlo localisation on the distance field (mcl_kernels.hip) ----------------------------------------------
static int check_mcl_shape(const char *fn, int F, int P)
{
    REQUIRE_IN(fn, F >= 1, "F < 1");
    REQUIRE_IN(fn, P >= 1 && P <= (1 << 20), "P outside [1, 2^20]");
    REQUIRE_IN(fn, (long)F * P < (1L << 31), "F * P >= 2^31");
    return SLAM_OK;
}

static int check_mcl_weigh(const char *fn, const slam_grid *g, const double *poses, const double *motion, const double *noise,
                           const float *ranges, const double *cos_t, const double *sin_t, int F, int P, int n, float max_range,
                           int cap)
{
    REQUIRE_IN(fn, g && poses && ranges && cos_t && sin_t, "null pointer");
    TRY(check_mcl_shape(fn, F, P));
    REQUIRE_IN(fn, n >= 1 && n <= 4096, "n outside [1, 4096]");
    REQUIRE_IN(fn, (long)F * n < (1L << 31), "F * n >= 2^31");
    REQUIRE_IN(fn, cap >= 1 && cap <= 32767, "cap outside [1, 32767]");
    REQUIRE_IN(fn, max_range > 0, "max_range must be > 0");
    REQUIRE_IN(fn, motion || !noise, "noise without motion");
    return SLAM_OK;
}

int slam_mcl_weigh_dev(slam_ctx *c, slam_grid *g, double *poses, const double *motion, const double *noise, const float *ranges,
                       const double *cos_t, const double *sin_t, const int32_t *grid_of_filter, int F, int P, int n,
                       float max_range, int cap, const int16_t *field, int32_t *acc, int32_t *cost_out, int32_t *used_out)
{
    TRY(use(c));
    TRY(check_mcl_weigh(__func__, g, poses, motion, noise, ranges, cos_t, sin_t, F, P, n, max_range, cap));
    int16_t *built = nullptr;
    if (!field) TRY(build_field(c, g, cap, Layout(), built));
    else TRY(grid_on_main(c));
    MclWeighArgs a;
    a.g = g->d; a.field = field ? field : built;
    a.poses = poses; a.motion = motion; a.noise = noise; a.ranges = ranges; a.cos_t = cos_t; a.sin_t = sin_t;
    a.maps = grid_of_filter; a.F = F; a.P = P; a.n = n; a.max_range = max_range; a.cap = cap;
    a.acc = acc; a.cost_out = cost_out; a.used_out = used_out;
    Timed t(c, SLAM_K_GRID);
    HIPCHK(launch_mcl_weigh(a, c->mcl_shape, c->stream));
    return SLAM_OK;
}

int slam_mcl_weigh(slam_ctx *c, slam_grid *g, double *poses, const double *motion, const double *noise, const float *ranges,
                   const double *cos_t, const double *sin_t, const int32_t *grid_of_filter, int F, int P, int n, float max_range,
                   int cap, const int16_t *field, int32_t *acc, int32_t *cost_out, int32_t *used_out)
{
    TRY(use(c));
    TRY(check_mcl_weigh(__func__, g, poses, motion, noise, ranges, cos_t, sin_t, F, P, n, max_range, cap));
    const size_t FP = (size_t)F * P;
    double *d_p, *d_m, *d_n, *d_c, *d_s; float *d_r; int32_t *d_g, *d_acc, *d_cost, *d_used; int16_t *d_f;
    Staging s(c);
    s.inout(d_p, poses, FP * 3).in(d_m, motion, (size_t)F * 3).in(d_n, noise, FP * 3).in(d_r, ranges, (size_t)F * n).in(d_c, cos_t, n)
        .in(d_s, sin_t, n).in(d_g, grid_of_filter, F).in(d_f, field, (size_t)g->d.G * g->d.xw * g->d.yw).inout(d_acc, acc, FP)
        .out(d_cost, cost_out, FP).out(d_used, used_out, F);
    TRY(s.upload());
    TRY(slam_mcl_weigh_dev(c, g, d_p, d_m, d_n, d_r, d_c, d_s, d_g, F, P, n, max_range, cap, d_f, d_acc, d_cost, d_used));
    return s.download();
}

static int check_mcl_resample(const char *fn, const double *poses, const int32_t *acc, const uint32_t *table, int T, int shift,
                              const double *u0, double ess_frac, int F, int P, const double *poses_out, const double *est_out,
                              const int32_t *info_out)
{
    REQUIRE_IN(fn, poses && acc && table && u0 && poses_out && est_out && info_out, "null pointer");
    TRY(check_mcl_shape(fn, F, P));
    REQUIRE_IN(fn, T >= 1 && T <= 65536, "T outside [1, 65536]");
    REQUIRE_IN(fn, shift >= 0 && shift <= 30, "shift outside [0, 30]");
    REQUIRE_IN(fn, ess_frac >= 0, "ess_frac must be >= 0 and not NaN");
    REQUIRE_IN(fn, poses_out != poses, "poses_out must not be poses");
    return SLAM_OK;
}

int slam_mcl_resample_dev(slam_ctx *c, const double *poses, int32_t *acc, const uint32_t *table, int T, int shift, const double *u0,
                          double ess_frac, int F, int P, double *poses_out, int32_t *ancestors_out, double *est_out,
                          int32_t *info_out)
{
    TRY(use(c));
    TRY(streams_on_main(c));
    TRY(check_mcl_resample(__func__, poses, acc, table, T, shift, u0, ess_frac, F, P, poses_out, est_out, info_out));
    const size_t FP = (size_t)F * P, FB = (size_t)F * mcl_scan_blocks(P);
    MclResampleArgs a;
    Layout ws;
    ws.add(a.keys, F).add(a.live, F).add(a.cum, FP).add(a.bsum, FB).add(a.bq, FB).add(a.bpart, FB * 4).add(a.fpar, (size_t)F * 2);
    TRY(reserve(c, c->scratch, ws));
    a.poses = poses; a.acc = acc; a.table = table; a.T = T; a.shift = shift; a.u0 = u0; a.ess_frac = ess_frac; a.F = F; a.P = P;
    a.poses_out = poses_out; a.ancestors_out = ancestors_out; a.est_out = est_out; a.info_out = info_out;
    HIPCHK(hipMemsetAsync(a.keys, 0xff, (size_t)F * 8, c->stream));
    HIPCHK(hipMemsetAsync(a.live, 0, (size_t)F * 4, c->stream));
    Timed t(c, SLAM_K_GRID);
    HIPCHK(launch_mcl_resample(a, c->stream));
    return SLAM_OK;
}

int slam_mcl_resample(slam_ctx *c, const double *poses, int32_t *acc, const uint32_t *table, int T, int shift, const double *u0,
                      double ess_frac, int F, int P, double *poses_out, int32_t *ancestors_out, double *est_out, int32_t *info_out)
{
    TRY(use(c));
    TRY(check_mcl_resample(__func__, poses, acc, table, T, shift, u0, ess_frac, F, P, poses_out, est_out, info_out));
    for (int f = 0; f < F; ++f) REQUIRE(u0[f] >= 0.0 && u0[f] < 1.0, "u0 outside [0, 1)");
    for (int k = 0; k < T; ++k) REQUIRE(table[k] <= (1u << 20), "table entry above 2^20");
    const size_t FP = (size_t)F * P;
    double *d_p, *d_u, *d_po, *d_est; int32_t *d_acc, *d_anc, *d_info; uint32_t *d_t;
    Staging s(c);
    s.in(d_p, poses, FP * 3).inout(d_acc, acc, FP).in(d_t, table, T).in(d_u, u0, F).out(d_po, poses_out, FP * 3)
        .out(d_anc, ancestors_out, FP).out(d_est, est_out, (size_t)F * 4).out(d_info, info_out, (size_t)F * 4);
    TRY(s.upload());
    TRY(slam_mcl_resample_dev(c, d_p, d_acc, d_t, T, shift, d_u, ess_frac, F, P, d_po, d_anc, d_est, d_info));
    return s.download();
}

// ---- grid FastSLAM: a map per particle that follows resampling ------------------------------
static int check_mcl_weigh_maps(const char *fn, const slam_grid *g, const int32_t *grid_of_particle, int F, int P)
{
    REQUIRE_IN(fn, grid_of_particle || (long)F * P <= g->d.G, "grid_of_particle is null and F * P > G");
    return SLAM_OK;
}

int slam_mcl_weigh_maps_dev(slam_ctx *c, slam_grid *g, double *poses, const double *motion, const double *noise, const float *ranges,
                            const double *cos_t, const double *sin_t, const int32_t *grid_of_particle, int F, int P, int n,
                            float max_range, int cap, const int16_t *field, int32_t *acc, int32_t *cost_out, int32_t *used_out)
{
    TRY(use(c));
    TRY(check_mcl_weigh(__func__, g, poses, motion, noise, ranges, cos_t, sin_t, F, P, n, max_range, cap));
    TRY(check_mcl_weigh_maps(__func__, g, grid_of_particle, F, P));
    int16_t *built = nullptr;
    if (!field) TRY(build_field(c, g, cap, Layout(), built));
    else TRY(grid_on_main(c));
    MclWeighArgs a;
    a.g = g->d; a.field = field ? field : built;
    a.poses = poses; a.motion = motion; a.noise = noise; a.ranges = ranges; a.cos_t = cos_t; a.sin_t = sin_t;
    a.own_maps = 1; a.pmaps = grid_of_particle; a.F = F; a.P = P; a.n = n; a.max_range = max_range; a.cap = cap;
    a.acc = acc; a.cost_out = cost_out; a.used_out = used_out;
    Timed t(c, SLAM_K_GRID);
    HIPCHK(launch_mcl_weigh(a, c->mcl_shape, c->stream));
    return SLAM_OK;
}

int slam_mcl_weigh_maps(slam_ctx *c, slam_grid *g, double *poses, const double *motion, const double *noise, const float *ranges,
                        const double *cos_t, const double *sin_t, const int32_t *grid_of_particle, int F, int P, int n,
                        float max_range, int cap, const int16_t *field, int32_t *acc, int32_t *cost_out, int32_t *used_out)
{
    TRY(use(c));
    TRY(check_mcl_weigh(__func__, g, poses, motion, noise, ranges, cos_t, sin_t, F, P, n, max_range, cap));
    TRY(check_mcl_weigh_maps(__func__, g, grid_of_particle, F, P));
    const size_t FP = (size_t)F * P;
    double *d_p, *d_m, *d_n, *d_c, *d_s; float *d_r; int32_t *d_g, *d_acc, *d_cost, *d_used; int16_t *d_f;
    Staging s(c);
    s.inout(d_p, poses, FP * 3).in(d_m, motion, (size_t)F * 3).in(d_n, noise, FP * 3).in(d_r, ranges, (size_t)F * n).in(d_c, cos_t, n)
        .in(d_s, sin_t, n).in(d_g, grid_of_particle, FP).in(d_f, field, (size_t)g->d.G * g->d.xw * g->d.yw).inout(d_acc, acc, FP)
        .out(d_cost, cost_out, FP).out(d_used, used_out, F);
    TRY(s.upload());
    TRY(slam_mcl_weigh_maps_dev(c, g, d_p, d_m, d_n, d_r, d_c, d_s, d_g, F, P, n, max_range, cap, d_f, d_acc, d_cost, d_used));
    return s.download();
}

static int check_mcl_settle(const char *fn, const int32_t *ancestors, const double *poses_src, int F, int P, int map0,
                            const int32_t *settled_out, const double *poses_out)
{
    REQUIRE_IN(fn, ancestors && settled_out, "null pointer");
    REQUIRE_IN(fn, F >= 1, "F < 1");
    REQUIRE_IN(fn, P >= 1 && P <= kMclSettleMaxP, "P outside [1, 4096]");
    REQUIRE_IN(fn, (long)F * P < (1L << 31), "F * P >= 2^31");
    REQUIRE_IN(fn, map0 >= 0 && (long)map0 + (long)F * P < (1L << 31), "map0 < 0 or map0 + F * P >= 2^31");
    REQUIRE_IN(fn, !poses_out || poses_src, "poses_out without poses_src");
    REQUIRE_IN(fn, !poses_out || poses_out != poses_src, "poses_out must not be poses_src");
    return SLAM_OK;
}

int slam_mcl_settle_dev(slam_ctx *c, const int32_t *ancestors, const double *poses_src, int F, int P, int map0, int32_t *settled_out,
                        double *poses_out, int32_t *map_src_out, int32_t *moved_out)
{
    TRY(use(c));
    TRY(streams_on_main(c));
    TRY(check_mcl_settle(__func__, ancestors, poses_src, F, P, map0, settled_out, poses_out));
    MclSettleArgs a;
    a.ancestors = ancestors; a.poses_src = poses_src; a.F = F; a.P = P; a.map0 = map0;
    a.settled = settled_out; a.poses_out = poses_out; a.map_src = map_src_out; a.moved = moved_out; a.status = c->status;
    Timed t(c, SLAM_K_GRID);
    HIPCHK(launch_mcl_settle(a, c->stream));
    return SLAM_OK;
}

int slam_mcl_settle(slam_ctx *c, const int32_t *ancestors, const double *poses_src, int F, int P, int map0, int32_t *settled_out,
                    double *poses_out, int32_t *map_src_out, int32_t *moved_out)
{
    TRY(use(c));
    TRY(check_mcl_settle(__func__, ancestors, poses_src, F, P, map0, settled_out, poses_out));
    const size_t FP = (size_t)F * P;
    for (size_t i = 0; i < FP; ++i) REQUIRE(ancestors[i] >= 0 && ancestors[i] < P, "ancestor outside [0, P)");
    int32_t *d_a, *d_set, *d_map, *d_mov; double *d_p, *d_po;
    Staging s(c);
    s.in(d_a, ancestors, FP).in(d_p, poses_out ? poses_src : nullptr, FP * 3).out(d_set, settled_out, FP).out(d_po, poses_out, FP * 3)
        .out(d_map, map_src_out, FP).out(d_mov, moved_out, F);
    TRY(s.upload());
    TRY(slam_mcl_settle_dev(c, d_a, d_p, F, P, map0, d_set, d_po, d_map, d_mov));
    return s.download();
}

static int check_copy_maps(const char *fn, const slam_grid *g, const int32_t *src, int first, int count)
{
    REQUIRE_IN(fn, g && src, "null pointer");
    REQUIRE_IN(fn, first >= 0 && count >= 1 && (long)first + count <= g->d.G, "first < 0, count < 1 or first + count > G");
    return SLAM_OK;
}

int slam_grid_copy_maps_dev(slam_ctx *c, slam_grid *g, const int32_t *src, int first, int count, int32_t *copied_out)
{
    TRY(use(c));
    TRY(check_copy_maps(__func__, g, src, first, count));
    TRY(grid_on_main(c));
    // a live pmap is copied with its counters: one that was current stays current, a stale one stays marked stale
    Timed t(c, SLAM_K_GRID);
    HIPCHK(launch_grid_copy_maps(g->d, src, first, count, copied_out, c->stream));
    return SLAM_OK;
}

int slam_grid_copy_maps(slam_ctx *c, slam_grid *g, const int32_t *src, int first, int count, int32_t *copied_out)
{
    TRY(use(c));
    TRY(check_copy_maps(__func__, g, src, first, count));
    for (int k = 0; k < count; ++k) {
        const int s = src[k];
        const bool kept = s == first + k || s < 0 || s >= g->d.G;
        REQUIRE(kept || s < first || s - first >= count || src[s - first] == s, "a source is itself a destination of this call");
    }
    int32_t *d_src, *d_out;
    Staging s(c);
    s.in(d_src, src, count).out(d_out, copied_out, count);
    TRY(s.upload());
    TRY(slam_grid_copy_maps_dev(c, g, d_src, first, count, d_out));
    return s.download();
}

static int check_update_particles(const char *fn, const slam_grid *g, const float *ranges, const double *cos_t, const double *sin_t,
                                  const double *poses, int F, int P, int n, int map0)
{
    REQUIRE_IN(fn, g && ranges && cos_t && sin_t && poses, "null pointer");
    REQUIRE_IN(fn, F >= 1 && P >= 1 && n >= 1 && n <= 65535, "F < 1, P < 1 or n outside [1, 65535]");
    REQUIRE_IN(fn, map0 >= 0 && (long)map0 + (long)F * P <= g->d.G, "map0 < 0 or map0 + F * P > G");
    return SLAM_OK;
}

// One scan per particle into its own map, through the window path as slam_particles_dev casts its hypotheses: a live
// pmap stays current.  A launch takes at most 65 535 particles (one workgroup row each).  The caller has checked the
// arguments and joined the internal streams (slam_grid_update_particles_dev, and slam_track_dev once per scan).
static int cast_particles(slam_ctx *c, slam_grid *g, const float *ranges, const double *cos_t, const double *sin_t,
                          const double *poses, const int32_t *acc, int F, int P, int n, int map0)
{
    g->pristine = false;
    const long L = (long)F * P, span = 65535;
    Timed t(c, SLAM_K_GRID);
    for (long l0 = 0; l0 < L; l0 += span) {
        const int cnt = (int)std::min(span, L - l0);
        GridDev d = g->d;                                              // the chunk's maps
        const size_t off = ((size_t)map0 + (size_t)l0) * d.xw * d.yw;
        d.G = cnt; d.pass += off; d.hit += off;
        if (d.pmap_live) d.pmap_live += off;
        CastRequest r;
        r.ranges = ranges; r.cos_t = cos_t; r.sin_t = sin_t; r.poses = poses + 3 * (size_t)l0; r.acc = acc ? acc + l0 : nullptr;
        r.L = cnt; r.scans = 1; r.n = n; r.particles = true; r.per_filter = P; r.first_particle = l0; r.group = 1;
        r.lds_hits = c->win_lds_hits;
        HIPCHK(launch_cast(d, plan_cast(d, c->grid_mode, r), r, nullptr, 0, c->stream));
    }
    return SLAM_OK;
}

int slam_grid_update_particles_dev(slam_ctx *c, slam_grid *g, const float *ranges, const double *cos_t, const double *sin_t,
                                   const double *poses, const int32_t *acc, int F, int P, int n, int map0)
{
    TRY(use(c));
    TRY(check_update_particles(__func__, g, ranges, cos_t, sin_t, poses, F, P, n, map0));
    TRY(grid_on_main(c));
    return cast_particles(c, g, ranges, cos_t, sin_t, poses, acc, F, P, n, map0);
}

int slam_grid_update_particles(slam_ctx *c, slam_grid *g, const float *ranges, const double *cos_t, const double *sin_t,
                               const double *poses, const int32_t *acc, int F, int P, int n, int map0)
{
    TRY(use(c));
    TRY(check_update_particles(__func__, g, ranges, cos_t, sin_t, poses, F, P, n, map0));
    const size_t FP = (size_t)F * P;
    float *d_r; double *d_c, *d_s, *d_p; int32_t *d_a;
    Staging s(c);
    s.in(d_r, ranges, (size_t)F * n).in(d_c, cos_t, n).in(d_s, sin_t, n).in(d_p, poses, FP * 3).in(d_a, acc, FP);
    TRY(s.upload());
    TRY(slam_grid_update_particles_dev(c, g, d_r, d_c, d_s, d_p, d_a, F, P, n, map0));
    return check_status_sync(c);
}

// ---- the scan-to-map tracker: match, refine, integrate per scan (track_kernels.hip, include/slam_track.h) -----------
static int check_track(const char *fn, const slam_grid *g, const float *ranges, int L, int S, const double *cos_t, const double *sin_t,
                       int n, const double *rot_off, const double *rot_off_cs, int K, int nx, int ny, double step, int iters,
                       double damping, double step_cells, double step_rad, float max_range, int cap, int min_used, double gate_dist,
                       double gate_turn, int map0, const double *state, const double *poses_out, const int32_t *info_out)
{
    REQUIRE_IN(fn, g && rot_off && state && poses_out && info_out, "null pointer");
    REQUIRE_IN(fn, L >= 1 && S >= 1, "L < 1 or S < 1");
    REQUIRE_IN(fn, n >= 1 && (long)L * S * n < (1L << 31), "n < 1 or L * S * n >= 2^31");
    // (the matcher's and the refinement's own checks, on the arrays they will be given: the outputs are workspace)
    TRY(check_match(fn, g, ranges, state, L, cos_t, sin_t, n, rot_off_cs, K, nx, ny, step, max_range, cap, info_out, info_out));
    TRY(check_refine(fn, g, ranges, state, L, cos_t, sin_t, n, iters, damping, step_cells, step_rad, max_range, cap, poses_out, poses_out,
                     info_out));
    REQUIRE_IN(fn, map0 >= 0 && (long)map0 + L <= g->d.G, "map0 < 0 or map0 + L > G");
    REQUIRE_IN(fn, min_used >= 1, "min_used < 1");
    REQUIRE_IN(fn, gate_dist >= 0 && gate_turn >= 0, "gate_dist and gate_turn must be >= 0 (+inf: never)");      // (false for NaN)
    return SLAM_OK;
}

int slam_track_dev(slam_ctx *c, slam_grid *g, const float *ranges, const double *motion, int L, int S, const double *cos_t,
                   const double *sin_t, int n, const double *rot_off, const double *rot_off_cs, int K, int nx, int ny, double step,
                   int iters, double damping, double step_cells, double step_rad, float max_range, int cap, int min_used,
                   double gate_dist, double gate_turn, int map0, double *state, double *poses_out, int32_t *info_out, double *trace_out)
{
    TRY(use(c));
    TRY(check_track(__func__, g, ranges, L, S, cos_t, sin_t, n, rot_off, rot_off_cs, K, nx, ny, step, iters, damping, step_cells,
                    step_rad, max_range, cap, min_used, gate_dist, gate_turn, map0, state, poses_out, info_out));
    TRY(grid_on_main(c));
    // Every piece of every scan's workspace, reserved ONCE: growing the arena synchronises and frees, which nothing may do
    // while the loop's kernels are in flight.
    TrackArgs a;
    FieldPieces fp;
    int16_t *field = nullptr;
    Layout ws;
    field_layout(g, ws, fp, field);
    ws.add(a.scan, (size_t)L * n).add(a.pred, (size_t)L * 5).add(a.centres, (size_t)L * 2).add(a.rot_cs, (size_t)L * K * 2)
        .add(a.match_maps, L).add(a.keys, L).add(a.best, L).add(a.best_cost, L).add(a.used, L).add(a.start, (size_t)L * 3)
        .add(a.refine_maps, L).add(a.refined, (size_t)L * 3).add(a.refine_cost, (size_t)L * 2).add(a.refine_status, L).add(a.acc, L)
        .add(a.cast_pose, (size_t)L * 3);
    TRY(reserve(c, c->scratch, ws));
    a.ranges = ranges; a.motion = motion; a.rot_off = rot_off; a.rot_off_cs = rot_off_cs;
    a.L = L; a.S = S; a.n = n; a.K = K; a.nx = nx; a.ny = ny; a.step = step; a.min_used = min_used; a.map0 = map0;
    a.gate_dist = gate_dist; a.gate_turn = gate_turn; a.scale = g->d.scale; a.off_x = g->d.off_x; a.off_y = g->d.off_y;
    a.state = state; a.poses_out = poses_out; a.info_out = info_out; a.trace_out = trace_out;
    MatchArgs m;
    m.g = g->d; m.field = field; m.ranges = a.scan; m.range_stride = n; m.centres = a.centres; m.maps = a.match_maps;
    m.cos_t = cos_t; m.sin_t = sin_t; m.rot_cs = a.rot_cs; m.B = L; m.n = n; m.K = K; m.nx = nx; m.ny = ny; m.step = step;
    m.max_range = max_range; m.cap = cap; m.keys = a.keys; m.best_out = a.best; m.best_cost_out = a.best_cost; m.used_out = a.used;
    RefineArgs r;
    r.g = g->d; r.field = field; r.ranges = a.scan; r.range_stride = n; r.poses = a.start; r.maps = a.refine_maps;
    r.cos_t = cos_t; r.sin_t = sin_t; r.B = L; r.n = n; r.iters = iters; r.damping = damping; r.step_xy = step_cells / g->d.scale;
    r.step_rad = step_rad; r.max_range = max_range; r.cap = cap; r.pose_out = a.refined; r.cost_out = a.refine_cost;
    r.status_out = a.refine_status;
    for (int s = 0; s < S; ++s) {
        TRY(enqueue_field(c, g, cap, fp, field));                     // the map as every earlier scan left it
        {
            Timed t(c, SLAM_K_GRID);
            HIPCHK(launch_track_predict(a, s, c->stream));
            HIPCHK(launch_match(m, c->stream));
            HIPCHK(launch_track_seed(a, c->stream));
            HIPCHK(launch_refine(r, c->stream));
            HIPCHK(launch_track_decide(a, s, c->stream));
        }
        TRY(cast_particles(c, g, a.scan, cos_t, sin_t, a.cast_pose, a.acc, L, 1, n, map0));
    }
    return SLAM_OK;
}

int slam_track(slam_ctx *c, slam_grid *g, const float *ranges, const double *motion, int L, int S, const double *cos_t,
               const double *sin_t, int n, const double *rot_off, const double *rot_off_cs, int K, int nx, int ny, double step, int iters,
               double damping, double step_cells, double step_rad, float max_range, int cap, int min_used, double gate_dist,
               double gate_turn, int map0, double *state, double *poses_out, int32_t *info_out, double *trace_out)
{
    TRY(use(c));
    TRY(check_track(__func__, g, ranges, L, S, cos_t, sin_t, n, rot_off, rot_off_cs, K, nx, ny, step, iters, damping, step_cells,
                    step_rad, max_range, cap, min_used, gate_dist, gate_turn, map0, state, poses_out, info_out));
    const size_t LS = (size_t)L * S;
    float *d_r; double *d_m, *d_c, *d_s, *d_ro, *d_rc, *d_st, *d_po, *d_tr; int32_t *d_in;
    Staging s(c);
    s.in(d_r, ranges, LS * n).in(d_m, motion, LS * 3).in(d_c, cos_t, n).in(d_s, sin_t, n).in(d_ro, rot_off, K)
        .in(d_rc, rot_off_cs, (size_t)K * 2).inout(d_st, state, (size_t)L * SLAM_TRACK_STATE_LEN).out(d_po, poses_out, LS * 3)
        .out(d_in, info_out, LS * SLAM_TRACK_INFO_LEN).out(d_tr, trace_out, LS * SLAM_TRACK_TRACE_LEN);
    TRY(s.upload());
    TRY(slam_track_dev(c, g, d_r, d_m, L, S, d_c, d_s, n, d_ro, d_rc, K, nx, ny, step, iters, damping, step_cells, step_rad, max_range,
                       cap, min_used, gate_dist, gate_turn, map0, d_st, d_po, d_in, d_tr));
    TRY(s.download());
    return check_status_sync(c);
}

int slam_bresenham_batch(slam_ctx *c, const int32_t *starts, const int32_t *ends, int B, const int64_t *offsets,
                         int32_t *lens_out, int32_t *cells_out, int64_t total_cells)
{
    TRY(use(c));
    REQUIRE(starts && ends && lens_out, "null pointer");
    REQUIRE(B > 0, "B must be positive");
    REQUIRE(!cells_out || (offsets && total_cells >= 0), "cells_out needs offsets and total_cells");
    for (int b = 0; b < B; ++b) {
        int64_t dx = (int64_t)ends[2 * b] - starts[2 * b], dy = (int64_t)ends[2 * b + 1] - starts[2 * b + 1];
        int64_t len = std::max(std::llabs(dx), std::llabs(dy)) + 1;
        if (len > 2 * (int64_t)kMaxRayCells) return fail(SLAM_ERR_OVERFLOW, "line %d longer than 2^21 cells", b);
        if (cells_out && (offsets[b] < 0 || offsets[b] + len > total_cells))
            return fail(SLAM_ERR_INVALID, "line %d does not fit cells_out", b);
    }
    int32_t *d_s, *d_e, *d_l, *d_c; int64_t *d_o;
    Staging s(c);
    s.in(d_s, starts, (size_t)B * 2).in(d_e, ends, (size_t)B * 2).in(d_o, cells_out ? offsets : nullptr, B);
    s.out(d_l, lens_out, B).out(d_c, cells_out, cells_out ? (size_t)total_cells * 2 : 0);
    TRY(s.upload());
    {
        Timed t(c, SLAM_K_BRESENHAM);
        HIPCHK(launch_bresenham(d_s, d_e, B, d_o, d_l, d_c, c->stream));
    }
    return s.download();
}

/* ---- fused replay ------------------------------------------------------------------ */

static int check_replay(const char *fn, const float *ranges, const double *cos_t, const double *sin_t, int L, int n_scan,
                        int n, int dtype, int max_iter, const double *pose0, const double *poses_out)
{
    REQUIRE_IN(fn, ranges && cos_t && sin_t && pose0 && poses_out, "null pointer");
    REQUIRE_IN(fn, L > 0 && n_scan >= 2 && n > 0, "need L > 0, n_scan >= 2, n > 0");
    REQUIRE_IN(fn, max_iter >= 0, "max_iter must be >= 0");
    REQUIRE_IN(fn, dtype_size(dtype), "unknown dtype");
    REQUIRE_IN(fn, n <= 8192, "n too large (max 8192 beams)");
    REQUIRE_IN(fn, (long)L * (n_scan - 1) < (1L << 31), "too many scan pairs for one launch");
    return SLAM_OK;
}

int slam_replay_dev(slam_ctx *c, const float *ranges, const double *cos_t, const double *sin_t, int L, int n_scan, int n,
                    int dtype, int max_iter, double tol, const double *pose0, slam_grid *grid, const int32_t *grid_of_traj,
                    void *pts_ws, double *poses_out, double *T_out, int32_t *iters_out)
{
    TRY(use(c));
    TRY(check_replay(__func__, ranges, cos_t, sin_t, L, n_scan, n, dtype, max_iter, pose0, poses_out));
    (void)pts_ws;   // kept in the ABI; the point buffers are no longer materialised
    const long pairs = (long)L * (n_scan - 1);
    const bool piped = c->pipeline && grid;     // three stages on three streams: ICP | compose | map
    if (!piped) TRY(streams_on_main(c));        // everything on the main stream: pose0 may be a row of a piped replay's poses_out
    double *T = T_out;
    if (!T) {
        if (piped) {                            // two alternating buffers: compose of replay k reads T while ICP k+1 runs
            size_t need = align_up((size_t)pairs * 72);
            if (need > c->pipe_T_bytes) {
                TRY(join_from_grid(c));
                HIPCHK(hipStreamSynchronize(c->stream));
                for (double *&t : c->pipe_T) {
                    if (t) HIPCHK(hipFree(t));
                    t = nullptr;
                    if (hipMalloc(reinterpret_cast<void **>(&t), need) != hipSuccess)
                        return fail(SLAM_ERR_NOMEM, "hipMalloc(%zu bytes) for T", need);
                }
                c->pipe_T_bytes = need;
            }
            T = c->pipe_T[c->cast_pos];
        } else {
            TRY(reserve(c, c->scratch, Layout().add(T, (size_t)pairs * 9)));
        }
    }
    if (c->pipeline)        // is an earlier replay's compose / ray cast still reading these buffers?
        for (int k = 0; k < 2; ++k)
            if (c->cast_poses[k] && (c->cast_poses[k] == poses_out || c->cast_T[k] == T)) {
                HIPCHK(hipStreamWaitEvent(c->stream, c->ev_cast[k], 0));
                HIPCHK(hipStreamWaitEvent(c->cstream, c->ev_cast[k], 0));
                c->cast_poses[k] = c->cast_T[k] = nullptr;
            }
    {
        // polar -> Cartesian is fused into the ICP kernel: scan k-1 / k of stream l are read as raw
        // ranges and turned into points (of storage type `dtype`) in registers
        IcpArgs a;
        a.tar = a.src = nullptr; a.prior = nullptr;
        a.ranges = ranges; a.cos_t = cos_t; a.sin_t = sin_t;
        a.tar_scan_stride = a.src_scan_stride = n;
        a.tar_stride = a.src_stride = 0;
        a.ppt = n_scan - 1;
        a.B = (int)pairs; a.n_tar = n; a.n_src = n; a.max_iter = max_iter; a.tol = tol;
        a.T_out = T; a.iters_out = iters_out; a.err_out = nullptr;
        a.status = c->status; a.qpt_pref = c->icp_qpt; a.team_mode = c->icp_team; a.one_wave = c->icp_one_wave; a.f32_filter = c->icp_f32_filter;
        if (grid && c->replay_reset) {
            // option "replay_reset": the map starts from zero for this replay.  On one stream the scan-matching launch
            // clears the counters on its way (they are next touched by the ray cast behind it); maps with a live pmap and
            // the three-stream pipeline go through slam_grid_reset.
            if (piped || grid->pmap_live) {
                TRY(slam_grid_reset(c, grid));
            } else {
                a.zero_ptr = grid->d.pass; a.zero_bytes = grid->state_bytes;
                grid->pristine = true;
            }
        }
        Timed t(c, SLAM_K_ICP);
        HIPCHK(launch_icp(a, dtype, c->stream));
    }
    if (!piped) {
        {
            Timed t(c, SLAM_K_COMPOSE);
            HIPCHK(launch_pose_compose(T, pose0, L, n_scan - 1, poses_out, c->stream));
        }
        if (grid) {
            TRY(grid_on_main(c));
            Timed t(c, SLAM_K_GRID);
            TRY(cast_replay(c, grid, ranges, cos_t, sin_t, poses_out, nullptr, L, n_scan, n, grid_of_traj, c->stream));
        }
        return SLAM_OK;
    }
    // compose waits for the ICP (and everything before it on the main stream: pose0, ranges)
    HIPCHK(hipEventRecord(c->ev_icp, c->stream));
    HIPCHK(hipStreamWaitEvent(c->cstream, c->ev_icp, 0));
    {
        Timed t(c, SLAM_K_COMPOSE, c->cstream);
        HIPCHK(launch_pose_compose(T, pose0, L, n_scan - 1, poses_out, c->cstream));
    }
    HIPCHK(hipEventRecord(c->ev_pose, c->cstream));
    HIPCHK(hipStreamWaitEvent(c->gstream, c->ev_pose, 0));
    c->gdirty = true;
    c->mgrid = false;
    {
        Timed t(c, SLAM_K_GRID, c->gstream);
        TRY(cast_replay(c, grid, ranges, cos_t, sin_t, poses_out, nullptr, L, n_scan, n, grid_of_traj, c->gstream));
    }
    HIPCHK(hipEventRecord(c->ev_cast[c->cast_pos], c->gstream));
    c->cast_poses[c->cast_pos] = poses_out;
    c->cast_T[c->cast_pos] = T;
    c->cast_pos ^= 1;
    return SLAM_OK;
}

int slam_replay(slam_ctx *c, const float *ranges, const double *cos_t, const double *sin_t, int L, int n_scan, int n,
                int dtype, int max_iter, double tol, const double *pose0, slam_grid *grid, const int32_t *grid_of_traj,
                double *poses_out, double *T_out, int32_t *iters_out)
{
    TRY(use(c));
    TRY(check_replay(__func__, ranges, cos_t, sin_t, L, n_scan, n, dtype, max_iter, pose0, poses_out));
    if (grid && grid_of_traj)
        for (int l = 0; l < L; ++l) REQUIRE(grid_of_traj[l] >= 0 && grid_of_traj[l] < grid->d.G, "grid_of_traj out of range");
    const size_t pairs = (size_t)L * (n_scan - 1);
    float *d_r; double *d_c, *d_s, *d_0, *d_T, *d_P; int32_t *d_g, *d_it;
    Staging s(c);
    s.in(d_r, ranges, (size_t)L * n_scan * n).in(d_c, cos_t, n).in(d_s, sin_t, n).in(d_0, pose0, (size_t)L * 3)
        .in(d_g, grid ? grid_of_traj : nullptr, L);
    s.out_always(d_T, T_out, pairs * 9).out(d_P, poses_out, pairs * 3).out_always(d_it, iters_out, pairs);
    TRY(s.upload());
    TRY(slam_replay_dev(c, d_r, d_c, d_s, L, n_scan, n, dtype, max_iter, tol, d_0, grid, d_g, nullptr, d_P, d_T, d_it));
    // "pipeline" option with a map: compose ran on cstream and the ray cast on gstream (which
    // waited for compose): the copies below are issued on the main stream, which must first see
    // both (join_from_grid records on gstream, i.e. after ev_pose of cstream).
    TRY(join_from_grid(c));
    TRY(s.download());
    return check_status_sync(c);
}

/* ---- particle hypotheses ----------------------------------------------------------- */

static int check_particles(const char *fn, const float *ranges2, const double *cos_t, const double *sin_t, int n, int dtype,
                           const double *pose_prev, int P, int max_iter, const slam_grid *grid, const double *poses_out)
{
    REQUIRE_IN(fn, ranges2 && cos_t && sin_t && pose_prev && poses_out, "null pointer");
    REQUIRE_IN(fn, P > 0 && n > 0 && n <= 8192, "need P > 0 and 0 < n <= 8192");
    REQUIRE_IN(fn, max_iter >= 0, "max_iter must be >= 0");
    REQUIRE_IN(fn, dtype_size(dtype), "unknown dtype");
    REQUIRE_IN(fn, !grid || grid->d.G >= P, "the grid object needs one map per particle");
    return SLAM_OK;
}

int slam_particles_dev(slam_ctx *c, const float *ranges2, const double *cos_t, const double *sin_t, int n, int dtype,
                       const double *prior, const double *pose_prev, int P, int max_iter, double tol, slam_grid *grid,
                       void *pts_ws, double *poses_out, double *T_out, int32_t *iters_out)
{
    TRY(use(c));
    REQUIRE(T_out, "null pointer");
    TRY(check_particles(__func__, ranges2, cos_t, sin_t, n, dtype, pose_prev, P, max_iter, grid, poses_out));
    (void)pts_ws;   // kept in the ABI; the point buffers are no longer materialised
    // Chunks (option "particle_chunks", off by default): matcher and pose step of chunk k on the context's stream, its ray
    // cast on a second stream behind an event, beside the matcher of chunk k + 1.  The matcher is bound by vector issue and
    // the ray cast by memory traffic, so the two should share the chip well - they do not (measured, round 4: 10 000
    // hypotheses 1.14 ms per step in one piece, 1.19 / 1.35 / 1.61 in 2 / 4 / 8 chunks): a ray-cast workgroup holds half a
    // CU's LDS for its window and the matcher's workgroups a quarter of its registers each, both for their whole lives, so
    // workgroups of the two kernels displace each other on a CU instead of filling each other's stalls.
    // Kept as an option because the chunks are also the unit a caller could overlap with work of its own; hypotheses are
    // independent (ICP.process / Mapping.update per hypothesis), so chunking changes no result.
    int chunks = c->particle_chunks > 1 ? c->particle_chunks : 1;
    if (!grid || chunks > P) chunks = 1;
    if (chunks == 1) TRY(grid_on_main(c));
    else if (c->pipeline) TRY(join_from_grid(c));
    if (chunks > 1) {
        if (!c->pstream) {
            HIPCHK(hipStreamCreateWithFlags(&c->pstream, hipStreamNonBlocking));
            HIPCHK(hipEventCreateWithFlags(&c->pev_join, hipEventDisableTiming));
        }
        while ((int)c->pev_pose.size() < chunks) {
            hipEvent_t e0 = nullptr, e1 = nullptr;
            HIPCHK(hipEventCreateWithFlags(&e0, hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&e1, hipEventDisableTiming));
            c->pev_pose.push_back(e0);
            c->pev_cast.push_back(e1);
        }
    }
    double *heading_cs = nullptr;               // cos / sin of the new headings: written by the pose step, read by the ray cast
    if (grid) {
        TRY(reserve(c, c->scratch, Layout().add(heading_cs, (size_t)P * 2)));
        grid->pristine = false;
    }
    for (int k = 0; k < chunks; ++k) {
        const int p0 = (int)((long)P * k / chunks), pc = (int)((long)P * (k + 1) / chunks) - p0;
        {
            IcpArgs a;
            a.tar = a.src = nullptr; a.prior = prior ? prior + 6 * (size_t)p0 : nullptr;
            a.ranges = ranges2; a.cos_t = cos_t; a.sin_t = sin_t;
            a.tar_scan_stride = a.src_scan_stride = 0;   // every hypothesis matches the same scan pair
            a.tar_stride = a.src_stride = 0;
            a.ppt = 0;
            a.B = pc; a.n_tar = n; a.n_src = n; a.max_iter = max_iter; a.tol = tol;
            a.T_out = T_out + 9 * (size_t)p0; a.iters_out = iters_out ? iters_out + p0 : nullptr; a.err_out = nullptr;
            a.status = c->status; a.team_mode = c->icp_team; a.one_wave = c->icp_one_wave; a.f32_filter = c->icp_f32_filter;
            // (queries per lane by the size of the BATCH: its chunks share the chip with one another's ray casts)
            a.qpt_pref = c->icp_qpt > 0 ? c->icp_qpt : (P >= 2500 ? 3 : 0);
            Timed t(c, SLAM_K_ICP, nullptr, k == 0);
            HIPCHK(launch_icp(a, dtype, c->stream));
        }
        {
            Timed t(c, SLAM_K_COMPOSE, nullptr, k == 0);
            HIPCHK(launch_pose_compose(T_out + 9 * (size_t)p0, pose_prev + 3 * (size_t)p0, pc, 1, poses_out + 3 * (size_t)p0, c->stream,
                                       prior ? prior + 6 * (size_t)p0 : nullptr, heading_cs ? heading_cs + 2 * (size_t)p0 : nullptr));
        }
        if (grid) {
            hipStream_t st = c->stream;
            if (chunks > 1) {
                HIPCHK(hipEventRecord(c->pev_pose[k], c->stream));
                HIPCHK(hipStreamWaitEvent(c->pstream, c->pev_pose[k], 0));
                st = c->pstream;
            }
            GridDev d = grid->d;                                       // the chunk's maps
            const size_t off = (size_t)p0 * d.xw * d.yw;
            d.G = pc; d.pass += off; d.hit += off;
            if (d.pmap_live) d.pmap_live += off;
            CastRequest r;                                             // one scan per hypothesis into its own map (no scratch)
            r.ranges = ranges2; r.cos_t = cos_t; r.sin_t = sin_t; r.poses = poses_out + 3 * (size_t)p0;
            r.heading_cs = heading_cs + 2 * (size_t)p0;
            r.L = pc; r.scans = 1; r.n = n; r.particles = true; r.group = 1; r.lds_hits = c->win_lds_hits;
            Timed t(c, SLAM_K_GRID, nullptr, k == 0);
            HIPCHK(launch_cast(d, plan_cast(d, c->grid_mode, r), r, nullptr, 0, st));
            if (chunks > 1) HIPCHK(hipEventRecord(c->pev_cast[k], c->pstream));
        }
    }
    if (chunks > 1) {
        // The ray casts on the second stream read the caller's ranges2 / cos_t / sin_t / poses_out and the heading scratch: the
        // context's stream waits for them here, so that - as for every *_dev entry point - work enqueued behind this call is
        // ordered behind ALL of it (a caller overwriting ranges2 for the next scan pair, slam_replay_dev carving
        // the same scratch).  The overlap this option is for is the one INSIDE a batch: cast of chunk k beside the matcher of k + 1.
        c->pdirty = true;
        TRY(join_particles(c));
        if (c->pipeline) c->mgrid = true;      // map work the map stream has not seen: its next piece forks from the main stream
    }
    return SLAM_OK;
}

int slam_particles(slam_ctx *c, const float *ranges2, const double *cos_t, const double *sin_t, int n, int dtype,
                   const double *prior, const double *pose_prev, int P, int max_iter, double tol, slam_grid *grid,
                   double *poses_out, double *T_out, int32_t *iters_out)
{
    TRY(use(c));
    TRY(check_particles(__func__, ranges2, cos_t, sin_t, n, dtype, pose_prev, P, max_iter, grid, poses_out));
    float *d_r; double *d_c, *d_s, *d_pr, *d_p0, *d_P, *d_T; int32_t *d_it;
    Staging s(c);
    s.in(d_r, ranges2, 2 * (size_t)n).in(d_c, cos_t, n).in(d_s, sin_t, n).in(d_pr, prior, (size_t)P * 6).in(d_p0, pose_prev, (size_t)P * 3);
    s.out(d_P, poses_out, (size_t)P * 3).out_always(d_T, T_out, (size_t)P * 9).out_always(d_it, iters_out, P);
    TRY(s.upload());
    TRY(slam_particles_dev(c, d_r, d_c, d_s, n, dtype, d_pr, d_p0, P, max_iter, tol, grid, nullptr, d_P, d_T, d_it));
    TRY(s.download());
    return check_status_sync(c);
}

/* ---- scan-to-map observation ------------------------------------- */

static int check_map_obstacles(const char *fn, const int8_t *map, int width, int height, const double *ox, const double *oy,
                               int cap, const int *count)
{
    REQUIRE_IN(fn, map && ox && oy && count, "null pointer");
    REQUIRE_IN(fn, width > 0 && height > 0 && cap >= 0, "bad sizes");
    return SLAM_OK;
}

int slam_map_obstacles(slam_ctx *c, const int8_t *map, int width, int height, int wire_layout, double resolution,
                       double origin_x, double origin_y, double *ox, double *oy, int cap, int *count_out)
{
    TRY(use(c));
    TRY(check_map_obstacles(__func__, map, width, height, ox, oy, cap, count_out));
    int8_t *d_m; double *d_x, *d_y; int *d_k;
    Staging s(c);
    s.in(d_m, map, (size_t)width * height).work(d_x, cap).work(d_y, cap).work(d_k, 1);
    TRY(s.upload());
    HIPCHK(launch_map_obstacles(d_m, width, height, wire_layout, resolution, origin_x, origin_y, d_x, d_y, cap, d_k, c->stream));
    int k = 0;
    D2H(&k, d_k, sizeof(int));
    HIPCHK(hipStreamSynchronize(c->stream));
    *count_out = k;
    int got = k < cap ? k : cap;
    if (got > 0) {
        D2H(ox, d_x, (size_t)got * 8);
        D2H(oy, d_y, (size_t)got * 8);
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return SLAM_OK;
}

int slam_map_obstacles_dev(slam_ctx *c, const int8_t *map, int width, int height, int wire_layout, double resolution,
                           double origin_x, double origin_y, double *ox, double *oy, int cap, int *count_dev)
{
    TRY(use(c));
    TRY(streams_on_main(c));
    TRY(check_map_obstacles(__func__, map, width, height, ox, oy, cap, count_dev));
    HIPCHK(launch_map_obstacles(map, width, height, wire_layout, resolution, origin_x, origin_y, ox, oy, cap, count_dev, c->stream));
    return SLAM_OK;
}

static int check_virtual_scan(const char *fn, const double *ox, const double *oy, int K, const double *poses, int B,
                              double angle_min, double angle_increment, int n)
{
    REQUIRE_IN(fn, (K == 0 || (ox && oy)) && poses, "null pointer");
    REQUIRE_IN(fn, K >= 0 && B > 0 && n > 0 && n <= 8192, "bad sizes");
    REQUIRE_IN(fn, angle_increment != 0.0 && std::isfinite(angle_increment) && std::isfinite(angle_min), "bad angles");
    return SLAM_OK;
}

int slam_virtual_scan_dev(slam_ctx *c, const double *ox, const double *oy, int K, const double *poses, int B,
                          double angle_min, double angle_increment, int n, double *ranges_out)
{
    TRY(use(c));
    TRY(streams_on_main(c));
    REQUIRE(ranges_out, "null pointer");
    TRY(check_virtual_scan(__func__, ox, oy, K, poses, B, angle_min, angle_increment, n));
    HIPCHK(launch_virtual_scan(ox, oy, K, poses, B, angle_min, angle_increment, n, ranges_out, c->stream));
    return SLAM_OK;
}

int slam_virtual_scan(slam_ctx *c, const double *ox, const double *oy, int K, const double *poses, int B, double angle_min,
                      double angle_increment, int n, double *ranges_out)
{
    TRY(use(c));
    REQUIRE(ranges_out, "null pointer");
    TRY(check_virtual_scan(__func__, ox, oy, K, poses, B, angle_min, angle_increment, n));
    double *d_x, *d_y, *d_p, *d_r;
    Staging s(c);
    s.in(d_x, ox, K).in(d_y, oy, K).in(d_p, poses, (size_t)B * 3).out(d_r, ranges_out, (size_t)B * n);
    TRY(s.upload());
    TRY(slam_virtual_scan_dev(c, d_x, d_y, K, d_p, B, angle_min, angle_increment, n, d_r));
    return s.download();
}

static int check_scan_to_points_f64(const char *fn, const double *ranges, const double *cos_t, const double *sin_t, int B,
                                    int n, const double *pts_out)
{
    REQUIRE_IN(fn, ranges && cos_t && sin_t && pts_out, "null pointer");
    REQUIRE_IN(fn, B > 0 && n > 0, "bad sizes");
    return SLAM_OK;
}

int slam_scan_to_points_f64_dev(slam_ctx *c, const double *ranges, const double *cos_t, const double *sin_t, int B, int n,
                                double *pts_out)
{
    TRY(use(c));
    TRY(streams_on_main(c));
    TRY(check_scan_to_points_f64(__func__, ranges, cos_t, sin_t, B, n, pts_out));
    HIPCHK(launch_ranges64_to_points(ranges, cos_t, sin_t, B, n, pts_out, c->stream));
    return SLAM_OK;
}

int slam_scan_to_points_f64(slam_ctx *c, const double *ranges, const double *cos_t, const double *sin_t, int B, int n,
                            double *pts_out)
{
    TRY(use(c));
    TRY(check_scan_to_points_f64(__func__, ranges, cos_t, sin_t, B, n, pts_out));
    double *d_r, *d_c, *d_s, *d_p;
    Staging s(c);
    s.in(d_r, ranges, (size_t)B * n).in(d_c, cos_t, n).in(d_s, sin_t, n).out(d_p, pts_out, (size_t)B * 2 * n);
    TRY(s.upload());
    TRY(slam_scan_to_points_f64_dev(c, d_r, d_c, d_s, B, n, d_p));
    return s.download();
}

static int check_map_observation(const char *fn, const double *ox, const double *oy, int K, const double *poses,
                                 const double *src, int B, int n, const double *cos_t, const double *sin_t, double angle_min,
                                 double angle_increment, int max_iter, const double *T_out)
{
    REQUIRE_IN(fn, src && cos_t && sin_t && T_out, "null pointer");
    REQUIRE_IN(fn, max_iter >= 0, "max_iter must be >= 0");
    return check_virtual_scan(fn, ox, oy, K, poses, B, angle_min, angle_increment, n);
}

int slam_map_observation_dev(slam_ctx *c, const double *ox, const double *oy, int K, const double *poses, const double *src,
                             int B, int n, int src_shared, const double *cos_t, const double *sin_t, double angle_min,
                             double angle_increment, int max_iter, double tol, double *vranges_ws, double *vpts_ws,
                             double *T_out, int32_t *iters_out)
{
    TRY(use(c));
    TRY(streams_on_main(c));
    REQUIRE(vranges_ws && vpts_ws, "null pointer");
    TRY(check_map_observation(__func__, ox, oy, K, poses, src, B, n, cos_t, sin_t, angle_min, angle_increment, max_iter, T_out));
    TRY(slam_virtual_scan_dev(c, ox, oy, K, poses, B, angle_min, angle_increment, n, vranges_ws));
    HIPCHK(launch_ranges64_to_points(vranges_ws, cos_t, sin_t, B, n, vpts_ws, c->stream));
    return slam_icp_batch_dev(c, vpts_ws, src, B, n, n, SLAM_F64, 0, src_shared, nullptr, max_iter, tol, T_out, iters_out,
                              nullptr);
}

int slam_map_observation(slam_ctx *c, const double *ox, const double *oy, int K, const double *poses, const double *src,
                         int B, int n, int src_shared, const double *cos_t, const double *sin_t, double angle_min,
                         double angle_increment, int max_iter, double tol, double *T_out, int32_t *iters_out)
{
    TRY(use(c));
    TRY(check_map_observation(__func__, ox, oy, K, poses, src, B, n, cos_t, sin_t, angle_min, angle_increment, max_iter, T_out));
    double *d_x, *d_y, *d_p, *d_s, *d_c, *d_sn, *d_vr, *d_vp, *d_T; int32_t *d_it;
    Staging s(c);
    s.in(d_x, ox, K).in(d_y, oy, K).in(d_p, poses, (size_t)B * 3).in(d_s, src, (size_t)(src_shared ? 1 : B) * 2 * n)
        .in(d_c, cos_t, n).in(d_sn, sin_t, n);
    s.work(d_vr, (size_t)B * n).work(d_vp, (size_t)B * 2 * n).out(d_T, T_out, (size_t)B * 9).out_always(d_it, iters_out, B);
    TRY(s.upload());
    TRY(slam_map_observation_dev(c, d_x, d_y, K, d_p, d_s, B, n, src_shared, d_c, d_sn, angle_min, angle_increment, max_iter,
                                 tol, d_vr, d_vp, d_T, d_it));
    return s.download();
}

/* ---- DWA local planner ------------------------------------------------------------------ */

int slam_dwa_shape(const double *config, int *rows_out, int *nv_cap_out, int *nw_cap_out)
{
    if (!rows_out || !nv_cap_out || !nw_cap_out) return fail(SLAM_ERR_INVALID, "slam_dwa_shape: null pointer");
    return dwa_config(config, nullptr, rows_out, nv_cap_out, nw_cap_out);
}

static int check_dwa_obstacles(const char *fn, const double *states, const double *goals, const double *obstacles, int M,
                               const double *config, int B, const DwaOut &o, DwaArgs &a)
{
    REQUIRE_IN(fn, obstacles, "null pointer");
    REQUIRE_IN(fn, M > 0, "M must be > 0 (np.min of an empty obstacle set raises, dwa.py:157)");
    return check_dwa(fn, states, goals, config, B, o, a);
}

int slam_dwa_dev(slam_ctx *c, const double *states, const double *goals, const double *obstacles, const int32_t *counts,
                 int M, int shared, const double *config, int B, double *u_out, double *cost_out, int32_t *index_out,
                 int32_t *counts_out, double *costs_out, int s_cap, double *traj_out)
{
    TRY(use(c));
    TRY(streams_on_main(c));
    const DwaOut o{u_out, cost_out, index_out, counts_out, costs_out, s_cap, traj_out};
    DwaArgs a;
    TRY(check_dwa_obstacles(__func__, states, goals, obstacles, M, config, B, o, a));
    a.states = states;
    a.goals = goals;
    a.obs = obstacles;
    a.ob_stride = shared ? 0 : 2L * M;
    a.M = M;
    a.counts = counts;
    a.count_stride = shared ? 0 : 1;
    a.B = B;
    a.tile_cap = M < kDwaTile ? M : kDwaTile;
    return dwa_launch(c, a, o);
}

int slam_dwa(slam_ctx *c, const double *states, const double *goals, const double *obstacles, const int32_t *counts,
             int M, int shared, const double *config, int B, double *u_out, double *cost_out, int32_t *index_out,
             int32_t *counts_out, double *costs_out, int s_cap, double *traj_out)
{
    TRY(use(c));
    DwaArgs a;
    TRY(check_dwa_obstacles(__func__, states, goals, obstacles, M, config, B,
                            DwaOut{u_out, cost_out, index_out, counts_out, costs_out, s_cap, traj_out}, a));
    const int sets = shared ? 1 : B;
    if (counts)
        for (int b = 0; b < sets; ++b)
            if (counts[b] < 1 || counts[b] > M)
                return fail(SLAM_ERR_INVALID, "slam_dwa: counts[%d] = %d outside [1, M = %d] (np.min of an empty set raises, dwa.py:157)",
                            b, counts[b], M);
    const size_t Bz = (size_t)B;
    double *d_st, *d_g, *d_ob, *d_u, *d_c, *d_cs, *d_t; int32_t *d_k, *d_i, *d_n;
    Staging s(c);
    s.in(d_st, states, Bz * 5).in(d_g, goals, Bz * 2).in(d_ob, obstacles, (size_t)sets * 2 * M).in(d_k, counts, sets);
    s.out(d_u, u_out, Bz * 2).out(d_c, cost_out, Bz).out(d_i, index_out, Bz).out(d_n, counts_out, Bz * 2)
        .out(d_cs, costs_out, Bz * s_cap).out(d_t, traj_out, Bz * a.rows * 5);
    TRY(s.upload());
    TRY(slam_dwa_dev(c, d_st, d_g, d_ob, d_k, M, shared, config, B, d_u, d_c, d_i, d_n, d_cs, s_cap, d_t));
    TRY(s.download());
    return check_status_sync(c);
}

static int check_dwa_scans(const char *fn, const double *states, const double *goals, const float *ranges, int n,
                           const double *cos_t, const double *sin_t, double threshold, const double *config, int B,
                           const DwaOut &o, DwaArgs &a)
{
    REQUIRE_IN(fn, ranges && cos_t && sin_t, "null pointer");
    REQUIRE_IN(fn, n > 0 && n <= kDwaMaxBeams, "n must be in [1, 4095]");
    REQUIRE_IN(fn, !std::isnan(threshold), "threshold is NaN");
    return check_dwa(fn, states, goals, config, B, o, a);
}

int slam_dwa_scans_dev(slam_ctx *c, const double *states, const double *goals, const float *ranges, int n, int shared,
                       const double *cos_t, const double *sin_t, double threshold, const double *config, int B,
                       double *u_out, double *cost_out, int32_t *index_out, int32_t *counts_out, double *costs_out,
                       int s_cap, double *traj_out)
{
    TRY(use(c));
    TRY(streams_on_main(c));
    const DwaOut o{u_out, cost_out, index_out, counts_out, costs_out, s_cap, traj_out};
    DwaArgs a;
    TRY(check_dwa_scans(__func__, states, goals, ranges, n, cos_t, sin_t, threshold, config, B, o, a));
    a.states = states;
    a.goals = goals;
    a.ranges = ranges;
    a.cos_t = cos_t;
    a.sin_t = sin_t;
    a.scan_stride = shared ? 0 : n;
    a.n = n;
    a.threshold = threshold;
    a.B = B;
    a.tile_cap = n + 1;
    return dwa_launch(c, a, o);
}

int slam_dwa_scans(slam_ctx *c, const double *states, const double *goals, const float *ranges, int n, int shared,
                   const double *cos_t, const double *sin_t, double threshold, const double *config, int B,
                   double *u_out, double *cost_out, int32_t *index_out, int32_t *counts_out, double *costs_out,
                   int s_cap, double *traj_out)
{
    TRY(use(c));
    DwaArgs a;
    TRY(check_dwa_scans(__func__, states, goals, ranges, n, cos_t, sin_t, threshold, config, B,
                        DwaOut{u_out, cost_out, index_out, counts_out, costs_out, s_cap, traj_out}, a));
    const size_t Bz = (size_t)B;
    float *d_r; double *d_st, *d_g, *d_ct, *d_sn, *d_u, *d_c, *d_cs, *d_t; int32_t *d_i, *d_n;
    Staging s(c);
    s.in(d_st, states, Bz * 5).in(d_g, goals, Bz * 2).in(d_r, ranges, (size_t)(shared ? 1 : B) * n).in(d_ct, cos_t, n).in(d_sn, sin_t, n);
    s.out(d_u, u_out, Bz * 2).out(d_c, cost_out, Bz).out(d_i, index_out, Bz).out(d_n, counts_out, Bz * 2)
        .out(d_cs, costs_out, Bz * s_cap).out(d_t, traj_out, Bz * a.rows * 5);
    TRY(s.upload());
    TRY(slam_dwa_scans_dev(c, d_st, d_g, d_r, n, shared, d_ct, d_sn, threshold, config, B, d_u, d_c, d_i, d_n, d_cs, s_cap, d_t));
    TRY(s.download());
    return check_status_sync(c);
}

/* ---- A* global planner ------------------------------------------------------------------ */

int slam_astar_dev(slam_ctx *c, const int8_t *maps, int G, int H, int W, int wire_layout, int span, int r,
                   const int32_t *starts, const int32_t *goals, const int32_t *map_of_query, int B, int path_cap,
                   int32_t *status_out, int32_t *path_len_out, int32_t *path_out, int32_t *expansions_out,
                   int8_t *inflated_out)
{
    TRY(use(c));
    TRY(check_astar(__func__, maps, G, H, W, span, r, starts, goals, map_of_query, B, path_cap, status_out, path_len_out,
                    path_out, expansions_out));
    AstarArgs a{};
    a.G = G;
    a.H = H;
    a.W = W;
    a.starts = starts;
    a.goals = goals;
    a.map_of_query = map_of_query;
    a.B = B;
    a.path_cap = path_cap;
    a.status = status_out;
    a.path_len = path_len_out;
    a.path = path_out;
    a.expansions = expansions_out;
    return astar_run(c, maps, G, H, W, wire_layout, span, r, inflated_out, &a);
}

int slam_astar(slam_ctx *c, const int8_t *maps, int G, int H, int W, int wire_layout, int span, int r,
               const int32_t *starts, const int32_t *goals, const int32_t *map_of_query, int B, int path_cap,
               int32_t *status_out, int32_t *path_len_out, int32_t *path_out, int32_t *expansions_out,
               int8_t *inflated_out)
{
    TRY(use(c));
    TRY(check_astar(__func__, maps, G, H, W, span, r, starts, goals, map_of_query, B, path_cap, status_out, path_len_out,
                    path_out, expansions_out));
    if (map_of_query)
        for (int b = 0; b < B; ++b)
            if (map_of_query[b] < 0 || map_of_query[b] >= G)
                return fail(SLAM_ERR_INVALID, "slam_astar: map_of_query[%d] = %d outside [0, G = %d)", b, map_of_query[b], G);
    const size_t Bz = (size_t)B, maps_n = (size_t)G * H * W;
    int8_t *d_m, *d_inf; int32_t *d_s, *d_g, *d_q, *d_st, *d_len, *d_p, *d_e;
    Staging s(c);
    s.in(d_m, maps, maps_n).in(d_s, starts, Bz * 2).in(d_g, goals, Bz * 2).in(d_q, map_of_query, Bz);
    s.out_always(d_st, status_out, Bz).out_always(d_len, path_len_out, Bz).out(d_p, path_out, Bz * path_cap * 2)
        .out_always(d_e, expansions_out, Bz).out(d_inf, inflated_out, maps_n);
    TRY(s.upload());
    TRY(slam_astar_dev(c, d_m, G, H, W, wire_layout, span, r, d_s, d_g, d_q, B, path_cap, d_st, d_len, d_p, d_e, d_inf));
    TRY(s.download());
    return check_status_sync(c);
}

int slam_astar_inflate_dev(slam_ctx *c, const int8_t *maps, int G, int H, int W, int wire_layout, int span, int r,
                           int8_t *inflated_out)
{
    TRY(use(c));
    TRY(check_astar_maps(__func__, maps, G, H, W, span, r));
    REQUIRE(inflated_out, "null pointer");
    return astar_run(c, maps, G, H, W, wire_layout, span, r, inflated_out, nullptr);
}

int slam_astar_inflate(slam_ctx *c, const int8_t *maps, int G, int H, int W, int wire_layout, int span, int r,
                       int8_t *inflated_out)
{
    TRY(use(c));
    TRY(check_astar_maps(__func__, maps, G, H, W, span, r));
    REQUIRE(inflated_out, "null pointer");
    const size_t maps_n = (size_t)G * H * W;
    int8_t *d_m, *d_o;
    Staging s(c);
    s.in(d_m, maps, maps_n).out_always(d_o, inflated_out, maps_n);
    TRY(s.upload());
    TRY(slam_astar_inflate_dev(c, d_m, G, H, W, wire_layout, span, r, d_o));
    TRY(s.download());
    return check_status_sync(c);
}

/* ---- landmark EKF-SLAM node ----------------------------------------------------------------- */

static int check_landmarks(const char *fn, const float *ranges, const double *cos_t, const double *sin_t, int S, int n,
                           int lm_cap, const int32_t *count_out, const int32_t *overflow_out, const int32_t *ids_out,
                           const double *means_out, const double *z_out)
{
    REQUIRE_IN(fn, ranges && cos_t && sin_t && count_out && overflow_out && ids_out && means_out && z_out, "null pointer");
    REQUIRE_IN(fn, S > 0 && n > 0 && n <= kLandmarkMaxBeams, "need S > 0 and 1 <= n <= 4096");
    REQUIRE_IN(fn, lm_cap >= 1 && lm_cap <= 1024, "need 1 <= lm_cap <= 1024");
    return SLAM_OK;
}

int slam_landmarks_dev(slam_ctx *c, const float *ranges, const double *cos_t, const double *sin_t, int S, int n,
                       double range_threshold, double radius_max_th, int lm_cap, int32_t *count_out, int32_t *overflow_out,
                       int32_t *ids_out, double *means_out, double *z_out, int32_t *labels_out)
{
    TRY(use(c));
    TRY(streams_on_main(c));
    TRY(check_landmarks(__func__, ranges, cos_t, sin_t, S, n, lm_cap, count_out, overflow_out, ids_out, means_out, z_out));
    LandmarkArgs a{ranges, cos_t, sin_t, S, n, range_threshold, radius_max_th, lm_cap, count_out, overflow_out, ids_out,
                   means_out, z_out, labels_out, c->status};
    HIPCHK(launch_landmarks(a, c->stream));
    return SLAM_OK;
}

int slam_landmarks(slam_ctx *c, const float *ranges, const double *cos_t, const double *sin_t, int S, int n,
                   double range_threshold, double radius_max_th, int lm_cap, int32_t *count_out, int32_t *overflow_out,
                   int32_t *ids_out, double *means_out, double *z_out, int32_t *labels_out)
{
    TRY(use(c));
    TRY(check_landmarks(__func__, ranges, cos_t, sin_t, S, n, lm_cap, count_out, overflow_out, ids_out, means_out, z_out));
    const size_t Sz = (size_t)S, slots = Sz * lm_cap;
    float *d_r; double *d_c, *d_s, *d_m, *d_z; int32_t *d_cnt, *d_of, *d_id, *d_lab;
    Staging s(c);
    s.in(d_r, ranges, Sz * n).in(d_c, cos_t, n).in(d_s, sin_t, n);
    s.out_always(d_cnt, count_out, Sz).out_always(d_of, overflow_out, Sz).out_always(d_id, ids_out, slots)
        .out_always(d_m, means_out, slots * 2).out_always(d_z, z_out, slots * 2).out(d_lab, labels_out, Sz * (n - 1));
    TRY(s.upload());
    TRY(slam_landmarks_dev(c, d_r, d_c, d_s, S, n, range_threshold, radius_max_th, lm_cap, d_cnt, d_of, d_id, d_m, d_z, d_lab));
    TRY(s.download());
    return check_status_sync(c);
}

static int check_ekf_lm(const char *fn, const double *u, const int32_t *step_counts, const int64_t *z_off, const double *z,
                        int64_t nz, int B, int steps, int max_lm, const double *x_out, const double *P_out,
                        const int32_t *nlm_out, const int32_t *status_out)
{
    REQUIRE_IN(fn, u && step_counts && z_off && x_out && P_out && nlm_out && status_out, "null pointer");
    REQUIRE_IN(fn, nz >= 0 && (z || nz == 0), "z is null");
    REQUIRE_IN(fn, B > 0 && steps > 0 && (long)B * steps < (1L << 31), "need B > 0, steps > 0, B * steps < 2^31");
    REQUIRE_IN(fn, max_lm >= 0 && max_lm <= kEkfMaxLm, "need 0 <= max_lm <= 32");
    return SLAM_OK;
}

int slam_ekf_lm_dev(slam_ctx *c, const double *x0, const double *u, const int32_t *step_counts, const int64_t *z_off,
                    const double *z, int64_t nz, int B, int steps, int max_lm, double *x_out, double *P_out,
                    int32_t *nlm_out, int32_t *status_out)
{
    TRY(use(c));
    TRY(streams_on_main(c));
    TRY(check_ekf_lm(__func__, u, step_counts, z_off, z, nz, B, steps, max_lm, x_out, P_out, nlm_out, status_out));
    EkfArgs a{};
    a.B = B; a.steps_max = steps; a.max_lm = max_lm;
    a.x0 = x0; a.steps = step_counts; a.u = u; a.z = z; a.z_off = z_off; a.nz = nz;
    a.x_out = x_out; a.P_out = P_out; a.nlm_hist = nlm_out; a.status_out = status_out; a.status = c->status;
    HIPCHK(launch_ekf_lm(a, c->stream));
    return SLAM_OK;
}

int slam_ekf_lm(slam_ctx *c, const double *x0, const double *u, const int32_t *step_counts, const int64_t *z_off,
                const double *z, int64_t nz, int B, int steps, int max_lm, double *x_out, double *P_out, int32_t *nlm_out,
                int32_t *status_out)
{
    TRY(use(c));
    TRY(check_ekf_lm(__func__, u, step_counts, z_off, z, nz, B, steps, max_lm, x_out, P_out, nlm_out, status_out));
    const size_t Bz = (size_t)B, N = 3 + 2 * (size_t)max_lm, rows = Bz * steps;
    for (size_t k = 0; k <= rows; ++k)
        REQUIRE(z_off[k] >= (k ? z_off[k - 1] : 0) && z_off[k] <= nz, "z_off must ascend within [0, nz]");
    double *d_x0, *d_u, *d_z, *d_x, *d_P; int32_t *d_sc, *d_nlm, *d_st; int64_t *d_off;
    Staging s(c);
    s.in(d_x0, x0, Bz * 3).in(d_u, u, rows * 3).in(d_sc, step_counts, Bz).in(d_off, z_off, rows + 1).in(d_z, z, (size_t)nz * 2);
    s.out_always(d_x, x_out, Bz * N).out_always(d_P, P_out, Bz * N * N).out_always(d_nlm, nlm_out, rows).out_always(d_st, status_out, Bz);
    TRY(s.upload());
    TRY(slam_ekf_lm_dev(c, d_x0, d_u, d_sc, d_off, d_z, nz, B, steps, max_lm, d_x, d_P, d_nlm, d_st));
    TRY(s.download());
    return check_status_sync(c);
}

static int check_node_replay(const char *fn, const float *ranges, const double *cos_t, const double *sin_t, int L, int n_scan,
                             int n, int dtype, int max_iter, int lm_cap, int max_lm, const double *pose0,
                             const int32_t *kept_out, const int32_t *kept_count_out, const double *xest_out,
                             const int32_t *nlm_out, const double *x_final_out, const double *P_final_out,
                             const int32_t *status_out)
{
    REQUIRE_IN(fn, ranges && cos_t && sin_t && pose0 && kept_out && kept_count_out && xest_out && nlm_out && x_final_out &&
                       P_final_out && status_out, "null pointer");
    REQUIRE_IN(fn, L > 0 && L <= 65535 && n_scan >= 2 && n > 0 && n <= kLandmarkMaxBeams, "need 0 < L <= 65535, n_scan >= 2, 1 <= n <= 4096");
    REQUIRE_IN(fn, (long)L * n_scan < (1L << 31), "too many scans for one call");
    REQUIRE_IN(fn, max_iter >= 0, "max_iter must be >= 0");
    REQUIRE_IN(fn, dtype_size(dtype), "unknown dtype");
    REQUIRE_IN(fn, lm_cap >= 1 && lm_cap <= 1024, "need 1 <= lm_cap <= 1024");
    REQUIRE_IN(fn, max_lm >= 0 && max_lm <= kEkfMaxLm, "need 0 <= max_lm <= 32");
    return SLAM_OK;
}

int slam_node_replay_dev(slam_ctx *c, const float *ranges, const double *cos_t, const double *sin_t, int L, int n_scan, int n,
                         int dtype, int max_iter, double tol, double range_threshold, double radius_max_th, int lm_cap,
                         int max_lm, const double *pose0, slam_grid *grid, const int32_t *grid_of_traj, int32_t *kept_out,
                         int32_t *kept_count_out, double *xest_out, int32_t *nlm_out, double *x_final_out, double *P_final_out,
                         double *T_out, int32_t *iters_out, int32_t *status_out)
{
    TRY(use(c));
    TRY(streams_on_main(c));      // (pose0 and the scans are read before the map is touched)
    TRY(check_node_replay(__func__, ranges, cos_t, sin_t, L, n_scan, n, dtype, max_iter, lm_cap, max_lm, pose0, kept_out,
                          kept_count_out, xest_out, nlm_out, x_final_out, P_final_out, status_out));
    const size_t S = (size_t)L * n_scan, pairs = (size_t)L * (n_scan - 1), slots = S * lm_cap;
    int32_t *cnt, *ovf, *ids;
    double *means, *z, *cast_poses, *T = T_out;
    float *kr;
    Layout ws;
    ws.add(cnt, S).add(ovf, S).add(ids, slots).add(means, slots * 2).add(z, slots * 2).add(kr, S * n).add(cast_poses, pairs * 3);
    if (!T) ws.add(T, pairs * 9);
    TRY(reserve(c, c->scratch, ws));
    {   // 1. extraction of every scan (:79); 2. the kept scans of every trajectory (:74-82), moved to the front
        LandmarkArgs a{ranges, cos_t, sin_t, (long)S, n, range_threshold, radius_max_th, lm_cap, cnt, ovf, ids, means, z, nullptr, c->status};
        HIPCHK(launch_landmarks(a, c->stream));
        HIPCHK(launch_node_keep(cnt, L, n_scan, kept_out, kept_count_out, c->stream));
        HIPCHK(launch_node_gather(ranges, kept_out, kept_count_out, L, n_scan, n, kr, c->stream));
    }
    {   // 3. the scan matcher on (previous kept, current kept) (:109-113)
        IcpArgs a;
        a.tar = a.src = nullptr; a.prior = nullptr;
        a.ranges = kr; a.cos_t = cos_t; a.sin_t = sin_t;
        a.tar_scan_stride = a.src_scan_stride = n;
        a.tar_stride = a.src_stride = 0;
        a.ppt = n_scan - 1;
        a.B = (int)pairs; a.n_tar = n; a.n_src = n; a.max_iter = max_iter; a.tol = tol;
        a.T_out = T; a.iters_out = iters_out; a.err_out = nullptr;
        a.status = c->status; a.qpt_pref = c->icp_qpt; a.team_mode = c->icp_team; a.one_wave = c->icp_one_wave; a.f32_filter = c->icp_f32_filter;
        a.batch_invariant = 1;      // a trajectory's result does not depend on how many run beside it
        Timed t(c, SLAM_K_ICP);
        HIPCHK(launch_icp(a, dtype, c->stream));
    }
    {   // 4. T2u and 5. the filter (:85-86, :125-128)
        EkfArgs a{};
        a.B = L; a.steps_max = n_scan - 1; a.max_lm = max_lm;
        a.x0 = pose0; a.steps = kept_count_out; a.steps_bias = 1; a.T = T; a.z = z;
        a.kept = kept_out; a.lm_count = cnt; a.lm_overflow = ovf; a.lm_cap = lm_cap;
        a.x_out = x_final_out; a.P_out = P_final_out; a.nlm_hist = nlm_out; a.status_out = status_out;
        a.x_hist = xest_out; a.cast_poses = grid ? cast_poses : nullptr; a.status = c->status;
        HIPCHK(launch_ekf_lm(a, c->stream));
    }
    if (grid) {   // 6. every kept scan cast from its xEst (:88-90)
        TRY(grid_on_main(c));
        Timed t(c, SLAM_K_GRID);
        TRY(cast_replay(c, grid, kr, cos_t, sin_t, cast_poses, nullptr, L, n_scan, n, grid_of_traj, c->stream));
    }
    return SLAM_OK;
}

int slam_node_replay(slam_ctx *c, const float *ranges, const double *cos_t, const double *sin_t, int L, int n_scan, int n,
                     int dtype, int max_iter, double tol, double range_threshold, double radius_max_th, int lm_cap, int max_lm,
                     const double *pose0, slam_grid *grid, const int32_t *grid_of_traj, int32_t *kept_out,
                     int32_t *kept_count_out, double *xest_out, int32_t *nlm_out, double *x_final_out, double *P_final_out,
                     double *T_out, int32_t *iters_out, int32_t *status_out)
{
    TRY(use(c));
    TRY(check_node_replay(__func__, ranges, cos_t, sin_t, L, n_scan, n, dtype, max_iter, lm_cap, max_lm, pose0, kept_out,
                          kept_count_out, xest_out, nlm_out, x_final_out, P_final_out, status_out));
    if (grid && grid_of_traj)
        for (int l = 0; l < L; ++l) REQUIRE(grid_of_traj[l] >= 0 && grid_of_traj[l] < grid->d.G, "grid_of_traj out of range");
    const size_t Lz = (size_t)L, S = Lz * n_scan, pairs = Lz * (n_scan - 1), N = 3 + 2 * (size_t)max_lm;
    float *d_r; double *d_c, *d_s, *d_0, *d_xe, *d_xf, *d_Pf, *d_T; int32_t *d_g, *d_k, *d_kc, *d_nlm, *d_it, *d_st;
    Staging s(c);
    s.in(d_r, ranges, S * n).in(d_c, cos_t, n).in(d_s, sin_t, n).in(d_0, pose0, Lz * 3).in(d_g, grid ? grid_of_traj : nullptr, Lz);
    s.out_always(d_k, kept_out, S).out_always(d_kc, kept_count_out, Lz).out_always(d_xe, xest_out, pairs * 3)
        .out_always(d_nlm, nlm_out, pairs).out_always(d_xf, x_final_out, Lz * N).out_always(d_Pf, P_final_out, Lz * N * N)
        .out_always(d_T, T_out, pairs * 9).out(d_it, iters_out, pairs).out_always(d_st, status_out, Lz);
    TRY(s.upload());
    TRY(slam_node_replay_dev(c, d_r, d_c, d_s, L, n_scan, n, dtype, max_iter, tol, range_threshold, radius_max_th, lm_cap, max_lm,
                             d_0, grid, d_g, d_k, d_kc, d_xe, d_nlm, d_xf, d_Pf, d_T, d_it, d_st));
    TRY(s.download());
    return check_status_sync(c);
}

/* ---- fusion-localization node (W9), batched ------------------------------------------------ */

static int check_loc_replay(const char *fn, const float *ranges, int S, int n_scan, int n, const int32_t *stream_of_traj,
                            const double *ox, const double *oy, const int64_t *obs_off, int M, int64_t K, int L,
                            const double *cos_t, const double *sin_t, double angle_min, double angle_increment, int max_iter,
                            const double *xest_out, const double *xodom_out, const double *P_final_out,
                            const int32_t *status_out)
{
    REQUIRE_IN(fn, ranges && obs_off && cos_t && sin_t && xest_out && xodom_out && P_final_out && status_out, "null pointer");
    REQUIRE_IN(fn, K >= 0 && (K == 0 || (ox && oy)), "K >= 0 obstacles need ox and oy");
    REQUIRE_IN(fn, L > 0 && L <= 65535 && n > 0 && n <= kLocMaxBeams && n_scan >= 1, "need 0 < L <= 65535, n_scan >= 1, 1 <= n <= 4096");
    REQUIRE_IN(fn, S > 0 && M > 0, "need at least one stream and one map");
    REQUIRE_IN(fn, stream_of_traj || S == L, "without stream_of_traj every trajectory has its own stream: S must equal L");
    REQUIRE_IN(fn, (long)L * n_scan < (1L << 31) && (long)S * (2L * n_scan - 1) < (1L << 31), "too many scans for one call");
    REQUIRE_IN(fn, max_iter >= 0, "max_iter must be >= 0");
    REQUIRE_IN(fn, angle_increment != 0.0 && std::isfinite(angle_increment) && std::isfinite(angle_min), "bad angles");
    return SLAM_OK;
}

int slam_loc_replay_dev(slam_ctx *c, const float *ranges, int S, int n_scan, int n, const int32_t *stream_of_traj,
                        const double *ox, const double *oy, const int64_t *obs_off, int M, int64_t K,
                        const int32_t *map_of_traj, const double *pose0, int L, const double *cos_t, const double *sin_t,
                        double angle_min, double angle_increment, int max_iter, double tol, double *xest_out,
                        double *xodom_out, double *P_final_out, int32_t *status_out, double *T_obs_out,
                        int32_t *iters_obs_out, double *T_odom_out, double *tar_pts_out)
{
    TRY(use(c));
    TRY(streams_on_main(c));
    TRY(check_loc_replay(__func__, ranges, S, n_scan, n, stream_of_traj, ox, oy, obs_off, M, K, L, cos_t, sin_t, angle_min,
                         angle_increment, max_iter, xest_out, xodom_out, P_final_out, status_out));
    const size_t Lz = (size_t)L, pairs = (size_t)S * (2 * (size_t)n_scan - 1);
    double *pair_pts, *T_stream, *tar, *src, *T_step, *state;
    int32_t *it_step;
    Layout ws;
    ws.add(pair_pts, pairs * 4 * n).add(T_stream, pairs * 9).add(tar, Lz * 2 * n).add(src, Lz * 2 * n).add(T_step, Lz * 9)
        .add(it_step, Lz).add(state, Lz * kLocStateDoubles);
    TRY(reserve(c, c->scratch, ws));
    IcpArgs icp;
    icp.prior = nullptr; icp.ranges = nullptr; icp.cos_t = icp.sin_t = nullptr; icp.tar_scan_stride = icp.src_scan_stride = 0;
    icp.ppt = 0; icp.n_tar = n; icp.n_src = n; icp.max_iter = max_iter; icp.tol = tol; icp.err_out = nullptr;
    icp.status = c->status; icp.qpt_pref = c->icp_qpt; icp.team_mode = c->icp_team; icp.one_wave = c->icp_one_wave; icp.f32_filter = c->icp_f32_filter;
    icp.batch_invariant = 1;        // a trajectory's result does not depend on how many run beside it
    {   // the solves that depend on the stream alone, once per stream: every T2 (:100) and T1 of the steps after the first (:78)
        HIPCHK(launch_loc_stream_pairs(ranges, cos_t, sin_t, S, n_scan, n, pair_pts, c->stream));
        icp.tar = pair_pts; icp.src = pair_pts + 2 * (size_t)n; icp.tar_stride = icp.src_stride = 4L * n;
        icp.B = (int)pairs; icp.T_out = T_stream; icp.iters_out = nullptr;
        Timed t(c, SLAM_K_ICP);
        HIPCHK(launch_icp(icp, SLAM_F64, c->stream));
    }
    LocArgs a{};
    a.L = L; a.S = S; a.M = M; a.n = n; a.n_scan = n_scan;
    a.ranges = ranges; a.stream_of_traj = stream_of_traj; a.map_of_traj = map_of_traj;
    a.ox = ox; a.oy = oy; a.obs_off = obs_off; a.K = K; a.pose0 = pose0; a.cos_t = cos_t; a.sin_t = sin_t;
    a.angle_min = angle_min; a.angle_increment = angle_increment;
    a.T_stream = T_stream; a.T_step = T_step; a.iters_step = it_step; a.state = state; a.tar_pts = tar; a.src_pts = src;
    a.xest_out = xest_out; a.xodom_out = xodom_out; a.P_final_out = P_final_out; a.status_out = status_out;
    a.T_obs_out = T_obs_out; a.T_odom_out = T_odom_out; a.iters_obs_out = iters_obs_out; a.tar_pts_out = tar_pts_out;
    a.status = c->status;
    icp.tar = tar; icp.src = src; icp.tar_stride = icp.src_stride = 2L * n;
    icp.B = L; icp.T_out = T_step; icp.iters_out = it_step;
    for (int s = 0; s <= n_scan; ++s) {   // step s: finish step s - 1, then virtual scan at xEst + the scan -> the scan matcher (:152-157)
        a.step = s; a.body = s < n_scan;
        HIPCHK(launch_loc_step(a, c->stream));
        if (!a.body) break;
        Timed t(c, SLAM_K_ICP);
        HIPCHK(launch_icp(icp, SLAM_F64, c->stream));
    }
    return SLAM_OK;
}

int slam_loc_replay(slam_ctx *c, const float *ranges, int S, int n_scan, int n, const int32_t *stream_of_traj,
                    const double *ox, const double *oy, const int64_t *obs_off, int M, const int32_t *map_of_traj,
                    const double *pose0, int L, const double *cos_t, const double *sin_t, double angle_min,
                    double angle_increment, int max_iter, double tol, double *xest_out, double *xodom_out,
                    double *P_final_out, int32_t *status_out, double *T_obs_out, int32_t *iters_obs_out, double *T_odom_out,
                    double *tar_pts_out)
{
    TRY(use(c));
    REQUIRE(obs_off && M > 0, "need obs_off with M + 1 entries, M >= 1");
    for (int m = 0; m < M; ++m) REQUIRE(obs_off[m] >= 0 && obs_off[m] <= obs_off[m + 1], "obs_off must ascend from >= 0");
    const int64_t K = obs_off[M];
    TRY(check_loc_replay(__func__, ranges, S, n_scan, n, stream_of_traj, ox, oy, obs_off, M, K, L, cos_t, sin_t, angle_min,
                         angle_increment, max_iter, xest_out, xodom_out, P_final_out, status_out));
    for (int l = 0; l < L; ++l) {
        REQUIRE(!stream_of_traj || (stream_of_traj[l] >= 0 && stream_of_traj[l] < S), "stream_of_traj out of range");
        REQUIRE(!map_of_traj || (map_of_traj[l] >= 0 && map_of_traj[l] < M), "map_of_traj out of range");
    }
    const size_t Lz = (size_t)L, steps = Lz * n_scan;
    float *d_r; double *d_c, *d_s, *d_x, *d_y, *d_0, *d_xe, *d_xo, *d_P, *d_To, *d_Td, *d_tp; int64_t *d_off;
    int32_t *d_sot, *d_mot, *d_st, *d_it;
    Staging s(c);
    s.in(d_r, ranges, (size_t)S * n_scan * n).in(d_c, cos_t, n).in(d_s, sin_t, n).in(d_x, K ? ox : nullptr, K).in(d_y, K ? oy : nullptr, K)
        .in(d_off, obs_off, (size_t)M + 1).in(d_0, pose0, Lz * 3).in(d_sot, stream_of_traj, Lz).in(d_mot, map_of_traj, Lz);
    s.out(d_xe, xest_out, steps * 3).out(d_xo, xodom_out, steps * 3).out(d_P, P_final_out, Lz * 9).out(d_st, status_out, Lz)
        .out(d_To, T_obs_out, steps * 9).out(d_it, iters_obs_out, steps).out(d_Td, T_odom_out, steps * 9)
        .out(d_tp, tar_pts_out, steps * 2 * n);
    TRY(s.upload());
    TRY(slam_loc_replay_dev(c, d_r, S, n_scan, n, d_sot, d_x, d_y, d_off, M, K, d_mot, d_0, L, d_c, d_s, angle_min,
                            angle_increment, max_iter, tol, d_xe, d_xo, d_P, d_st, d_To, d_it, d_Td, d_tp));
    TRY(s.download());
    return check_status_sync(c);
}

}  // extern "C"
