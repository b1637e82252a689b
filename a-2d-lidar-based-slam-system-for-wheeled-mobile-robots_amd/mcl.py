"""Monte Carlo localisation on the map's distance field (``slam_mcl_weigh`` / ``slam_mcl_resample``).

F particle filters of P particles each: every scan moves the particles by the odometry step (plus noise the caller
makes), costs the scan from every particle on the likelihood field of its filter's map - the window matcher's cost
for one candidate whose rotation is the particle's own - and resamples systematically when the effective sample
size falls below ``ess_frac * P``.  The reference has no counterpart (it only writes its map); weights are integers
from a table indexed by the accumulated cost, so a filter's particles, ancestors and counts do not depend on the
batch it runs in.

    mcl_weight_table     the table: rint(2^20 exp(-(k << shift) / (2 sigma^2)))
    mcl_weigh_host / mcl_resample_host    the two operators on NumPy arrays
    mcl_settle_host      ``slam_mcl_settle``: the resampled set rearranged so that every survivor keeps its slot
    DeviceMCL            device-resident filters on a DeviceGrid, steps enqueued without a synchronise
    MCL                  one filter on a ``Mapping``, NumPy in and out
"""
from __future__ import annotations

import numpy as np

from . import _abi

MCL_DEAD = _abi.MCL_DEAD


def mcl_weight_table(sigma_cells, shift=0, T=4096, floor=0):
    """uint32 [T]: entry k is the weight of a particle whose accumulated cost is ``k << shift`` above its filter's
    smallest: ``rint(2^20 exp(-(k << shift) / (2 sigma_cells^2)))``, at least ``floor`` (0: a particle further than the
    table reaches gets no weight)."""
    k = np.arange(int(T), dtype=np.int64) << int(shift)
    t = np.rint(float(1 << 20) * np.exp(-k.astype(np.float64) / (2.0 * float(sigma_cells) ** 2)))
    return np.maximum(t, float(floor)).astype(np.uint32)


def _handles(grid):
    """(context handle, grid handle) of a DeviceGrid."""
    return grid._ctx.handle, grid._h


def _opt(a, dtype, shape):
    return None if a is None else np.ascontiguousarray(np.asarray(a, dtype=dtype).reshape(shape))


def mcl_weigh_host(grid, poses, ranges, cos_t, sin_t, motion=None, noise=None, max_range=30.0, cap=64, grid_of_filter=None,
                   field=None, acc=None, grid_of_particle=None, own_maps=False):
    """``slam_mcl_weigh`` on NumPy arrays: poses [F, P, 3], ranges float32 [F, n], cos_t / sin_t [n], motion [F, 3],
    noise [F, P, 3] (only with motion), grid_of_filter int32 [F], field int16 [G, xw, yw] as ``grid_distance_field_host``
    gives it at the same ``cap`` (None: rebuilt), acc int32 [F, P] (None: nothing is accumulated).  Returns (poses
    after the motion, cost int32 [F, P] with -1 for dead particles, acc or None, used int32 [F]); the inputs are not
    changed.  ``grid_of_particle`` int32 [F, P] or ``own_maps=True`` (particle (f, p) on map f * P + p) take
    ``slam_mcl_weigh_maps``: every particle is weighed on its own map."""
    if grid_of_particle is not None or own_maps:
        if grid_of_filter is not None:
            raise ValueError("grid_of_filter and grid_of_particle / own_maps exclude each other")
    p = np.array(poses, dtype=np.float64, order="C")
    if p.ndim != 3 or p.shape[2] != 3:
        raise ValueError("poses must be [F, P, 3]")
    F, P = p.shape[:2]
    ct = np.ascontiguousarray(np.asarray(cos_t, dtype=np.float64).reshape(-1))
    n = ct.shape[0]
    st = _opt(sin_t, np.float64, (n,))
    r = _opt(ranges, np.float32, (F, n))
    a = None if acc is None else np.array(acc, dtype=np.int32, order="C").reshape(F, P)
    f = None if field is None else np.ascontiguousarray(np.asarray(field, dtype=np.int16))
    cost, used = np.empty((F, P), dtype=np.int32), np.empty(F, dtype=np.int32)
    ch, gh = _handles(grid)
    own = grid_of_particle is not None or own_maps
    fn = _abi.lib().slam_mcl_weigh_maps if own else _abi.lib().slam_mcl_weigh
    maps = _opt(grid_of_particle, np.int32, (F, P)) if own else _opt(grid_of_filter, np.int32, (F,))
    _abi.check(fn(ch, gh, _abi.ptr(p), _abi.ptr(_opt(motion, np.float64, (F, 3))), _abi.ptr(_opt(noise, np.float64, (F, P, 3))),
                  _abi.ptr(r), _abi.ptr(ct), _abi.ptr(st), _abi.ptr(maps), F, P, n, float(max_range), int(cap), _abi.ptr(f), _abi.ptr(a),
                  _abi.ptr(cost), _abi.ptr(used)))
    return p, cost, a, used


def mcl_settle_host(context, ancestors, poses_src=None, map0=0):
    """``slam_mcl_settle`` on NumPy arrays: ancestors int32 [F, P] as ``mcl_resample_host`` gives them, poses_src
    [F, P, 3] the particles BEFORE that resampling (or None).  Every surviving particle keeps its slot; the slots of
    particles that died take the surplus copies in ascending order.  Returns (settled int32 [F, P], poses [F, P, 3] =
    poses_src[settled] or None, map_src int32 [F, P] = map0 + f * P + settled, moved int32 [F])."""
    anc = np.ascontiguousarray(np.asarray(ancestors, dtype=np.int32))
    if anc.ndim != 2:
        raise ValueError("ancestors must be [F, P]")
    F, P = anc.shape
    src = _opt(poses_src, np.float64, (F, P, 3))
    settled, map_src, moved = np.empty((F, P), dtype=np.int32), np.empty((F, P), dtype=np.int32), np.empty(F, dtype=np.int32)
    out = None if src is None else np.empty((F, P, 3), dtype=np.float64)
    _abi.check(_abi.lib().slam_mcl_settle(context.handle, _abi.ptr(anc), _abi.ptr(src), F, P, int(map0), _abi.ptr(settled),
                                          _abi.ptr(out), _abi.ptr(map_src), _abi.ptr(moved)))
    return settled, out, map_src, moved


def mcl_resample_host(context, poses, acc, table, u0, shift=0, ess_frac=0.5):
    """``slam_mcl_resample`` on NumPy arrays: poses [F, P, 3], acc int32 [F, P], table uint32 [T] (entries up to 2^20),
    u0 [F] in [0, 1).  Returns (poses [F, P, 3], acc, ancestors int32 [F, P], est [F, 4] = (x, y, theta, ESS) taken
    before resampling, info int32 [F, 4] = (best, live, resampled, amin)); the inputs are not changed."""
    p = np.ascontiguousarray(np.asarray(poses, dtype=np.float64))
    if p.ndim != 3 or p.shape[2] != 3:
        raise ValueError("poses must be [F, P, 3]")
    F, P = p.shape[:2]
    a = np.array(acc, dtype=np.int32, order="C").reshape(F, P)
    t = np.ascontiguousarray(np.asarray(table, dtype=np.uint32).reshape(-1))
    u = _opt(u0, np.float64, (F,))
    out, anc = np.empty_like(p), np.empty((F, P), dtype=np.int32)
    est, info = np.empty((F, 4), dtype=np.float64), np.empty((F, 4), dtype=np.int32)
    _abi.check(_abi.lib().slam_mcl_resample(context.handle, _abi.ptr(p), _abi.ptr(a), _abi.ptr(t), t.shape[0], int(shift), _abi.ptr(u),
                                            float(ess_frac), F, P, _abi.ptr(out), _abi.ptr(anc), _abi.ptr(est), _abi.ptr(info)))
    return out, a, anc, est, info


class DeviceMCL:
    """F filters of P particles resident on the device, on the context of ``grid`` (a :class:`DeviceGrid`).

    Beams: ``cos_t`` / ``sin_t`` [n], or ``angle_min`` / ``angle_max`` / ``n`` (``_abi.trig_tables``).  ``table``:
    the weight table (default ``mcl_weight_table(2.0, shift)``).  ``static_map=True`` builds the distance field once,
    now (again with :meth:`refresh_field`), and every step reads it; otherwise every step rebuilds it from the live
    counters.  ``generator`` (a ``torch.Generator`` on the device) draws the noise - normal, ``noise_sigma`` per
    component - and the resampling offsets of steps that are not given them.

    torch allocates and draws; the kernels run on the context's stream, ordered against torch's current stream without
    a host synchronise (``slam_stream_order``)."""

    def __init__(self, grid, F, P, cos_t=None, sin_t=None, angle_min=None, angle_max=None, n=None, cap=64, max_range=30.0,
                 table=None, shift=0, ess_frac=0.5, grid_of_filter=None, static_map=False, generator=None,
                 noise_sigma=(0.01, 0.01, 0.005)):
        import torch
        if not torch.cuda.is_available():
            raise _abi.SlamError("DeviceMCL needs a GPU (torch.cuda.is_available() is False); no CPU fallback")
        self.torch, self.grid, self.ctx = torch, grid, grid._ctx
        self.dev = torch.device("cuda", self.ctx.device)
        self.F, self.P = int(F), int(P)
        if cos_t is None:
            cos_t, sin_t = _abi.trig_tables(angle_min, angle_max, int(n))
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).to(self.dev)
        self.cos_t, self.sin_t = up(cos_t, np.float64).reshape(-1), up(sin_t, np.float64).reshape(-1)
        self.n = int(self.cos_t.shape[0])
        self.cap, self.max_range, self.shift, self.ess_frac = int(cap), float(max_range), int(shift), float(ess_frac)
        tab = mcl_weight_table(2.0, shift) if table is None else np.asarray(table, dtype=np.uint32).reshape(-1)
        self.table = up(np.ascontiguousarray(tab).view(np.int32), np.int32)        # the uint32 bits (torch has no uint32 arithmetic to need)
        self.T = int(tab.shape[0])
        self.gof = None if grid_of_filter is None else up(grid_of_filter, np.int32).reshape(self.F)
        self.generator = generator
        self.noise_sigma = up(noise_sigma, np.float64).reshape(3)
        new = lambda shape, dt: torch.zeros(shape, dtype=dt, device=self.dev)
        self.poses, self._spare = new((self.F, self.P, 3), torch.float64), new((self.F, self.P, 3), torch.float64)
        self.acc, self.cost, self.ancestors = (new((self.F, self.P), torch.int32) for _ in range(3))
        self.used = new((self.F,), torch.int32)
        self._est, self._info = new((self.F, 4), torch.float64), new((self.F, 4), torch.int32)
        self.est, self.info = self._est, self._info
        self.est_hist = self.info_hist = None
        self.field = None
        self._held = None                      # the inputs of the steps enqueued last: kept until torch is ordered behind them
        torch.cuda.synchronize(self.dev)
        if static_map:
            self.refresh_field()

    def _torch_stream(self):
        return self.torch.cuda.current_stream(self.dev).cuda_stream

    def _begin(self):
        """Order torch's current stream behind everything enqueued on the context so far, and only then let go of the
        tensors those kernels read.  torch's caching allocator knows nothing of the context's stream: a block freed
        earlier could be handed out again, and overwritten by torch, while a queued kernel still reads it."""
        self.ctx.stream_order(self._torch_stream(), 0)
        self._held = None

    def __del__(self):
        try:
            if self._held is not None and self.ctx._h is not None:
                self._begin()
        except Exception:
            pass

    def refresh_field(self):
        """Build the distance field of the map as it stands now and keep it (``static_map``)."""
        self.field = self.grid.distance_field(self.cap, out=self.field)

    def set_particles(self, poses):
        """poses [F, P, 3] (NumPy or torch): the particles of every filter; accumulated costs start at 0."""
        torch = self.torch
        self._begin()                                             # torch's copies wait for the steps enqueued so far
        src = poses if torch.is_tensor(poses) else torch.from_numpy(np.ascontiguousarray(np.asarray(poses, dtype=np.float64)))
        self.poses.copy_(src.reshape(self.F, self.P, 3))
        self.acc.zero_()

    def _weigh_resample(self, ranges, motion, noise, u0, est, info):
        L, h = _abi.lib(), self.ctx.handle
        _abi.check(L.slam_mcl_weigh_dev(h, self.grid._h, _abi.ptr(self.poses), _abi.ptr(motion), _abi.ptr(noise), _abi.ptr(ranges),
                                        _abi.ptr(self.cos_t), _abi.ptr(self.sin_t), _abi.ptr(self.gof), self.F, self.P, self.n,
                                        self.max_range, self.cap, _abi.ptr(self.field), _abi.ptr(self.acc), _abi.ptr(self.cost),
                                        _abi.ptr(self.used)))
        _abi.check(L.slam_mcl_resample_dev(h, _abi.ptr(self.poses), _abi.ptr(self.acc), _abi.ptr(self.table), self.T, self.shift,
                                           _abi.ptr(u0), self.ess_frac, self.F, self.P, _abi.ptr(self._spare), _abi.ptr(self.ancestors),
                                           _abi.ptr(est), _abi.ptr(info)))
        self.poses, self._spare = self._spare, self.poses

    def _draw(self, shape, normal):
        torch = self.torch
        if self.generator is None:
            raise ValueError("noise / u0 not given and no torch.Generator was passed at construction")
        if normal:
            return torch.randn(shape, dtype=torch.float64, device=self.dev, generator=self.generator) * self.noise_sigma
        return torch.rand(shape, dtype=torch.float64, device=self.dev, generator=self.generator).clamp_(max=float(np.nextafter(1.0, 0.0)))

    def _check(self, name, t, shape, dtype):
        if not self.torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous():
            raise ValueError("%s must be a contiguous %s device tensor of shape %r" % (name, dtype, shape))

    def step(self, ranges, motion=None, noise=None, u0=None):
        """One scan: ranges float32 [F, n], motion float64 [F, 3] or None, noise float64 [F, P, 3] and u0 float64 [F]
        in [0, 1) (device tensors, or drawn with the generator; no noise without motion).  Enqueues weigh + resample;
        ``est`` / ``info`` / ``ancestors`` / ``cost`` / ``used`` hold the step's outputs, ``poses`` / ``acc`` the
        state after it.  No synchronise: the tensors given are read by kernels that may still be queued when this
        returns.  The filter keeps a reference to them, and to those it drew, until the next call has ordered torch's
        stream behind these kernels; a caller that overwrites them in place orders itself with
        ``ctx.stream_order`` or ``results()`` first."""
        torch = self.torch
        self._begin()
        self._check("ranges", ranges, (self.F, self.n), torch.float32)
        if motion is not None:
            self._check("motion", motion, (self.F, 3), torch.float64)
            if noise is None and self.generator is not None:
                noise = self._draw((self.F, self.P, 3), True)
        if noise is not None:
            self._check("noise", noise, (self.F, self.P, 3), torch.float64)
        u0 = self._draw((self.F,), False) if u0 is None else u0
        self._check("u0", u0, (self.F,), torch.float64)
        self.ctx.stream_order(self._torch_stream(), 1)            # the kernels wait for what torch has made so far
        self.est, self.info = self._est, self._info               # (after run() they were views of the history)
        self._weigh_resample(ranges, motion, noise, u0, self.est, self.info)
        self._held = (ranges, motion, noise, u0)

    def run(self, ranges, motion=None, noise=None, u0=None):
        """S scans: ranges [S, F, n], motion [S, F, 3], noise [S, F, P, 3], u0 [S, F] (drawn up front when absent).
        Enqueues the S steps back to back and keeps every step's estimate and counts in ``est_hist`` / ``info_hist``
        [S, F, 4] (``est`` / ``info`` are the last step's).  No synchronise; the inputs are kept as :meth:`step` keeps
        them."""
        torch = self.torch
        self._begin()                                             # also: the history the steps before may still be read from
        S = int(ranges.shape[0])
        self._check("ranges", ranges, (S, self.F, self.n), torch.float32)
        if motion is not None:
            self._check("motion", motion, (S, self.F, 3), torch.float64)
            if noise is None and self.generator is not None:
                noise = self._draw((S, self.F, self.P, 3), True)
        if noise is not None:
            self._check("noise", noise, (S, self.F, self.P, 3), torch.float64)
        u0 = self._draw((S, self.F), False) if u0 is None else u0
        self._check("u0", u0, (S, self.F), torch.float64)
        self.est_hist = torch.empty((S, self.F, 4), dtype=torch.float64, device=self.dev)
        self.info_hist = torch.empty((S, self.F, 4), dtype=torch.int32, device=self.dev)
        self.ctx.stream_order(self._torch_stream(), 1)
        for k in range(S):
            self._weigh_resample(ranges[k], None if motion is None else motion[k], None if noise is None else noise[k], u0[k],
                                 self.est_hist[k], self.info_hist[k])
        self.est, self.info = self.est_hist[S - 1], self.info_hist[S - 1]
        self._held = (ranges, motion, noise, u0)

    def results(self):
        """Synchronises and returns a dict of NumPy arrays: poses, acc, est, info, ancestors, cost, used, and after
        :meth:`run` est_hist / info_hist."""
        self.ctx.synchronize()
        out = {k: getattr(self, k).cpu().numpy() for k in ("poses", "acc", "est", "info", "ancestors", "cost", "used")}
        if self.est_hist is not None:
            out["est_hist"], out["info_hist"] = self.est_hist.cpu().numpy(), self.info_hist.cpu().numpy()
        return out


class MCL:
    """One particle filter on a :class:`Mapping`, NumPy in and out.

    ``rng``: a ``numpy.random.Generator`` that draws the initial particles, the motion noise (normal,
    ``noise_sigma`` per component) and the resampling offsets.  The map's field is rebuilt at every update unless
    ``static_map`` is set (then :meth:`refresh_field` rebuilds it)."""

    def __init__(self, mapping, n_particles, rng, cap=64, max_range=30.0, sigma_cells=2.0, shift=0, T=4096, ess_frac=0.5,
                 noise_sigma=(0.01, 0.01, 0.005), static_map=False):
        self.mapping, self.P, self.rng = mapping, int(n_particles), rng
        self.cap, self.max_range, self.shift, self.ess_frac = int(cap), float(max_range), int(shift), float(ess_frac)
        self.table = mcl_weight_table(sigma_cells, shift, T)
        self.noise_sigma = np.asarray(noise_sigma, dtype=np.float64).reshape(3)
        self.static_map = bool(static_map)
        self.field = None
        self.particles = np.zeros((self.P, 3))
        self.acc = np.zeros(self.P, dtype=np.int32)
        self.pose, self.ess, self.info = np.full(3, np.nan), 0.0, None
        if self.static_map:
            self.refresh_field()

    def refresh_field(self):
        self.field = self.mapping.distance_field(self.cap)[None]

    def init(self, pose, spread):
        """Particles uniform within +-spread (x, y, theta) of ``pose``."""
        pose = np.asarray(pose, dtype=np.float64).reshape(3)
        self.particles = pose + self.rng.uniform(-1.0, 1.0, (self.P, 3)) * np.asarray(spread, dtype=np.float64).reshape(3)
        self.acc = np.zeros(self.P, dtype=np.int32)
        return self.particles

    def init_global(self, ranges, angle_min, angle_max, spread, **locate_kw):
        """Start without a pose: locate the scan in the map (``Mapping.locate_scan``, which takes ``locate_kw``), then
        :meth:`init` around the answer.  Returns (pose [3], cost, used beams) of the localisation."""
        locate_kw.setdefault("max_range", self.max_range)
        locate_kw.setdefault("cap", self.cap)
        pose, cost, used = self.mapping.locate_scan(ranges, angle_min, angle_max, **locate_kw)
        self.init(pose, spread)
        return pose, cost, used

    def update(self, ranges, angle_min, angle_max, u=None):
        """One scan: ``u`` the odometry step (dx, dy, dtheta) in the robot frame since the last scan, or None.
        Returns (pose [3], ess): the weighted estimate taken before resampling."""
        r = np.ascontiguousarray(np.asarray(ranges, dtype=np.float32).reshape(1, -1))
        ct, st = _abi.trig_tables(angle_min, angle_max, r.shape[1])
        motion = noise = None
        if u is not None:
            motion = np.asarray(u, dtype=np.float64).reshape(1, 3)
            noise = self.rng.normal(0.0, 1.0, (1, self.P, 3)) * self.noise_sigma
        poses, _cost, acc, _used = mcl_weigh_host(self.mapping.grid, self.particles[None], r, ct, st, motion=motion, noise=noise,
                                                  max_range=self.max_range, cap=self.cap, field=self.field if self.static_map else None,
                                                  acc=self.acc[None])
        u0 = np.array([min(self.rng.uniform(), np.nextafter(1.0, 0.0))])
        out, acc, _anc, est, info = mcl_resample_host(self.mapping._ctx, poses, acc, self.table, u0, shift=self.shift,
                                                      ess_frac=self.ess_frac)
        self.particles, self.acc, self.info = out[0], acc[0], info[0]
        self.pose, self.ess = est[0, :3].copy(), float(est[0, 3])
        return self.pose, self.ess
