"""Grid FastSLAM: Rao-Blackwellised particle-filter SLAM with an occupancy grid per particle.

Particle (f, p) of F filters of P particles owns map ``f * P + p`` of one :class:`DeviceGrid`.  A scan is five calls:

    slam_mcl_weigh_maps          every particle moved by the odometry step and weighed on ITS OWN map's distance field
    slam_mcl_resample            weights, estimate, effective sample size, systematic resampling
    slam_mcl_settle              the resampled set rearranged so that every surviving particle keeps its slot
    slam_grid_copy_maps          only the maps of slots whose particle died are copied, in place, from a survivor's map
    slam_grid_update_particles   the scan integrated into every particle's map from its new pose

The heaviest particle always survives systematic resampling and keeps its slot, so ``info[f, 0]`` (``best``) names its
pose and its map after the step as well.  The reference has no counterpart: its map is built from one pose estimate.

    DeviceGridSLAM   F filters resident on the device, steps enqueued without a synchronise
    GridSLAM         one filter, NumPy in and out
"""
from __future__ import annotations

import numpy as np

from . import _abi
from .grid import (DeviceGrid, _first, _one_or_many, clearance_cells2, frontier_dict, grid_copy_maps_host, grid_frontiers_host,
                   grid_travel_host, grid_update_particles_host, grid_view_gain_host, nearest_goal, pose_cell, travel_goal,
                   view_poses, view_tables)
from .mcl import mcl_resample_host, mcl_settle_host, mcl_weigh_host, mcl_weight_table


class DeviceGridSLAM:
    """F filters of P particles and their F * P maps (``xw`` x ``yw`` cells of ``reso`` metres, :meth:`DeviceGrid.metric`)
    resident on the device.

    Beams: ``cos_t`` / ``sin_t`` [n], or ``angle_min`` / ``angle_max`` / ``n``.  ``table``: the weight table (default
    ``mcl_weight_table(2.0, shift)``).  ``generator`` (a ``torch.Generator`` on the device) draws the noise - normal,
    ``noise_sigma`` per component - and the resampling offsets of steps that are not given them.  ``live_pmap`` keeps
    the maps' pmap resident on the device.

    torch allocates and draws; the kernels run on the context's stream, ordered against torch's current stream without
    a host synchronise (``slam_stream_order``), as :class:`DeviceMCL` does."""

    def __init__(self, F, P, xw, yw, reso, cos_t=None, sin_t=None, angle_min=None, angle_max=None, n=None, cap=64, max_range=30.0,
                 table=None, shift=0, ess_frac=0.5, generator=None, noise_sigma=(0.01, 0.01, 0.005), context=None, live_pmap=False,
                 **grid_kw):
        import torch
        if not torch.cuda.is_available():
            raise _abi.SlamError("DeviceGridSLAM needs a GPU (torch.cuda.is_available() is False); no CPU fallback")
        self.torch = torch
        self.F, self.P = int(F), int(P)
        self.grid = DeviceGrid.metric(self.F * self.P, xw, yw, reso, context=context, **grid_kw)
        self.ctx = self.grid._ctx
        self.dev = torch.device("cuda", self.ctx.device)
        if live_pmap:
            self.grid.live_pmap()
        if cos_t is None:
            cos_t, sin_t = _abi.trig_tables(angle_min, angle_max, int(n))
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).to(self.dev)
        self.cos_t, self.sin_t = up(cos_t, np.float64).reshape(-1), up(sin_t, np.float64).reshape(-1)
        self.n = int(self.cos_t.shape[0])
        self.cap, self.max_range, self.shift, self.ess_frac = int(cap), float(max_range), int(shift), float(ess_frac)
        tab = mcl_weight_table(2.0, shift) if table is None else np.asarray(table, dtype=np.uint32).reshape(-1)
        self.table = up(np.ascontiguousarray(tab).view(np.int32), np.int32)
        self.T = int(tab.shape[0])
        self.generator = generator
        self.noise_sigma = up(noise_sigma, np.float64).reshape(3)
        new = lambda shape, dt: torch.zeros(shape, dtype=dt, device=self.dev)
        FP = (self.F, self.P)
        self.poses, self._moved_poses, self._gathered = (new(FP + (3,), torch.float64) for _ in range(3))
        self.acc, self.cost, self.ancestors, self.settled, self.map_src = (new(FP, torch.int32) for _ in range(5))
        self.copied = new((self.F * self.P,), torch.int32)
        self.used, self._moved = new((self.F,), torch.int32), new((self.F,), torch.int32)
        self._est, self._info = new((self.F, 4), torch.float64), new((self.F, 4), torch.int32)
        self.est, self.info, self.moved = self._est, self._info, self._moved
        self.est_hist = self.info_hist = self.moved_hist = None
        self._held = None
        torch.cuda.synchronize(self.dev)

    def _torch_stream(self):
        return self.torch.cuda.current_stream(self.dev).cuda_stream

    def _begin(self):
        """Order torch's current stream behind everything enqueued on the context so far, and only then let go of the
        tensors those kernels read (:meth:`DeviceMCL._begin`)."""
        self.ctx.stream_order(self._torch_stream(), 0)
        self._held = None

    def __del__(self):
        try:
            if self._held is not None and self.ctx._h is not None:
                self._begin()
        except Exception:
            pass

    def set_particles(self, poses):
        """poses [F, P, 3] (NumPy or torch), or one pose [3] for every particle; accumulated costs start at 0.  The maps
        are not touched (``grid.reset()`` clears them)."""
        torch = self.torch
        self._begin()
        src = poses if torch.is_tensor(poses) else torch.from_numpy(np.ascontiguousarray(np.asarray(poses, dtype=np.float64)))
        self.poses.copy_(src.reshape(1, 1, 3).expand(self.F, self.P, 3) if src.numel() == 3 else src.reshape(self.F, self.P, 3))
        self.acc.zero_()

    def _step(self, ranges, motion, noise, u0, est, info, moved):
        L, h, g, p = _abi.lib(), self.ctx.handle, self.grid._h, _abi.ptr
        _abi.check(L.slam_mcl_weigh_maps_dev(h, g, p(self.poses), p(motion), p(noise), p(ranges), p(self.cos_t), p(self.sin_t), None,
                                             self.F, self.P, self.n, self.max_range, self.cap, None, p(self.acc), p(self.cost),
                                             p(self.used)))
        _abi.check(L.slam_mcl_resample_dev(h, p(self.poses), p(self.acc), p(self.table), self.T, self.shift, p(u0), self.ess_frac,
                                           self.F, self.P, p(self._gathered), p(self.ancestors), p(est), p(info)))
        _abi.check(L.slam_mcl_settle_dev(h, p(self.ancestors), p(self.poses), self.F, self.P, 0, p(self.settled), p(self._moved_poses),
                                         p(self.map_src), p(moved)))
        _abi.check(L.slam_grid_copy_maps_dev(h, g, p(self.map_src), 0, self.F * self.P, p(self.copied)))
        _abi.check(L.slam_grid_update_particles_dev(h, g, p(ranges), p(self.cos_t), p(self.sin_t), p(self._moved_poses), p(self.acc),
                                                    self.F, self.P, self.n, 0))
        self.poses, self._moved_poses = self._moved_poses, self.poses

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

    def _inputs(self, ranges, motion, noise, u0, lead):
        torch = self.torch
        self._check("ranges", ranges, lead + (self.F, self.n), torch.float32)
        if motion is not None:
            self._check("motion", motion, lead + (self.F, 3), torch.float64)
            if noise is None and self.generator is not None:
                noise = self._draw(lead + (self.F, self.P, 3), True)
        if noise is not None:
            self._check("noise", noise, lead + (self.F, self.P, 3), torch.float64)
        u0 = self._draw(lead + (self.F,), False) if u0 is None else u0
        self._check("u0", u0, lead + (self.F,), torch.float64)
        return noise, u0

    def step(self, ranges, motion=None, noise=None, u0=None):
        """One scan: ranges float32 [F, n], motion float64 [F, 3] or None, noise float64 [F, P, 3] and u0 float64 [F] in
        [0, 1) (device tensors, or drawn with the generator; no noise without motion).  Enqueues weigh_maps (the field
        rebuilt), resample, settle, copy_maps and update_particles (from the settled poses and the post-resample
        ``acc``).  ``est`` / ``info`` / ``moved`` / ``ancestors`` / ``settled`` / ``copied`` / ``cost`` / ``used`` hold
        the step's outputs, ``poses`` / ``acc`` and the grid the state after it.  No synchronise; the inputs are kept
        as :meth:`DeviceMCL.step` keeps them."""
        self._begin()
        noise, u0 = self._inputs(ranges, motion, noise, u0, ())
        self.ctx.stream_order(self._torch_stream(), 1)            # the kernels wait for what torch has made so far
        self.est, self.info, self.moved = self._est, self._info, self._moved
        self._step(ranges, motion, noise, u0, self.est, self.info, self.moved)
        self._held = (ranges, motion, noise, u0)

    def run(self, ranges, motion=None, noise=None, u0=None):
        """S scans: ranges [S, F, n], motion [S, F, 3], noise [S, F, P, 3], u0 [S, F] (drawn up front when absent).
        Enqueues the S steps back to back and keeps every step's estimate, counts and number of moved slots in
        ``est_hist`` / ``info_hist`` [S, F, 4] and ``moved_hist`` [S, F].  No synchronise."""
        torch = self.torch
        self._begin()
        S = int(ranges.shape[0])
        noise, u0 = self._inputs(ranges, motion, noise, u0, (S,))
        self.est_hist = torch.empty((S, self.F, 4), dtype=torch.float64, device=self.dev)
        self.info_hist = torch.empty((S, self.F, 4), dtype=torch.int32, device=self.dev)
        self.moved_hist = torch.empty((S, self.F), dtype=torch.int32, device=self.dev)
        self.ctx.stream_order(self._torch_stream(), 1)
        for k in range(S):
            self._step(ranges[k], None if motion is None else motion[k], None if noise is None else noise[k], u0[k],
                       self.est_hist[k], self.info_hist[k], self.moved_hist[k])
        self.est, self.info, self.moved = self.est_hist[S - 1], self.info_hist[S - 1], self.moved_hist[S - 1]
        self._held = (ranges, motion, noise, u0)

    def results(self):
        """Synchronises and returns a dict of NumPy arrays: poses, acc, est, info, moved, ancestors, settled, map_src,
        copied, cost, used, and after :meth:`run` est_hist / info_hist / moved_hist."""
        self.ctx.synchronize()
        names = ("poses", "acc", "est", "info", "moved", "ancestors", "settled", "map_src", "copied", "cost", "used")
        out = {k: getattr(self, k).cpu().numpy() for k in names}
        if self.est_hist is not None:
            out.update(est_hist=self.est_hist.cpu().numpy(), info_hist=self.info_hist.cpu().numpy(),
                       moved_hist=self.moved_hist.cpu().numpy())
        return out

    def best(self, f=0):
        """(slot, pose [3]) of filter f's best particle of the last step; synchronises."""
        self.ctx.synchronize()
        b = int(self.info[f, 0].item())
        return b, (self.poses[f, b].cpu().numpy() if b >= 0 else np.full(3, np.nan))

    def best_map(self, f=0):
        """pmap int8 [xw, yw] of the map of filter f's best particle (``info[f, 0]``) as it stands after the last step."""
        b, _ = self.best(f)
        if b < 0:
            raise _abi.SlamError("filter %d has no live particle" % f)
        return self.grid.read(f * self.P + b, want=("pmap",))["pmap"]

    def frontiers(self, radius=2, min_unknown=13, min_clear2=0, cap=64, min_size=5, max_clusters=256, labels=False):
        """The frontiers (:meth:`DeviceGrid.frontiers`) of every filter's best particle's map, one query per filter on map
        ``f * P + info[f, 0]``; the map index is formed on the device and a filter with no live particle (``info[f, 0]
        < 0``) asks for no map: its counts are (-1, -1).  Returns the device tensors; no synchronise."""
        torch = self.torch
        self._begin()
        maps = self._best_maps()
        out = (torch.empty((self.F, 2), dtype=torch.int32, device=self.dev),
               torch.empty((self.F, int(max_clusters), 8), dtype=torch.int32, device=self.dev),
               torch.empty((self.F, int(max_clusters), 2), dtype=torch.int64, device=self.dev))
        if labels:
            out += (torch.empty((self.F, self.grid.xw, self.grid.yw), dtype=torch.int32, device=self.dev),)
        self.ctx.stream_order(self._torch_stream(), 1)
        self.grid.frontiers(maps, radius=radius, min_unknown=min_unknown, min_clear2=min_clear2, cap=cap, min_size=min_size,
                            max_clusters=max_clusters, out=out)
        self._held = (maps,) + out
        return out

    def _best_maps(self):
        """int32 [F] on the device: map ``f * P + info[f, 0]`` of every filter, -1 for a filter with no live particle."""
        torch = self.torch
        best = self.info[:, 0]
        return torch.where(best >= 0, torch.arange(self.F, dtype=torch.int32, device=self.dev) * self.P + best,
                           torch.full_like(best, -1)).to(torch.int32).contiguous()

    def _best_cells(self):
        """int32 [F, 1, 2] on the device: the cell of every filter's best particle by the map's rule, ``int(scale * (v +
        off))`` truncated toward zero; (-1, -1) for a filter with no live particle."""
        torch = self.torch
        best = self.info[:, 0].to(torch.int64)
        xy = self.poses[torch.arange(self.F, device=self.dev), best.clamp(min=0), :2]
        cell = pose_cell(xy, self.grid.scale, self.grid.off_x, self.grid.off_y)
        return torch.where((best >= 0).reshape(-1, 1), cell, torch.full_like(cell, -1)).reshape(self.F, 1, 2).contiguous()

    def travel(self, goals=None, foot=0, through_unknown=False, min_clear2=0, cap=64, path_cap=0, cost=True, dirs=False):
        """The travel-cost field (:meth:`DeviceGrid.travel`) of every filter's best particle's map from that particle's
        cell, one query per filter on map ``f * P + info[f, 0]``; source and map index are formed on the device, and a
        filter with no live particle asks for no map: its status is -1.  goals: int32 [F, Q, 2] device tensor or None.
        Returns the dict of device tensors; no synchronise."""
        self._begin()
        maps, src = self._best_maps(), self._best_cells()
        self.ctx.stream_order(self._torch_stream(), 1)
        out = self.grid.travel(src, maps, goals=goals, foot=foot, through_unknown=through_unknown, min_clear2=min_clear2, cap=cap,
                               path_cap=path_cap, cost=cost, dirs=dirs)
        self._held = (maps, src, goals) + tuple(out.values())
        return out

    def view_gain(self, reps, n=360, max_range=None, skip=1, return_seen=False):
        """What a scan from each cell of ``reps`` (int32 [F, M, 2] device tensor, e.g. the representatives of
        :meth:`frontiers`' table) would reveal of its filter's best particle's map (:meth:`DeviceGrid.view_gain`): the
        views stand at the cell centres, heading 0, with the ``n`` beams of :func:`view_tables` over the full circle to
        ``max_range`` (default: the filter's).  Poses and map indices are formed on the device.  Returns counts int32
        [F, M, 4] (``_abi.VIEW_*``), rows of -1 for a cell with a negative coordinate and for a filter with no live
        particle, and with ``return_seen`` also the bit words [F, M, xw, ceil(yw / 32)].  No synchronise."""
        torch = self.torch
        self._begin()
        F, M = int(reps.shape[0]), int(reps.shape[1])
        if F != self.F or reps.dim() != 3 or int(reps.shape[2]) != 2:
            raise ValueError("reps must be [F, M, 2]")
        tables = self._view_tables = getattr(self, "_view_tables", None) or {}
        if int(n) not in tables:
            tables[int(n)] = tuple(torch.from_numpy(t).to(self.dev) for t in view_tables(int(n)))
        ct, st = tables[int(n)]
        poses = view_poses(reps, self.grid.scale, self.grid.off_x, self.grid.off_y)
        poses = torch.where((reps >= 0).all(dim=-1, keepdim=True), poses, torch.full_like(poses, float("nan"))).reshape(F * M, 3).contiguous()
        maps = self._best_maps().reshape(F, 1).expand(F, M).reshape(F * M).contiguous()
        self.ctx.stream_order(self._torch_stream(), 1)
        out = self.grid.view_gain(poses, ct, st, max_range=self.max_range if max_range is None else max_range, skip=skip,
                                  grid_of_batch=maps, return_seen=return_seen)
        self._held = (reps, poses, maps, ct, st) + (out if return_seen else (out,))
        if return_seen:
            return out[0].reshape(F, M, -1), out[1].reshape(F, M, self.grid.xw, -1)
        return out.reshape(F, M, -1)

    def next_goals(self, foot=0, through_unknown=False, radius=2, min_unknown=13, min_clear2=0, cap=64, min_size=5, max_clusters=256,
                   by="travel", bias=100, n=360, max_range=None, skip=1):
        """Every filter's next exploration goal by travel cost: the frontiers of its best particle's map
        (:meth:`frontiers`), their representatives passed device to device as the goals of :meth:`travel`, and of the
        kept clusters the one with the smallest cost >= 0, ties to the lowest label - chosen with torch ops.  Returns
        (cell int32 [F, 2], cost int32 [F], status int32 [F]) on the device; cell (-1, -1) and cost -1 where no kept
        cluster is reachable.  No synchronise.
        ``by="gain"``, next-best-view: the representatives also go device to device into :meth:`view_gain` (``n``,
        ``max_range``, ``skip``), and of the kept clusters with cost c >= 0 and u > 0 unknown cells in view the one with
        the largest u / (c + ``bias``) wins, compared exactly in int64 (u_k * (c_l + bias) > u_l * (c_k + bias)), ties to
        the lower cost, then to the lower label (:func:`gain_goal`).  Returns (cell, cost, status, unknown int32 [F]);
        cell (-1, -1), cost -1 and unknown -1 where there is no candidate.  ``bias`` (default 100) is in travel-cost
        units; it is a starting value, not a tuned one."""
        if by not in ("travel", "gain"):
            raise ValueError("by must be 'travel' or 'gain'")
        torch = self.torch
        table = self.frontiers(radius=radius, min_unknown=min_unknown, min_clear2=min_clear2, cap=cap, min_size=min_size,
                               max_clusters=max_clusters)[1]
        held = self._held
        self.ctx.stream_order(self._torch_stream(), 0)           # torch's copy of the representatives waits for the table
        reps = table[:, :, 2:4].contiguous()
        maps, src = self._best_maps(), self._best_cells()
        self.ctx.stream_order(self._torch_stream(), 1)
        out = self.grid.travel(src, maps, goals=reps, foot=foot, through_unknown=through_unknown, min_clear2=min_clear2, cap=cap,
                               cost=False)
        if by == "gain":
            return self._gain_goals(reps, out, held + (maps, src), int(bias), n, max_range, skip)
        self.ctx.stream_order(self._torch_stream(), 0)
        gc = out["goal_cost"].to(torch.int64)
        key = torch.where(gc >= 0, gc, torch.full_like(gc, 2 ** 62))
        k = torch.argmin(key, dim=1)                  # the first of equal costs: the lowest label
        rows = torch.arange(self.F, device=self.dev)
        ok = gc[rows, k] >= 0
        cell = torch.where(ok.reshape(-1, 1), reps[rows, k], torch.full((self.F, 2), -1, dtype=torch.int32, device=self.dev))
        costs = torch.where(ok, out["goal_cost"][rows, k], torch.full((self.F,), -1, dtype=torch.int32, device=self.dev))
        self._held = held + (maps, src, reps) + tuple(out.values())
        return cell, costs, out["status"]

    def _gain_goals(self, reps, travel, held, bias, n, max_range, skip):
        """The rule of ``next_goals(by="gain")`` on the device: a knock-out over the clusters in label order, so the left
        of every pair has the lower label and keeps a full tie."""
        torch = self.torch
        if bias < 1:
            raise ValueError("bias must be >= 1")
        counts = self.view_gain(reps, n=n, max_range=max_range, skip=skip)
        held = held + self._held + tuple(travel.values())
        self.ctx.stream_order(self._torch_stream(), 0)           # torch reads the costs and the counts after the kernels
        F, M = int(reps.shape[0]), int(reps.shape[1])
        width = 1
        while width < max(M, 1):
            width *= 2
        c = torch.full((F, width), -1, dtype=torch.int64, device=self.dev)
        u = torch.zeros((F, width), dtype=torch.int64, device=self.dev)
        c[:, :M] = travel["goal_cost"].to(torch.int64)
        u[:, :M] = counts[:, :, _abi.VIEW_UNKNOWN].to(torch.int64)
        ok = (c >= 0) & (u > 0)                       # (a row beyond the kept clusters is (-1, -1): no cost, no view)
        k = torch.arange(width, dtype=torch.int64, device=self.dev).reshape(1, -1).expand(F, width)
        while width > 1:
            cl, cr, ul, ur, okl, okr, kl, kr = c[:, 0::2], c[:, 1::2], u[:, 0::2], u[:, 1::2], ok[:, 0::2], ok[:, 1::2], k[:, 0::2], k[:, 1::2]
            lhs, rhs = ur * (cl + bias), ul * (cr + bias)
            right = okr & (~okl | (lhs > rhs) | ((lhs == rhs) & (cr < cl)))
            c, u, ok, k = torch.where(right, cr, cl), torch.where(right, ur, ul), okl | okr, torch.where(right, kr, kl)
            width //= 2
        rows = torch.arange(F, device=self.dev)
        ok, k = ok[:, 0], k[:, 0].clamp(max=max(M - 1, 0))
        neg = torch.full((F,), -1, dtype=torch.int32, device=self.dev)
        cell = torch.where(ok.reshape(-1, 1), reps[rows, k], torch.full((F, 2), -1, dtype=torch.int32, device=self.dev))
        costs = torch.where(ok, c[:, 0].to(torch.int32), neg)
        unknown = torch.where(ok, u[:, 0].to(torch.int32), neg)
        self._held = held + (counts,)
        return cell, costs, travel["status"], unknown

    @property
    def trajectory(self):
        """The per-step estimates [S, F, 3] of the last :meth:`run` (or [1, F, 3] of the last :meth:`step`); synchronises."""
        self.ctx.synchronize()
        e = self.est_hist if self.est_hist is not None and self.est is not self._est else self.est[None]
        return e[..., :3].cpu().numpy()


class GridSLAM:
    """One filter with a map per particle, NumPy in and out: the counterpart of :class:`MCL` that builds its own maps.

    ``rng``: a ``numpy.random.Generator`` that draws the motion noise (normal, ``noise_sigma`` per component) and the
    resampling offsets, in that order at every update."""

    def __init__(self, xw, yw, reso, n_particles, rng, cap=64, max_range=30.0, sigma_cells=2.0, shift=0, T=4096, ess_frac=0.5,
                 noise_sigma=(0.01, 0.01, 0.005), context=None, **grid_kw):
        self.P, self.rng = int(n_particles), rng
        self.grid = DeviceGrid.metric(self.P, xw, yw, reso, context=context, **grid_kw)
        self.cap, self.max_range, self.shift, self.ess_frac = int(cap), float(max_range), int(shift), float(ess_frac)
        self.table = mcl_weight_table(sigma_cells, shift, T)
        self.noise_sigma = np.asarray(noise_sigma, dtype=np.float64).reshape(3)
        self.particles = np.zeros((self.P, 3))
        self.acc = np.zeros(self.P, dtype=np.int32)
        self.pose, self.ess, self.info, self.moved, self.best = np.full(3, np.nan), 0.0, None, 0, 0
        self.trajectory = []

    def init(self, pose):
        """Every particle at ``pose`` (x, y, theta): SLAM starts from a known pose, the noise spreads them."""
        self.particles = np.tile(np.asarray(pose, dtype=np.float64).reshape(1, 3), (self.P, 1))
        self.acc = np.zeros(self.P, dtype=np.int32)
        return self.particles

    def update(self, ranges, angle_min, angle_max, u=None, noise=None, u0=None):
        """One scan: ``u`` the odometry step (dx, dy, dtheta) in the robot frame since the last scan, or None.  ``noise``
        [P, 3] / ``u0``: given instead of drawn.  Returns (pose [3], ess): the weighted estimate taken before resampling;
        ``best_pose`` is the best particle's pose and :attr:`pmap` its map."""
        r = np.ascontiguousarray(np.asarray(ranges, dtype=np.float32).reshape(1, -1))
        ct, st = _abi.trig_tables(angle_min, angle_max, r.shape[1])
        motion = None
        if u is not None:
            motion = np.asarray(u, dtype=np.float64).reshape(1, 3)
            noise = self.rng.normal(0.0, 1.0, (1, self.P, 3)) * self.noise_sigma if noise is None else np.asarray(noise).reshape(1, self.P, 3)
        else:
            noise = None
        moved, _cost, acc, _used = mcl_weigh_host(self.grid, self.particles[None], r, ct, st, motion=motion, noise=noise,
                                                  max_range=self.max_range, cap=self.cap, acc=self.acc[None], own_maps=True)
        u0 = np.array([min(self.rng.uniform(), np.nextafter(1.0, 0.0)) if u0 is None else float(u0)])
        ctx = self.grid._ctx
        _out, acc, anc, est, info = mcl_resample_host(ctx, moved, acc, self.table, u0, shift=self.shift, ess_frac=self.ess_frac)
        _settled, poses, map_src, nmoved = mcl_settle_host(ctx, anc, moved)
        grid_copy_maps_host(self.grid, map_src[0])
        grid_update_particles_host(self.grid, r, ct, st, poses, acc=acc)
        self.particles, self.acc, self.info, self.moved = poses[0], acc[0], info[0], int(nmoved[0])
        self.pose, self.ess, self.best = est[0, :3].copy(), float(est[0, 3]), int(info[0, 0])
        self.trajectory.append(self.pose)
        return self.pose, self.ess

    def frontiers(self, radius=2, min_unknown=13, clearance=0.0, min_size=5, max_clusters=256, cap=64):
        """:meth:`Mapping.frontiers` on the best particle's map."""
        c2 = clearance_cells2(clearance, self.grid.scale, cap)
        got = grid_frontiers_host(self.grid, [max(self.best, 0)], radius=radius, min_unknown=min_unknown, min_clear2=c2, cap=cap,
                                  min_size=min_size, max_clusters=max_clusters)
        return frontier_dict(*_first(got), self.grid.scale, self.grid.off_x, self.grid.off_y)

    def view_gain(self, pose_or_poses, angle_min, angle_max, n, max_range=30.0, skip=1, return_seen=False):
        """:meth:`Mapping.view_gain` on the best particle's map."""
        p, one = _one_or_many(pose_or_poses)
        ct, st = _abi.trig_tables(angle_min, angle_max, int(n))
        return _first(grid_view_gain_host(self.grid, p, ct, st, max_range=max_range, skip=skip,
                                          grid_of_batch=[max(self.best, 0)] * p.shape[0], return_seen=return_seen), one)

    def next_goal(self, by="distance", **kw):
        """The nearest-frontier rule from the best particle's pose on its map, in a straight line or with ``by="travel"``
        by travel cost (:meth:`Mapping.next_goal`)."""
        if by == "distance":
            return nearest_goal(self.frontiers(**kw), self.best_pose)
        if by != "travel":
            raise ValueError("by must be 'distance' or 'travel'")
        foot, through = kw.pop("foot", 0), kw.pop("through_unknown", False)
        fr = self.frontiers(**kw)
        if fr["point"].shape[0] == 0 or self.best < 0:
            return None
        cap = kw.get("cap", 64)
        src = np.array([[pose_cell(self.best_pose, self.grid.scale, self.grid.off_x, self.grid.off_y)]], dtype=np.int32)
        got = grid_travel_host(self.grid, src, [self.best], goals=fr["cell"].reshape(1, -1, 2), foot=foot, through_unknown=through,
                               min_clear2=clearance_cells2(kw.get("clearance", 0.0), self.grid.scale, cap), cap=cap, cost=False)
        k = travel_goal(fr, got["goal_cost"][0])
        return None if k is None else fr["point"][k].copy()

    @property
    def best_pose(self):
        return self.particles[self.best].copy() if self.best >= 0 else np.full(3, np.nan)

    @property
    def pmap(self):
        """pmap int8 [xw, yw] of the best particle's map."""
        return self.grid.read(max(self.best, 0), want=("pmap",))["pmap"]
