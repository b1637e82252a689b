"""Batched, device-resident form of the whole W9 node (fusion localization): the scan-to-map
observation, the two odometry solves and the 3x3 pose filter for many trajectories per call.

``Localization.laserCallback`` runs the node one processed scan per call, with three host round
trips and a NumPy filter in between, for one robot.  Here the same chain - W9/localization.py:66-126
with laserEstimation (:128-150), laserToNumpy (:170-176), calc_odometry (:159-168) and EKF.estimate
(W9/ekf.py:17-87) - runs for L trajectories in lockstep (``slam_loc_replay``): trajectory l replays
stream ``stream_of_traj[l]`` of ``ranges [S, n_scan, n]`` against map ``map_of_traj[l]`` from
``pose0[l]``.  That is global localization from hundreds of start-pose hypotheses of one recorded
stream, or many recorded streams against their maps.  Every scan of a stream is one PROCESSED
scan (the node's every-6th-message rule is applied by whoever records the stream).
"""
from __future__ import annotations

import numpy as np

from . import _abi
from .param import get_param

LOC_OK, LOC_NONFINITE, LOC_BAD_ROUTE = _abi.LOC_OK, _abi.LOC_NONFINITE, _abi.LOC_BAD_ROUTE


def _streams(ranges):
    r = np.ascontiguousarray(np.asarray(ranges, dtype=np.float32))
    if r.ndim == 2:
        r = r[None]
    if r.ndim != 3:
        raise ValueError("ranges must be [S, n_scan, n] or [n_scan, n], got shape %r" % (r.shape,))
    return r


def _maps(obstacles):
    """One 2xK array or a list of them -> (ox [K], oy [K], obs_off [M + 1] int64) over one concatenated list."""
    if isinstance(obstacles, np.ndarray) and obstacles.ndim == 2:
        obstacles = [obstacles]
    maps = [np.asarray(o, dtype=np.float64).reshape(2, -1) for o in obstacles]
    if not maps:
        raise ValueError("need at least one obstacle list (it may be empty: a 2x0 array)")
    off = np.zeros(len(maps) + 1, dtype=np.int64)
    off[1:] = np.cumsum([m.shape[1] for m in maps])
    cat = np.concatenate(maps, axis=1)
    return np.ascontiguousarray(cat[0]), np.ascontiguousarray(cat[1]), off


def _routes(L, S, stream_of_traj, map_of_traj):
    sot = None if stream_of_traj is None else np.ascontiguousarray(np.asarray(stream_of_traj, dtype=np.int32).reshape(-1))
    mot = None if map_of_traj is None else np.ascontiguousarray(np.asarray(map_of_traj, dtype=np.int32).reshape(-1))
    for name, a in (("stream_of_traj", sot), ("map_of_traj", mot)):
        if a is not None and a.shape[0] != L:
            raise ValueError("%s has %d entries for %d trajectories" % (name, a.shape[0], L))
    return sot, mot


def _count(S, pose0, stream_of_traj, map_of_traj):
    """Number of trajectories: the length of whichever per-trajectory argument is given, else one per stream."""
    if pose0 is not None:
        return int(np.asarray(pose0).reshape(-1, 3).shape[0])
    for a in (stream_of_traj, map_of_traj):
        if a is not None:
            return int(np.asarray(a).reshape(-1).shape[0])
    return S


def _increment(angle_min, angle_max, n, angle_increment):
    if angle_increment is not None:
        return float(angle_increment)
    return (float(angle_max) - float(angle_min)) / (n - 1) if n > 1 else 1.0


def _shape_results(o, L, n_scan, n):
    o["P"] = o["P"].reshape(L, 3, 3)
    o["T_obs"] = o["T_obs"].reshape(L, n_scan, 3, 3)
    o["T_odom"] = o["T_odom"].reshape(L, n_scan, 3, 3)
    if "tar_pts" in o:
        o["tar_pts"] = o["tar_pts"].reshape(L, n_scan, 2, n)
    return o


def loc_replay_host(ranges, angle_min, angle_max, obstacles, pose0=None, stream_of_traj=None, map_of_traj=None,
                    max_iter=None, tolerance=None, angle_increment=None, target_points=False, context=None):
    """Host-pointer form of the node (``slam_loc_replay``): ranges float32 [S, n_scan, n] or [n_scan, n],
    ``obstacles`` a 2xK array or a list of them -> the dict :meth:`DeviceLocalizationReplay.results` returns;
    with ``target_points=True`` also ``tar_pts`` [L, n_scan, 2, n], the virtual scan's points of every step."""
    ctx = context or _abi.default_context()
    r = _streams(ranges)
    S, n_scan, n = r.shape
    L = _count(S, pose0, stream_of_traj, map_of_traj)
    ox, oy, off = _maps(obstacles)
    sot, mot = _routes(L, S, stream_of_traj, map_of_traj)
    p0 = None if pose0 is None else np.ascontiguousarray(np.asarray(pose0, dtype=np.float64).reshape(L, 3))
    max_iter = get_param('/icp/max_iter', 30) if max_iter is None else max_iter
    tolerance = get_param('/icp/tolerance', 0.001) if tolerance is None else tolerance
    ct, st = _abi.trig_tables(angle_min, angle_max, n)
    o = {"xest": np.empty((L, n_scan, 3)), "xodom": np.empty((L, n_scan, 3)), "P": np.empty((L, 9)),
         "status": np.empty(L, dtype=np.int32), "T_obs": np.empty((L, n_scan, 9)),
         "iters_obs": np.empty((L, n_scan), dtype=np.int32), "T_odom": np.empty((L, n_scan, 9))}
    if target_points:
        o["tar_pts"] = np.empty((L, n_scan, 2 * n))
    _abi.check(_abi.lib().slam_loc_replay(
        ctx.handle, _abi.ptr(r), S, n_scan, n, _abi.ptr(sot), _abi.ptr(ox), _abi.ptr(oy), _abi.ptr(off), off.shape[0] - 1,
        _abi.ptr(mot), _abi.ptr(p0), L, _abi.ptr(ct), _abi.ptr(st), float(angle_min),
        _increment(angle_min, angle_max, n, angle_increment), int(max_iter), float(tolerance), _abi.ptr(o["xest"]),
        _abi.ptr(o["xodom"]), _abi.ptr(o["P"]), _abi.ptr(o["status"]), _abi.ptr(o["T_obs"]), _abi.ptr(o["iters_obs"]),
        _abi.ptr(o["T_odom"]), _abi.ptr(o.get("tar_pts"))))
    return _shape_results(o, L, n_scan, n)


class DeviceLocalizationReplay:
    """Streams, maps and start poses resident in HBM; ``run()`` enqueues the whole node for every trajectory
    (two launches per step, no host traffic, no synchronisation).  torch is used for allocation only, as in
    ``DeviceReplay``.  Pass a ``context`` to share one stream and workspace between several replays."""

    def __init__(self, ranges_f32, angle_min, angle_max, obstacles, pose0=None, stream_of_traj=None, map_of_traj=None,
                 context=None, max_iter=None, tolerance=None, angle_increment=None, device=0):
        import torch
        if not torch.cuda.is_available():
            raise _abi.SlamError("DeviceLocalizationReplay needs a GPU (torch.cuda.is_available() is False); no CPU fallback")
        self.torch = torch
        self.dev = torch.device("cuda", context.device if context is not None else device)
        torch.cuda.set_device(self.dev)
        self.ctx = context or _abi.Context(self.dev.index, torch.cuda.current_stream(self.dev).cuda_stream)
        r = _streams(ranges_f32)
        self.S, self.n_scan, self.n = r.shape
        self.L = _count(self.S, pose0, stream_of_traj, map_of_traj)
        if stream_of_traj is None and self.S != self.L:
            raise ValueError("%d streams for %d trajectories: pass stream_of_traj" % (self.S, self.L))
        ox, oy, off = _maps(obstacles)
        self.M, self.K = off.shape[0] - 1, int(off[-1])
        sot, mot = _routes(self.L, self.S, stream_of_traj, map_of_traj)
        for name, a, hi in (("stream_of_traj", sot, self.S), ("map_of_traj", mot, self.M)):
            if a is not None and a.size and (a.min() < 0 or a.max() >= hi):
                raise ValueError("%s out of range" % name)
        self.max_iter = int(get_param('/icp/max_iter', 30) if max_iter is None else max_iter)
        self.tol = float(get_param('/icp/tolerance', 0.001) if tolerance is None else tolerance)
        self.angle_min = float(angle_min)
        self.angle_increment = _increment(angle_min, angle_max, self.n, angle_increment)
        ct, st = _abi.trig_tables(angle_min, angle_max, self.n)
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.ranges, self.cos_t, self.sin_t = up(r), up(ct), up(st)
        self.ox, self.oy, self.obs_off = up(ox), up(oy), up(off)
        self.sot, self.mot = up(sot), up(mot)
        self.pose0 = None if pose0 is None else up(np.asarray(pose0, dtype=np.float64).reshape(self.L, 3))
        L, K = self.L, self.n_scan
        f64, i32 = torch.float64, torch.int32
        self.xest = torch.empty((L, K, 3), dtype=f64, device=self.dev)
        self.xodom = torch.empty((L, K, 3), dtype=f64, device=self.dev)
        self.P = torch.empty((L, 9), dtype=f64, device=self.dev)
        self.status = torch.empty(L, dtype=i32, device=self.dev)
        self.T_obs = torch.empty((L, K, 9), dtype=f64, device=self.dev)
        self.iters_obs = torch.empty((L, K), dtype=i32, device=self.dev)
        self.T_odom = torch.empty((L, K, 9), dtype=f64, device=self.dev)
        torch.cuda.synchronize(self.dev)

    @classmethod
    def from_localization(cls, loc, ranges_f32, angle_min, angle_max, **kw):
        """The obstacle list of a :class:`Localization` after ``updateMap`` (``loc.obstacle``, 2xK)."""
        return cls(ranges_f32, angle_min, angle_max, np.asarray(loc.obstacle, dtype=np.float64), **kw)

    def run(self):
        """One pass over every trajectory, enqueued on the context's stream."""
        p = lambda t: None if t is None else t.data_ptr()
        _abi.check(_abi.lib().slam_loc_replay_dev(
            self.ctx.handle, p(self.ranges), self.S, self.n_scan, self.n, p(self.sot), p(self.ox), p(self.oy),
            p(self.obs_off), self.M, self.K, p(self.mot), p(self.pose0), self.L, p(self.cos_t), p(self.sin_t),
            self.angle_min, self.angle_increment, self.max_iter, self.tol, p(self.xest), p(self.xodom), p(self.P),
            p(self.status), p(self.T_obs), p(self.iters_obs), p(self.T_odom), None))

    @property
    def steps_per_run(self):
        return self.L * self.n_scan

    def results(self):
        """dict: per step ``xest`` / ``xodom`` [L, n_scan, 3], ``T_obs`` / ``T_odom`` [L, n_scan, 3, 3] (map
        observation, first odometry transform), ``iters_obs`` [L, n_scan]; final ``P`` [L, 3, 3]; ``status`` [L]
        (``LOC_*``).  From the step at which a trajectory stops its per-step entries are NaN / -1."""
        self.ctx.check_status()
        o = {k: getattr(self, k).cpu().numpy() for k in ("xest", "xodom", "P", "status", "T_obs", "iters_obs", "T_odom")}
        return _shape_results(o, self.L, self.n_scan, self.n)
