"""Drop-in for the reference's DWA local planner (course_agv_nav/scripts/dwa.py), scored on
the GPU (slam_dwa in include/slam_hip.h), plus its batched forms.

    from dwa import *            ->   from <package>.dwa import *

``RobotType``, ``Config`` and ``calc_dynamic_window`` are the reference's host code restated
(dwa.py:18-55, :65-83); ``dwa_control`` scores every sample of the window in one launch and
returns what the reference returns: ``(u, trajectory)`` with u = [v, omega] and the winning
trajectory, (rows x 5) - 21 x 5 by default - or the state alone (1 x 5) when no sample wins.
The rectangle collision test is the reference's as it executes: axis-aligned in the planning
frame (include/slam_hip.h).  There is no CPU implementation of the scoring.
"""
from __future__ import annotations

import ctypes as C
import math
from enum import Enum

import numpy as np

from . import _abi
from ._abi import check, ptr

CONFIG_FIELDS = ("max_speed", "min_speed", "max_yawrate", "max_accel", "max_dyawrate", "dt", "v_reso", "yawrate_reso",
                 "predict_time", "to_goal_cost_gain", "speed_cost_gain", "obstacle_cost_gain", "robot_type",
                 "robot_radius", "robot_width", "robot_length")


class RobotType(Enum):
    circle = 0
    rectangle = 1


class Config:
    """dwa.py:22-55: the same attributes and defaults; v_reso / yawrate_reso are derived once,
    at construction, from max_accel, max_dyawrate and dt, as in the reference."""

    def __init__(self):
        self.max_speed = 0.8
        self.min_speed = -0.5
        self.max_yawrate = 100.0 * math.pi / 180.0
        self.max_accel = 1
        self.max_dyawrate = 100.0 * math.pi / 180.0
        self.dt = 0.1
        self.v_reso = self.max_accel * self.dt / 10.0
        self.yawrate_reso = self.max_dyawrate * self.dt / 10.0
        self.predict_time = 2
        self.to_goal_cost_gain = 1.0
        self.speed_cost_gain = 0.1
        self.obstacle_cost_gain = 1.0
        self.robot_type = RobotType.rectangle
        self.robot_radius = 0.4
        self.robot_width = 0.3
        self.robot_length = 0.6

    @property
    def robot_type(self):
        return self._robot_type

    @robot_type.setter
    def robot_type(self, value):
        if not isinstance(value, RobotType):
            raise TypeError("robot_type must be an instance of RobotType")
        self._robot_type = value


def config_array(config):
    """The double[SLAM_DWA_CONFIG_LEN] of a Config (or of a dict with the same keys)."""
    get = config.get if isinstance(config, dict) else (lambda k: getattr(config, k))
    out = []
    for f in CONFIG_FIELDS:
        v = get(f)
        out.append(float(v.value if isinstance(v, RobotType) else v))
    return np.array(out, dtype=np.float64)


def shape(config):
    """(rows, nv_cap, nw_cap) of a config: trajectory rows and the bounds of the two sample axes
    (slam_dwa_shape).  Raises SlamError for a config the reference could not run."""
    rows, nv, nw = C.c_int(), C.c_int(), C.c_int()
    check(_abi.lib().slam_dwa_shape(ptr(config_array(config)), C.byref(rows), C.byref(nv), C.byref(nw)))
    return rows.value, nv.value, nw.value


def calc_dynamic_window(x, config):
    """dwa.py:65-83 (host glue)."""
    Vs = [config.min_speed, config.max_speed, -config.max_yawrate, config.max_yawrate]
    Vd = [x[3] - config.max_accel * config.dt, x[3] + config.max_accel * config.dt,
          x[4] - config.max_dyawrate * config.dt, x[4] + config.max_dyawrate * config.dt]
    return [max(Vs[0], Vd[0]), min(Vs[1], Vd[1]), max(Vs[2], Vd[2]), min(Vs[3], Vd[3])]


def _f64(a, shape_=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a if shape_ is None else a.reshape(shape_)


def dwa_batch_host(states, goals, config, ob=None, counts=None, shared=False, scans=None, angle_min=None,
                   angle_increment=None, threshold=None, want_costs=False, want_traj=False, ctx=None):
    """B planners through slam_dwa / slam_dwa_scans from host arrays.

    states [B][5], goals [B][2].  Obstacles either ``ob`` [B][M][2] (or [M][2] with shared=True)
    with optional ``counts`` [B] (or [1]), or ``scans`` float32 [B][n] (or [n] shared) with the
    beam angles angle_min + angle_increment * i and ``threshold`` (default max_speed *
    predict_time, local_planner.py:34).  Returns a dict: u [B][2], cost [B], index [B],
    counts [B][2] (nv, nw), and when asked costs [B][nv_cap * nw_cap], traj [B][rows][5]."""
    c = ctx or _abi.default_context()
    cfg = config_array(config)
    rows, nvc, nwc = shape(config)
    states = _f64(states, (-1, 5))
    B = states.shape[0]
    goals = _f64(goals, (B, 2))
    s_cap = max(nvc * nwc, 1)
    out = dict(u=np.empty((B, 2)), cost=np.empty(B), index=np.empty(B, np.int32), counts=np.empty((B, 2), np.int32))
    if want_costs:
        out["costs"] = np.full((B, s_cap), np.nan)
    if want_traj:
        out["traj"] = np.empty((B, rows, 5))
    tail = (ptr(out["u"]), ptr(out["cost"]), ptr(out["index"]), ptr(out["counts"]), ptr(out.get("costs")), s_cap,
            ptr(out.get("traj")))
    L = _abi.lib()
    if scans is not None:
        r = np.ascontiguousarray(scans, dtype=np.float32)
        n = r.shape[-1]
        ct, st = _abi.beam_tables(angle_min, angle_increment, n)
        thr = float(config_array(config)[0] * config_array(config)[8]) if threshold is None else float(threshold)
        check(L.slam_dwa_scans(c.handle, ptr(states), ptr(goals), ptr(r), n, int(bool(shared)), ptr(ct), ptr(st), thr,
                               ptr(cfg), B, *tail))
    else:
        o = _f64(ob)
        M = o.shape[-2]
        soa = np.ascontiguousarray(np.swapaxes(o.reshape(-1, M, 2), 1, 2))      # [.][2][M]
        k = None if counts is None else np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
        check(L.slam_dwa(c.handle, ptr(states), ptr(goals), ptr(soa), ptr(k), M, int(bool(shared)), ptr(cfg), B, *tail))
    return out


def dwa_control(x, config, goal, ob, ctx=None):
    """dwa.py:10-16 on the device: (u, trajectory) exactly shaped as the reference's."""
    r = dwa_batch_host(np.asarray(x, dtype=np.float64)[None], np.asarray(goal, dtype=np.float64)[None], config,
                       ob=np.asarray(ob, dtype=np.float64).reshape(1, -1, 2), want_traj=True, ctx=ctx)
    if r["index"][0] < 0:
        return [0.0, 0.0], np.array([np.asarray(x, dtype=np.float64)])
    return [float(r["u"][0, 0]), float(r["u"][0, 1])], r["traj"][0]


class DeviceDWA:
    """Batched DWA on device-resident tensors (torch tensors on the context's device, passed by
    data_ptr(); outputs allocated here as torch tensors).  One call = one launch, no host
    synchronise: slam_dwa_dev / slam_dwa_scans_dev on the context's stream."""

    def __init__(self, config, device=0, ctx=None):
        import torch
        self.ctx = ctx or _abi.default_context(device)
        self.cfg = config_array(config)
        self.rows, self.nv_cap, self.nw_cap = shape(config)
        self.threshold = float(self.cfg[0] * self.cfg[8])
        self.dev = torch.device("cuda", self.ctx.device)
        self._tables = {}

    def _outputs(self, B, want_costs, want_traj):
        import torch
        s_cap = max(self.nv_cap * self.nw_cap, 1)
        f = dict(dtype=torch.float64, device=self.dev)
        out = dict(u=torch.empty((B, 2), **f), cost=torch.empty(B, **f),
                   index=torch.empty(B, dtype=torch.int32, device=self.dev),
                   counts=torch.empty((B, 2), dtype=torch.int32, device=self.dev))
        if want_costs:
            out["costs"] = torch.full((B, s_cap), float("nan"), **f)
        if want_traj:
            out["traj"] = torch.empty((B, self.rows, 5), **f)
        return out, (ptr(out["u"]), ptr(out["cost"]), ptr(out["index"]), ptr(out["counts"]), ptr(out.get("costs")),
                     s_cap, ptr(out.get("traj")))

    def tables(self, angle_min, angle_increment, n):
        import torch
        key = (float(angle_min), float(angle_increment), int(n))
        t = self._tables.get(key)
        if t is None:
            ct, st = _abi.beam_tables(angle_min, angle_increment, n)
            t = self._tables[key] = (torch.from_numpy(ct).to(self.dev), torch.from_numpy(st).to(self.dev))
        return t

    def run(self, states, goals, ob=None, counts=None, shared=False, want_costs=False, want_traj=False):
        """states [B][5], goals [B][2] float64; ob [B][2][M] (or [2][M] shared) float64 device
        tensors in the ABI's x-row-then-y-row layout; counts int32 [B] (or [1]) or None."""
        B = int(states.shape[0])
        M = int(ob.shape[-1])
        out, tail = self._outputs(B, want_costs, want_traj)
        check(_abi.lib().slam_dwa_dev(self.ctx.handle, ptr(states), ptr(goals), ptr(ob), ptr(counts), M,
                                      int(bool(shared)), ptr(self.cfg), B, *tail))
        return out

    def run_scans(self, states, goals, ranges, angle_min, angle_increment, shared=False, threshold=None,
                  want_costs=False, want_traj=False):
        """ranges float32 [B][n] (or [n] shared) device tensor; obstacles formed in the launch as
        LocalPlanner.laserCallback forms them."""
        B = int(states.shape[0])
        n = int(ranges.shape[-1])
        ct, st = self.tables(angle_min, angle_increment, n)
        out, tail = self._outputs(B, want_costs, want_traj)
        thr = self.threshold if threshold is None else float(threshold)
        check(_abi.lib().slam_dwa_scans_dev(self.ctx.handle, ptr(states), ptr(goals), ptr(ranges), n,
                                            int(bool(shared)), ptr(ct), ptr(st), thr, ptr(self.cfg), B, *tail))
        return out
