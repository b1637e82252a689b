"""Batched, device-resident form of the whole W12 node: landmark extraction,
the landmark EKF and the map cast from its ``xEst`` for many trajectories per call.

``SLAM_EKF(landmarks=True)`` runs the node one scan per call with ``Extraction`` and ``EKF`` on
the host between two device calls.  Here the same chain - W12m/slam_ekf.py:63-95 with
extraction.py:24-89 and ekf_lm.py:15-50 - runs over ``ranges [L, n_scan, n]`` of already-decimated
scans: ``slam_landmarks`` (one workgroup per scan), the kept-scan rule (a scan without a landmark
is dropped before the odometry, so the scan matcher's target does not advance), the scan matcher
on (previous kept, current kept), ``slam_ekf_lm`` (one wave per trajectory) and the ray cast of
every kept scan from its ``xEst``.  ``landmarks_host`` and ``ekf_lm_host`` are the two new
operators on their own.
"""
from __future__ import annotations

import numpy as np

from . import _abi
from .param import get_param
from .grid import DeviceGrid

NODE_OK, NODE_REF_RAISES, NODE_LM_CAP, NODE_OBS_CAP = _abi.NODE_OK, _abi.NODE_REF_RAISES, _abi.NODE_LM_CAP, _abi.NODE_OBS_CAP


def _thresholds(range_threshold, radius_max_th):
    if range_threshold is None:
        range_threshold = get_param('/extraction/range_threshold', 1.0)    # extraction.py:19
    if radius_max_th is None:
        radius_max_th = get_param('/extraction/radius_max_th', 0.3)        # extraction.py:21
    return float(range_threshold), float(radius_max_th)


def landmarks_host(ranges, angle_min, angle_max, lm_cap=8, range_threshold=None, radius_max_th=None, labels=False,
                   context=None):
    """``Extraction.process`` + ``SLAM_EKF.observation`` for S scans (``slam_landmarks``): ranges float32
    [S, n] or [n] -> dict with ``count`` [S], ``overflow`` [S], ``ids`` [S, lm_cap] (-1 unused),
    ``means`` [S, lm_cap, 2], ``z`` [S, lm_cap, 2] and, with ``labels=True``, ``labels`` [S, n-1]."""
    ctx = context or _abi.default_context()
    r = np.ascontiguousarray(np.asarray(ranges, dtype=np.float32))
    if r.ndim == 1:
        r = r[None]
    S, n = r.shape
    rt, rm = _thresholds(range_threshold, radius_max_th)
    ct, st = _abi.trig_tables(angle_min, angle_max, n)
    out = {"count": np.empty(S, dtype=np.int32), "overflow": np.empty(S, dtype=np.int32),
           "ids": np.empty((S, lm_cap), dtype=np.int32), "means": np.empty((S, lm_cap, 2)), "z": np.empty((S, lm_cap, 2))}
    if labels:
        out["labels"] = np.empty((S, max(n - 1, 0)), dtype=np.int32)
    _abi.check(_abi.lib().slam_landmarks(ctx.handle, _abi.ptr(r), _abi.ptr(ct), _abi.ptr(st), S, n, rt, rm, int(lm_cap),
                                         _abi.ptr(out["count"]), _abi.ptr(out["overflow"]), _abi.ptr(out["ids"]),
                                         _abi.ptr(out["means"]), _abi.ptr(out["z"]), _abi.ptr(out.get("labels"))))
    return out


def ekf_lm_host(u, z, x0=None, max_lm=16, context=None):
    """``EKF.estimate`` along B trajectories (``slam_ekf_lm``).  ``u``: one array [steps, 3] per trajectory (or
    one [B, steps, 3] array); ``z``: per trajectory a list with one [m, 2+] array of (range, bearing) rows per
    step.  Trajectories may differ in length.  Returns dict with ``x`` [B, N], ``P`` [B, N, N] (N = 3 + 2
    max_lm, zero beyond the state), ``nlm`` [B, steps] (-1: step not run) and ``status`` [B]."""
    ctx = context or _abi.default_context()
    us = [np.asarray(v, dtype=np.float64).reshape(-1, 3) for v in u]
    B = len(us)
    counts = np.array([v.shape[0] for v in us], dtype=np.int32)
    steps = max(1, int(counts.max()) if B else 1)
    ub = np.zeros((B, steps, 3))
    off = np.zeros(B * steps + 1, dtype=np.int64)
    rows = []
    total = 0
    for b in range(B):
        ub[b, :counts[b]] = us[b]
        if len(z[b]) != counts[b]:
            raise ValueError("trajectory %d: %d steps of u, %d of z" % (b, counts[b], len(z[b])))
        for s in range(steps):
            if s < counts[b]:
                zs = np.asarray(z[b][s], dtype=np.float64)
                zs = zs[:, :2] if zs.ndim == 2 and zs.size else np.zeros((0, 2))
                rows.append(zs)
                total += zs.shape[0]
            off[b * steps + s + 1] = total
    zz = np.ascontiguousarray(np.concatenate(rows)) if total else np.zeros((0, 2))
    p0 = None if x0 is None else np.ascontiguousarray(np.asarray(x0, dtype=np.float64).reshape(B, 3))
    N = 3 + 2 * int(max_lm)
    out = {"x": np.empty((B, N)), "P": np.empty((B, N, N)), "nlm": np.empty((B, steps), dtype=np.int32),
           "status": np.empty(B, dtype=np.int32)}
    _abi.check(_abi.lib().slam_ekf_lm(ctx.handle, _abi.ptr(p0), _abi.ptr(ub), _abi.ptr(counts), _abi.ptr(off),
                                      _abi.ptr(zz) if total else None, total, B, steps, int(max_lm), _abi.ptr(out["x"]),
                                      _abi.ptr(out["P"]), _abi.ptr(out["nlm"]), _abi.ptr(out["status"])))
    return out


def node_replay_host(ranges, angle_min, angle_max, grid=None, grid_of_traj=None, pose0=None, max_lm=16, lm_cap=8,
                     max_iter=None, tolerance=None, dtype="f64", range_threshold=None, radius_max_th=None, context=None):
    """Host-pointer form of the node (``slam_node_replay``): ranges float32 [L, n_scan, n] or [n_scan, n] ->
    the dict :meth:`DeviceNodeReplay.results` returns."""
    ctx = context or _abi.default_context()
    r = np.ascontiguousarray(np.asarray(ranges, dtype=np.float32))
    if r.ndim == 2:
        r = r[None]
    L, n_scan, n = r.shape
    rt, rm = _thresholds(range_threshold, radius_max_th)
    max_iter = get_param('/icp/max_iter', 30) if max_iter is None else max_iter
    tolerance = get_param('/icp/tolerance', 0.001) if tolerance is None else tolerance
    ct, st = _abi.trig_tables(angle_min, angle_max, n)
    p0 = np.zeros((L, 3)) if pose0 is None else np.ascontiguousarray(np.asarray(pose0, dtype=np.float64).reshape(L, 3))
    got = None if grid_of_traj is None else np.ascontiguousarray(np.asarray(grid_of_traj, dtype=np.int32))
    N = 3 + 2 * int(max_lm)
    o = {"kept": np.empty((L, n_scan), dtype=np.int32), "kept_count": np.empty(L, dtype=np.int32),
         "xest": np.empty((L, n_scan - 1, 3)), "nlm": np.empty((L, n_scan - 1), dtype=np.int32), "x": np.empty((L, N)),
         "P": np.empty((L, N, N)), "T": np.empty((L, n_scan - 1, 9)), "iters": np.empty((L, n_scan - 1), dtype=np.int32),
         "status": np.empty(L, dtype=np.int32)}
    _abi.check(_abi.lib().slam_node_replay(
        ctx.handle, _abi.ptr(r), _abi.ptr(ct), _abi.ptr(st), L, n_scan, n, _abi.DTYPES[dtype], int(max_iter), float(tolerance),
        rt, rm, int(lm_cap), int(max_lm), _abi.ptr(p0), grid._h if grid is not None else None, _abi.ptr(got),
        _abi.ptr(o["kept"]), _abi.ptr(o["kept_count"]), _abi.ptr(o["xest"]), _abi.ptr(o["nlm"]), _abi.ptr(o["x"]),
        _abi.ptr(o["P"]), _abi.ptr(o["T"]), _abi.ptr(o["iters"]), _abi.ptr(o["status"])))
    o["T"] = o["T"].reshape(L, n_scan - 1, 3, 3)
    return o


class DeviceNodeReplay:
    """L scan streams resident in HBM; ``run()`` enqueues the whole node for all of them
    (extraction -> kept scans -> scan matching -> landmark EKF -> ray cast from xEst) with no host
    traffic and no synchronisation.  torch is used for allocation only, as in ``DeviceReplay``."""

    def __init__(self, ranges, angle_min, angle_max, grid_of_traj=None, max_lm=16, lm_cap=8, grid=None, max_iter=None,
                 tolerance=None, dtype="f64", pose0=None, range_threshold=None, radius_max_th=None, device=0):
        import torch
        if not torch.cuda.is_available():
            raise _abi.SlamError("DeviceNodeReplay needs a GPU (torch.cuda.is_available() is False); no CPU fallback")
        self.torch = torch
        self.dev = torch.device("cuda", device)
        torch.cuda.set_device(self.dev)
        self.ctx = _abi.Context(device, torch.cuda.current_stream(self.dev).cuda_stream)
        r = np.ascontiguousarray(np.asarray(ranges, dtype=np.float32))
        if r.ndim == 2:
            r = r[None]
        self.L, self.n_scan, self.n = r.shape
        self.code = _abi.DTYPES[dtype]
        self.max_lm, self.lm_cap = int(max_lm), int(lm_cap)
        self.rt, self.rm = _thresholds(range_threshold, radius_max_th)
        self.max_iter = int(get_param('/icp/max_iter', 30) if max_iter is None else max_iter)
        self.tol = float(get_param('/icp/tolerance', 0.001) if tolerance is None else tolerance)
        ct, st = _abi.trig_tables(angle_min, angle_max, self.n)
        self.ranges = torch.from_numpy(r).to(self.dev)
        self.cos_t = torch.from_numpy(ct).to(self.dev)
        self.sin_t = torch.from_numpy(st).to(self.dev)
        p0 = np.zeros((self.L, 3)) if pose0 is None else np.asarray(pose0, dtype=np.float64).reshape(self.L, 3)
        self.pose0 = torch.from_numpy(np.ascontiguousarray(p0)).to(self.dev)
        L, K, N = self.L, self.n_scan - 1, 3 + 2 * self.max_lm
        f64, i32 = torch.float64, torch.int32
        self.kept = torch.empty((L, self.n_scan), dtype=i32, device=self.dev)
        self.kept_count = torch.empty(L, dtype=i32, device=self.dev)
        self.xest = torch.empty((L, K, 3), dtype=f64, device=self.dev)
        self.nlm = torch.empty((L, K), dtype=i32, device=self.dev)
        self.x = torch.empty((L, N), dtype=f64, device=self.dev)
        self.P = torch.empty((L, N, N), dtype=f64, device=self.dev)
        self.T = torch.empty((L, K, 9), dtype=f64, device=self.dev)
        self.iters = torch.empty((L, K), dtype=i32, device=self.dev)
        self.status = torch.empty(L, dtype=i32, device=self.dev)
        self.grid = grid
        self.got = None
        if grid_of_traj is not None:
            self.got = torch.from_numpy(np.ascontiguousarray(np.asarray(grid_of_traj, dtype=np.int32))).to(self.dev)
        torch.cuda.synchronize(self.dev)

    def make_grid(self, G, xw, yw, reso, **kw):
        self.grid = DeviceGrid.metric(G, xw, yw, reso, context=self.ctx, **kw)
        return self.grid

    def run(self, reset_grid=True):
        """One pass over every trajectory; the maps start from zero unless ``reset_grid`` is false."""
        if self.grid is not None and reset_grid:
            self.grid.reset()
        _abi.check(_abi.lib().slam_node_replay_dev(
            self.ctx.handle, self.ranges.data_ptr(), self.cos_t.data_ptr(), self.sin_t.data_ptr(), self.L, self.n_scan,
            self.n, self.code, self.max_iter, self.tol, self.rt, self.rm, self.lm_cap, self.max_lm, self.pose0.data_ptr(),
            self.grid._h if self.grid is not None else None, self.got.data_ptr() if self.got is not None else None,
            self.kept.data_ptr(), self.kept_count.data_ptr(), self.xest.data_ptr(), self.nlm.data_ptr(), self.x.data_ptr(),
            self.P.data_ptr(), self.T.data_ptr(), self.iters.data_ptr(), self.status.data_ptr()))

    @property
    def scans_per_run(self):
        return self.L * self.n_scan

    def results(self):
        """dict: ``kept`` [L, n_scan] (-1 behind the kept scans), ``kept_count`` [L]; per step ``xest`` [L, n_scan-1, 3]
        (NaN: step not run), ``nlm`` (-1 likewise), ``T`` [L, n_scan-1, 3, 3], ``iters``; final ``x`` [L, N],
        ``P`` [L, N, N]; ``status`` [L] (``NODE_*``)."""
        self.ctx.check_status()
        o = {k: getattr(self, k).cpu().numpy() for k in ("kept", "kept_count", "xest", "nlm", "x", "P", "T", "iters", "status")}
        o["T"] = o["T"].reshape(self.L, self.n_scan - 1, 3, 3)
        return o
