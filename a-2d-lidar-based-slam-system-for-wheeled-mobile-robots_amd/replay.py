"""Batched, device-resident form of the hot path: many scans per launch.

The drop-in classes (``ICP``, ``Mapping``, ``SLAM_EKF``) process one scan per call, as the
reference's callbacks do.  The benchmark configurations of BASELINE.json batch the same
operators: a replay of L scan streams (configs[1], [3], [4]) or a particle batch
(configs[2]).  This module keeps their buffers resident in HBM (torch tensors are used
only as device allocations) and drives ``slam_replay_dev`` / ``slam_icp_batch_dev`` /
``slam_grid_update_dev`` on one stream.

The maps they write into, and every query on a map, live in ``grid.py``; the names that used to be
defined here are re-exported below.
"""
from __future__ import annotations

import numpy as np

from . import _abi
from .grid import (DeviceGrid, _batch_args, _tables, _travel_shapes, _window_ok, frontier_dict, frontier_points,  # noqa: F401
                   gain_goal, grid_copy_maps_host, grid_distance_field_host, grid_frontiers_host, grid_locate_host,
                   grid_match_host, grid_raycast_host, grid_score_host, grid_travel_host, grid_update_particles_host,
                   grid_view_gain_host, locate_pose, locate_rotations, match_pose, match_rotations, nearest_goal,
                   travel_goal, view_poses, view_tables)


def replay_host(ranges, angle_min, angle_max, grid=None, max_iter=30, tolerance=0.001, pose0=None,
                dtype="f64", grid_of_traj=None, context=None):
    """Host-pointer form (``slam_replay``): ranges float32 [L, n_scan, n] or [n_scan, n]
    -> (poses [L, n_scan-1, 3], T [L, n_scan-1, 3, 3], iters [L, n_scan-1]).  ``grid`` is a
    :class:`DeviceGrid` or ``None``."""
    ctx = context or _abi.default_context()
    r = np.ascontiguousarray(np.asarray(ranges, dtype=np.float32))
    squeeze = r.ndim == 2
    if squeeze:
        r = r[None]
    L, n_scan, n = r.shape
    ct, st = _abi.trig_tables(angle_min, angle_max, n)
    p0 = np.zeros((L, 3)) if pose0 is None else np.ascontiguousarray(np.asarray(pose0, dtype=np.float64).reshape(L, 3))
    poses = np.empty((L, n_scan - 1, 3))
    T = np.empty((L, n_scan - 1, 9))
    it = np.empty((L, n_scan - 1), dtype=np.int32)
    got = None if grid_of_traj is None else np.ascontiguousarray(np.asarray(grid_of_traj, dtype=np.int32))
    _abi.check(_abi.lib().slam_replay(ctx.handle, _abi.ptr(r), _abi.ptr(ct), _abi.ptr(st), L, n_scan, n,
                                      _abi.DTYPES[dtype], int(max_iter), float(tolerance), _abi.ptr(p0),
                                      grid._h if grid is not None else None, _abi.ptr(got), _abi.ptr(poses),
                                      _abi.ptr(T), _abi.ptr(it)))
    T = T.reshape(L, n_scan - 1, 3, 3)
    if squeeze:
        return poses[0], T[0], it[0]
    return poses, T, it


def icp_batch_host(tar, src, max_iter=30, tolerance=0.001, dtype="f64", prior=None, context=None):
    """tar [B,2,M] or [2,M] (shared), src [B,2,N] or [2,N] (shared) ->
    (T [B,3,3], iters [B], mean_err [B]).  ``prior`` [B,2,3]: per-pair affine applied to
    the source first (particle hypotheses)."""
    ctx = context or _abi.default_context()
    code = _abi.DTYPES[dtype]
    npdt = _abi.NP_DTYPES[code]
    tar = np.ascontiguousarray(np.asarray(tar, dtype=npdt))
    src = np.ascontiguousarray(np.asarray(src, dtype=npdt))
    tar_shared, src_shared = tar.ndim == 2, src.ndim == 2
    if prior is not None:
        prior = np.ascontiguousarray(np.asarray(prior, dtype=np.float64).reshape(-1, 6))
    B = (prior.shape[0] if prior is not None else 1) if (tar_shared and src_shared) else (src if tar_shared else tar).shape[0]
    T = np.empty((B, 9))
    it = np.empty(B, dtype=np.int32)
    err = np.empty(B)
    _abi.check(_abi.lib().slam_icp_batch(ctx.handle, _abi.ptr(tar), _abi.ptr(src), B, tar.shape[-1], src.shape[-1],
                                         code, int(tar_shared), int(src_shared), _abi.ptr(prior), int(max_iter),
                                         float(tolerance), _abi.ptr(T), _abi.ptr(it), _abi.ptr(err)))
    return T.reshape(B, 3, 3), it, err


def prior_matrices(priors):
    """(dx, dy, dtheta) perturbations [P,3] -> 2x3 matrices [P,2,3] (rotation by dtheta,
    then translation), the form ``slam_icp_batch`` / ``slam_particles`` take."""
    pr = np.asarray(priors, dtype=np.float64).reshape(-1, 3)
    m = np.zeros((pr.shape[0], 2, 3))
    m[:, 0, 0], m[:, 0, 1], m[:, 0, 2] = np.cos(pr[:, 2]), -np.sin(pr[:, 2]), pr[:, 0]
    m[:, 1, 0], m[:, 1, 1], m[:, 1, 2] = np.sin(pr[:, 2]), np.cos(pr[:, 2]), pr[:, 1]
    return m


def particles_host(ranges_prev, ranges_cur, angle_min, angle_max, prior_mats, pose_prev, grid=None, max_iter=30,
                   tolerance=0.001, dtype="f64", context=None):
    """P pose hypotheses of one scan pair (``slam_particles``, BASELINE.json configs[2]):
    per hypothesis an ICP solve on the prior-perturbed source, one dead-reckoning step from
    ``pose_prev[p]`` and a ray cast of the current scan into map p of ``grid`` (a
    :class:`DeviceGrid` with G >= P maps, or None).  Returns (poses [P,3], T [P,3,3], iters [P])."""
    ctx = context or _abi.default_context()
    r2 = np.ascontiguousarray(np.stack([np.asarray(ranges_prev, dtype=np.float32), np.asarray(ranges_cur, dtype=np.float32)]))
    n = r2.shape[1]
    ct, st = _abi.trig_tables(angle_min, angle_max, n)
    pm = None if prior_mats is None else np.ascontiguousarray(np.asarray(prior_mats, dtype=np.float64).reshape(-1, 6))
    pp = np.ascontiguousarray(np.asarray(pose_prev, dtype=np.float64).reshape(-1, 3))
    P = pp.shape[0]
    if pm is not None and pm.shape[0] != P:
        raise ValueError("prior_mats and pose_prev disagree on the number of hypotheses")
    poses, T, it = np.empty((P, 3)), np.empty((P, 9)), np.empty(P, dtype=np.int32)
    _abi.check(_abi.lib().slam_particles(ctx.handle, _abi.ptr(r2), _abi.ptr(ct), _abi.ptr(st), n, _abi.DTYPES[dtype],
                                         _abi.ptr(pm), _abi.ptr(pp), P, int(max_iter), float(tolerance),
                                         grid._h if grid is not None else None, _abi.ptr(poses), _abi.ptr(T), _abi.ptr(it)))
    return poses, T.reshape(P, 3, 3), it


class DeviceReplay:
    """L scan streams resident in HBM; ``run()`` enqueues one pass of the hot path
    (points -> ICP -> pose composition -> ray casting) with no host traffic.

    torch is used for allocation only; the kernels run on the context's stream, which is
    torch's current stream so torch events / synchronize see them."""

    def __init__(self, ranges, angle_min, angle_max, grid=None, max_iter=30, tolerance=0.001, dtype="f64",
                 pose0=None, grid_of_traj=None, device=0):
        import torch
        if not torch.cuda.is_available():
            raise _abi.SlamError("DeviceReplay needs a GPU (torch.cuda.is_available() is False); no CPU fallback")
        self.torch = torch
        self.dev = torch.device("cuda", device)
        torch.cuda.set_device(self.dev)
        stream = torch.cuda.current_stream(self.dev).cuda_stream
        self.ctx = _abi.Context(device, stream)
        r = np.ascontiguousarray(np.asarray(ranges, dtype=np.float32))
        if r.ndim == 2:
            r = r[None]
        self.L, self.n_scan, self.n = r.shape
        self.code = _abi.DTYPES[dtype]
        ct, st = _abi.trig_tables(angle_min, angle_max, self.n)
        self.ranges = torch.from_numpy(r).to(self.dev)
        self.cos_t = torch.from_numpy(ct).to(self.dev)
        self.sin_t = torch.from_numpy(st).to(self.dev)
        p0 = np.zeros((self.L, 3)) if pose0 is None else np.asarray(pose0, dtype=np.float64).reshape(self.L, 3)
        self.pose0 = torch.from_numpy(np.ascontiguousarray(p0)).to(self.dev)
        pairs = self.L * (self.n_scan - 1)
        self.poses = torch.empty((self.L, self.n_scan - 1, 3), dtype=torch.float64, device=self.dev)
        self.T = torch.empty((pairs, 9), dtype=torch.float64, device=self.dev)
        self.iters = torch.empty(pairs, dtype=torch.int32, device=self.dev)
        self.grid = grid
        self.got = None
        if grid_of_traj is not None:
            self.got = torch.from_numpy(np.ascontiguousarray(np.asarray(grid_of_traj, dtype=np.int32))).to(self.dev)
        self.max_iter, self.tol = int(max_iter), float(tolerance)
        torch.cuda.synchronize(self.dev)

    def make_grid(self, G, xw, yw, reso, **kw):
        self.grid = DeviceGrid.metric(G, xw, yw, reso, context=self.ctx, **kw)
        return self.grid

    def run(self, reset_grid=True, poses_out=None, T_out=None):
        """One pass.  ``poses_out`` / ``T_out``: optional float64 device tensors
        [L, n_scan-1, 3] / [L*(n_scan-1), 9] to receive the poses / transforms instead of
        ``self.poses`` / ``self.T`` (e.g. slots of a ring: with the context's "pipeline" option
        consecutive replays overlap only if they write different buffers); they become
        ``self.poses`` / ``self.T``."""
        for name, buf in (("poses", poses_out), ("T", T_out)):
            if buf is not None:
                cur = getattr(self, name)
                if tuple(buf.shape) != tuple(cur.shape) or buf.dtype != cur.dtype or not buf.is_contiguous():
                    raise ValueError("%s_out must be a contiguous float64 tensor of shape %r" % (name, tuple(cur.shape)))
                setattr(self, name, buf)
        if self.grid is not None:          # (the reset rides on the scan-matching launch: context option "replay_reset")
            want = 1 if reset_grid else 0
            # the option is the CONTEXT's: another replay on it, or its owner, may have set it since this one ran last
            if want != self.ctx.options.get("replay_reset", 0):
                self.ctx.set_option("replay_reset", want)
        _abi.check(_abi.lib().slam_replay_dev(
            self.ctx.handle, self.ranges.data_ptr(), self.cos_t.data_ptr(), self.sin_t.data_ptr(), self.L, self.n_scan,
            self.n, self.code, self.max_iter, self.tol, self.pose0.data_ptr(),
            self.grid._h if self.grid is not None else None, self.got.data_ptr() if self.got is not None else None,
            None, self.poses.data_ptr(), self.T.data_ptr(), self.iters.data_ptr()))

    @property
    def scans_per_run(self):
        return self.L * (self.n_scan - 1)

    def results(self):
        self.ctx.check_status()
        return (self.poses.cpu().numpy(), self.T.cpu().numpy().reshape(self.L, self.n_scan - 1, 3, 3),
                self.iters.cpu().numpy().reshape(self.L, self.n_scan - 1))
