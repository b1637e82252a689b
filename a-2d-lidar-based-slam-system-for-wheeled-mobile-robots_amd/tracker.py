"""The scan-to-map tracker (``slam_track``, include/slam_track.h): every scan is matched against the map as it stands
(``slam_grid_match``'s rule), refined below the cell (``slam_grid_refine``'s) and, behind a keyframe gate, integrated
into the map (``slam_grid_update_particles``'s) - S scans of L trajectories in one call, a map per trajectory.

    track_host(...)   NumPy arrays in and out (the host form)
    DeviceTracker     torch tensors resident on the device, no synchronise (the device form)
    ScanTracker       one trajectory on a :class:`Mapping`, one scan per ``update``, in the idiom of ``MCL.update``

The defaults - 11 rotations of 0.01 rad, a 9 x 9 window of one cell, 10 refinement iterations with damping 0.01 and
steps of 0.5 cell / 0.02 rad, cap 64, ``min_used`` 1 and a gate of (0.2 m, 0.1 rad) - are those of ONE experiment
(a 40-scan synthetic run on a 400 x 400 map of 0.05 m), not the result of tuning."""
from __future__ import annotations

import numpy as np

from . import _abi

DEFAULTS = dict(n_rot=11, rot_step=0.01, nx=4, ny=4, step=None, iters=10, damping=0.01, step_cells=0.5, step_rad=0.02,
                max_range=30.0, cap=64, min_used=1, gate_dist=0.2, gate_turn=0.1)


def track_rotations(n_rot=11, rot_step=0.01):
    """(rot_off [K], rot_off_cs [K, 2]) of the tracker's rotations: offsets (k - n_rot // 2) * rot_step from the predicted
    heading, with their cosines and sines by NumPy.  The library forms the table of a scan from these and from the cosine
    and sine of the predicted heading by the angle-sum identities."""
    off = (np.arange(int(n_rot)) - int(n_rot) // 2) * float(rot_step)
    return np.ascontiguousarray(off), np.ascontiguousarray(np.stack([np.cos(off), np.sin(off)], axis=-1))


def new_state(poses):
    """The state [L, 8] of trajectories that start at ``poses`` [L, 3] with nothing integrated yet (keyed = 0)."""
    p = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    st = np.zeros((p.shape[0], _abi.TRACK_STATE_LEN), dtype=np.float64)
    st[:, :3] = p
    return st


def _params(grid, kw):
    p = dict(DEFAULTS)
    unknown = set(kw) - set(p)
    if unknown:
        raise TypeError("unknown tracker parameter(s): %s" % ", ".join(sorted(unknown)))
    p.update(kw)
    if p["step"] is None:
        p["step"] = 1.0 / grid.scale                 # a window of one cell
    return p


def _call(fn, grid, ranges, motion, L, S, cos_t, sin_t, n, rot_off, rot_off_cs, p, map0, state, poses, info, trace):
    _abi.check(fn(grid._ctx.handle, grid._h, _abi.ptr(ranges), _abi.ptr(motion), int(L), int(S), _abi.ptr(cos_t), _abi.ptr(sin_t),
                  int(n), _abi.ptr(rot_off), _abi.ptr(rot_off_cs), int(rot_off.shape[0]), int(p["nx"]), int(p["ny"]), float(p["step"]),
                  int(p["iters"]), float(p["damping"]), float(p["step_cells"]), float(p["step_rad"]), float(p["max_range"]),
                  int(p["cap"]), int(p["min_used"]), float(p["gate_dist"]), float(p["gate_turn"]), int(map0), _abi.ptr(state),
                  _abi.ptr(poses), _abi.ptr(info), _abi.ptr(trace)))


def track_host(grid, ranges, state, cos_t, sin_t, motion=None, map0=0, rot_off=None, rot_off_cs=None, return_trace=False, **kw):
    """``slam_track`` on NumPy arrays: ranges float32 [L, S, n], state float64 [L, 8] (:func:`new_state`), motion float64
    [L, S, 3] or None, the beam tables [n].  Trajectory l tracks in, and integrates into, map ``map0 + l`` of ``grid``.
    ``rot_off`` / ``rot_off_cs``: the rotation offsets and their cosines and sines (default :func:`track_rotations` of
    ``n_rot``, ``rot_step``); the other keywords are those of ``DEFAULTS``.  Returns (state [L, 8] after the call, poses
    [L, S, 3], info int32 [L, S, 4] = (best, best cost, used, flags ``_abi.TRACK_*``)) and with ``return_trace`` also
    trace float64 [L, S, 13]."""
    p = _params(grid, kw)
    r = np.ascontiguousarray(np.asarray(ranges, dtype=np.float32))
    if r.ndim != 3:
        raise ValueError("ranges must be [L, S, n]")
    L, S, n = r.shape
    ct = np.ascontiguousarray(np.asarray(cos_t, dtype=np.float64).reshape(-1))
    st = np.ascontiguousarray(np.asarray(sin_t, dtype=np.float64).reshape(-1))
    if ct.shape[0] != n or st.shape[0] != n:
        raise ValueError("cos_t and sin_t must be [n]")
    m = None if motion is None else np.ascontiguousarray(np.asarray(motion, dtype=np.float64).reshape(L, S, 3))
    if rot_off is None:
        rot_off, rot_off_cs = track_rotations(p["n_rot"], p["rot_step"])
    ro = np.ascontiguousarray(np.asarray(rot_off, dtype=np.float64).reshape(-1))
    rc = np.ascontiguousarray(np.asarray(rot_off_cs, dtype=np.float64).reshape(ro.shape[0], 2))
    state = np.array(np.asarray(state, dtype=np.float64).reshape(L, _abi.TRACK_STATE_LEN), order="C")
    poses = np.empty((L, S, 3), dtype=np.float64)
    info = np.empty((L, S, _abi.TRACK_INFO_LEN), dtype=np.int32)
    trace = np.empty((L, S, _abi.TRACK_TRACE_LEN), dtype=np.float64) if return_trace else None
    _call(_abi.lib().slam_track, grid, r, m, L, S, ct, st, n, ro, rc, p, map0, state, poses, info, trace)
    return (state, poses, info, trace) if return_trace else (state, poses, info)


class DeviceTracker:
    """L trajectories tracked on the device, on the context of ``grid`` (a :class:`DeviceGrid`); trajectory l owns map
    ``map0 + l``.  Beams: ``cos_t`` / ``sin_t`` [n] (NumPy).  The keywords are those of ``DEFAULTS`` (see the module's
    note on where they come from); ``rot_off`` / ``rot_off_cs`` replace the default rotations.

    torch allocates; the kernels run on the context's stream, ordered against torch's current stream without a host
    synchronise (``slam_stream_order``).  The tensors given to :meth:`run` / :meth:`step` are kept until the next call
    has ordered torch's stream behind the kernels that read them, as :class:`DeviceMCL` keeps its inputs."""

    def __init__(self, grid, L, cos_t, sin_t, map0=0, rot_off=None, rot_off_cs=None, trace=True, **kw):
        import torch
        if not torch.cuda.is_available():
            raise _abi.SlamError("DeviceTracker needs a GPU (torch.cuda.is_available() is False); no CPU fallback")
        self.torch, self.grid, self.ctx = torch, grid, grid._ctx
        self.dev = torch.device("cuda", self.ctx.device)
        self.L, self.map0 = int(L), int(map0)
        self.p = _params(grid, kw)
        if rot_off is None:
            rot_off, rot_off_cs = track_rotations(self.p["n_rot"], self.p["rot_step"])
        up = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).to(self.dev)
        self.cos_t, self.sin_t = up(cos_t).reshape(-1), up(sin_t).reshape(-1)
        self.n = int(self.cos_t.shape[0])
        self.rot_off, self.rot_off_cs = up(rot_off).reshape(-1), up(rot_off_cs).reshape(-1, 2)
        self.state = torch.zeros((self.L, _abi.TRACK_STATE_LEN), dtype=torch.float64, device=self.dev)
        self.want_trace = bool(trace)
        self.poses = self.info = self.trace = None
        self._held = None
        torch.cuda.synchronize(self.dev)

    def _torch_stream(self):
        return self.torch.cuda.current_stream(self.dev).cuda_stream

    def _begin(self):
        self.ctx.stream_order(self._torch_stream(), 0)      # torch waits for the kernels enqueued so far, then lets their inputs go
        self._held = None

    def __del__(self):
        try:
            if self._held is not None and self.ctx._h is not None:
                self._begin()
        except Exception:
            pass

    def set_poses(self, poses, key=None, keyed=False):
        """Start (or restart) every trajectory at ``poses`` [L, 3] (NumPy or torch).  ``keyed=False``: nothing is integrated
        yet, so the first scan is placed at the prediction and integrated.  ``keyed=True``: the map is given (tracking
        in a prebuilt map); ``key`` [L, 3] is the key pose the gate measures from (default: ``poses``)."""
        torch = self.torch
        self._begin()
        as_t = lambda a: a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))
        self.state.zero_()
        self.state[:, 0:3] = as_t(poses).reshape(self.L, 3).to(self.dev)
        if keyed:
            self.state[:, 3:6] = self.state[:, 0:3] if key is None else as_t(key).reshape(self.L, 3).to(self.dev)
            self.state[:, 6] = 1.0

    def _check(self, name, t, shape, dtype):
        if not self.torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous():
            raise ValueError("%s must be a contiguous %s device tensor of shape %r" % (name, dtype, shape))

    def run(self, ranges, motion=None):
        """S scans: ranges float32 [L, S, n], motion float64 [L, S, 3] or None (device tensors).  Enqueues the whole loop
        (``slam_track_dev``); ``poses`` [L, S, 3], ``info`` [L, S, 4] and ``trace`` [L, S, 13] hold its outputs and
        ``state`` the state after it.  No synchronise."""
        torch = self.torch
        self._begin()
        S = int(ranges.shape[1]) if ranges.dim() == 3 else -1
        self._check("ranges", ranges, (self.L, S, self.n), torch.float32)
        if motion is not None:
            self._check("motion", motion, (self.L, S, 3), torch.float64)
        new = lambda dt, k: torch.empty((self.L, S, k), dtype=dt, device=self.dev)
        self.poses, self.info = new(torch.float64, 3), new(torch.int32, _abi.TRACK_INFO_LEN)
        self.trace = new(torch.float64, _abi.TRACK_TRACE_LEN) if self.want_trace else None
        self.ctx.stream_order(self._torch_stream(), 1)            # the kernels wait for what torch has made so far
        _call(_abi.lib().slam_track_dev, self.grid, ranges, motion, self.L, S, self.cos_t, self.sin_t, self.n, self.rot_off,
              self.rot_off_cs, self.p, self.map0, self.state, self.poses, self.info, self.trace)
        self._held = (ranges, motion)

    def step(self, ranges, motion=None):
        """One scan: ranges float32 [L, n], motion float64 [L, 3] or None; :meth:`run` with S = 1."""
        self.run(ranges.reshape(self.L, 1, self.n), None if motion is None else motion.reshape(self.L, 1, 3))

    @property
    def trajectory(self):
        """The poses of the scans of the last :meth:`run` / :meth:`step`: a device tensor [L, S, 3] (no synchronise)."""
        return self.poses

    def results(self):
        """Synchronises and returns a dict of NumPy arrays: poses, info, trace (None without it) and state."""
        self.ctx.synchronize()
        get = lambda t: None if t is None else t.cpu().numpy()
        return dict(poses=get(self.poses), info=get(self.info), trace=get(self.trace), state=get(self.state))


class ScanTracker:
    """One trajectory on a :class:`Mapping`, NumPy in and out: ``update`` places a scan in the map and, behind the
    keyframe gate, integrates it.  ``pose``: where the trajectory starts.  ``keyed=True`` tracks in the map as it is
    given (with ``gate_dist = gate_turn = inf`` it is never changed); otherwise the first scan is integrated at
    ``pose`` (+) its ``u``.  The keywords are those of ``DEFAULTS`` (see the module's note on where they come from)."""

    def __init__(self, mapping, pose=(0.0, 0.0, 0.0), keyed=False, **kw):
        self.mapping = mapping
        self.kw = kw
        self.state = new_state(np.asarray(pose, dtype=np.float64).reshape(1, 3))
        if keyed:
            self.state[0, 3:6] = self.state[0, 0:3]
            self.state[0, 6] = 1.0
        self.pose, self.info = self.state[0, :3].copy(), None
        self.trajectory = []

    def update(self, scan, angle_min, angle_max, u=None):
        """One scan: ``u`` the odometry step (dx, dy, dtheta) in the robot frame since the last scan, or None.
        Returns (pose [3], info): info a dict of best, cost, used and the flags matched, refined, integrated, lost."""
        r = np.ascontiguousarray(np.asarray(scan, dtype=np.float32).reshape(1, 1, -1))
        ct, st = _abi.trig_tables(angle_min, angle_max, r.shape[2])
        motion = None if u is None else np.asarray(u, dtype=np.float64).reshape(1, 1, 3)
        try:
            self.state, poses, info = track_host(self.mapping.grid, r, self.state, ct, st, motion=motion, **self.kw)
        finally:
            self.mapping._datamap_stale = True
        best, cost, used, flags = (int(v) for v in info[0, 0])
        self.pose = poses[0, 0].copy()
        self.info = dict(best=best, cost=cost, used=used, matched=bool(flags & _abi.TRACK_MATCHED),
                         refined=bool(flags & _abi.TRACK_REFINED), integrated=bool(flags & _abi.TRACK_INTEGRATED),
                         lost=bool(flags & _abi.TRACK_LOST))
        self.trajectory.append(self.pose)
        if flags & _abi.TRACK_INTEGRATED:
            self.mapping._fetch_pmap()
        return self.pose, self.info
