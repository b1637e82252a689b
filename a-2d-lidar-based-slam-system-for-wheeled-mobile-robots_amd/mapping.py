"""``Mapping`` occupancy-grid accumulator on the GPU.

Mirrors W12m/mapping.py:8-51: ``Mapping(xw, yw, xyreso)`` holds ``pmap`` (50 = unknown,
0 = free, 100 = occupied) and ``datamap``; ``update(ox, oy, center_x, center_y)`` casts one
ray per beam from the centre to each world-frame endpoint and returns the live ``pmap``.
The rays are walked by libslamhip's ray-cast kernels (float-error Bresenham, integer
pass / hit counters; ``plan_cast`` picks which) through ``slam_grid_update``; ``pmap``
comes from ``slam_grid_read``.

Fidelity notes:
* the reference converts world coordinates with ``int(10 * (x + 10))`` whatever ``xyreso``
  is (mapping.py:33-36).  That is the default here; pass ``index_scale`` / ``index_offset``
  (or use :meth:`Mapping.metric`) for grids of another resolution such as 400x400 @ 0.05 m.
* ``datamap`` is rebuilt as ``0.01*pass + 20*hit`` from the counters; it equals the
  reference's running float sum to ~1e-12, ``pmap`` is exact.
* ``hit_inc=4`` gives the w12-mapping-online variant (W12o/mapping.py:46).  There the
  reference's own ``pmap`` depends on the order in which a cell's +4 and +0.01 arrived when
  the pass count sits exactly on a threshold (e.g. 2 hits + 200 passes: 8 + 200 x 0.01 is
  occupied if the passes came first, free if the hits did); the device applies the
  hits-first order (include/slam_hip.h, slam_grid_create).
* NaN coordinates raise ``ValueError`` and infinite ``oy`` / centre raise ``OverflowError``
  as ``int()`` does in the reference.  The reference stops at the offending beam (earlier
  beams are already in the map, later ones are not); so does ``update``.  A cell index
  beyond 2^20 also raises ``OverflowError`` (the reference would walk that ray for hours).
"""
from __future__ import annotations

import numpy as np

from . import _abi
from .grid import (DeviceGrid, _first, _one_or_many, clearance_cells2, frontier_dict, frontier_points, gain_goal,
                   grid_distance_field_host, grid_frontiers_host, grid_locate_host, grid_match_host, grid_raycast_host,
                   grid_refine_host, grid_score_host, grid_travel_host, grid_view_gain_host, locate_pose, locate_rotations,
                   match_pose, match_rotations, nearest_goal, pose_cell, refine_normal, travel_goal, view_poses, view_tables)


class Mapping:
    def __init__(self, xw, yw, xyreso, index_scale=10.0, index_offset=10.0, index_offset_y=None,
                 free_inc=0.01, hit_inc=20.0, thresh=10.0, context=None):
        self.width_x = xw * xyreso
        self.width_y = yw * xyreso
        self.xyreso = xyreso
        self.xw = int(xw)
        self.yw = int(yw)
        self.pmap = 50 * np.ones((self.xw, self.yw))   # default 50: unknown (mapping.py:14)
        self._datamap = np.zeros((self.xw, self.yw))   # mapping.py:15, fetched on demand (see ``datamap``)
        self._datamap_stale = False
        self.minx = -self.width_x / 2.0
        self.maxx = self.width_x / 2.0
        self.miny = -self.width_y / 2.0
        self.maxy = self.width_y / 2.0
        self.index_scale = float(index_scale)
        self.index_offset_x = float(index_offset)
        self.index_offset_y = float(index_offset if index_offset_y is None else index_offset_y)
        self.grid = DeviceGrid(1, self.xw, self.yw, self.index_scale, self.index_offset_x, self.index_offset_y, free_inc, hit_inc,
                               thresh, context)
        self._ctx = self.grid._ctx
        self._p8 = np.empty((self.xw, self.yw), dtype=np.int8)
        self.grid.live_pmap()       # one scan per call owns the map: the ray cast keeps pmap current on the device itself

    @property
    def _grid(self):
        """The map's raw handle, ``grid._h``, under the name callers outside the package knew it by."""
        return self.grid._h

    @property
    def datamap(self):
        """The evidence map of mapping.py:15 (float64 [xw, yw]).  ``update`` only brings ``pmap``
        back from the device; this view (8 bytes per cell) is read when it is asked for."""
        if self._datamap_stale:
            _abi.check(_abi.lib().slam_grid_read(self._ctx.handle, self.grid._h, 0, None, _abi.ptr(self._datamap), None, None))
            self._datamap_stale = False
        return self._datamap

    def _fetch_pmap(self):
        _abi.check(_abi.lib().slam_grid_read(self._ctx.handle, self.grid._h, 0, _abi.ptr(self._p8), None, None, None))
        self.pmap[...] = self._p8
        self._datamap_stale = True
        return self.pmap

    @classmethod
    def metric(cls, xw, yw, xyreso, **kw):
        """Grid whose index rule follows its resolution: scale = 1/xyreso, offsets = half
        the map width (the reference's rule is the xyreso = 0.1, 20 m special case)."""
        scale = round(1.0 / xyreso) if abs(round(1.0 / xyreso) - 1.0 / xyreso) < 1e-9 else 1.0 / xyreso
        return cls(xw, yw, xyreso, index_scale=scale, index_offset=xw / (2.0 * scale),
                   index_offset_y=yw / (2.0 * scale), **kw)

    def __del__(self):
        try:
            self.grid.close()
        except Exception:
            pass

    def update(self, ox, oy, center_x, center_y):
        ox = np.ascontiguousarray(np.asarray(ox, dtype=np.float64).reshape(-1))
        oy = np.ascontiguousarray(np.asarray(oy, dtype=np.float64).reshape(-1))
        n = len(ox)
        if len(oy) < n:
            raise IndexError("oy is shorter than ox")
        if n == 0:
            return self.pmap
        cx = np.array([float(np.asarray(center_x).reshape(-1)[0])])
        cy = np.array([float(np.asarray(center_y).reshape(-1)[0])])
        L = _abi.lib()
        try:
            _abi.check(L.slam_grid_update(self._ctx.handle, self.grid._h, _abi.ptr(ox), _abi.ptr(oy), _abi.ptr(cx),
                                          _abi.ptr(cy), 1, n, None))
        finally:
            self._datamap_stale = True            # on a NaN / inf beam the beams before it were still applied
        return self._fetch_pmap()

    def update_scans(self, ranges, angle_min, angle_max, poses, centres=None):
        """S raw scans at once (``slam_grid_update_scans``): ranges [S, n] (inf -> 30 m), poses
        [S, 3] the xEst each scan is transformed with (W12m/slam_ekf.py:89), centres [S, 2] the
        ray origins (default: the pose; w12-mapping-online passes the /tf position,
        W12o/slam_ekf.py:104).  Returns the live ``pmap``."""
        r = np.ascontiguousarray(np.asarray(ranges, dtype=np.float32))
        if r.ndim == 1:
            r = r[None]
        S, n = r.shape
        p = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(S, 3))
        c = None if centres is None else np.ascontiguousarray(np.asarray(centres, dtype=np.float64).reshape(S, 2))
        ct, st = _abi.trig_tables(angle_min, angle_max, n)
        L = _abi.lib()
        try:
            _abi.check(L.slam_grid_update_scans(self._ctx.handle, self.grid._h, _abi.ptr(r), _abi.ptr(ct), _abi.ptr(st),
                                                _abi.ptr(p), _abi.ptr(c), S, n))
        finally:
            self._datamap_stale = True
        return self._fetch_pmap()

    def raycast(self, pose, angle_min, angle_max, n, max_range=30.0, skip=1, return_cells=False):
        """The scan this map would give from ``pose`` (x, y, theta): ``n`` beams of ``linspace(angle_min, angle_max,
        n)`` cast to ``max_range`` along the lines ``update`` walks (``slam_grid_raycast``).  Returns ranges float32
        [n] to the centre of the first occupied cell from path index ``skip`` on (1: not the robot's own cell) -
        inf where the ray meets none, NaN for a pose the reference's ``int()`` would raise on - and with
        ``return_cells`` also the cells int32 [n, 2], (-1, -1) where there is none."""
        p = np.asarray(pose, dtype=np.float64).reshape(3)
        ct, st = _abi.trig_tables(angle_min, angle_max, int(n))
        return _first(grid_raycast_host(self.grid, p, ct, st, max_range=max_range, skip=skip, return_cells=return_cells))

    def score_scan(self, ranges, angle_min, angle_max, pose, skip=1):
        """How a measured scan sits in this map seen from ``pose`` (``slam_grid_scan_score``): the seven counts
        int32 [7], indexed by ``_abi.RAY_EMPTY .. RAY_BAD``, of beams formed as ``update_scans`` forms them."""
        r = np.asarray(ranges, dtype=np.float32).reshape(-1)
        p = np.asarray(pose, dtype=np.float64).reshape(3)
        ct, st = _abi.trig_tables(angle_min, angle_max, r.shape[0])
        return _first(grid_score_host(self.grid, r, p, ct, st, skip=skip))

    def distance_field(self, cap=64):
        """The distance field of this map (``slam_grid_distance_field``): int16 [xw, yw], the squared cell distance
        to the nearest occupied cell, capped at ``cap`` (1 .. 32767); ``cap`` everywhere while nothing is occupied.
        Rebuilt from the live counters on every call."""
        return _first(grid_distance_field_host(self.grid, cap))

    def refine_scan(self, ranges, angle_min, angle_max, pose, iters=10, damping=1e-3, max_step=(0.5, 0.02), max_range=30.0, cap=64,
                    return_normal=False):
        """``pose`` (x, y, theta) moved below the cell to where the scan fits this map (``slam_grid_refine``): ``iters``
        damped Gauss-Newton steps on the smooth distance field, each clamped to ``max_step`` = (cells in x and y, radians).
        The cost is the sum over the used beams of the squared interpolated distance, in cells.  Returns (pose [3], cost,
        used beams) and with ``return_normal`` also H [3, 3] and g [3] of the fit at the returned pose: the information
        matrix of the scan-to-map constraint, up to the measurement variance, and its gradient.  The device rule has no
        decisions; THIS method adds one on the host: when the end costs more than the start, the start pose and its cost
        (and, with ``return_normal``, its H and g, from a call of no iterations) are returned.  A pose the call cannot
        answer (status 1) comes back unchanged with cost -1."""
        r = np.asarray(ranges, dtype=np.float32).reshape(-1)
        p = np.asarray(pose, dtype=np.float64).reshape(3)
        ct, st = _abi.trig_tables(angle_min, angle_max, r.shape[0])
        kw = dict(damping=damping, step_cells=max_step[0], step_rad=max_step[1], max_range=max_range, cap=cap, return_normal=return_normal)
        got = _first(grid_refine_host(self.grid, r, p, ct, st, iters=iters, **kw))
        if got[1][1] > got[1][0]:                   # the end costs more: keep the start
            got = _first(grid_refine_host(self.grid, r, p, ct, st, iters=0, **kw)) if return_normal else (p.copy(), got[1][[0, 0]], got[2])
        out = (got[0], float(got[1][1]), int(got[2]))
        return out + refine_normal(got[4]) if return_normal else out

    def match_scan(self, ranges, angle_min, angle_max, pose, window=(4, 4), step=None, n_rot=11, rot_step=0.01,
                   max_range=30.0, cap=64, return_costs=False, refine=0):
        """Where a measured scan fits this map best near ``pose`` (x, y, theta) (``slam_grid_match``): every pose of
        the window - ``n_rot`` rotations theta + (k - n_rot // 2) * rot_step, (2 window[0] + 1) x (2 window[1] + 1)
        translations of ``step`` (default: one cell, 1 / index_scale) - costs the sum over the beams shorter than
        ``max_range`` of the distance-field value at the beam's end cell (``cap`` off the map).  Returns (pose [3],
        cost, used beams) of the cheapest candidate, ties to the lowest (rotation, x, y) index, and with
        ``return_costs`` also the cost volume int32 [n_rot, 2 window[0] + 1, 2 window[1] + 1].  ``refine`` = k > 0: the
        winner is then moved below the cell by :meth:`refine_scan` with k iterations at the same ``max_range`` and
        ``cap``, and (pose, cost, used) are that call's - the cost a float, in squared cells of the smooth field; a
        window without a winner is returned as it is.  ``refine`` = 0: nothing but the window match."""
        r = np.asarray(ranges, dtype=np.float32).reshape(-1)
        p = np.asarray(pose, dtype=np.float64).reshape(3)
        nx, ny = int(window[0]), int(window[1])
        step = 1.0 / self.index_scale if step is None else float(step)
        ct, st = _abi.trig_tables(angle_min, angle_max, r.shape[0])
        th, rot = match_rotations(p[2:3], n_rot, rot_step)
        got = _first(grid_match_host(self.grid, r, p[None, :2], ct, st, rot, nx, ny, step, max_range=max_range, cap=cap,
                                     return_costs=return_costs))
        out = (match_pose(p[None, :2], th, got[0], nx, ny, step)[0], int(got[1]), int(got[2]))
        if int(refine) > 0 and got[0] >= 0:
            out = self.refine_scan(r, angle_min, angle_max, out[0], iters=int(refine), max_range=max_range, cap=cap)
        return out + got[3:]

    def locate_scan(self, ranges, angle_min, angle_max, n_rot=256, levels=5, region=None, max_range=30.0, cap=64):
        """Where in this map a measured scan was taken (``slam_grid_locate``): the cheapest of ``n_rot`` rotations over the
        full circle x every cell of the map - or of ``region`` = (i0, j0, ni, nj) - as the robot's cell, found exactly by
        branch and bound on a ``levels``-deep pyramid of the distance field.  Returns (pose [3] at the cell's centre,
        cost, used beams)."""
        r = np.asarray(ranges, dtype=np.float32).reshape(-1)
        ct, st = _abi.trig_tables(angle_min, angle_max, r.shape[0])
        _, rot = locate_rotations(n_rot)
        reg = None if region is None else np.asarray(region, dtype=np.int32).reshape(1, 4)
        best, cost, used = grid_locate_host(self.grid, r, ct, st, rot, levels=levels, region=reg, max_range=max_range, cap=cap, B=1)
        pose = locate_pose(best, self.index_scale, self.index_offset_x, self.index_offset_y, rot)[0]
        return pose, int(cost[0]), int(used[0])

    def frontiers(self, radius=2, min_unknown=13, clearance=0.0, min_size=5, max_clusters=256, cap=64):
        """Where to go next to see more of this map (``slam_grid_frontiers``): the free cells that border unknown space
        with at least ``min_unknown`` unknown cells in their (2 radius + 1)^2 window and at least ``clearance`` metres
        from every occupied cell (``min_clear2 = ceil((clearance * scale)^2)``, an error when it exceeds ``cap``), in
        8-connected clusters of at least ``min_size`` cells.  Returns a dict of arrays over the kept clusters, in label
        order: ``label``, ``size``, ``cell`` [K, 2] (the representative, a member cell), ``point`` [K, 2] (its centre in
        world coordinates), ``centroid`` [K, 2] (world, from the sums), ``bbox`` [K, 4]; and ``count`` (the true number
        of kept clusters, also beyond ``max_clusters``) and ``n_frontier``.  The defaults (2, 13, 5) come from one
        experiment on the synthetic room; they are not tuned."""
        c2 = clearance_cells2(clearance, self.index_scale, cap)
        got = grid_frontiers_host(self.grid, radius=radius, min_unknown=min_unknown, min_clear2=c2, cap=cap, min_size=min_size,
                                  max_clusters=max_clusters)
        return frontier_dict(*_first(got), self.index_scale, self.index_offset_x, self.index_offset_y)

    def next_goal(self, pose, by="distance", **kw):
        """``by="distance"``, the nearest-frontier rule: the representative point [2] of the kept cluster
        (:meth:`frontiers`, ``**kw``) whose point is nearest to the pose's (x, y); None when no cluster is kept -
        exploration is complete.  ``by="travel"``: the representative of the kept cluster with the smallest travel cost
        >= 0 from the pose's cell (:meth:`travel_field`), ties to the lowest label; None when no kept cluster is
        reachable - exploration is complete for this robot, even if frontiers exist behind walls.  ``foot``,
        ``through_unknown`` and ``clearance`` are taken from ``kw``; the clearance is shared with the frontier call.
        ``by="gain"``, next-best-view: among the kept clusters with travel cost c >= 0 and u > 0 unknown cells in view
        from their representative's cell centre (heading 0, the ``n`` beams (default 360) of :func:`view_tables` over the
        full circle to ``max_range`` (default 30 m)), the one with the largest u / (c + ``bias``), compared exactly as
        integers (:func:`gain_goal`), ties to the lower cost, then to the lower label; None when there is none.
        ``bias`` (default 100) is in travel-cost units; it is a starting value, not a tuned one."""
        if by == "distance":
            return nearest_goal(self.frontiers(**kw), pose)
        if by == "gain":
            return self._gain_goal(pose, **kw)
        if by != "travel":
            raise ValueError("by must be 'distance', 'travel' or 'gain'")
        foot, through = kw.pop("foot", 0), kw.pop("through_unknown", False)
        fr = self.frontiers(**kw)
        if fr["point"].shape[0] == 0:
            return None
        got = self._travel(pose, kw.get("clearance", 0.0), foot, through, kw.get("cap", 64), goals=fr["cell"], cost=False)
        k = travel_goal(fr, got["goal_cost"][0])
        return None if k is None else fr["point"][k].copy()

    def _gain_goal(self, pose, bias=100, n=360, max_range=30.0, skip=1, **kw):
        foot, through = kw.pop("foot", 0), kw.pop("through_unknown", False)
        fr = self.frontiers(**kw)
        if fr["point"].shape[0] == 0:
            return None
        got = self._travel(pose, kw.get("clearance", 0.0), foot, through, kw.get("cap", 64), goals=fr["cell"], cost=False)
        views = view_poses(fr["cell"], self.index_scale, self.index_offset_x, self.index_offset_y)
        counts = grid_view_gain_host(self.grid, views, *view_tables(n), max_range=max_range, skip=skip)
        k = gain_goal(fr, got["goal_cost"][0], counts[:, _abi.VIEW_UNKNOWN], bias)
        return None if k is None else fr["point"][k].copy()

    def view_gain(self, pose_or_poses, angle_min, angle_max, n, max_range=30.0, skip=1, return_seen=False):
        """What a scan from a pose would reveal of this map (``slam_grid_view_gain``): ``n`` beams of
        ``linspace(angle_min, angle_max, n)`` cast to ``max_range`` as :meth:`raycast` casts them, and the SET of map cells
        they see - path indices ``skip`` up to and including each beam's first occupied cell, or to its end - counted:
        int32 [4] = (unknown, free, occupied cells, beams that found nothing) (``_abi.VIEW_*``), a row of -1 for a pose
        the index rule rejects.  poses [B, 3] give [B, 4].  With ``return_seen`` also the set as bit words uint32
        [xw, ceil(yw / 32)] ([B, ...]): bit ``y & 31`` of word ``y >> 5`` in row x."""
        p, one = _one_or_many(pose_or_poses)
        ct, st = _abi.trig_tables(angle_min, angle_max, int(n))
        return _first(grid_view_gain_host(self.grid, p, ct, st, max_range=max_range, skip=skip, return_seen=return_seen), one)

    def pose_cell(self, pose):
        """The cell (x, y) of a pose by the map's own rule, ``int(scale * (v + off))``, truncated toward zero."""
        return pose_cell(pose, self.index_scale, self.index_offset_x, self.index_offset_y)

    def _travel(self, pose, clearance, foot, through_unknown, cap, goals=None, path_cap=0, cost=True):
        c2 = clearance_cells2(clearance, self.index_scale, cap)
        src = np.array([[self.pose_cell(pose)]], dtype=np.int32)
        gl = None if goals is None else np.asarray(goals, dtype=np.int32).reshape(1, -1, 2)
        return grid_travel_host(self.grid, src, goals=gl, foot=foot, through_unknown=through_unknown, min_clear2=c2, cap=cap,
                                path_cap=path_cap, cost=cost)

    def travel_field(self, pose, clearance=0.0, foot=0, through_unknown=False, cap=64):
        """What it costs to drive from the pose's cell (:meth:`pose_cell`) to every cell (``slam_grid_travel``): int32
        [xw, yw], 10 a straight move and 14 a diagonal one, no corner cutting, -1 where the robot cannot go.  Free cells
        are travelable, unknown ones with ``through_unknown``, both only ``clearance`` metres from every occupied cell
        (``min_clear2 = ceil((clearance * scale)^2)``, an error beyond ``cap``); the cells within ``foot`` of the robot
        are, whatever the map says."""
        return self._travel(pose, clearance, foot, through_unknown, cap)["cost"][0]

    def travel_path(self, pose, goal_xy, clearance=0.0, foot=0, through_unknown=False, cap=64, path_cap=256):
        """The cheapest way from the pose to the cell of the world point ``goal_xy``: (points float64 [len, 2] - the cell
        centres (:func:`frontier_points`), the robot's cell first - and the cost), or None when the goal is unreachable.
        ``path_cap`` is grown and the call repeated when the path is longer."""
        goal = self.pose_cell(goal_xy)
        while True:
            got = self._travel(pose, clearance, foot, through_unknown, cap, goals=[goal], path_cap=path_cap, cost=False)
            n = int(got["path_len"][0, 0])
            if n == 0:
                return None
            if n <= int(path_cap):
                cells = got["path"][0, 0, :n]
                return frontier_points(cells, self.index_scale, self.index_offset_x, self.index_offset_y), int(got["goal_cost"][0, 0])
            path_cap = n

    def counters(self):
        """(pass, hit) uint32 [xw, yw]: the integer evidence behind ``datamap``."""
        got = self.grid.read(0, want=("pass", "hit"))
        return got["pass"], got["hit"]

    def occupancy_grid_data(self):
        """int8 [yw*xw] in the OccupancyGrid layout of publishMap
        (W12m/slam_ekf.py:270-271): data[y*width + x] = pmap[x][y]."""
        return self.grid.occupancy_grid_data(0)

    def visits(self):
        return self.grid.visits()
