"""The A* global planner (course_agv_nav/scripts/global_planner.py) on the GPU (slam_astar).

    find_path(map, start, goal).start_find()   drop-in (:133-238): the reference's return values
                                               and in-place mutations
    GlobalPlanner                              the node without ROS (:14-121), in the style of
                                               LocalPlanner: topics become calls
    astar_host / inflate_host                  B queries over G host maps in one call
    DeviceAStar                                B queries on device tensors; from_grid() plans on a
                                               DeviceGrid's live pmap with no host round trip

Semantics are the reference's as it executes, quirks included: the
inflation is its in-place greedy loop over rows / columns [r, span - r) (129 and 2 in the
reference; a SLAM map of 400 x 400 needs span = min(H, W) to be inflated at all), the start and
goal are shifted by -1, the heuristic overestimates, and world points use swapped origins plus
a constant 0.25.
"""
from __future__ import annotations

import numpy as np

from . import _abi
from ._abi import check, ptr

OK, INVALID_START, INVALID_GOAL, NO_PATH, EDGE, TRUNCATED, BAD_MAP = range(7)
STATUS_NAMES = ("OK", "INVALID_START", "INVALID_GOAL", "NO_PATH", "EDGE", "TRUNCATED", "BAD_MAP")
SPAN, R = 129, 2          # start_find's hard-coded bound and inflation radius (:149-150)


def _maps3(maps, wire_layout):
    m = np.asarray(maps)
    if m.dtype != np.int8:
        m = m.astype(np.int64)
        if m.size and (m.min() < -128 or m.max() > 127):
            raise ValueError("map values must fit int8")
        m = m.astype(np.int8)
    m = np.ascontiguousarray(m)
    if m.ndim == 2:
        m = m[None]
    G, a, b = m.shape
    H, W = (a, b) if wire_layout else (b, a)
    return m, G, H, W


def inflate_host(maps, span=SPAN, r=R, wire_layout=True, ctx=None):
    """start_find's inflation (:148-155) of G maps: int8 [G][H][W] row-major (a 2-D map gives [H][W])."""
    m, G, H, W = _maps3(maps, wire_layout)
    out = np.empty((G, H, W), np.int8)
    c = ctx or _abi.default_context()
    check(_abi.lib().slam_astar_inflate(c.handle, ptr(m), G, H, W, int(bool(wire_layout)), int(span), int(r), ptr(out)))
    return out if np.asarray(maps).ndim == 3 else out[0]


def astar_host(maps, starts, goals, map_of_query=None, span=SPAN, r=R, wire_layout=True, path_cap=1024,
               want_inflated=False, ctx=None):
    """B queries over G maps (slam_astar).  maps: [G][H][W] wire layout (or [G][W][H] pmap layout
    with wire_layout=False), a 2-D map for G = 1; starts / goals [B][2] (row, col) as find_path
    receives them.  Returns dict(status [B], path_len [B], path [B][path_cap][2] start -> goal,
    expansions [B], inflated [G][H][W] when asked)."""
    m, G, H, W = _maps3(maps, wire_layout)
    s = np.ascontiguousarray(np.asarray(starts, dtype=np.int32).reshape(-1, 2))
    g = np.ascontiguousarray(np.asarray(goals, dtype=np.int32).reshape(-1, 2))
    B = s.shape[0]
    q = None if map_of_query is None else np.ascontiguousarray(np.asarray(map_of_query, dtype=np.int32).reshape(B))
    out = dict(status=np.empty(B, np.int32), path_len=np.empty(B, np.int32),
               path=np.full((B, path_cap, 2), -1, np.int32), expansions=np.empty(B, np.int32))
    if want_inflated:
        out["inflated"] = np.empty((G, H, W), np.int8)
    c = ctx or _abi.default_context()
    check(_abi.lib().slam_astar(c.handle, ptr(m), G, H, W, int(bool(wire_layout)), int(span), int(r), ptr(s), ptr(g),
                                ptr(q), B, int(path_cap), ptr(out["status"]), ptr(out["path_len"]),
                                ptr(out["path"]) if path_cap > 0 else None, ptr(out["expansions"]),
                                ptr(out.get("inflated"))))
    return out


def plan_one(map_rows, start, goal, span=SPAN, r=R, ctx=None):
    """One query on a row-major map: (status, path [L][2] start -> goal, expansions, inflated map).
    The path buffer holds every cell of the map up to 2^16 cells, so the call is repeated (with the
    reported length as the capacity) only for a path longer than that."""
    cap = min(int(np.asarray(map_rows).size), 1 << 16)
    while True:
        o = astar_host(map_rows, [start], [goal], span=span, r=r, path_cap=cap, want_inflated=True, ctx=ctx)
        st, L = int(o["status"][0]), int(o["path_len"][0])
        if st != TRUNCATED:
            return st, o["path"][0, :L].copy(), int(o["expansions"][0]), o["inflated"][0]
        cap = L


class find_path:
    """Drop-in for find_path (:133-238).  The constructor shifts start and goal by -1 in place, as
    the reference does; start_find() inflates `map` in place and returns the path as a list of
    [row, col] from the goal to the start, "None" for a start or goal that is not free after
    inflation, and raises IndexError where the reference does (an unreachable goal, start ==
    goal, a map smaller than the 129-cell bound) or would index outside the map."""

    def __init__(self, map, start, goal, ctx=None, span=SPAN, r=R):
        self.map = map
        self.start = start
        self.start[0] -= 1
        self.start[1] -= 1
        self.goal = goal
        self.goal[0] -= 1
        self.goal[1] -= 1
        self.ctx = ctx
        self.span, self.r = span, r
        self.path = []
        self.expansions = 0

    def start_find(self):
        rows = np.asarray(self.map)
        H, W = rows.shape
        if self.span > min(H, W):
            raise IndexError("index %d is out of bounds for a %d x %d map" % (min(H, W), H, W))
        st, path, self.expansions, infl = plan_one(rows, [self.start[0] + 1, self.start[1] + 1],
                                                   [self.goal[0] + 1, self.goal[1] + 1], self.span, self.r, self.ctx)
        if isinstance(self.map, np.ndarray):
            self.map[...] = infl
        else:
            for i in range(H):
                for j in range(W):
                    self.map[i][j] = int(infl[i, j])
        if st in (INVALID_START, INVALID_GOAL):
            return "None"
        if st == NO_PATH:
            raise IndexError("list index out of range")        # open_list[0] of an empty list (:172)
        if st == EDGE:
            raise IndexError("the search reached the map's edge (the reference wraps or raises there)")
        self.path = [[int(a), int(b)] for a, b in path[::-1]]
        return self.path


class GlobalPlanner:
    """GlobalPlanner (:14-121) without ROS.  The node's topics become calls:
        map_callback(msg)          /map: an OccupancyGrid-like object (data, info.width / height /
                                   resolution / origin.position) or the dict SLAM_EKF.publishMap builds
        init_pose_callback(x, y)   the robot's world position (/gazebo/model_states, :43-47)
        goal_pose_callback(x, y)   /course_agv/goal (:49-59): plans when the goal is on the map
        publish(path_xy)           hook for /course_agv/global_path; receives current_path
    current_path accumulates the poses of every plan, as the reference's Path does; plan() returns
    this plan's own world path.  start_map_point is shifted by -1 on every plan (find_path mutates
    it), as in the reference, until the next init_pose_callback."""

    def __init__(self, publish=None, ctx=None, span=SPAN, r=R):
        self.origin_x = self.origin_y = 0.0
        self.resolution = 0.0
        self.width = self.height = 0
        self.map = None
        self.current_path = []
        self.start_map_point = []
        self.goal_map_point = []
        self.path_map = []
        self.if_start_find_path = False
        self.publish = publish
        self.ctx = ctx
        self.span, self.r = span, r

    def map_callback(self, msg):
        if isinstance(msg, dict):
            data, w, h, res = msg["data"], msg["width"], msg["height"], msg["resolution"]
            ox, oy = msg["origin"][0], msg["origin"][1]
        else:
            info = msg.info
            data, w, h, res = msg.data, info.width, info.height, info.resolution
            ox, oy = info.origin.position.x, info.origin.position.y
        self.origin_x, self.origin_y = float(ox), float(oy)
        self.resolution = float(res)
        self.width, self.height = int(w), int(h)
        self.map = np.array(data, dtype=np.int8).reshape(self.height, self.width)

    def WorldTomap(self, wx, wy):
        if wx < self.origin_x or wy < self.origin_y:
            return [-1, -1]
        mx = int((wx - self.origin_x) / self.resolution)
        my = int((wy - self.origin_y) / self.resolution)
        if mx < self.width and my < self.height:
            return [my, mx]
        return [-1, -1]

    def mapToWorld(self, wy, wx):
        mx = wx * self.resolution + self.origin_x + 0.25
        my = wy * self.resolution + self.origin_y + 0.25
        return [my, mx]

    def init_pose_callback(self, x, y):
        self.start_map_point = self.WorldTomap(x, y)

    def goal_pose_callback(self, x, y):
        self.path_map = []
        self.if_start_find_path = True
        self.goal_map_point = self.WorldTomap(x, y)
        if self.goal_map_point == [-1, -1]:
            return None
        return self.start_find_path()

    def start_find_path(self):
        if not self.if_start_find_path:
            return None
        temp = find_path(self.map, self.start_map_point, self.goal_map_point, ctx=self.ctx, span=self.span, r=self.r)
        self.path_map = temp.start_find()
        if isinstance(self.path_map, str):     # "None": the reference then fails on "None".reverse()
            raise AttributeError("'str' object has no attribute 'reverse' (find_path returned \"None\")")
        self.path_map.reverse()
        return self.publisher_path()

    def publisher_path(self):
        own = [self.mapToWorld(p[1], p[0]) for p in self.path_map]
        self.current_path.extend(own)
        if self.publish is not None:
            self.publish(np.array(self.current_path, dtype=np.float64).reshape(-1, 2))
        return np.array(own, dtype=np.float64).reshape(-1, 2)

    def plan(self, start_xy, goal_xy):
        """init_pose_callback then goal_pose_callback: this plan's world path [L][2] (x, y), start -> goal."""
        self.init_pose_callback(*start_xy)
        return self.goal_pose_callback(*goal_xy)


class DeviceAStar:
    """B queries over G device-resident maps (torch int8 tensors, passed by data_ptr()): one call
    enqueues the inflation and the search on the context's stream (slam_astar_dev), no host
    synchronise; outputs are torch tensors allocated here."""

    def __init__(self, H, W, G=1, wire_layout=True, span=SPAN, r=R, device=0, ctx=None):
        import torch
        self.ctx = ctx or _abi.default_context(device)
        self.G, self.H, self.W = int(G), int(H), int(W)
        self.wire_layout, self.span, self.r = bool(wire_layout), int(span), int(r)
        self.dev = torch.device("cuda", self.ctx.device)
        self._grid = None

    @classmethod
    def from_grid(cls, grid, span=None, r=R):
        """Plans on a DeviceGrid's live pmap ([G][xw][yw], layout 0: row = y, column = x) on the
        grid's context; span defaults to min(H, W) so that a SLAM-sized map is inflated."""
        H, W = grid.yw, grid.xw
        self = cls(H, W, G=grid.G, wire_layout=False, span=min(H, W) if span is None else span, r=r, ctx=grid._ctx)
        self._grid = grid
        return self

    def maps_ptr(self, maps=None):
        if maps is not None:
            return ptr(maps)
        if self._grid is None:
            raise ValueError("no maps given and no grid attached")
        return self._grid.live_pmap()

    def run(self, starts, goals, maps=None, map_of_query=None, path_cap=1024, want_inflated=False):
        """starts / goals: int32 [B][2] device tensors (row, col as find_path receives them);
        maps: int8 device tensor in this planner's layout (None: the attached grid's live pmap)."""
        import torch
        B = int(starts.shape[0])
        i32 = dict(dtype=torch.int32, device=self.dev)
        out = dict(status=torch.empty(B, **i32), path_len=torch.empty(B, **i32),
                   path=torch.empty((B, max(path_cap, 1), 2), **i32), expansions=torch.empty(B, **i32))
        if want_inflated:
            out["inflated"] = torch.empty((self.G, self.H, self.W), dtype=torch.int8, device=self.dev)
        check(_abi.lib().slam_astar_dev(self.ctx.handle, self.maps_ptr(maps), self.G, self.H, self.W,
                                        int(self.wire_layout), self.span, self.r, ptr(starts), ptr(goals),
                                        ptr(map_of_query), B, int(path_cap), ptr(out["status"]), ptr(out["path_len"]),
                                        ptr(out["path"]) if path_cap > 0 else None, ptr(out["expansions"]),
                                        ptr(out.get("inflated"))))
        return out

    def inflate(self, maps=None):
        import torch
        out = torch.empty((self.G, self.H, self.W), dtype=torch.int8, device=self.dev)
        check(_abi.lib().slam_astar_inflate_dev(self.ctx.handle, self.maps_ptr(maps), self.G, self.H, self.W,
                                                int(self.wire_layout), self.span, self.r, ptr(out)))
        return out
