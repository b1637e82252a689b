"""NumPy restatement of the reference's DWA local planner, the checker of the GPU kernel.

NAV = "W12_LiDAR SLAM/w12-mapping/course_agv_nav/scripts".  The spec is NAV/dwa.py as it
executes (not as it reads):
  - samples: numpy.arange over the dynamic window, v outer, omega inner (dwa.py:95-96);
  - rollout: row 0 is the state, then one row per pass of `while time <= predict_time`
    (dwa.py:115-124), each step yaw first, then x, then y (dwa.py:57-63);
  - obstacle cost: rectangle robots are tested axis-aligned in the planning frame - the
    rotation of dwa.py:135-142 collapses to a multiplication by [-1] (`np.reshape(-1, 1)`)
    - circle robots by hypot <= robot_radius; cost inf on collision, else 1 / min(hypot)
    over every (row, obstacle) pair (dwa.py:126-160);
  - final cost summed left to right (dwa.py:101-105); `min_cost >= final_cost` selection
    from inf (dwa.py:108): NaN never wins, ties go to the later sample.
This module is written from that description; it is test infrastructure and the product
never imports it.
"""
from __future__ import annotations

import math

import numpy as np

CIRCLE, RECTANGLE = 0, 1

# Config fields in the order of the C ABI's double[SLAM_DWA_CONFIG_LEN] (include/slam_hip.h).
FIELDS = ("max_speed", "min_speed", "max_yawrate", "max_accel", "max_dyawrate", "dt", "v_reso", "yawrate_reso",
          "predict_time", "to_goal_cost_gain", "speed_cost_gain", "obstacle_cost_gain", "robot_type",
          "robot_radius", "robot_width", "robot_length")


def default_config(**over):
    c = dict(max_speed=0.8, min_speed=-0.5, max_yawrate=100.0 * math.pi / 180.0, max_accel=1.0,
             max_dyawrate=100.0 * math.pi / 180.0, dt=0.1, predict_time=2.0, to_goal_cost_gain=1.0,
             speed_cost_gain=0.1, obstacle_cost_gain=1.0, robot_type=RECTANGLE, robot_radius=0.4,
             robot_width=0.3, robot_length=0.6)
    c.update(over)
    if "v_reso" not in over:
        c["v_reso"] = c["max_accel"] * c["dt"] / 10.0
    if "yawrate_reso" not in over:
        c["yawrate_reso"] = c["max_dyawrate"] * c["dt"] / 10.0
    return c


def config_array(c):
    return np.array([float(c[f]) for f in FIELDS], dtype=np.float64)


def arange(start, stop, step):
    """numpy's float arange, element by element (what np.arange returns)."""
    q = (stop - start) / step
    if not q > 0:
        return np.zeros(0)
    n = int(math.ceil(q))
    out = np.empty(n)
    out[0] = start
    if n > 1:
        a1 = start + step
        out[1] = a1
        d = a1 - start
        for i in range(2, n):
            out[i] = start + i * d
    return out


def dynamic_window(x, c):
    vs = [c["min_speed"], c["max_speed"], -c["max_yawrate"], c["max_yawrate"]]
    vd = [x[3] - c["max_accel"] * c["dt"], x[3] + c["max_accel"] * c["dt"],
          x[4] - c["max_dyawrate"] * c["dt"], x[4] + c["max_dyawrate"] * c["dt"]]
    return [max(vs[0], vd[0]), min(vs[1], vd[1]), max(vs[2], vd[2]), min(vs[3], vd[3])]


def n_steps(c):
    t, k = 0, 0
    while t <= c["predict_time"]:
        k += 1
        t += c["dt"]
    return k


def rollout(x, v, w, c, steps):
    tr = np.empty((steps + 1, 5))
    tr[0] = x
    px, py, yaw = float(x[0]), float(x[1]), float(x[2])
    dt = c["dt"]
    for k in range(1, steps + 1):
        yaw += w * dt
        px += v * math.cos(yaw) * dt
        py += v * math.sin(yaw) * dt
        tr[k] = (px, py, yaw, v, w)
    return tr


def obstacle_cost(tr, ob, c):
    dx = tr[:, 0] - ob[:, 0][:, None]
    dy = tr[:, 1] - ob[:, 1][:, None]
    r = np.hypot(dx, dy)
    if int(c["robot_type"]) == RECTANGLE:
        lx = (ob[:, None] - tr[:, 0:2]).reshape(-1, 2) * np.array([-1.0])
        hl, hw = c["robot_length"] / 2, c["robot_width"] / 2
        if np.any((lx[:, 0] <= hl) & (lx[:, 1] <= hw) & (lx[:, 0] >= -hl) & (lx[:, 1] >= -hw)):
            return float("inf")
    elif np.any(r <= c["robot_radius"]):
        return float("inf")
    return 1.0 / np.min(r)


def goal_cost(tr, goal):
    a = math.atan2(goal[1] - tr[-1, 1], goal[0] - tr[-1, 0]) - tr[-1, 2]
    return abs(math.atan2(math.sin(a), math.cos(a)))


def plan(x, c, goal, ob):
    """Every sample of one control step.  Returns dict: u [2], traj [rows or 1][5], index
    (-1: none wins), cost (the winner's, inf when none), nv, nw, costs [nv*nw]."""
    x = np.asarray(x, dtype=np.float64)
    ob = np.asarray(ob, dtype=np.float64).reshape(-1, 2)
    dw = dynamic_window(x, c)
    vs, ws = arange(dw[0], dw[1], c["v_reso"]), arange(dw[2], dw[3], c["yawrate_reso"])
    steps = n_steps(c)
    costs = np.empty(len(vs) * len(ws))
    best, best_i, best_u, best_tr = float("inf"), -1, [0.0, 0.0], x[None].copy()
    s = 0
    for v in vs:
        for w in ws:
            tr = rollout(x, float(v), float(w), c, steps)
            f = c["to_goal_cost_gain"] * goal_cost(tr, goal)
            f = f + c["speed_cost_gain"] * (c["max_speed"] - tr[-1, 3])
            f = f + c["obstacle_cost_gain"] * obstacle_cost(tr, ob, c)
            costs[s] = f
            if best >= f:
                best, best_i, best_u, best_tr = f, s, [float(v), float(w)], tr
            s += 1
    return dict(u=np.array(best_u), traj=best_tr, index=best_i, cost=best, nv=len(vs), nw=len(ws), costs=costs)


def scan_obstacles(ranges, angle_min, angle_increment, threshold):
    """LocalPlanner.laserCallback's preprocessing (local_planner.py:57-68): sentinel (100, 100),
    then every beam with r < threshold at a = angle_min + angle_increment * i."""
    ob = [[100.0, 100.0]]
    for i, r in enumerate(ranges):
        a = angle_min + angle_increment * i
        r = float(r)
        if r < threshold:
            ob.append([math.cos(a) * r, math.sin(a) * r])
    return np.array(ob)


class LocalPlannerRef:
    """LocalPlanner (local_planner.py:22-165) without ROS: the path and pose arrive as arrays."""

    def __init__(self, config=None):
        self.c = config or default_config()
        self.threshold = self.c["max_speed"] * self.c["predict_time"]
        self.vx = self.vw = 0.0
        self.goal_index = 0
        self.path = None
        self.ob = np.array([[100.0, 100.0]])

    def path_callback(self, path_xy, pose=None):
        self.path = np.asarray(path_xy, dtype=np.float64)
        self.goal_index = 0
        self.vx = self.vw = 0.0
        if pose is not None:
            self._goal(pose)

    def _goal(self, pose):
        px, py, yaw = (float(v) for v in pose)
        ind = self.goal_index
        self.goal_index = len(self.path) - 1
        while ind < len(self.path):
            if math.hypot(self.path[ind, 0] - px, self.path[ind, 1] - py) < self.threshold:
                self.goal_index = ind
            ind += 1
        gx, gy = self.path[self.goal_index]
        dx, dy = gx - px, gy - py
        return np.array([math.cos(yaw) * dx + math.sin(yaw) * dy, -math.sin(yaw) * dx + math.cos(yaw) * dy])

    def laser_callback(self, ranges, angle_min, angle_increment):
        self.ob = scan_obstacles(ranges, angle_min, angle_increment, self.threshold)

    def plan_once(self, pose):
        goal = self._goal(pose)
        r = plan([0.0, 0.0, 0.0, self.vx, self.vw], self.c, goal, self.ob)
        self.vx = r["u"][0] * 0.5 + self.vx * (1 - 0.5)
        self.vw = r["u"][1] * 0.5 + self.vw * (1 - 0.5)
        return self.vx, self.vw
