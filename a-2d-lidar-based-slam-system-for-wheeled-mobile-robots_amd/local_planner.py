"""LocalPlanner (course_agv_nav/scripts/local_planner.py:22-165) without ROS, its DWA step on
the GPU (slam_dwa_scans: the scan's obstacle preprocessing is fused into the launch).

The node's topics become calls, as SLAM_EKF and Localization do here:
    pathCallback(path_xy, pose=None)   /course_agv/global_path (initPlanning, :46-85)
    laserCallback(msg)                 /course_agv/laser/scan (:57-69; ranges, angle_min, angle_increment)
    planOnce(pose)                     one pass of planThreadFunc (:135-150); the /map -> /robot_base
                                       transform arrives as pose = (x, y, yaw)
    publish(vx, vw)                    hook for /course_agv/velocity (:152-159)
The goal is chosen as updateGlobalPose does it (:87-117): the last path point within
`threshold` of the robot from the current goal index on (else the path's end), moved into the
robot frame.
"""
from __future__ import annotations

import math

import numpy as np

from . import _abi
from ._abi import check, ptr
from .dwa import Config, RobotType, config_array


class LocalPlanner:
    def __init__(self, publish=None, ctx=None):
        self.arrive = 0.1
        self.x = self.y = self.yaw = 0.0
        self.vx = self.vw = 0.0
        self.plan_config = Config()
        self.plan_config.robot_type = RobotType.rectangle
        c = self.plan_config
        self.threshold = c.max_speed * c.predict_time
        self.publish = publish
        self.ctx = ctx
        self.path = None
        self.goal_index = 0
        self.goal_dis = float("inf")
        self.plan_goal = None
        self._scan = None          # (float32 ranges, cos table, sin table)
        self._tables = {}

    def pathCallback(self, path_xy, pose=None):
        """initPlanning (:71-85).  pose: the robot pose at the time the path arrives (the
        reference looks it up from tf there); None skips that goal-index pass."""
        self.path = np.asarray(path_xy, dtype=np.float64).reshape(-1, 2)
        self.goal_index = 0
        self.vx = 0.0
        self.vw = 0.0
        if pose is not None:
            self.updateGlobalPose(pose)
        self.plan_x = np.array([0.0, 0.0, 0.0, self.vx, self.vw])

    def laserCallback(self, msg):
        n = len(msg.ranges)
        key = (float(msg.angle_min), float(msg.angle_increment), n)
        t = self._tables.get(key)
        if t is None:
            t = self._tables[key] = _abi.beam_tables(msg.angle_min, msg.angle_increment, n)
        self._scan = (np.ascontiguousarray(msg.ranges, dtype=np.float32), t[0], t[1])

    def updateGlobalPose(self, pose):
        self.x, self.y, self.yaw = (float(v) for v in pose)
        ind = self.goal_index
        self.goal_index = len(self.path) - 1
        while ind < len(self.path):
            if math.hypot(self.path[ind, 0] - self.x, self.path[ind, 1] - self.y) < self.threshold:
                self.goal_index = ind
            ind += 1
        gx, gy = self.path[self.goal_index]
        dx, dy = gx - self.x, gy - self.y
        cy, sy = math.cos(self.yaw), math.sin(self.yaw)
        self.plan_goal = np.array([cy * dx + sy * dy, -sy * dx + cy * dy])           # goal in /robot_base
        self.goal_dis = math.hypot(self.x - self.path[-1, 0], self.y - self.path[-1, 1])

    def planOnce(self, pose):
        """One control step: goal, plan_x = [0, 0, 0, vx, vw], DWA, alpha = 0.5 smoothing."""
        self.updateGlobalPose(pose)
        self.plan_x = [0.0, 0.0, 0.0, self.vx, self.vw]
        u = self._dwa(np.array(self.plan_x, dtype=np.float64), self.plan_goal)
        alpha = 0.5
        self.vx = u[0] * alpha + self.vx * (1 - alpha)
        self.vw = u[1] * alpha + self.vw * (1 - alpha)
        self.publishVel()
        return self.vx, self.vw

    @property
    def arrived(self):
        return self.goal_dis < self.arrive

    def publishVel(self, zero=False):
        vx, vw = self.vx, self.vw
        if zero:
            self.vx = 0
            self.vw = 0
        if self.publish is not None:
            self.publish(vx, vw)

    def _dwa(self, x, goal):
        c = self.ctx or _abi.default_context()
        cfg = config_array(self.plan_config)
        u, cost, idx = np.empty(2), np.empty(1), np.empty(1, np.int32)
        g = np.ascontiguousarray(goal, dtype=np.float64)
        L = _abi.lib()
        if self._scan is None or len(self._scan[0]) == 0:     # no beams: the sentinel alone (:61)
            ob = np.array([100.0, 100.0])
            check(L.slam_dwa(c.handle, ptr(x), ptr(g), ptr(ob), None, 1, 0, ptr(cfg), 1, ptr(u), ptr(cost), ptr(idx),
                             None, None, 0, None))
        else:
            r, ct, st = self._scan
            check(L.slam_dwa_scans(c.handle, ptr(x), ptr(g), ptr(r), len(r), 0, ptr(ct), ptr(st), self.threshold,
                                   ptr(cfg), 1, ptr(u), ptr(cost), ptr(idx), None, None, 0, None))
        return float(u[0]), float(u[1])
