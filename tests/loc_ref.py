"""NumPy restatement of the W9 node as a chain, the checker of ``slam_loc_replay``.

W9 = "W9_Fusion Localization (LiDAR Odometry)/course_agv_slam/scripts".  One step of
``Localization.laserCallback`` (localization.py:66-126) for a processed scan is
  T1 = ICP.process(previous scan, scan)       first calc_odometry (:78); the very first target is the
                                              map's virtual scan at the start pose (:159-168)
  xOdom = compose(xOdom, T1)                  (:79-83)
  T2 = ICP.process(scan, scan)                second calc_odometry (:100)
  t  = calc_map_observation at xEst           (:152-157), z = compose(xEst, t) (:113-118)
  xEst, PEst = EKF.estimate(xEst, PEst, z, T2)   (W9/ekf.py:17-87)
The operators come from ``oracle.oracle_np``; this module adds only the chain and the 3x3 filter,
written from that description.  It is test infrastructure and the product never imports it.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import oracle_np as on

NOISE = np.diag([0.2, 0.2, math.pi / 60]) ** 2          # ekf.py:6-13: R of the prediction = Q of the innovation


def ekf_estimate(x_est, p_est, z, t):
    """ekf.py:17-87: odom_model / jacob_f predict with the odometry transform t, the pose z corrects."""
    x_pred = np.array(on.compose_pose(x_est, t), dtype=float)
    j = np.eye(3)
    j[0, 2] = -t[0, 2] * t[1, 0] - t[1, 2] * t[0, 0]
    j[1, 2] = t[0, 2] * t[0, 0] - t[1, 2] * t[1, 0]
    p_pred = j.dot(p_est).dot(j.T) + NOISE
    k = p_pred.dot(np.linalg.inv(p_pred + NOISE))
    return x_pred + k.dot(np.asarray(z, dtype=float) - x_pred), (np.eye(3) - k).dot(p_pred)


def stream_solves(ranges, angle_min, angle_max, max_iter=30, tol=0.001):
    """What depends on the stream alone: (T1 of the steps after the first [n_scan - 1], T2 [n_scan])."""
    pcs = [on.laser_to_numpy(np.asarray(r, dtype=np.float64), angle_min, angle_max) for r in ranges]
    t1 = [on.icp_process(pcs[s - 1], pcs[s], max_iter, tol) for s in range(1, len(pcs))]
    t2 = [on.icp_process(pc, pc, max_iter, tol) for pc in pcs]
    return t1, t2


def chain(ranges, obstacle, angle_min, angle_max, pose0=(0.0, 0.0, 0.0), max_iter=30, tol=0.001, solves=None, nudge=0.0,
          angle_increment=None):
    """The node over one stream ``ranges [n_scan, n]`` against ``obstacle [2, K]`` from ``pose0``.
    ``solves``: what :func:`stream_solves` returned (computed when None).  ``nudge`` is added to every
    component of xEst after every step (the stability probe of the tests).  ``angle_increment``: the message's
    own, which bins the virtual scan (localization.py:139) while the points of both scans come from
    linspace(angle_min, angle_max) (:170-176); None: (angle_max - angle_min) / (n - 1).  Returns dict of ``xest``,
    ``xodom`` [n_scan, 3], ``P`` [3, 3], ``T_obs``, ``T_odom`` [n_scan, 3, 3], ``iters_obs`` [n_scan]."""
    ranges = np.asarray(ranges)
    n_scan, n = ranges.shape
    inc = (angle_max - angle_min) / (n - 1) if angle_increment is None else float(angle_increment)
    t1s, t2s = solves if solves is not None else stream_solves(ranges, angle_min, angle_max, max_iter, tol)
    xest, xodom, pest = [float(v) for v in pose0], [float(v) for v in pose0], np.eye(3)
    out = {"xest": [], "xodom": [], "T_obs": [], "T_odom": [], "iters_obs": []}
    for s in range(n_scan):
        src = on.laser_to_numpy(ranges[s].astype(np.float64), angle_min, angle_max)
        tar = on.laser_to_numpy(on.laser_estimation(obstacle, xest, angle_min, inc, n), angle_min, angle_max)
        t, it, _ = on.icp_process(tar, src, max_iter, tol, return_info=True)
        t1 = t if s == 0 else t1s[s - 1]            # step 0: the same pair as the map observation (:159-168)
        xodom = on.compose_pose(xodom, t1)
        z = on.compose_pose(xest, t)
        xest, pest = ekf_estimate(xest, pest, z, t2s[s])
        out["xest"].append(np.array(xest, dtype=float))
        out["xodom"].append(np.array(xodom, dtype=float))
        out["T_obs"].append(t)
        out["T_odom"].append(t1)
        out["iters_obs"].append(it)
        xest = [float(v) + nudge for v in xest]
    o = {k: np.array(v) for k, v in out.items()}
    o["P"] = pest
    return o


def stable(ranges, obstacle, angle_min, angle_max, pose0=(0.0, 0.0, 0.0), eps=1e-11, bound=1e-10, max_iter=30, tol=0.001,
           angle_increment=None):
    """(reference run, worst deviation of the runs nudged by +-eps): the chain is discontinuous where an
    obstacle changes its beam bin or a nearest neighbour changes; inputs are usable when the worst
    deviation stays below ``bound``.  The nudge accumulates by eps a step, so a run of n_scan steps is
    judged against :func:`stable_bound`; the default ``bound`` is that of the 8-step runs at eps = 1e-11."""
    kw = dict(max_iter=max_iter, tol=tol, angle_increment=angle_increment)
    solves = stream_solves(ranges, angle_min, angle_max, max_iter, tol)
    ref = chain(ranges, obstacle, angle_min, angle_max, pose0, solves=solves, **kw)
    worst = 0.0
    for e in (eps, -eps):
        o = chain(ranges, obstacle, angle_min, angle_max, pose0, solves=solves, nudge=e, **kw)
        if not np.array_equal(o["iters_obs"], ref["iters_obs"]):
            return ref, float("inf")
        for k in ("xest", "xodom", "P", "T_obs", "T_odom"):
            # the nudge itself moves xest by eps per step; what must not happen is a jump
            worst = max(worst, float(np.max(np.abs(o[k] - ref[k]))))
    return ref, worst


def stable_bound(eps, n_scan):
    """What a run of ``n_scan`` steps nudged by ``eps`` a step may deviate by without a jump: the accumulated
    nudge is eps * n_scan, the filter and the compositions pass it on with gains near 1; 4x leaves room."""
    return 4.0 * eps * n_scan
