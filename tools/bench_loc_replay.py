#!/usr/bin/env python3
"""Throughput of the batched W9 node (slam_loc_replay_dev) on one MI355X, beside the same work done with what
the library had before it.

L in {1, 64, 1024, 8192} start-pose hypotheses (within +-0.3 m / +-0.1 rad of the true start) of ONE 200-scan,
360-beam stream against the obstacle list of the course map (tests/golden/g5_map_observation.npz ``map_data``
through Localization.updateMap).  Three ways:
  new       DeviceLocalizationReplay.run(): host clock around the call and a synchronise of the context's stream,
            after --warmup calls, median of --iters calls (at most 3 from L = 1024 on);
  (a)       Localization.laserCallback per trajectory: wall time of --host-traj trajectories, scaled to L (it
            has no batch dimension);
  (b)       a host loop over the steps: slam_map_observation with B = L per step, the stream-only odometry
            solves once per step (ICP.process), the compositions and the 3x3 filters in NumPy over L.
Every figure is steps/s = L * scans / time.  One trajectory of the batch is compared with (a) before anything
is timed.  Prints one JSON line per leg, then the whole result, and writes it to --out.

Usage:  python tools/bench_loc_replay.py [--iters 5] [--warmup 2] [--batches 1,64,1024,8192] [--out profiles/loc_replay_bench.json]
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "a-2d-lidar-based-slam-system-for-wheeled-mobile-robots_amd"
AMIN, AMAX = -3.14159, 3.14159


def msg_of(slam, r):
    return slam.LaserScan(ranges=tuple(float(v) for v in r), angle_min=AMIN, angle_max=AMAX,
                          angle_increment=(AMAX - AMIN) / (len(r) - 1))


def host_class(slam, obstacle, scans, pose0):
    """(a): the drop-in node, one processed scan per call."""
    loc = slam.Localization()
    loc.obstacle = obstacle
    loc.xEst, loc.xOdom = [float(v) for v in pose0], [float(v) for v in pose0]
    msgs = [msg_of(slam, r) for r in scans]
    t0 = time.perf_counter()
    for m in msgs:
        loc.laser_count = 5
        loc.laserCallback(m)
    return time.perf_counter() - t0, loc


def compose_batch(x, T):
    yaw = np.arctan2(T[:, 1, 0], T[:, 0, 0])
    c, s = np.cos(x[:, 2]), np.sin(x[:, 2])
    return np.stack([x[:, 0] + c * T[:, 0, 2] - s * T[:, 1, 2], x[:, 1] + s * T[:, 0, 2] + c * T[:, 1, 2], x[:, 2] + yaw], axis=1)


def host_loop(slam, obstacle, scans, pose0):
    """(b): per step one slam_map_observation over every hypothesis, the rest in NumPy."""
    L = pose0.shape[0]
    loc = slam.Localization()
    loc.obstacle = obstacle
    noise = slam.localization.EKF.NOISE
    msgs = [msg_of(slam, r) for r in scans]
    t0 = time.perf_counter()
    x, xo, P = pose0.copy(), pose0.copy(), np.tile(np.eye(3), (L, 1, 1))
    tar = None
    for s, m in enumerate(msgs):
        src = loc.laserToNumpy(m)
        t, _ = loc.map_observation_batch(m, x, src_pc=src)
        T1 = t if s == 0 else np.broadcast_to(loc.icp.process(tar, src), (L, 3, 3))
        T2 = np.broadcast_to(loc.icp.process(src, src), (L, 3, 3))
        tar = src
        xo = compose_batch(xo, T1)
        z = compose_batch(x, t)
        xp = compose_batch(x, T2)
        J = np.tile(np.eye(3), (L, 1, 1))
        J[:, 0, 2] = -T2[:, 0, 2] * T2[:, 1, 0] - T2[:, 1, 2] * T2[:, 0, 0]
        J[:, 1, 2] = T2[:, 0, 2] * T2[:, 0, 0] - T2[:, 1, 2] * T2[:, 1, 0]
        Pp = J @ P @ J.transpose(0, 2, 1) + noise
        K = Pp @ np.linalg.inv(Pp + noise)
        x = xp + (K @ (z - xp)[:, :, None])[:, :, 0]
        P = (np.eye(3) - K) @ Pp
    return time.perf_counter() - t0, x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batches", default="1,64,1024,8192")
    ap.add_argument("--scans", type=int, default=200)
    ap.add_argument("--host-traj", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loc_replay_bench.json"))
    a = ap.parse_args()
    slam = importlib.import_module(PKG)
    g5 = np.load(os.path.join(ROOT, "tests", "golden", "g5_map_observation.npz"))
    loc = slam.Localization()
    loc.updateMap(types.SimpleNamespace(data=g5["map_data"], info=types.SimpleNamespace(
        height=200, width=200, resolution=0.1, origin=types.SimpleNamespace(position=types.SimpleNamespace(x=-10.0, y=-10.0)))))
    obstacle = np.ascontiguousarray(loc.obstacle)
    rep_syn = slam.synthetic.make_replay(a.scans, 360, seed=1, stride=6)
    scans, start = rep_syn.ranges, rep_syn.poses_true[0]
    res = dict(metric="loc_steps_per_s", scans=a.scans, beams=360, obstacles=int(obstacle.shape[1]), legs=[])

    rng = np.random.default_rng(3)
    host_s, ref = [], None
    for l in range(a.host_traj):
        p = start + (rng.uniform(-1, 1, size=3) * np.array([0.3, 0.3, 0.1]) if l else 0.0)
        dt, node = host_class(slam, obstacle, scans, p)
        host_s.append(dt)
        if ref is None:
            ref = node
    per_traj = float(np.median(host_s))
    res["host_class"] = dict(trajectories=len(host_s), ms_per_trajectory=round(per_traj * 1e3, 2),
                             steps_per_s=round(a.scans / per_traj, 1))

    for L in [int(v) for v in a.batches.split(",")]:
        p0 = start + rng.uniform(-1, 1, size=(L, 3)) * np.array([0.3, 0.3, 0.1])
        p0[0] = start
        rep = slam.DeviceLocalizationReplay(scans, AMIN, AMAX, obstacle, pose0=p0, stream_of_traj=np.zeros(L, dtype=np.int32))
        for _ in range(max(1, a.warmup)):
            rep.run()
        out = rep.results()
        check = dict(status_ok=int((out["status"] == 0).sum()),
                     xest_err_vs_host_class=float(np.max(np.abs(out["xest"][0, -1] - np.asarray(ref.xEst, dtype=float)))))
        iters = a.iters if L < 1024 else min(a.iters, 3)
        ms = []
        for _ in range(iters):
            rep.ctx.synchronize()
            t0 = time.perf_counter()
            rep.run()
            rep.ctx.synchronize()                 # the context's own stream: the clock stops when the device is done
            ms.append((time.perf_counter() - t0) * 1e3)
        med = float(np.median(ms))
        rep.ctx.timing_enable(True, only=["icp"])
        rep.run()
        rep.ctx.synchronize()
        icp_ms = rep.ctx.timing_read()["icp"][0]
        rep.ctx.timing_enable(False)
        del rep
        host_loop(slam, obstacle, scans[:3], p0)                      # warm-up of (b)'s staging and kernels
        dt_b, xb = host_loop(slam, obstacle, scans, p0)                # (raises, as the host class does, if a transform is not finite)
        steps = L * a.scans
        leg = dict(L=L, ms_per_call=round(med, 3), ms_min=round(float(np.min(ms)), 3), ms_max=round(float(np.max(ms)), 3),
                   steps_per_s=round(steps / med * 1e3, 1), scan_matcher_ms=round(icp_ms, 3),
                   step_kernel_and_gaps_ms=round(med - icp_ms, 3),
                   host_loop_ms=round(dt_b * 1e3, 2), host_loop_steps_per_s=round(steps / dt_b, 1),
                   host_class_steps_per_s=res["host_class"]["steps_per_s"],
                   ratio_over_host_loop=round(dt_b * 1e3 / med, 2),
                   ratio_over_host_class=round(per_traj * L * 1e3 / med, 1),
                   host_loop_xest_err=float(np.max(np.abs(xb - out["xest"][:, -1]))), check=check)
        res["legs"].append(leg)
        print(json.dumps(leg), flush=True)
    res["timing"] = ("new: host clock around DeviceLocalizationReplay.run() + a synchronise of its stream, after --warmup calls, median of the timed calls; "
                     "scan_matcher_ms: the library's own events on every scan-matcher launch of one more call, the rest is "
                     "k_loc_step, the pair gather and the gaps between launches; (a) host_class: wall time of "
                     "Localization.laserCallback over the stream on one host thread, per trajectory; (b) host_loop: wall "
                     "time of one pass, after a 3-step warm-up")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
