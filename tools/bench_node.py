#!/usr/bin/env python3
"""Throughput of the batched landmark EKF-SLAM node (slam_node_replay_dev) on one MI355X, beside the same
trajectories run scan by scan through SLAM_EKF(landmarks=True).

L in {1, 32, 1024} trajectories x 200 scans x 360 beams on the landmark world (a 10 m x 8 m room with four
poles of 8 cm radius; 32 distinct seeded trajectories, repeated for L = 1024), one 200 x 200 map per
trajectory.  The batched call is timed with HIP events on the context's stream (median of --iters calls, map
reset included); the kernel families the library times itself (slam_timing_read: scan matching and ray cast)
are read in a separate pass.  The scan-by-scan side runs --host-traj trajectories through the drop-in node -
one library call for the odometry and one for the map per kept scan, Extraction and EKF in NumPy between them -
and is reported per trajectory (it has no batch dimension).  One trajectory of the batch is compared with the
node's own result before anything is timed.  Prints one JSON line and writes it to --out.

Usage:  python tools/bench_node.py [--iters 5] [--batches 1,32,1024] [--host-traj 2] [--out profiles/node_replay_bench.json]
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "a-2d-lidar-based-slam-system-for-wheeled-mobile-robots_amd"
AMIN, AMAX = -3.14159, 3.14159
POLES = ((1.5, 1.0), (-1.8, -0.9), (0.5, -2.0), (-2.5, 1.5))


def host_trajectory(slam, scans):
    node = slam.SLAM_EKF(landmarks=True)
    t0 = time.perf_counter()
    for r in scans:
        node.laser_count = 4                      # the scans are already decimated (slam_ekf.py:65-67)
        node.laserCallback(slam.LaserScan(ranges=tuple(float(v) for v in r), angle_min=AMIN, angle_max=AMAX))
    return time.perf_counter() - t0, node


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--batches", default="1,32,1024")
    ap.add_argument("--scans", type=int, default=200)
    ap.add_argument("--host-traj", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "node_replay_bench.json"))
    a = ap.parse_args()
    slam = importlib.import_module(PKG)
    syn = slam.synthetic
    world = syn.World(5.0, 4.0, POLES, 0.08)
    distinct = []
    for seed in range(32):
        poses = syn.trajectory(world, a.scans * 5, 100 + seed)[::5]
        distinct.append(syn.scans_from_poses(world, poses, 360, 100 + seed))
    distinct = np.stack(distinct).astype(np.float32)
    res = dict(metric="node_trajectories_per_s", scans=a.scans, beams=360, legs=[])

    host_s, ref = [], None
    for l in range(a.host_traj):
        try:
            dt, node = host_trajectory(slam, distinct[l])
        except ValueError:                        # the reference's own failure (ekf_lm.py:37-38): not a timing
            continue
        host_s.append(dt)
        if ref is None:
            ref, ref_l = node, l
    if not host_s:
        raise SystemExit("no trajectory ran through the scan-by-scan node")
    res["scan_by_scan"] = dict(trajectories=len(host_s), ms_per_trajectory=round(float(np.median(host_s)) * 1e3, 2),
                               trajectories_per_s=round(1.0 / float(np.median(host_s)), 3))

    for L in [int(v) for v in a.batches.split(",")]:
        scans = distinct[np.arange(L) % 32]
        rep = slam.DeviceNodeReplay(scans, AMIN, AMAX, grid_of_traj=np.arange(L), max_lm=16, lm_cap=8)
        grid = rep.make_grid(L, 200, 200, 0.1)
        rep.run()
        out = rep.results()
        check = dict(status_ok=int((out["status"] == 0).sum()))
        if ref is not None and ref_l < L:
            n = len(ref.xEst)
            check.update(traj=ref_l, state_err=float(np.max(np.abs(out["x"][ref_l, :n] - ref.xEst[:, 0]))),
                         map_equal=bool(np.array_equal(grid.read(ref_l)["pmap"], ref.mapping.pmap.astype(np.int8))))
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
        for e0, e1 in ev:
            e0.record()
            rep.run()
            e1.record()
        torch.cuda.synchronize()
        ms = [e0.elapsed_time(e1) for e0, e1 in ev]
        med = float(np.median(ms))
        rep.ctx.timing_enable(True)
        rep.run()
        fam = {k: round(v[0], 4) for k, v in rep.ctx.timing_read().items() if v[1]}
        rep.ctx.timing_enable(False)
        leg = dict(L=L, ms_per_call=round(med, 4), ms_min=round(float(np.min(ms)), 4),
                   trajectories_per_s=round(L / med * 1e3, 1), scans_per_s=round(L * a.scans / med * 1e3, 1),
                   kept_scans=int(out["kept_count"].sum()), family_ms=fam,
                   rest_ms=round(med - sum(fam.values()), 4),
                   speedup_over_scan_by_scan=round(L / med * 1e3 / res["scan_by_scan"]["trajectories_per_s"], 1), check=check)
        res["legs"].append(leg)
        print(json.dumps(leg), flush=True)
        del rep, grid
    res["timing"] = ("batched: HIP events around DeviceNodeReplay.run() (map reset + extraction + kept scans + scan matching + "
                     "filter + ray cast), median of --iters calls; family_ms: the library's own per-family events in a separate "
                     "call, rest_ms = the call minus them (extraction, kept-scan gather, filter, reset); scan by scan: wall "
                     "time of SLAM_EKF(landmarks=True).laserCallback over one trajectory on one host thread")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
