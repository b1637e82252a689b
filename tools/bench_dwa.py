#!/usr/bin/env python3
"""Throughput of the DWA local planner (slam_dwa_dev / slam_dwa_scans_dev) on one MI355X.

For B in {1, 256, 4096, 65536} planners - each with its own 360-beam synthetic scan at a random
pose in a small room, the default Config (21 x 5 trajectories, 20 x 20 .. 21 x 21 samples) and a
random state and goal - times both forms with HIP events (torch.cuda.Event on the context's
stream) and reports planners/s, point-obstacle pair tests/s (the reference's count: samples x
21 rows x obstacles, summed over planners) and ms per launch; plus the NumPy oracle's time per
plan on the host for comparison.  Prints one JSON line (and writes it to --out when given).

Usage:  python tools/bench_dwa.py [--iters 20] [--batches 1,256,4096,65536] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "a-2d-lidar-based-slam-system-for-wheeled-mobile-robots_amd"


def main():
    import importlib

    import torch

    import dwa_ref
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batches", default="1,256,4096,65536")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    slam = importlib.import_module(PKG)
    syn = slam.synthetic
    c = dwa_ref.default_config()
    n = 360
    am, inc = syn.ANGLE_MIN, (syn.ANGLE_MAX - syn.ANGLE_MIN) / (n - 1)
    thr = c["max_speed"] * c["predict_time"]
    rng = np.random.default_rng(1)
    P = 512                                        # distinct scans, reused round-robin by larger batches
    poses = np.stack([rng.uniform(-1.6, 1.6, P), rng.uniform(-1.2, 1.2, P), rng.uniform(-np.pi, np.pi, P)], 1)
    scans = syn.scans_from_poses(syn.World.room(0.45), poses, n, seed=1)
    obs = [dwa_ref.scan_obstacles(s, am, inc, thr) for s in scans]
    Mx = max(len(o) for o in obs)
    # the context enqueues on a torch stream made current here, so torch's events bracket the launches
    ts = torch.cuda.Stream()
    torch.cuda.set_stream(ts)
    ctx = slam.Context(0, stream=ts.cuda_stream)
    dd = slam.DeviceDWA(c, ctx=ctx)
    dev = dd.dev
    res = dict(metric="dwa_planners_per_s", config="default Config, rectangle, 360-beam scans",
               obstacles_mean=float(np.mean([len(o) for o in obs])), legs=[])
    for B in [int(v) for v in a.batches.split(",")]:
        idx = np.arange(B) % P
        states = np.zeros((B, 5))
        states[:, 3] = rng.uniform(-0.5, 0.8, B)
        states[:, 4] = rng.uniform(-1.7, 1.7, B)
        goals = rng.uniform(-3, 3, (B, 2))
        cnt = np.array([len(obs[i]) for i in idx], dtype=np.int32)
        ob = np.zeros((B, 2, Mx))
        for b, i in enumerate(idx):
            ob[b, 0, :cnt[b]] = obs[i][:, 0]
            ob[b, 1, :cnt[b]] = obs[i][:, 1]
        t_st, t_g = torch.from_numpy(states).to(dev), torch.from_numpy(goals).to(dev)
        t_ob, t_cnt = torch.from_numpy(ob).to(dev), torch.from_numpy(cnt).to(dev)
        t_sc = torch.from_numpy(np.ascontiguousarray(scans[idx])).to(dev)
        for form in ("obstacles", "scans"):
            def once():
                if form == "obstacles":
                    return dd.run(t_st, t_g, t_ob, counts=t_cnt)
                return dd.run_scans(t_st, t_g, t_sc, am, inc)
            out = once()
            torch.cuda.synchronize()
            S = (out["counts"][:, 0].long() * out["counts"][:, 1].long()).cpu().numpy()
            pairs = float(np.sum(S * 21 * cnt))
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
            for e0, e1 in ev:
                e0.record()
                once()
                e1.record()
            torch.cuda.synchronize()
            ms = [e0.elapsed_time(e1) for e0, e1 in ev]
            med = float(np.median(ms))
            res["legs"].append(dict(B=B, form=form, ms_per_launch=round(med, 4), ms_min=round(float(np.min(ms)), 4),
                                    planners_per_s=round(B / med * 1e3, 1), pair_tests_per_s=float("%.4g" % (pairs / med * 1e3)),
                                    pairs_per_launch=pairs))
    t0 = time.perf_counter()
    k = 3
    for i in range(k):
        dwa_ref.plan([0, 0, 0, 0.3, 0.1], c, [1.5, 0.2], obs[i])
    res["oracle_ms_per_plan_host"] = round((time.perf_counter() - t0) / k * 1e3, 2)
    res["timing"] = "HIP events around each launch on the context's stream, median of --iters back-to-back launches"
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
