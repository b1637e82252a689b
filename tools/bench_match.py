#!/usr/bin/env python3
"""Time of slam_grid_match_dev on one MI355X beside slam_grid_scan_score_dev over the IDENTICAL list of candidate poses
(before the matcher, scoring every pose with one Bresenham walk per beam was the only way to rank them), and of
slam_grid_distance_field_dev alone.

Map: the course map (tests/golden/g5_map_observation.npz ``map_data``, 200 x 200 at 0.1 m) at 400 x 400, scale 20 -
every cell doubled - loaded through slam_grid_counters_dev, as tools/bench_raycast.py loads it.  The scan is the
expected scan (slam_grid_raycast, 360 beams, 30 m) of a pose drawn from the free cells; --hyps hypotheses (74) start
from poses within +-0.15 m / +-0.03 rad of it, each with --rot rotations (11, 0.01 rad apart) x (2 * 4 + 1)^2 translations
of one cell: 74 x 891 = 65 934 candidates.  The score call gets those candidates as 65 934 poses.

Per operator: --warmup calls, then --iters rounds that alternate the two operators; per call the host clock around the
*_dev call and a synchronise of the context's stream, and in a second pass the library's own events on the launches
("finalize": packing the occupied bits, and for the matcher the field; "grid": the match / the trace).

Usage:  python tools/bench_match.py [--iters 15] [--warmup 3] [--hyps 74] [--out profiles/match_bench.json]
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
N = 360


def load_map(slam, torch, ctx, course, k):
    """The 200 x 200 course map with every cell k times in x and y, as a DeviceGrid of scale 10 k."""
    side = 200 * k
    g = slam.DeviceGrid(1, side, side, 10.0 * k, 10.0, 10.0, context=ctx)
    pm = np.kron(course.reshape(200, 200).T, np.ones((k, k), dtype=np.int8))      # [x][y]
    p, h = g.counters_torch()
    p.copy_(torch.from_numpy((pm == 0).astype(np.int32)).to(p.device).reshape(p.shape))
    h.copy_(torch.from_numpy((pm == 100).astype(np.int32)).to(p.device).reshape(p.shape))
    torch.cuda.synchronize()
    return g, pm


def stats(ms):
    return dict(ms_per_call=round(float(np.median(ms)), 4), ms_min=round(float(np.min(ms)), 4), ms_max=round(float(np.max(ms)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hyps", type=int, default=74)
    ap.add_argument("--rot", type=int, default=11)
    ap.add_argument("--window", type=int, default=4)
    ap.add_argument("--cap", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_bench.json"))
    a = ap.parse_args()
    import torch
    slam = importlib.import_module(PKG)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = slam.Context(0, torch.cuda.current_stream(dev).cuda_stream)
    course = np.load(os.path.join(ROOT, "tests", "golden", "g5_map_observation.npz"))["map_data"]
    g, pm = load_map(slam, torch, ctx, course, 2)
    scale, step, nx, K, B = 20.0, 1.0 / 20.0, a.window, a.rot, a.hyps
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    ct, st = slam._abi.trig_tables(AMIN, AMAX, N)
    rng = np.random.default_rng(11)
    free = np.argwhere(course.reshape(200, 200).T == 0)
    c = free[rng.integers(0, len(free))]
    true = np.array([(c[0] + 0.5) / 10.0 - 10.0, (c[1] + 0.5) / 10.0 - 10.0, rng.uniform(-np.pi, np.pi)])
    scan = slam.grid_raycast_host(g, true[None], ct, st, max_range=30.0)[0]
    scan = np.where(np.isfinite(scan), scan, np.inf).astype(np.float32)
    start = true + np.concatenate([[np.zeros(3)], rng.uniform(-1.0, 1.0, (B - 1, 3)) * np.array([0.15, 0.15, 0.03])])
    thetas, rot = slam.match_rotations(start[:, 2], K, 0.01)
    centres = np.ascontiguousarray(start[:, :2])
    # the same candidates as poses, in the matcher's flat order (k, i, j)
    off = (np.arange(2 * nx + 1) - nx).astype(np.float64) * step
    cand = np.empty((B, K, 2 * nx + 1, 2 * nx + 1, 3))
    cand[..., 0] = (centres[:, 0, None] + off[None, :])[:, None, :, None]
    cand[..., 1] = (centres[:, 1, None] + off[None, :])[:, None, None, :]
    cand[..., 2] = thetas[:, :, None, None]
    cand = cand.reshape(-1, 3)
    n_cand = cand.shape[0]

    d_scan, d_ctr, d_ct, d_st, d_rot, d_cand = up(scan), up(centres), up(ct), up(st), up(rot), up(cand)
    best = torch.empty(B, dtype=torch.int32, device=dev)
    cost = torch.empty(B, dtype=torch.int32, device=dev)
    used = torch.empty(B, dtype=torch.int32, device=dev)
    counts = torch.empty((n_cand, 7), dtype=torch.int32, device=dev)
    field = torch.empty((1, 400, 400), dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    ops = dict(
        match=lambda: g.match(d_scan, d_ctr, d_ct, d_st, d_rot, nx, nx, step, max_range=30.0, cap=a.cap, best_out=best, cost_out=cost,
                              used_out=used),
        score=lambda: g.score(d_scan, d_cand, d_ct, d_st, counts_out=counts),
        field=lambda: g.distance_field(a.cap, out=field))
    for _ in range(max(1, a.warmup)):
        for fn in ops.values():
            fn()
    ctx.synchronize()
    host = {k: [] for k in ops}
    for _ in range(a.iters):                          # alternating: both operators see the same neighbours on the machine
        for k, fn in ops.items():
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            host[k].append((time.perf_counter() - t0) * 1e3)
    events = {k: dict(grid=[], finalize=[]) for k in ops}
    ctx.timing_enable(True, only=["grid", "finalize"])
    for _ in range(a.iters):
        for k, fn in ops.items():
            fn()
            t = ctx.timing_read()
            events[k]["grid"].append(t["grid"][0])
            events[k]["finalize"].append(t["finalize"][0])
    ctx.timing_enable(False)

    res = dict(metric="candidates_per_s", map="course map 400 x 400, scale 20", beams=N, used_beams=int(used[0].item()), hypotheses=B,
               rotations=K, window=[2 * nx + 1, 2 * nx + 1], step=step, cap=a.cap, candidates=n_cand, iters=a.iters, warmup=a.warmup)
    for k in ops:
        r = stats(host[k])
        r["kernel_ms"] = {fam: stats(v) for fam, v in events[k].items()}
        r["kernel_ms_total"] = round(float(np.median(np.add(events[k]["grid"], events[k]["finalize"]))), 4)
        if k != "field":
            r["candidates_per_s"] = round(n_cand / r["ms_per_call"] * 1e3, 1)
        res[k] = r
    res["match_over_score_host_clock"] = round(res["match"]["ms_per_call"] / res["score"]["ms_per_call"], 4)
    res["match_over_score_kernels"] = round(res["match"]["kernel_ms_total"] / res["score"]["kernel_ms_total"], 4)
    # what the two say about the same candidates: the matcher's pose, and the candidate with the most hits
    hits = counts.cpu().numpy()[:, slam.RAY_HIT].reshape(B, -1)
    b_np, c_np = best.cpu().numpy(), cost.cpu().numpy()
    lead = int(np.argmin(c_np))
    pose = slam.match_pose(centres, thetas, b_np, nx, nx, step)
    res["true_pose"] = [round(float(v), 4) for v in true]
    res["match_best_pose"] = [round(float(v), 4) for v in pose[lead]]
    res["match_best_cost"] = int(c_np[lead])
    res["score_most_hits_pose"] = [round(float(v), 4) for v in cand[int(np.argmax(hits))]]
    res["score_most_hits"] = int(hits.max())
    res["timing"] = ("ms_per_call: host clock around the *_dev call + a synchronise of the context's stream, median / min / max of "
                     "--iters calls after --warmup, the operators alternating; kernel_ms: the library's own events on the launches of "
                     "--iters more calls, per family (finalize: occupied bits, row and column pass of the field; grid: match + unpack, "
                     "or the trace), kernel_ms_total their per-call sum's median")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
