#!/usr/bin/env python3
"""Time of slam_grid_frontiers_dev on one MI355X beside the only route that existed before it: the queried pmaps copied
to the host (1), and that copy plus the NumPy / Python restatement tests/frontier_ref.py on them (2).

Shapes: the course map (tests/golden/g5_map_observation.npz ``map_data``, 200 x 200 at 0.1 m) at 400 x 400, scale 20,
B = 1; and a grid of 1 024 maps of 400 x 400 as DeviceGridSLAM keeps them - the first three 360-beam scans of the
synthetic room (make_replay(6, 360, seed=4)) integrated into every map from its true pose plus a jitter per particle, so
part of the room is explored and no two maps are alike - at B = 1 024 and at B = 1 of G = 1 024.  Each with the defaults
(radius 2, min_unknown 13, min_size 5, 256 rows) at min_clear2 = 0 and at min_clear2 = 4 (cap 64), which rebuilds the
field of all G maps.

Per operator: --warmup calls, then --iters rounds that alternate the operators; the host clock around the call and a
synchronise of the context's stream; in a second pass the library's own events per family ("finalize": the field;
"grid": the frontier kernels).  The copy of one map is ``slam_grid_read``; of many, ``slam_grid_finalize_dev`` into a
device buffer (the live pmap makes it a device copy) followed by one copy of the queried maps into page-locked host
memory.  The restatement runs on at most --ref-maps of the copied maps and is scaled to B.

Usage:  python tools/bench_frontiers.py [--iters 15] [--warmup 3] [--out profiles/frontier_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "a-2d-lidar-based-slam-system-for-wheeled-mobile-robots_amd"
AMIN, AMAX = -3.14159, 3.14159
SIDE, N, G = 400, 360, 1024


def stats(ms):
    return dict(ms_per_call=round(float(np.median(ms)), 4), ms_min=round(float(np.min(ms)), 4), ms_max=round(float(np.max(ms)), 4),
                calls=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--maps", type=int, default=G)
    ap.add_argument("--ref-maps", type=int, default=4)
    ap.add_argument("--only", default="", help="only the shapes whose name contains this (a kernel trace of one shape)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontier_bench.json"))
    a = ap.parse_args()
    import torch
    import frontier_ref as F
    slam = importlib.import_module(PKG)
    abi = slam._abi
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = slam.Context(0, torch.cuda.current_stream(dev).cuda_stream)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)

    # the course map, one map
    course = np.load(os.path.join(ROOT, "tests", "golden", "g5_map_observation.npz"))["map_data"]
    pm = np.kron(course.reshape(200, 200).T, np.ones((2, 2), dtype=np.int8))
    one = slam.DeviceGrid(1, SIDE, SIDE, 20.0, 10.0, 10.0, context=ctx)
    one.live_pmap()
    p1, h1 = one.counters_torch()
    p1.copy_(up((pm == 0).astype(np.int32)).reshape(p1.shape))
    h1.copy_(up((pm == 100).astype(np.int32)).reshape(h1.shape))
    # the particle maps
    rep = slam.synthetic.make_replay(6, N, seed=4)
    ct, st = abi.trig_tables(AMIN, AMAX, N)
    many = slam.DeviceGrid.metric(a.maps, SIDE, SIDE, 0.05, context=ctx)
    many.live_pmap()
    rng = np.random.default_rng(7)
    d_ct, d_st = up(ct), up(st)
    held = []
    for k in range(3):
        poses = np.asarray(rep.poses_true[k], dtype=np.float64) + rng.normal(0.0, 1.0, (1, a.maps, 3)) * np.array([0.05, 0.05, 0.01])
        held.append((up(np.asarray(rep.ranges[k], dtype=np.float32)[None]), up(poses)))
        torch.cuda.synchronize()
        many.update_particles(held[-1][0], d_ct, d_st, held[-1][1])
    ctx.synchronize()

    res = dict(metric="ms_per_call", iters=a.iters, warmup=a.warmup, defaults=dict(radius=2, min_unknown=13, min_size=5, max_clusters=256),
               shapes={})
    cases = (("course_400x400_B1", one, 1, None), ("particles_G%d_B%d" % (a.maps, a.maps), many, a.maps, None),
             ("particles_G%d_B1" % a.maps, many, 1, up(np.array([a.maps // 2], dtype=np.int32))))
    for name, g, B, maps in cases:
        if a.only and a.only not in name:
            continue
        outs = {c2: g.frontiers(maps, B=B, min_clear2=c2) for c2 in (0, 4)}
        ctx.synchronize()
        pmap_dev = torch.empty((g.G, SIDE, SIDE), dtype=torch.int8, device=dev)
        pinned = torch.empty((B, SIDE, SIDE), dtype=torch.int8).pin_memory()
        first = 0 if maps is None else int(maps[0].item())

        def copy():
            if B == 1:                                     # one map: slam_grid_read, the route Mapping itself takes
                pinned[0].copy_(torch.from_numpy(g.read(first)["pmap"]))
                return
            abi.check(abi.lib().slam_grid_finalize_dev(ctx.handle, g._h, abi.ptr(pmap_dev)))
            ctx.stream_order(torch.cuda.current_stream(dev).cuda_stream, 0)      # torch's copy waits for it, no host synchronise
            pinned.copy_(pmap_dev[first:first + B], non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()

        ops = dict(frontiers=lambda: g.frontiers(maps, B=B, min_clear2=0, out=outs[0]),
                   frontiers_clear4=lambda: g.frontiers(maps, B=B, min_clear2=4, out=outs[4]), copy_to_host=copy)
        for fn in ops.values():
            for _ in range(a.warmup):
                fn()
        ctx.synchronize()
        host = {k: [] for k in ops}
        for _ in range(a.iters):
            for k, fn in ops.items():
                ctx.synchronize()
                t0 = time.perf_counter()
                fn()
                ctx.synchronize()
                host[k].append((time.perf_counter() - t0) * 1e3)
        events = {k: dict(grid=[], finalize=[]) for k in ("frontiers", "frontiers_clear4")}
        ctx.timing_enable(True, only=["grid", "finalize"])
        for _ in range(5):
            for k in events:
                ops[k]()
                t = ctx.timing_read()
                events[k]["grid"].append(t["grid"][0])
                events[k]["finalize"].append(t["finalize"][0])
        ctx.timing_enable(False)
        # the restatement on the copied maps, scaled from --ref-maps of them
        copy()
        host_pm = pinned.numpy()
        n_ref = min(B, a.ref_maps)
        t0 = time.perf_counter()
        ref = [F.frontiers(host_pm[b]) for b in range(n_ref)]
        ref_ms = (time.perf_counter() - t0) * 1e3 * B / n_ref
        count = outs[0][0].cpu().numpy()
        r = dict(queries=B, maps=g.G, bytes_copied=int(B * SIDE * SIDE))
        for k in ops:
            r[k] = stats(host[k])
        for k in events:
            r[k]["kernel_ms"] = {fam: stats(v) for fam, v in events[k].items()}
        r["restatement_ms_scaled_from_%d_maps" % n_ref] = round(ref_ms, 1)
        r["copy_plus_restatement_ms"] = round(r["copy_to_host"]["ms_per_call"] + ref_ms, 1)
        r["copy_over_frontiers"] = round(r["copy_to_host"]["ms_per_call"] / r["frontiers"]["ms_per_call"], 2)
        r["copy_min_over_frontiers_max"] = round(r["copy_to_host"]["ms_min"] / r["frontiers"]["ms_max"], 2)   # outside the spread of both iff > 1
        r["device_equals_restatement"] = bool(all(np.array_equal(count[b], ref[b][0]) and np.array_equal(outs[0][1][b].cpu().numpy(), ref[b][1])
                                                  for b in range(n_ref)))
        r["kept_clusters_per_map"] = dict(median=float(np.median(count[:, 0])), min=int(count[:, 0].min()), max=int(count[:, 0].max()))
        r["frontier_cells_per_map"] = dict(median=float(np.median(count[:, 1])), min=int(count[:, 1].min()), max=int(count[:, 1].max()))
        c4 = outs[4][0].cpu().numpy()
        r["kept_clusters_per_map_clear4"] = dict(median=float(np.median(c4[:, 0])), min=int(c4[:, 0].min()), max=int(c4[:, 0].max()))
        res["shapes"][name] = r
        print(name, json.dumps(r), file=sys.stderr)
        del pmap_dev, pinned
    res["timing"] = ("ms_per_call: host clock around the call + a synchronise of the context's stream, median / min / max of `calls` calls "
                     "after the warm-up, the operators alternating; kernel_ms: the library's own events on the launches of five more "
                     "calls, per family (finalize: occupied bits and field of all G maps; grid: the nine frontier kernels).  copy_to_host: "
                     "slam_grid_finalize_dev of the grid (a device copy of the live pmap) and one copy of the queried maps into "
                     "page-locked memory; of one map, slam_grid_read.  Not measured here: per-kernel times (a kernel trace of --only one shape gives "
                     "them), hardware counters, other map sizes, the guard build")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
