#!/usr/bin/env python3
"""Time of slam_grid_travel_dev on one MI355X beside the only routes that existed before it: (1) DeviceAStar over the same
(source, goal) pairs on the same pmaps - a different cost model (the reference planner's pmap convention, inflation and
f-ordering), so the times are set side by side and nothing is compared cell by cell; (2) the queried pmaps copied to the
host alone; (3) that copy plus the heap restatement tests/travel_ref.py on a few of them, scaled.

Shapes, as tools/bench_frontiers.py builds them: a grid of 1 024 maps of 400 x 400 as DeviceGridSLAM keeps them (the first
three 360-beam scans of the synthetic room integrated into every map from its true pose plus a jitter per particle) at
B = 1 024 - one source per map, the particle's own cell, foot 1 since three scans in place have turned that cell
occupied - and at B = 1 of G = 1 024; and the course map (tests/golden/g5_map_observation.npz at 400 x 400) at B = 1, from
the free cell that reaches most of it (of eight tried).  The goals are the representatives of slam_grid_frontiers at its defaults (256 rows with their -1
padding), passed device to device.  ``travel``: the goal outputs alone (no cost field leaves the workspace);
``travel_cost``: with cost_out [B, 400, 400] as well.

Per operator: --warmup calls, then --iters rounds that alternate the operators; the host clock around the call and a
synchronise of the context's stream; in a second pass the library's own events per family.  A* runs on at most
--astar-pairs of the pairs with a goal and is scaled to all of them.

Usage:  python tools/bench_travel.py [--iters 15] [--warmup 3] [--out profiles/travel_bench.json]
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
    ap.add_argument("--ref-maps", type=int, default=2)
    ap.add_argument("--astar-pairs", type=int, default=256)
    ap.add_argument("--only", default="", help="only the shapes whose name contains this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "travel_bench.json"))
    a = ap.parse_args()
    import torch
    import travel_ref as T
    slam = importlib.import_module(PKG)
    abi = slam._abi
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = slam.Context(0, torch.cuda.current_stream(dev).cuda_stream)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)

    # the course map, one map, from the free cell that reaches most of it
    course = np.load(os.path.join(ROOT, "tests", "golden", "g5_map_observation.npz"))["map_data"]
    pm = np.kron(course.reshape(200, 200).T, np.ones((2, 2), dtype=np.int8))
    one = slam.DeviceGrid(1, SIDE, SIDE, 20.0, 10.0, 10.0, context=ctx)
    one.live_pmap()
    p1, h1 = one.counters_torch()
    p1.copy_(up((pm == 0).astype(np.int32)).reshape(p1.shape))
    h1.copy_(up((pm == 100).astype(np.int32)).reshape(h1.shape))
    free = np.argwhere(pm == 0)
    tries = free[np.linspace(0, len(free) - 1, 8).astype(np.int64)]      # of eight free cells the one that reaches most of the map
    reach = [int((T.costs(T.traversable(pm, None, [c], 1, False, 0), [c]) >= 0).sum()) for c in tries]
    course_src = tries[int(np.argmax(reach))].astype(np.int32).reshape(1, 1, 2)
    # the particle maps, every source its particle's cell
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
    cells = np.stack([(many.scale * (poses[0, :, 0] + many.off_x)).astype(np.int64), (many.scale * (poses[0, :, 1] + many.off_y)).astype(np.int64)],
                     axis=-1).astype(np.int32).reshape(a.maps, 1, 2)

    res = dict(metric="ms_per_call", iters=a.iters, warmup=a.warmup, foot=1,
               frontier_defaults=dict(radius=2, min_unknown=13, min_size=5, max_clusters=256), shapes={})
    mid = a.maps // 2
    cases = (("particles_G%d_B%d" % (a.maps, a.maps), many, a.maps, None, cells),
             ("particles_G%d_B1" % a.maps, many, 1, up(np.array([mid], dtype=np.int32)), cells[mid:mid + 1]),
             ("course_400x400_B1", one, 1, None, course_src))
    for name, g, B, maps, src_h in cases:
        if a.only and a.only not in name:
            continue
        src = up(src_h)
        table = g.frontiers(maps, B=B)[1]
        ctx.synchronize()                                                  # torch's copy below runs on its own stream
        goals = table[:, :, 2:4].contiguous()
        torch.cuda.synchronize()
        new = lambda dtype, *shape: torch.empty(shape, dtype=dtype, device=dev)
        Q = int(goals.shape[1])
        out_goals = dict(status=new(torch.int32, B), goal_cost=new(torch.int32, B, Q), path_len=new(torch.int32, B, Q))
        out_cost = dict(out_goals, cost=new(torch.int32, B, SIDE, SIDE))
        pmap_dev = torch.empty((g.G, SIDE, SIDE), dtype=torch.int8, device=dev)
        pinned = torch.empty((B, SIDE, SIDE), dtype=torch.int8).pin_memory()
        first = 0 if maps is None else int(maps[0].item())

        def copy():
            if B == 1:                                     # one map: slam_grid_read, the route Mapping itself takes
                pinned[0].copy_(torch.from_numpy(g.read(first)["pmap"]))
                return
            abi.check(abi.lib().slam_grid_finalize_dev(ctx.handle, g._h, abi.ptr(pmap_dev)))
            ctx.stream_order(torch.cuda.current_stream(dev).cuda_stream, 0)
            pinned.copy_(pmap_dev[first:first + B], non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()

        ops = dict(travel=lambda: g.travel(src, maps, goals=goals, foot=1, cost=False, out=out_goals),
                   travel_cost=lambda: g.travel(src, maps, goals=goals, foot=1, out=out_cost), copy_to_host=copy)
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
        events = {k: dict(grid=[], finalize=[]) for k in ("travel", "travel_cost")}
        ctx.timing_enable(True, only=["grid", "finalize"])
        for _ in range(5):
            for k in events:
                ops[k]()
                t = ctx.timing_read()
                events[k]["grid"].append(t["grid"][0])
                events[k]["finalize"].append(t["finalize"][0])
        ctx.timing_enable(False)
        r = dict(queries=B, maps=g.G, goals_per_query=Q, bytes_copied=int(B * SIDE * SIDE))
        for k in ops:
            r[k] = stats(host[k])
        for k in events:
            r[k]["kernel_ms"] = {fam: stats(v) for fam, v in events[k].items()}
        status, gc = out_cost["status"].cpu().numpy(), out_cost["goal_cost"].cpu().numpy()
        g_h = goals.cpu().numpy()
        r["status_counts"] = {str(k): int(v) for k, v in zip(*np.unique(status, return_counts=True))}
        r["goals_with_a_cell"] = int((g_h[:, :, 0] >= 0).sum())
        r["goals_reached"] = int((gc >= 0).sum())
        r["cells_reached_per_map"] = dict(median=float(np.median((out_cost["cost"] >= 0).sum(dim=(1, 2)).cpu().numpy())))
        # (3) the restatement on the copied maps, scaled from --ref-maps of them
        copy()
        host_pm = pinned.numpy()
        n_ref = min(B, a.ref_maps)
        t0 = time.perf_counter()
        ref = [T.answer(host_pm[b], None, src_h[b], foot=1, goals=g_h[b]) for b in range(n_ref)]
        ref_ms = (time.perf_counter() - t0) * 1e3 * B / n_ref
        cost_h = out_cost["cost"][:n_ref].cpu().numpy()
        r["restatement_ms_scaled_from_%d_maps" % n_ref] = round(ref_ms, 1)
        r["copy_plus_restatement_ms"] = round(r["copy_to_host"]["ms_per_call"] + ref_ms, 1)
        r["device_equals_restatement"] = bool(all(np.array_equal(cost_h[b], ref[b]["cost"]) and np.array_equal(gc[b], ref[b]["goal_cost"])
                                                  for b in range(n_ref)))
        r["copy_over_travel"] = round(r["copy_to_host"]["ms_per_call"] / r["travel"]["ms_per_call"], 3)
        r["copy_min_over_travel_max"] = round(r["copy_to_host"]["ms_min"] / r["travel"]["ms_max"], 3)       # outside the spread of both iff > 1
        # (1) A* over the pairs that have a goal, at most --astar-pairs of them, scaled; (row, col) = (y, x)
        qb, qj = np.nonzero(g_h[:, :, 0] >= 0)
        if len(qb):
            take = np.linspace(0, len(qb) - 1, min(len(qb), a.astar_pairs)).astype(np.int64)
            starts = up(src_h[qb[take], 0][:, ::-1].astype(np.int32))
            ends = up(g_h[qb[take], qj[take]][:, ::-1].astype(np.int32))
            moq = up((qb[take] + first).astype(np.int32))
            planner = slam.DeviceAStar.from_grid(g)
            abi.check(abi.lib().slam_grid_finalize_dev(ctx.handle, g._h, abi.ptr(pmap_dev)))        # the live pmap is current
            run = lambda: planner.run(starts, ends, map_of_query=moq, path_cap=0)
            run()
            ctx.synchronize()
            ms = []
            for _ in range(max(a.iters // 3, 3)):
                ctx.synchronize()
                t0 = time.perf_counter()
                found = run()
                ctx.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
            r["astar"] = dict(stats(ms), pairs=len(take), pairs_in_all=len(qb),
                              ms_scaled_to_all_pairs=round(float(np.median(ms)) * len(qb) / len(take), 2),
                              status_counts={str(k): int(v) for k, v in zip(*np.unique(found["status"].cpu().numpy(), return_counts=True))})
        res["shapes"][name] = r
        print(name, json.dumps(r), file=sys.stderr)
        del pmap_dev, pinned, out_cost, out_goals
    res["timing"] = ("ms_per_call: host clock around the call + a synchronise of the context's stream, median / min / max of `calls` calls "
                     "after the warm-up, the operators alternating; kernel_ms: the library's own events on the launches of five more "
                     "calls, per family (grid: the four travel kernels; finalize: nothing at min_clear2 = 0).  copy_to_host: "
                     "slam_grid_finalize_dev of the grid and one copy of the queried maps into page-locked memory; of one map, "
                     "slam_grid_read.  astar: DeviceAStar.from_grid over (source, goal) pairs, another cost model - inflation of every map "
                     "of the grid is part of each call.  Not measured here: hardware counters, other tile sizes, the plain-sweep tile order, "
                     "one map across several workgroups, T or the field kept between calls")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
