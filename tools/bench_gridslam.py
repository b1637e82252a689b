#!/usr/bin/env python3
"""Time of a DeviceGridSLAM step and of each of its five parts on one MI355X.

Map: the course map (tests/golden/g5_map_observation.npz ``map_data``, 200 x 200 at 0.1 m) at 400 x 400, scale 20, as
tools/bench_mcl.py loads it, written into EVERY particle's map.  The scan is the expected scan (360 beams, 30 m) of a pose
drawn from the free cells; the particles lie within +-0.15 m / +-0.03 rad of it.  Shapes: F x P = 1 x 64, 16 x 64, 1 x 1 024.

Per shape, after --warmup rounds, --iters rounds that alternate the operators; per call the host clock around the *_dev
call(s) and a synchronise of the context's stream and of torch's (median, min - max):

    step                       DeviceGridSLAM.step
    weigh / resample / settle / copy / update    its five parts, each on the state one full step left behind
    copy_torch                 the yardstick of the copy: torch's device-to-device ``copy_`` of the SAME number of bytes between
                               the ``counters_torch()`` views (as many whole maps as the step's copy moved, pass and hit)
    gather_torch               what a user could do before: a torch gather of ALL F * P maps by ancestor into a second
                               buffer and a copy back (pass and hit) - the "second copy of the counters"

The ancestors of the timed copy are those of a real resample of the particles' weights (ess_frac = inf: it always
resamples).  bytes_per_s of the copy counts every byte read and written (2 x 8 bytes per cell of a copied map).

Usage:  python tools/bench_gridslam.py [--iters 15] [--warmup 3] [--out profiles/gridslam_bench.json]
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
SHAPES = ((1, 64), (16, 64), (1, 1024))
SIDE = 400


def stats(ms):
    return dict(ms_per_call=round(float(np.median(ms)), 4), ms_min=round(float(np.min(ms)), 4), ms_max=round(float(np.max(ms)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gridslam_bench.json"))
    a = ap.parse_args()
    import torch
    slam = importlib.import_module(PKG)
    abi = slam._abi
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = slam.Context(0)
    course = np.load(os.path.join(ROOT, "tests", "golden", "g5_map_observation.npz"))["map_data"]
    pm = np.kron(course.reshape(200, 200).T, np.ones((2, 2), dtype=np.int8))           # [x][y], 400 x 400
    ct, st = abi.trig_tables(AMIN, AMAX, N)
    rng = np.random.default_rng(11)
    free = np.argwhere(course.reshape(200, 200).T == 0)
    c = free[rng.integers(0, len(free))]
    true = np.array([(c[0] + 0.5) / 10.0 - 10.0, (c[1] + 0.5) / 10.0 - 10.0, rng.uniform(-np.pi, np.pi)])
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    one = slam.DeviceGrid(1, SIDE, SIDE, 20.0, 10.0, 10.0, context=ctx)
    p1, h1 = one.counters_torch()
    p1.copy_(up((pm == 0).astype(np.int32)).reshape(p1.shape))
    h1.copy_(up((pm == 100).astype(np.int32)).reshape(h1.shape))
    torch.cuda.synchronize()
    scan = slam.grid_raycast_host(one, true[None], ct, st, max_range=30.0)[0]
    scan = np.where(np.isfinite(scan), scan, np.inf).astype(np.float32)
    L, h = abi.lib(), ctx.handle
    res = dict(metric="ms_per_call", map="course map 400 x 400, scale 20, in every particle's map", beams=N, iters=a.iters, warmup=a.warmup,
               true_pose=[round(float(v), 4) for v in true], shapes={})
    for F, P in SHAPES:
        B = F * P
        d = slam.DeviceGridSLAM(F, P, SIDE, SIDE, 0.05, cos_t=ct, sin_t=st, context=ctx, ess_frac=float("inf"))
        gp, gh = d.grid.counters_torch()
        gp.copy_(p1.expand(B, SIDE, SIDE))
        gh.copy_(h1.expand(B, SIDE, SIDE))
        d.set_particles(true + rng.uniform(-1.0, 1.0, (F, P, 3)) * np.array([0.15, 0.15, 0.03]))
        ranges, motion = up(np.tile(scan, (F, 1))), up(np.zeros((F, 3)))
        noise, u0 = up(rng.normal(0.0, 1.0, (F, P, 3)) * np.array([0.005, 0.005, 0.002])), up(rng.uniform(0.0, 1.0, F))
        second_p, second_h = torch.empty_like(gp), torch.empty_like(gh)
        torch.cuda.synchronize()
        d.step(ranges, motion, noise, u0)                  # the state every part below is timed on: real ancestors, settled, map_src
        out = d.results()
        copied = int((out["copied"] == 1).sum())
        anc_flat = (torch.arange(F, device=dev)[:, None] * P + d.ancestors.long()).reshape(-1)
        spare = torch.empty((F, P, 3), dtype=torch.float64, device=dev)
        acc = d.acc.clone()
        g = d.grid._h
        p_ = abi.ptr

        def weigh():
            abi.check(L.slam_mcl_weigh_maps_dev(h, g, p_(d.poses), p_(motion), p_(noise), p_(ranges), p_(d.cos_t), p_(d.sin_t), None, F, P, N,
                                                30.0, d.cap, None, p_(acc), p_(d.cost), p_(d.used)))

        def resample():
            abi.check(L.slam_mcl_resample_dev(h, p_(d.poses), p_(acc), p_(d.table), d.T, 0, p_(u0), float("inf"), F, P, p_(spare),
                                              p_(d.ancestors), p_(d._est), p_(d._info)))

        def settle():
            abi.check(L.slam_mcl_settle_dev(h, p_(d.ancestors), p_(d.poses), F, P, 0, p_(d.settled), p_(spare), p_(d.map_src), p_(d._moved)))

        def copy():
            abi.check(L.slam_grid_copy_maps_dev(h, g, p_(d.map_src), 0, B, p_(d.copied)))

        def update():
            abi.check(L.slam_grid_update_particles_dev(h, g, p_(ranges), p_(d.cos_t), p_(d.sin_t), p_(d.poses), None, F, P, N, 0))

        def copy_torch():                                  # the same number of bytes, device to device, by torch
            if copied:
                second_p[:copied].copy_(gp[:copied])
                second_h[:copied].copy_(gh[:copied])

        def gather_torch():                                # every map by ancestor into a second buffer, and back
            torch.index_select(gp, 0, anc_flat, out=second_p)
            torch.index_select(gh, 0, anc_flat, out=second_h)
            gp.copy_(second_p)
            gh.copy_(second_h)

        ops = dict(step=lambda: d.step(ranges, motion, noise, u0), weigh=weigh, resample=resample, settle=settle, copy=copy, update=update,
                   copy_torch=copy_torch, gather_torch=gather_torch)
        keep_anc, keep_src = d.ancestors.clone(), d.map_src.clone()

        def before(k):
            if k == "resample":
                acc.zero_()
                weigh()
            if k in ("settle", "copy", "gather_torch"):    # a step in between has resampled again: the timed ancestors are the kept ones
                d.ancestors.copy_(keep_anc)
                d.map_src.copy_(keep_src)
        for _ in range(max(1, a.warmup)):
            for k, fn in ops.items():
                before(k)
                ctx.synchronize()
                torch.cuda.synchronize()
                fn()
        ctx.synchronize()
        host = {k: [] for k in ops}
        for _ in range(a.iters):
            for k, fn in ops.items():
                before(k)
                ctx.synchronize()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                ctx.synchronize()
                torch.cuda.synchronize()               # (the torch comparators run on torch's stream, not the context's)
                host[k].append((time.perf_counter() - t0) * 1e3)
        r = dict(F=F, P=P, maps=B, maps_copied=copied, moved=int(out["moved"].sum()))
        for k in ops:
            r[k] = stats(host[k])
        nbytes = copied * SIDE * SIDE * 4 * 2 * 2                              # pass and hit, read and written
        r["copy_bytes"] = nbytes
        for k in ("copy", "copy_torch"):
            r[k]["bytes_per_s"] = round(nbytes / (r[k]["ms_per_call"] * 1e-3), 1) if copied else 0.0
        r["gather_torch_bytes"] = B * SIDE * SIDE * 4 * 2 * 2 * 2
        r["copy_over_copy_torch"] = round(r["copy"]["ms_per_call"] / r["copy_torch"]["ms_per_call"], 4) if copied else None
        r["copy_over_gather_torch"] = round(r["copy"]["ms_per_call"] / r["gather_torch"]["ms_per_call"], 4)
        r["copy_bytes_over_gather_bytes"] = round(nbytes / r["gather_torch_bytes"], 4)
        res["shapes"]["%dx%d" % (F, P)] = r
        del d, gp, gh, second_p, second_h
        torch.cuda.empty_cache()
    res["timing"] = ("host clock around the call(s) + a synchronise of the context's stream and of torch's, median "
                     "/ min / max of --iters calls after --warmup, the operators alternating")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
