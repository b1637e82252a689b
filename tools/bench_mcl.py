#!/usr/bin/env python3
"""Time of slam_mcl_weigh_dev / slam_mcl_resample_dev and of DeviceMCL.step on one MI355X, beside the only route the
library offered for a particle filter before them: slam_grid_match_dev over the same particles as hypotheses with
K = 1, nx = ny = 0 and a rotation table made on the host (one workgroup per particle), whose making and upload are
timed beside it.

Map: the course map (tests/golden/g5_map_observation.npz ``map_data``, 200 x 200 at 0.1 m) at 400 x 400, scale 20, as
tools/bench_match.py loads it.  The scan is the expected scan (slam_grid_raycast, 360 beams, 30 m) of a pose drawn
from the free cells; every filter reads it, and its particles lie within +-0.15 m / +-0.03 rad of that pose.  Shapes:
F x P = 1 x 65 536, 64 x 1 024, 4 096 x 16.

Per shape: --warmup calls of every operator, then --iters rounds that alternate them; per call the host clock around
the *_dev call(s) and a synchronise of the context's stream, and in a second pass the library's own events on the
launches ("finalize": occupied bits and the field; "grid": weigh / resample / match).  The weigh is timed with the
field rebuilt per call and with a field given (static map), the latter also in each launch shape (context option
"mcl_shape": 0 lanes over particles, 1 a wave per particle, -1 the library's choice); a last section times the two
shapes alone at --beams other beam counts.

Usage:  python tools/bench_mcl.py [--iters 15] [--warmup 3] [--out profiles/mcl_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
PKG = "a-2d-lidar-based-slam-system-for-wheeled-mobile-robots_amd"
AMIN, AMAX = -3.14159, 3.14159
N = 360
SHAPES = ((1, 65536), (64, 1024), (4096, 16))


def stats(ms):
    return dict(ms_per_call=round(float(np.median(ms)), 4), ms_min=round(float(np.min(ms)), 4), ms_max=round(float(np.max(ms)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cap", type=int, default=64)
    ap.add_argument("--beams", type=int, nargs="*", default=[16, 32, 64, 80, 96, 112, 128, 192, 360, 1080])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mcl_bench.json"))
    a = ap.parse_args()
    import torch
    from bench_match import load_map
    slam = importlib.import_module(PKG)
    abi = slam._abi
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = slam.Context(0, torch.cuda.current_stream(dev).cuda_stream)
    course = np.load(os.path.join(ROOT, "tests", "golden", "g5_map_observation.npz"))["map_data"]
    g, _ = load_map(slam, torch, ctx, course, 2)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    ct, st = abi.trig_tables(AMIN, AMAX, N)
    rng = np.random.default_rng(11)
    free = np.argwhere(course.reshape(200, 200).T == 0)
    c = free[rng.integers(0, len(free))]
    true = np.array([(c[0] + 0.5) / 10.0 - 10.0, (c[1] + 0.5) / 10.0 - 10.0, rng.uniform(-np.pi, np.pi)])
    scan = slam.grid_raycast_host(g, true[None], ct, st, max_range=30.0)[0]
    scan = np.where(np.isfinite(scan), scan, np.inf).astype(np.float32)
    table = slam.mcl_weight_table(2.0, 0, 4096)
    d_ct, d_st = up(ct), up(st)
    L, h = abi.lib(), ctx.handle

    res = dict(metric="ms_per_call", map="course map 400 x 400, scale 20", beams=N, used_beams=int(np.sum(scan < 30.0)), cap=a.cap,
               iters=a.iters, warmup=a.warmup, true_pose=[round(float(v), 4) for v in true], shapes={})
    for F, P in SHAPES:
        B = F * P
        poses = true + rng.uniform(-1.0, 1.0, (F, P, 3)) * np.array([0.15, 0.15, 0.03])
        d_poses, d_out = up(poses), torch.empty((F, P, 3), dtype=torch.float64, device=dev)
        d_ranges = up(np.tile(scan, (F, 1)))
        new = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
        acc, acc0, cost, used, anc, info = new(F, P), new(F, P), new(F, P), new(F), new(F, P), new(F, 4)
        est = torch.empty((F, 4), dtype=torch.float64, device=dev)
        d_table, d_u0 = up(table.view(np.int32)), up(rng.uniform(0.0, 1.0, F))
        field = g.distance_field(a.cap)
        # the route through the matcher: every particle a hypothesis with one rotation of its own and a 1 x 1 window
        d_ctr = up(poses.reshape(B, 3)[:, :2])
        d_scans = up(scan) if F == 1 else up(np.tile(scan, (B, 1)))
        rot_host = lambda: np.ascontiguousarray(np.stack([np.cos(poses[..., 2]), np.sin(poses[..., 2])], axis=-1).reshape(B, 1, 2))
        d_rot = up(rot_host())
        best, bcost, bused = new(B), new(B), new(B)
        mcl = {s: slam.DeviceMCL(g, F, P, cos_t=ct, sin_t=st, cap=a.cap, table=table, ess_frac=0.5, static_map=s) for s in (False, True)}
        for m in mcl.values():
            m.set_particles(poses)
        zero_motion, d_noise = up(np.zeros((F, 3))), up(rng.normal(0.0, 1.0, (F, P, 3)) * np.array([0.005, 0.005, 0.002]))
        torch.cuda.synchronize()

        def weigh(fld, shape=-1, acc_buf=None):
            ctx.set_option("mcl_shape", shape)
            abi.check(L.slam_mcl_weigh_dev(h, g._h, abi.ptr(d_poses), None, None, abi.ptr(d_ranges), abi.ptr(d_ct), abi.ptr(d_st), None, F, P,
                                           N, 30.0, a.cap, abi.ptr(fld), abi.ptr(acc_buf), abi.ptr(cost), abi.ptr(used)))
            ctx.set_option("mcl_shape", -1)

        def resample():
            abi.check(L.slam_mcl_resample_dev(h, abi.ptr(d_poses), abi.ptr(acc), abi.ptr(d_table), 4096, 0, abi.ptr(d_u0), float("inf"),
                                              F, P, abi.ptr(d_out), abi.ptr(anc), abi.ptr(est), abi.ptr(info)))

        def rot_upload():
            d_rot.copy_(torch.from_numpy(rot_host()))

        ops = dict(
            weigh_rebuild=lambda: weigh(None, -1),
            weigh_static=lambda: weigh(field, -1),
            weigh_static_lanes=lambda: weigh(field, 0),
            weigh_static_wave=lambda: weigh(field, 1),
            resample=resample,
            step_rebuild=lambda: mcl[False].step(d_ranges, zero_motion, d_noise, d_u0),
            step_static=lambda: mcl[True].step(d_ranges, zero_motion, d_noise, d_u0),
            match_route=lambda: g.match(d_scans, d_ctr, d_ct, d_st, d_rot, 0, 0, 0.05, max_range=30.0, cap=a.cap, best_out=best,
                                        cost_out=bcost, used_out=bused),
            match_route_table=rot_upload)
        acc0.zero_()
        weigh(field, -1, acc0)                         # the accumulated costs every timed resample starts from
        ctx.synchronize()
        # (the device's cos / sin against NumPy's in the table: a particle may differ where one ulp moves a beam across a cell edge)
        ctx.synchronize()
        torch.cuda.synchronize()
        via_match = g.match(d_scans, d_ctr, d_ct, d_st, d_rot, 0, 0, 0.05, max_range=30.0, cap=a.cap)[1]
        ctx.synchronize()
        differ = int((cost.reshape(-1) != via_match).sum().item())

        def before(k):
            if k == "resample":
                acc.copy_(acc0)
        for _ in range(max(1, a.warmup)):
            for k, fn in ops.items():
                before(k)
                fn()
        ctx.synchronize()
        host = {k: [] for k in ops}
        for _ in range(a.iters):                      # alternating: every operator sees the same neighbours on the machine
            for k, fn in ops.items():
                before(k)
                ctx.synchronize()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                ctx.synchronize()
                host[k].append((time.perf_counter() - t0) * 1e3)
        events = {k: dict(grid=[], finalize=[]) for k in ops if k != "match_route_table"}
        ctx.timing_enable(True, only=["grid", "finalize"])
        for _ in range(a.iters):
            for k in events:
                before(k)
                torch.cuda.synchronize()
                ops[k]()
                t = ctx.timing_read()
                events[k]["grid"].append(t["grid"][0])
                events[k]["finalize"].append(t["finalize"][0])
        ctx.timing_enable(False)
        r = dict(F=F, P=P, particles=B, weigh_costs_differing_from_match=differ, resampled_filters=int(info[:, 2].sum().item()))
        for k in ops:
            r[k] = stats(host[k])
            if k in events:
                r[k]["kernel_ms"] = {fam: stats(v) for fam, v in events[k].items()}
                r[k]["kernel_ms_total"] = round(float(np.median(np.add(events[k]["grid"], events[k]["finalize"]))), 4)
        r["weigh_over_match_host_clock"] = round(r["weigh_rebuild"]["ms_per_call"] / r["match_route"]["ms_per_call"], 4)
        r["weigh_over_match_kernels"] = round(r["weigh_rebuild"]["kernel_ms_total"] / r["match_route"]["kernel_ms_total"], 4)
        r["weigh_wave_over_lanes_kernels"] = round(r["weigh_static_wave"]["kernel_ms_total"] / r["weigh_static_lanes"]["kernel_ms_total"], 4)
        res["shapes"]["%dx%d" % (F, P)] = r
        del mcl
    # the two launch shapes of the weigh at other beam counts (a field given, the library's events): what the automatic choice rests on
    res["shape_by_beams"] = {}
    for F, P in (SHAPES[0], SHAPES[2]):
        poses = true + rng.uniform(-1.0, 1.0, (F, P, 3)) * np.array([0.15, 0.15, 0.03])
        d_poses, cost = up(poses), torch.empty((F, P), dtype=torch.int32, device=dev)
        field = g.distance_field(a.cap)
        row = {}
        for n in a.beams:
            ctn, stn = abi.trig_tables(AMIN, AMAX, n)
            sc = slam.grid_raycast_host(g, true[None], ctn, stn, max_range=30.0)[0]
            sc = np.where(np.isfinite(sc), sc, np.inf).astype(np.float32)
            d_r, d_c, d_s = up(np.tile(sc, (F, 1))), up(ctn), up(stn)
            torch.cuda.synchronize()
            ms = {}
            for shape, name in ((0, "lanes"), (1, "wave")):
                ctx.set_option("mcl_shape", shape)
                call = lambda: abi.check(L.slam_mcl_weigh_dev(h, g._h, abi.ptr(d_poses), None, None, abi.ptr(d_r), abi.ptr(d_c), abi.ptr(d_s),
                                                               None, F, P, n, 30.0, a.cap, abi.ptr(field), None, abi.ptr(cost), None))
                for _ in range(max(1, a.warmup)):
                    call()
                ctx.timing_enable(True, only=["grid"])
                t = []
                for _ in range(a.iters):
                    call()
                    t.append(ctx.timing_read()["grid"][0])
                ctx.timing_enable(False)
                ms[name] = stats(t)
            ctx.set_option("mcl_shape", -1)
            ms["wave_over_lanes"] = round(ms["wave"]["ms_per_call"] / ms["lanes"]["ms_per_call"], 4)
            row[str(n)] = ms
        res["shape_by_beams"]["%dx%d" % (F, P)] = row
    res["timing"] = ("ms_per_call: host clock around the *_dev call(s) + a synchronise of the context's stream, median / min / max of --iters "
                     "calls after --warmup, the operators alternating; kernel_ms: the library's own events on the launches of --iters more "
                     "calls, per family (finalize: occupied bits and the field; grid: weigh / resample / match), kernel_ms_total their "
                     "per-call sum's median.  weigh_rebuild and match_route both rebuild the field; match_route_table is the host making "
                     "of the rotation table (numpy cos / sin) and its upload, which the match route needs per step and the weigh does not")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
