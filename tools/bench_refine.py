#!/usr/bin/env python3
"""Time of slam_grid_refine_dev on one MI355X, with the field given and with the field rebuilt by the call, beside
slam_mcl_weigh_dev on the same poses: one field lookup a beam there against four lookups and about 40 float64 operations
a beam here, times iters + 1 evaluations.  There is no earlier route to compare with, so no pass mark on time.

Map: the course map (tests/golden/g5_map_observation.npz ``map_data``, 200 x 200 at 0.1 m) at 400 x 400, 0.05 m - every
cell doubled - loaded through slam_grid_counters_dev.  Scan: 360 beams over the full circle, the map's own ray cast
(slam_grid_raycast) from a free cell with the largest clearance, to 30 m; beams that meet nothing are unused.  Poses: that
cell's centre plus offsets of up to a cell in x and y and 0.01 rad in heading, B of them, one shared scan.  10 iterations,
damping 1e-3, steps of 0.5 cell and 0.02 rad, cap 64.
B in {1, 74, 4096, 65536}.  Per (B, form): host clock around the _dev call and a synchronise of the context's stream after
--warmup calls, median / min / max of --iters calls; then one more call under the library's own events: the field
("finalize" family) and the refinement or the weigh ("grid") apart.  The first poses are compared with the NumPy
restatement (tests/refine_ref.py), whose own time per pose is recorded.

Usage:  python tools/bench_refine.py [--iters 7] [--warmup 2] [--batches 1,74,4096,65536] [--out profiles/refine_bench.json]
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
N, ITERS, CAP, MAX_RANGE = 360, 10, 64, 30.0
ARGS = dict(iters=ITERS, damping=1e-3, step_cells=0.5, step_rad=0.02, max_range=MAX_RANGE, cap=CAP)


def timed(ctx, fn, warmup, iters):
    for _ in range(max(1, warmup)):
        fn()
    ms = []
    for _ in range(iters):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ctx.timing_enable(True, only=["grid", "finalize"])
    fn()
    ctx.synchronize()
    t = ctx.timing_read()
    ctx.timing_enable(False)
    return dict(ms_per_call=round(float(np.median(ms)), 4), ms_min=round(float(np.min(ms)), 4), ms_max=round(float(np.max(ms)), 4),
                kernel_ms=round(t["grid"][0], 4), field_kernel_ms=round(t["finalize"][0], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batches", default="1,74,4096,65536")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_bench.json"))
    a = ap.parse_args()
    import torch
    slam = importlib.import_module(PKG)
    import refine_ref as R
    from bench_gain import load_maps
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = slam.Context(0, torch.cuda.current_stream(dev).cuda_stream)
    course = np.load(os.path.join(ROOT, "tests", "golden", "g5_map_observation.npz"))["map_data"]
    g, pm = load_maps(slam, torch, ctx, course, 2, 1)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    ct, st = slam.view_tables(N)
    field = slam.grid_distance_field_host(g, CAP)
    free = (pm == 0) & (field[0] == CAP)
    if not free.any():
        free = pm == 0
    cells = np.argwhere(free)
    cell = cells[np.argmin(np.abs(cells - np.array(pm.shape) / 2.0).sum(axis=1))]           # the open free cell nearest the middle
    true = slam.view_poses(cell[None], g.scale, g.off_x, g.off_y)[0]
    scan = slam.grid_raycast_host(g, true[None], ct, st, max_range=MAX_RANGE)[0]
    rng = np.random.default_rng(0)
    d_ct, d_st, d_scan, d_field = up(ct), up(st), up(scan), up(field)

    res = dict(metric="poses_per_s", beams=N, used_beams=int(np.isfinite(scan).sum()), iterations=ITERS, cap=CAP, map="course map at 400 x 400, 0.05 m",
               true_pose=true.tolist(), legs=[])

    def starts(B):
        c = 1.0 / g.scale
        return true + np.stack([rng.uniform(-c, c, B), rng.uniform(-c, c, B), rng.uniform(-0.01, 0.01, B)], axis=1)

    # the NumPy restatement on the host, eight poses, and the device against it
    p8 = starts(8)
    t0 = time.perf_counter()
    ref = R.batch(R.refine, field, g.scale, g.off_x, g.off_y, scan, p8, ct, st, *[ARGS[k] for k in ("iters", "damping", "step_cells", "step_rad", "max_range", "cap")])
    res["numpy_restatement_ms_per_pose"] = round((time.perf_counter() - t0) * 1e3 / 8, 2)
    got = slam.grid_refine_host(g, scan, p8, ct, st, **ARGS)
    res["max_pose_deviation_from_numpy"] = float(np.max(np.abs(got[0] - ref["pose"])))
    res["cost_start_end_of_first_poses"] = got[1][:3].tolist()
    res["heading_error_start_end_mean"] = [float(np.mean(np.abs(p8[:, 2] - true[2]))), float(np.mean(np.abs(got[0][:, 2] - true[2])))]

    for B in [int(v) for v in a.batches.split(",") if v]:
        d_p = up(starts(B))
        out = (torch.empty((B, 3), dtype=torch.float64, device=dev), torch.empty((B, 2), dtype=torch.float64, device=dev),
               torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
               torch.empty((B, 9), dtype=torch.float64, device=dev))
        leg = dict(B=B, beam_evaluations=B * N * (ITERS + 1))
        torch.cuda.synchronize()
        for name, f in (("field_given", d_field), ("field_rebuilt", None)):
            t = timed(ctx, lambda: g.refine(d_scan, d_p, d_ct, d_st, field=f, out=out, **ARGS), a.warmup, a.iters)
            t["poses_per_s"] = round(B / t["ms_per_call"] * 1e3, 1)
            leg["refine_" + name] = t
        o = [x.cpu().numpy() for x in out]
        leg["ended_above_start"] = int((o[1][:, 1] > o[1][:, 0]).sum())
        # slam_mcl_weigh_dev: one filter of B particles at the same poses, no motion, the field given or rebuilt
        cost = torch.empty((1, B), dtype=torch.int32, device=dev)
        used = torch.empty(1, dtype=torch.int32, device=dev)
        lib, A = slam._abi.lib(), slam._abi
        for name, f in (("field_given", d_field), ("field_rebuilt", None)):
            call = lambda: A.check(lib.slam_mcl_weigh_dev(ctx.handle, g._h, d_p.data_ptr(), None, None, d_scan.data_ptr(), d_ct.data_ptr(),     # noqa: E731
                                                          d_st.data_ptr(), None, 1, B, N, MAX_RANGE, CAP, A.ptr(f), None, cost.data_ptr(), used.data_ptr()))
            leg["mcl_weigh_" + name] = timed(ctx, call, a.warmup, a.iters)
        leg["ratio_to_mcl_weigh_field_given"] = round(leg["refine_field_given"]["ms_per_call"] / leg["mcl_weigh_field_given"]["ms_per_call"], 3)
        leg["kernel_ratio_to_mcl_weigh"] = round(leg["refine_field_given"]["kernel_ms"] / max(leg["mcl_weigh_field_given"]["kernel_ms"], 1e-6), 3)
        res["legs"].append(leg)
        print(json.dumps(leg), flush=True)
    res["timing"] = ("host clock around the *_dev call + a synchronise of the context's stream, after --warmup calls, median / min / max of the "
                     "timed calls; kernel_ms / field_kernel_ms: the library's own events on the launches of one more call; mcl_weigh: "
                     "slam_mcl_weigh_dev, one filter of B particles at the same poses with the same scan; numpy_restatement: "
                     "tests/refine_ref.py refine(), one pose of 360 beams and 10 iterations")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
