#!/usr/bin/env python3
"""Time of slam_grid_locate_dev on one MI355X at H = 5 beside the two ways to answer the same question without the
pyramid: the call's own H = 0 (brute force through the same code), and slam_grid_match_dev tiled over the same
rotations and cells (before this operator the only route; its cost expression rounds every beam's end for every
candidate anew, where locate shifts the discretised scan by whole cells, so the two optima need not be the same cell).

Map: the course map (tests/golden/g5_map_observation.npz ``map_data``, 200 x 200 at 0.1 m) at 400 x 400, scale 20 -
every cell doubled - loaded through slam_grid_counters_dev, as tools/bench_match.py loads it.  Each of the B scans is
the expected scan (slam_grid_raycast, 360 beams, 30 m) of a pose drawn from the free cells.  K = 256 rotations over the
full circle, every cell of the map a candidate: 40 960 000 candidates per scan.  The tiled matcher takes a scan as 256
hypotheses of 25 x 25 cells (K * 625 candidates each, under its 2^24 bound) with a rotation table per hypothesis.

Per operator: --warmup calls, then --iters rounds that alternate the operators; per call the host clock around the
*_dev call and a synchronise of the context's stream, and in a second pass the library's own events on the launches
("finalize": occupied bits, field, pyramid; "grid": the search / the match).  An operator whose single call takes longer
than --slow-ms is measured with --slow-iters calls after one; the JSON says how many each got.

Usage:  python tools/bench_locate.py [--iters 15] [--warmup 3] [--batches 1,64] [--out profiles/locate_bench.json]
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
N, SIDE, TILE = 360, 400, 25


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
    return dict(ms_per_call=round(float(np.median(ms)), 4), ms_min=round(float(np.min(ms)), 4), ms_max=round(float(np.max(ms)), 4),
                calls=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--slow-ms", type=float, default=1500.0)
    ap.add_argument("--slow-iters", type=int, default=3)
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--rot", type=int, default=256)
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--cap", type=int, default=64)
    ap.add_argument("--ws-mb", type=float, default=0.0, help="context option locate_ws_mb (0: the default)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "locate_bench.json"))
    a = ap.parse_args()
    import torch
    slam = importlib.import_module(PKG)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = slam.Context(0, torch.cuda.current_stream(dev).cuda_stream)
    if a.ws_mb:
        ctx.set_option("locate_ws_mb", a.ws_mb)
    course = np.load(os.path.join(ROOT, "tests", "golden", "g5_map_observation.npz"))["map_data"]
    g, pm = load_map(slam, torch, ctx, course, 2)
    K, H = a.rot, a.levels
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    ct, st = slam._abi.trig_tables(AMIN, AMAX, N)
    thetas, rot = slam.locate_rotations(K)
    d_ct, d_st, d_rot = up(ct), up(st), up(rot)
    rng = np.random.default_rng(11)
    free = np.argwhere(course.reshape(200, 200).T == 0)
    # the tiles of the matcher: centres of the middle cells of 16 x 16 windows of 25 x 25 cells
    mid = (np.arange(SIDE // TILE) * TILE + TILE // 2 + 0.5) / 20.0 - 10.0
    tile_ctr = np.stack(np.meshgrid(mid, mid, indexing="ij"), axis=-1).reshape(-1, 2)
    T = tile_ctr.shape[0]

    res = dict(metric="ms_per_call", map="course map 400 x 400, scale 20", beams=N, rotations=K, levels=H, cap=a.cap,
               candidates_per_scan=K * SIDE * SIDE, iters=a.iters, warmup=a.warmup, batches={})
    for B in [int(v) for v in a.batches.split(",")]:
        cells = free[rng.integers(0, len(free), B)]
        true = np.stack([(cells[:, 0] + 0.5) / 10.0 - 10.0, (cells[:, 1] + 0.5) / 10.0 - 10.0, rng.uniform(-np.pi, np.pi, B)], axis=1)
        scans = slam.grid_raycast_host(g, true, ct, st, max_range=30.0)
        scans = np.where(np.isfinite(scans), scans, np.inf).astype(np.float32)
        d_scans = up(scans)
        out5 = [torch.empty((B, 3), dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
                torch.empty(B, dtype=torch.int32, device=dev), torch.empty((B, H + 2), dtype=torch.int64, device=dev)]
        out0 = [torch.empty_like(out5[0]), torch.empty_like(out5[1]), torch.empty_like(out5[2]),
                torch.empty((B, 2), dtype=torch.int64, device=dev)]
        # the matcher's batch: B * T hypotheses, scan b for its T tiles, the same K rotations for every one of them
        m_scans = d_scans.repeat_interleave(T, dim=0).contiguous()
        m_ctr = up(np.tile(tile_ctr, (B, 1)))
        m_rot = d_rot[None].expand(B * T, K, 2).contiguous()
        m_out = [torch.empty(B * T, dtype=torch.int32, device=dev) for _ in range(3)]
        torch.cuda.synchronize()

        def locate(h, out):
            return lambda: g.locate(d_scans, d_ct, d_st, d_rot, levels=h, max_range=30.0, cap=a.cap, best_out=out[0], cost_out=out[1],
                                    used_out=out[2], stats_out=out[3])
        ops = dict(locate=locate(H, out5), brute=locate(0, out0),
                   tiled_match=lambda: g.match(m_scans, m_ctr, d_ct, d_st, m_rot, TILE // 2, TILE // 2, 1.0 / 20.0, max_range=30.0, cap=a.cap,
                                               best_out=m_out[0], cost_out=m_out[1], used_out=m_out[2]))
        plan = {}
        for k, fn in ops.items():                      # one call each: builds the workspaces, and says which operators are slow
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            first = (time.perf_counter() - t0) * 1e3
            fn()
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            one = (time.perf_counter() - t0) * 1e3
            plan[k] = (1, a.slow_iters) if one > a.slow_ms else (a.warmup, a.iters)
            print("B=%d %s: first call %.2f ms, third %.2f ms -> %d calls after %d" % ((B, k, first, one) + plan[k][::-1]), file=sys.stderr)
        for k, fn in ops.items():
            for _ in range(plan[k][0]):
                fn()
        ctx.synchronize()
        host = {k: [] for k in ops}
        for it in range(a.iters):                      # alternating: the operators see the same neighbours on the machine
            for k, fn in ops.items():
                if it >= plan[k][1]:
                    continue
                ctx.synchronize()
                t0 = time.perf_counter()
                fn()
                ctx.synchronize()
                host[k].append((time.perf_counter() - t0) * 1e3)
        events = {k: dict(grid=[], finalize=[]) for k in ops}
        ctx.timing_enable(True, only=["grid", "finalize"])
        for it in range(a.iters):
            for k, fn in ops.items():
                if it >= min(plan[k][1], 5):
                    continue
                fn()
                t = ctx.timing_read()
                events[k]["grid"].append(t["grid"][0])
                events[k]["finalize"].append(t["finalize"][0])
        ctx.timing_enable(False)

        r = dict(hypotheses=B)
        for k in ops:
            r[k] = stats(host[k])
            r[k]["kernel_ms"] = {fam: stats(v) for fam, v in events[k].items()}
            r[k]["kernel_ms_total"] = round(float(np.median(np.add(events[k]["grid"], events[k]["finalize"]))), 4)
        for k in ("brute", "tiled_match"):
            r[k + "_over_locate_host_clock"] = round(r[k]["ms_per_call"] / r["locate"]["ms_per_call"], 2)
            r[k + "_over_locate_kernels"] = round(r[k]["kernel_ms_total"] / r["locate"]["kernel_ms_total"], 2)
            r[k + "_min_over_locate_max"] = round(r[k]["ms_min"] / r["locate"]["ms_max"], 2)     # outside the spread of both iff > 1
        b5, c5, u5, s5 = (t.cpu().numpy() for t in out5)
        b0, c0, u0, s0 = (t.cpu().numpy() for t in out0)
        r["locate_equals_brute"] = bool(np.array_equal(b5, b0) and np.array_equal(c5, c0) and np.array_equal(u5, u0))
        r["evaluated_nodes_per_level_median"] = [int(v) for v in np.median(s5[:, :H + 1], axis=0)]
        r["evaluated_nodes_median"] = int(np.median(s5[:, :H + 1].sum(axis=1)))
        r["evaluated_nodes_max"] = int(s5[:, :H + 1].sum(axis=1).max())
        r["evaluated_share_median"] = round(float(np.median(s5[:, :H + 1].sum(axis=1)) / (K * SIDE * SIDE)), 6)
        r["incumbent_over_cost_median"] = round(float(np.median(s5[:, H + 1] / np.maximum(c5, 1))), 3)
        pose = slam.locate_pose(b5, g.scale, g.off_x, g.off_y, rot)
        err = pose - true
        err[:, 2] = (err[:, 2] + np.pi) % (2 * np.pi) - np.pi
        ok = (np.abs(err[:, 0]) <= 0.05) & (np.abs(err[:, 1]) <= 0.05) & (np.abs(err[:, 2]) <= 2 * np.pi / K)
        r["scans_located_within_a_cell_and_a_rotation_step"] = int(ok.sum())
        r["used_beams_median"] = int(np.median(u5))
        # the tiled matcher's answer per scan: the cheapest tile's best candidate
        mc = m_out[1].cpu().numpy().reshape(B, T)
        mb = m_out[0].cpu().numpy().reshape(B, T)
        lead = np.argmin(mc, axis=1)
        mpose = np.stack([slam.match_pose(tile_ctr[lead[b]][None], thetas[None], mb[b, lead[b]][None], TILE // 2, TILE // 2, 1.0 / 20.0)[0]
                          for b in range(B)])
        r["tiled_match_same_cell_and_rotation"] = int(np.sum(np.all(np.abs(mpose - pose) < 1e-9, axis=1)))
        if B == 1:
            r["true_pose"] = [round(float(v), 4) for v in true[0]]
            r["locate_pose"] = [round(float(v), 4) for v in pose[0]]
            r["locate_cost"], r["locate_stats"] = int(c5[0]), [int(v) for v in s5[0]]
            r["tiled_match_pose"], r["tiled_match_cost"] = [round(float(v), 4) for v in mpose[0]], int(mc[0, lead[0]])
        res["batches"][str(B)] = r
        del m_scans, m_rot
    res["timing"] = ("ms_per_call: host clock around the *_dev call + a synchronise of the context's stream, median / min / max of `calls` "
                     "calls after the warm-up, the operators alternating; kernel_ms: the library's own events on the launches of up to "
                     "five more calls, per family (finalize: occupied bits, field, pyramid; grid: the search, or the match + unpack), "
                     "kernel_ms_total their per-call sum's median.  tiled_match scores slam_grid_match's expression, locate and brute "
                     "the discretised-scan cost anchored at the cell's centre: the same candidates, not the same numbers")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
