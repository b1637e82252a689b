"""The planners, the map ray cast and the landmark extraction - A* inflation, A* search, DWA, slam_grid_raycast /
slam_grid_scan_score, slam_landmarks - over the seeded cases of tests/plan_cases.py, against the restatements under tests/
(the landmarks against the package's host class Extraction), through the C ABI's host forms; every third seed also
through the device form on torch tensors, two calls back to back without a synchronise in between.

Inflated maps, statuses, expansions, path lengths and paths, ray cells, classes and tallies, labels, ids and counts are
exact; ranges equal as float32 bits; the DWA follows check_against_oracle of tests/test_gpu_dwa.py, whose latitude (a
collision margin or two best costs within 1e-12) is granted only to planners that the restatement itself marks
(plan_cases.dwa_marked; tests/test_plan_cases.py caps them at 1 %) and never to a planner whose costs tie exactly.  The
search, the DWA and the ray cast also run their batch reversed and its first entry alone: the same rows.
tests/test_plan_cases.py asserts, without a device, which edges these cases reach.  A failure names (kind, seed):
plan_cases.case_of(kind, seed) rebuilds the case."""
import time

import numpy as np
import pytest

import astar_ref as A
import plan_cases as P
from conftest import pkg
from mcl_checks import same_bits
from test_gpu_dwa import check_against_oracle
from test_gpu_landmark_bounds import check_scans
from test_gpu_map_properties import counters, device_form, named, option, tag, untouched, up
from test_gpu_raycast_bounds import check as check_rays
from test_gpu_raycast_bounds import grid_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def slam():
    p = pkg()
    p._abi.default_context()   # fails loudly when there is no gfx950 device
    return p


@pytest.fixture(scope="module")
def ctx(slam):
    c = slam.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _clock(request):
    t = time.perf_counter()
    yield
    print("%s: %.1f s over %d seeds" % (request.node.name, time.perf_counter() - t, len(P.seeds())))


def host(o):
    return {k: v.cpu().numpy() for k, v in o.items()}


# ------------------------------------------------------------------ A* inflation
def test_inflate(slam, ctx):
    import torch
    for seed in P.seeds():
        c = P.case_of("inflate", seed)
        with named(c):
            want = P.answer(c)
            got = slam.inflate_host(c["maps"], span=c["span"], r=c["r"], wire_layout=c["wire"], ctx=ctx)
            assert got.dtype == np.int8 and got.shape == want.shape, tag(c)
            assert np.array_equal(got, want), tag(c) + (np.argwhere(got != want)[:4].tolist(),)
            if device_form(c):
                da = slam.DeviceAStar(c["H"], c["W"], G=c["G"], wire_layout=c["wire"], span=c["span"], r=c["r"], ctx=ctx)
                maps = up(c["maps"], ctx)
                torch.cuda.synchronize()
                o1 = da.inflate(maps)
                o2 = da.inflate(maps)
                ctx.synchronize()
                assert np.array_equal(o1.cpu().numpy(), want) and np.array_equal(o2.cpu().numpy(), want), tag(c) + ("device form",)
    ctx.check_status()


# ------------------------------------------------------------------ A* search
def check_search(c, o, plans, unique, bad=None, what="host form"):
    """The rows of ``o`` against the restatement's answer for each row's unique query; ``bad``: rows whose map_of_query
    entry names no map (BAD_MAP, nothing searched)."""
    B = len(unique)
    bad = np.zeros(B, dtype=bool) if bad is None else bad
    status = np.where(bad, A.BAD_MAP, np.array([p["status"] for p in plans])[unique])
    length = np.where(bad, 0, np.array([p["length"] for p in plans])[unique])
    closed = np.where(bad, 0, np.array([p["expansions"] for p in plans])[unique])
    for name, a, b in (("status", o["status"], status), ("path_len", o["path_len"], length), ("expansions", o["expansions"], closed)):
        assert a.dtype == np.int32 and a.shape == (B,), tag(c) + (what, name)
        assert np.array_equal(a, b), tag(c) + (what, name, np.flatnonzero(a != b)[:4].tolist())
    for u, p in enumerate(plans):                                      # every copy of a query: the one path, up to the capacity
        n = min(c["path_cap"], p["length"])
        rows = np.flatnonzero((unique == u) & ~bad)
        if n and len(rows):
            same = np.all(o["path"][rows, :n] == p["path"][:n][None], axis=(1, 2))
            assert np.all(same), tag(c) + (what, "path", u, rows[~same][:4].tolist())


def test_astar(slam, ctx):
    import torch
    for seed in P.seeds():
        c = P.case_of("astar", seed)
        with named(c):
            imaps, plans = P.answer(c)
            s, g, moq, unique = P.astar_batch(c)
            kw = dict(span=c["span"], r=c["r"], wire_layout=c["wire"], path_cap=c["path_cap"], ctx=ctx)
            got = slam.astar_host(c["maps"], s, g, map_of_query=moq, want_inflated=True, **kw)
            assert np.array_equal(got["inflated"], imaps), tag(c) + ("inflated",)
            check_search(c, got, plans, unique)
            # batch invariance: reversed (every query in another slot, after another query), and the first query alone
            for name, sel in (("reversed", slice(None, None, -1)), ("alone", slice(0, 1))):
                part = slam.astar_host(c["maps"], s[sel], g[sel], map_of_query=moq[sel], **kw)
                for k in ("status", "path_len", "expansions"):
                    assert np.array_equal(part[k], got[k][sel]), tag(c) + (name, k)
                written = np.arange(c["path_cap"])[None, :] < part["path_len"][:, None]      # cells past a path are not written
                assert np.array_equal(part["path"][written], got["path"][sel][written]), tag(c) + (name, "path")
            if device_form(c):
                da = slam.DeviceAStar(c["H"], c["W"], G=c["G"], wire_layout=c["wire"], span=c["span"], r=c["r"], ctx=ctx)
                q_bad = moq.copy()                                    # entries outside [0, G): the host form rejects them
                q_bad[::7], q_bad[3::11] = -1, c["G"]
                bad = (q_bad < 0) | (q_bad >= c["G"])
                maps, ts, tg, tq, tb = (up(a, ctx) for a in (c["maps"], s, g, moq, q_bad))
                torch.cuda.synchronize()
                o1 = da.run(ts, tg, maps=maps, map_of_query=tb, path_cap=c["path_cap"], want_inflated=True)
                o2 = da.run(ts, tg, maps=maps, map_of_query=tq, path_cap=c["path_cap"])
                ctx.synchronize()
                o1, o2 = host(o1), host(o2)
                assert np.array_equal(o1["inflated"], imaps), tag(c) + ("device form", "inflated")
                check_search(c, o1, plans, unique, bad, "device form, entries that name no map")
                check_search(c, o2, plans, unique, None, "device form")
                with pytest.raises(slam.SlamError):
                    slam.astar_host(c["maps"], s, g, map_of_query=q_bad, **kw)
    ctx.check_status()


# ------------------------------------------------------------------ DWA
DWA_KEYS = ("u", "cost", "index", "counts", "traj")


def dwa_same(a, b):
    """None, or the output in which two runs of the same planners differ in their bits; a planner's costs row is written
    up to its own window."""
    for k in DWA_KEYS:
        if not same_bits(a[k], np.ascontiguousarray(b[k])):
            return k
    used = np.arange(a["costs"].shape[1])[None, :] < (a["counts"][:, 0] * a["counts"][:, 1])[:, None]
    return None if same_bits(a["costs"][used], b["costs"][used]) else "costs"


def dwa_host(slam, ctx, c, sel=slice(None)):
    return slam.dwa_batch_host(c["states"][sel], c["goals"][sel], c["cfg"], ob=c["ob"][sel], counts=c["counts"][sel], want_costs=True,
                               want_traj=True, ctx=ctx)


def test_dwa(slam, ctx):
    import torch
    for seed in P.seeds():
        c = P.case_of("dwa", seed)
        with named(c):
            plans = P.answer(c)
            r = dwa_host(slam, ctx, c)
            for b, plan in enumerate(plans):
                x = c["states"][b]
                if plan is None:                                       # a v or omega that is not finite plans an empty window
                    assert tuple(r["counts"][b]) == (0, 0) and r["index"][b] == -1 and np.isposinf(r["cost"][b]), tag(c) + (b,)
                    assert np.array_equal(r["u"][b], [0.0, 0.0]), tag(c) + (b,)
                    continue
                want = check_against_oracle(r, b, x, c["cfg"], c["goals"][b], c["ob"][b, :c["counts"][b]])
                S = want["nv"] * want["nw"]
                differs = r["index"][b] != want["index"] or not np.array_equal(np.isinf(r["costs"][b, :S]), np.isinf(want["costs"]))
                if differs:                                            # that latitude is a condition: the restatement must have marked it
                    assert P.dwa_marked(c, b, plan), tag(c) + (b, "differs on a planner the restatement is sure of", int(r["index"][b]), want["index"])
                elif want["index"] >= 0:
                    assert same_bits(r["cost"][b], r["costs"][b, want["index"]]), tag(c) + (b,)
                    assert np.max(np.abs(r["traj"][b] - want["traj"])) < 1e-12, tag(c) + (b, "traj")
                else:
                    assert np.isposinf(r["cost"][b]) and same_bits(r["traj"][b, 0], x) and np.all(np.isnan(r["traj"][b, 1:])), tag(c) + (b,)
            for name, sel in (("reversed", slice(None, None, -1)), ("alone", slice(0, 1))):
                differs = dwa_same(dwa_host(slam, ctx, c, sel), {k: v[sel] for k, v in r.items()})
                assert differs is None, tag(c) + (name, differs)
            if device_form(c):
                dd = slam.DeviceDWA(c["cfg"], ctx=ctx)
                st, go, cn = up(c["states"], ctx), up(c["goals"], ctx), up(c["counts"], ctx)
                soa = up(np.swapaxes(c["ob"], 1, 2), ctx)
                torch.cuda.synchronize()
                o1 = dd.run(st, go, soa, counts=cn, want_costs=True, want_traj=True)
                o2 = dd.run(st, go, soa, counts=cn, want_costs=True, want_traj=True)
                ctx.synchronize()
                for o in (host(o1), host(o2)):
                    differs = dwa_same(o, r)
                    assert differs is None, tag(c) + ("device form", differs)
    ctx.check_status()


# ------------------------------------------------------------------ the map ray cast
def rays_host(slam, g, c, sel=slice(None), gob=None):
    gob = c["gob"] if gob is None else gob
    scan = c["scan"] if c["scan"].ndim == 1 else np.ascontiguousarray(c["scan"][sel])
    poses, gob = np.ascontiguousarray(c["poses"][sel]), np.ascontiguousarray(gob[sel])
    r, cells = slam.grid_raycast_host(g, poses, c["ct"], c["st"], max_range=c["max_range"], skip=c["skip"], grid_of_batch=gob, return_cells=True)
    counts, cls = slam.grid_score_host(g, scan, poses, c["ct"], c["st"], skip=c["skip"], grid_of_batch=gob, return_classes=True)
    return r, cells, counts, cls


def test_raycast(slam, ctx):
    import torch
    for seed in P.seeds():
        c = P.case_of("raycast", seed)
        with named(c):
            want = P.answer(c)
            g = grid_of(slam, ctx, c)                                  # (asserts the device's pmaps equal to NumPy's)
            before = counters(g)
            engines = []
            for lds in (0, 1):                                         # mask words from global memory, and from LDS
                with option(ctx, "raycast_lds", lds, -1):
                    engines.append(rays_host(slam, g, c))
                check_rays(engines[-1], want, "%s, raycast_lds %d" % (tag(c), lds))
            for a, b in zip(*engines):
                assert same_bits(a, b), tag(c) + ("the two engines differ",)
            got = engines[0]
            for name, sel in (("reversed", slice(None, None, -1)), ("alone", slice(0, 1))):
                for a, b in zip(rays_host(slam, g, c, sel), got):
                    assert same_bits(a, b[sel]), tag(c) + (name,)
            if device_form(c):
                want_bad = P.raycast_answer(c, c["gob_bad"])
                d = dict(poses=up(c["poses"], ctx), cos_t=up(c["ct"], ctx), sin_t=up(c["st"], ctx), skip=c["skip"])
                scan, good, bad = up(c["scan"], ctx), up(c["gob"], ctx), up(c["gob_bad"], ctx)
                torch.cuda.synchronize()
                s1 = g.score(scan, grid_of_batch=bad, return_classes=True, **d)
                r1 = g.raycast(max_range=c["max_range"], grid_of_batch=bad, return_cells=True, **d)
                r2 = g.raycast(max_range=c["max_range"], grid_of_batch=good, return_cells=True, **d)
                s2 = g.score(scan, grid_of_batch=good, return_classes=True, **d)
                ctx.synchronize()
                check_rays(tuple(t.cpu().numpy() for t in r1 + s1), want_bad, "%s, device form, entries that name no map" % (tag(c),))
                for a, b in zip(r2 + s2, got):
                    assert same_bits(a.cpu().numpy(), b), tag(c) + ("device form",)
            untouched(g, before, c)
            g.close()
    ctx.set_option("raycast_lds", -1)
    ctx.check_status()


# ------------------------------------------------------------------ landmark extraction
LM_KEYS = ("count", "overflow", "ids", "means", "z", "labels")


def landmarks_dev(slam, ctx, c):
    """slam_landmarks_dev twice back to back; the outputs of both."""
    import torch
    abi = pkg("_abi")
    S, n, cap = c["S"], c["n"], c["lm_cap"]
    dev = torch.device("cuda", ctx.device)
    ct, st = abi.trig_tables(c["amin"], c["amax"], n)
    r, dct, dst = up(c["ranges"], ctx), up(ct, ctx), up(st, ctx)
    i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
    runs = [dict(count=torch.full((S,), -9, **i32), overflow=torch.full((S,), -9, **i32), ids=torch.full((S, cap), -9, **i32),
                 means=torch.full((S, cap, 2), -9.0, **f64), z=torch.full((S, cap, 2), -9.0, **f64), labels=torch.full((S, n - 1), -9, **i32))
            for _ in range(2)]
    torch.cuda.synchronize()
    for o in runs:
        abi.check(abi.lib().slam_landmarks_dev(ctx.handle, abi.ptr(r), abi.ptr(dct), abi.ptr(dst), S, n, c["rt"], c["rm"], cap, abi.ptr(o["count"]),
                                               abi.ptr(o["overflow"]), abi.ptr(o["ids"]), abi.ptr(o["means"]), abi.ptr(o["z"]), abi.ptr(o["labels"])))
    ctx.synchronize()
    return [host(o) for o in runs]


def test_landmarks(slam, ctx):
    for seed in P.seeds():
        c = P.case_of("landmarks", seed)
        with named(c):
            out = check_scans(slam, c["ranges"], c["amin"], c["amax"], lm_cap=c["lm_cap"], rt=c["rt"], rm=c["rm"])
            if device_form(c):
                for o in landmarks_dev(slam, ctx, c):
                    for k in LM_KEYS:
                        assert same_bits(o[k], out[k]), tag(c) + ("device form", k)
    ctx.check_status()
    slam._abi.default_context().check_status()
