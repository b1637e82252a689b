"""Seeded cases of slam_grid_refine for the sweeps (tests/test_refine_cases.py on the host, tests/test_gpu_refine.py on
the device).

    case_of('refine', seed)     dict: pmaps int8 [G, xw, yw], fields int16 [G, xw, yw] (tests/match_ref.py at the case's cap),
                                scale, off_x, off_y, ranges float32 [n] or [B, n], poses [B, 3], maps int32 [B] (an entry
                                may name no map), ct / st [n], iters, damping, step_cells, step_rad, max_range, cap
    answer(case, fn)            tests/refine_ref.py's batch with fn = R.refine (NumPy) or R.refine_mp (50 digits)
    answer_mp(seed)             the 50-digit answer of a default case, computed once per process
    sure(ans)                   every u, v of every evaluation of the 50-digit run stayed SURE_MARGIN from an integer
    deviation(got, want)        (pose, cost, normal): the largest absolute pose deviation and the largest relative cost
                                and normal deviations of the answered hypotheses
    edges_of(case, ans)         the names of the edges the case reaches
    seeds()                     range(SLAM_HYP_EXAMPLES), default 60

Up to five hypotheses routed over up to three maps of one of four shapes under two index rules; random walls, and now and
then a map with nothing occupied; scans of random ranges that reach from a few cells to beyond the map, with non-finite and
over-range entries, now and then a scan with no used beam; now and then a start that is not finite.

Tolerance (the issue's rule).  E is the largest deviation of the NumPy restatement from the 50-digit one over the sure
default cases: absolute for poses, relative (to the largest magnitude of the hypothesis's costs, or of its normal entries)
for costs and normals.  The device may deviate from the 50-digit answer by 16 E - its sums run in another order and its
cos / sin may differ from libm's in the last place, each an error of the size of NumPy's own - and never by more than the
project's 1e-9 for poses.  Measured over the 60 default seeds (tests/test_refine_cases.py prints them):
    E_POSE 2.31e-13   E_COST 6.13e-15   E_NORMAL 8.26e-14      (16 E_POSE = 3.7e-12, well inside 1e-9)
The constants below are those figures rounded up to two digits."""
import functools
import os

import numpy as np

import match_ref as MR
import refine_ref as R

SHAPES = ((8, 8), (33, 17), (64, 64), (40, 65))
RULES = ((1.0, 0.0, 0.0), (10.0, 2.0, 3.0))            # (scale, off_x, off_y)
ITERS = (0, 1, 3, 10)
BEAMS = (1, 63, 64, 65, 360)
EDGES = ("an entry that names no map", "a map used twice", "a shared scan", "a scan per hypothesis",
         "a beam on a border cell: corner i + 1 or j + 1 off the map", "a beam that leaves the map", "a non-finite range",
         "an over-range range", "a scan with no used beam", "a non-finite start", "a map with nothing occupied")
SURE_MARGIN = 1e-9
E_POSE, E_COST, E_NORMAL = 2.4e-13, 6.2e-15, 8.3e-14
ALLOW_POSE, ALLOW_COST, ALLOW_NORMAL = min(16 * E_POSE, 1e-9), 16 * E_COST, 16 * E_NORMAL
ARGS = ("iters", "damping", "step_cells", "step_rad", "max_range", "cap")


def seeds():
    return range(int(os.environ.get("SLAM_HYP_EXAMPLES", "60")))


def random_map(rng, shape, empty=False):
    pm = np.full(shape, 50, dtype=np.int8)
    pm[rng.random(shape) < rng.choice((0.5, 0.7, 0.9))] = 0
    if not empty:
        pm[rng.random(shape) < rng.choice((0.03, 0.08, 0.15))] = 100
        pm[rng.integers(0, shape[0]), rng.integers(0, shape[1])] = 100
    return pm


def case_of(kind, seed):
    assert kind == "refine"
    rng = np.random.default_rng(2000 + seed)
    shape = SHAPES[(seed // 5) % len(SHAPES)]
    scale, off_x, off_y = RULES[(seed // 20) % len(RULES)]
    n, iters = BEAMS[seed % len(BEAMS)], ITERS[(seed // 5 + seed // 20) % len(ITERS)]
    G = int(rng.integers(1, 4))
    empty = int(rng.integers(0, G)) if rng.random() < 0.3 else -1
    pmaps = np.stack([random_map(rng, shape, g == empty) for g in range(G)])
    B = int(rng.integers(1, 6))
    maps = rng.integers(0, G, size=B).astype(np.int32)
    if B > 1 and rng.random() < 0.4:
        maps[1] = maps[0]
    if rng.random() < 0.3:
        maps[rng.integers(0, B)] = rng.choice((-1, G, G + 5))
    cells = np.stack([rng.integers(0, shape[0], size=B), rng.integers(0, shape[1], size=B)], axis=1)
    frac = rng.uniform(0.05, 0.95, size=(B, 2))
    poses = np.stack([(cells[:, 0] + frac[:, 0]) / scale - off_x, (cells[:, 1] + frac[:, 1]) / scale - off_y, rng.uniform(-3.2, 3.2, size=B)], axis=1)
    if rng.random() < 0.2:
        poses[rng.integers(0, B), rng.integers(0, 3)] = rng.choice((np.nan, np.inf, -np.inf))
    th = -np.pi + np.arange(n) * (2.0 * np.pi / n) + rng.uniform(0, 0.1)
    reach = float(rng.choice((4.0, 20.0, 90.0)))          # cells
    max_range = float(np.float32(reach / scale))
    shared = bool(rng.random() < 0.4)
    ranges = rng.uniform(0.5 / scale, 1.1 * max_range, size=(n,) if shared else (B, n)).astype(np.float32)
    ranges[rng.random(ranges.shape) < 0.05] = rng.choice((np.nan, np.inf))
    if rng.random() < 0.25:                               # a scan with no used beam
        (ranges if shared else ranges[rng.integers(0, B)])[...] = rng.choice((np.inf, np.float32(2.0 * max_range)))
    cap = int(rng.choice((64, 64, 9)))
    case = dict(pmaps=pmaps, scale=scale, off_x=off_x, off_y=off_y, ranges=np.ascontiguousarray(ranges), poses=np.ascontiguousarray(poses),
                maps=maps, ct=np.cos(th), st=np.sin(th), iters=int(iters), damping=float(rng.choice((1e-3, 1e-2, 0.1))),
                step_cells=float(rng.choice((0.5, 1.0))), step_rad=float(rng.choice((0.02, 0.05))), max_range=max_range, cap=cap)
    case["fields"] = np.stack([MR.field(pm, cap) for pm in pmaps])
    return case


def named(case):
    return (case["maps"] >= 0) & (case["maps"] < len(case["pmaps"]))


def answer(case, fn, rows=slice(None), **over):
    a = dict({k: case[k] for k in ARGS}, **over)
    r = case["ranges"] if case["ranges"].ndim == 1 else case["ranges"][rows]
    return R.batch(fn, case["fields"], case["scale"], case["off_x"], case["off_y"], r, case["poses"][rows], case["ct"], case["st"],
                   a["iters"], a["damping"], a["step_cells"], a["step_rad"], a["max_range"], a["cap"], maps=case["maps"][rows])


@functools.lru_cache(maxsize=None)
def answer_mp(seed):
    return answer(case_of("refine", seed), R.refine_mp)


def sure(ans):
    return bool(np.all(ans["margin"] >= SURE_MARGIN))


def deviation(got, want):
    """(pose, cost, normal) deviations of ``got`` from ``want`` over the answered hypotheses; statuses and used counts are
    asserted equal, and the rows that were not answered equal bit for bit."""
    assert np.array_equal(got["status"], want["status"]) and np.array_equal(got["used"], want["used"])
    ok = want["status"] == R.OK
    for k in ("pose", "cost", "normal"):
        assert np.array_equal(got[k][~ok], want[k][~ok], equal_nan=True), k
    if not ok.any():
        return 0.0, 0.0, 0.0
    rel = lambda k: float(np.max(np.abs(got[k][ok] - want[k][ok]) / np.maximum(np.max(np.abs(want[k][ok]), axis=1, keepdims=True), 1e-300)))   # noqa: E731
    return float(np.max(np.abs(got["pose"][ok] - want["pose"][ok]))), rel("cost"), rel("normal")


def edges_of(case, ans):
    out = set()
    G, (xw, yw) = len(case["pmaps"]), case["pmaps"].shape[1:]
    ok = named(case)
    if not ok.all():
        out.add(EDGES[0])
    if len(set(case["maps"][ok])) < int(ok.sum()):
        out.add(EDGES[1])
    out.add(EDGES[2] if case["ranges"].ndim == 1 else EDGES[3])
    r = case["ranges"]
    if not np.isfinite(r).all():
        out.add(EDGES[6])
    if (r[np.isfinite(r)] >= np.float32(case["max_range"])).any():
        out.add(EDGES[7])
    if not np.isfinite(case["poses"]).all():
        out.add(EDGES[9])
    for b in np.flatnonzero(ans["status"] == R.OK):
        if ans["used"][b] == 0:
            out.add(EDGES[8])
        if not (case["pmaps"][case["maps"][b]] == 100).any():
            out.add(EDGES[10])
        t, rr = R.used_beams(r if r.ndim == 1 else r[b], case["ct"], case["st"], case["max_range"])
        px, py, th = case["poses"][b]
        lx, ly = case["ct"][t] * rr, case["st"][t] * rr
        u = case["scale"] * (np.cos(th) * lx - np.sin(th) * ly + px + case["off_x"]) - 0.5
        v = case["scale"] * (np.sin(th) * lx + np.cos(th) * ly + py + case["off_y"]) - 0.5
        i, j = np.floor(u), np.floor(v)
        near = (i >= -1) & (i < xw) & (j >= -1) & (j < yw)
        if (near & ((i == -1) | (i == xw - 1) | (j == -1) | (j == yw - 1))).any():
            out.add(EDGES[4])
        if (~near).any():
            out.add(EDGES[5])
    return out
