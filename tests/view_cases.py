"""Seeded cases of slam_grid_view_gain for the sweeps (tests/test_view_cases.py on the host, tests/
test_gpu_view_properties.py on the device).

    case_of('view', seed)       dict: pmaps int8 [G, xw, yw], scale, off_x, off_y, poses [B, 3], maps int32 [B] (an entry may
                                name no map), ct / st [n], max_range, skip
    answer(case)                (counts int32 [B, 4], seen uint32 [B, xw, ceil(yw / 32)]) by tests/view_ref.py
    edges_of(case, ans)         the names of the edges the case reaches
    seeds()                     range(SLAM_HYP_EXAMPLES), default 60

Maps: random walls and free space in unknown space at sizes from the edge list - one row, a partial last word, exactly
two words, one more - under two index rules; views at random cells, some of them on an occupied cell; beams over the
full circle, from one beam to 90, reaching from a few cells to well beyond the map."""
import os

import numpy as np

import raycast_ref as R
import view_ref as V

SHAPES = ((1, 70), (37, 45), (64, 64), (33, 65), (20, 100), (5, 257), (48, 32))
RULES = ((1.0, 0.0, 0.0), (10.0, 2.0, 3.0))           # (scale, off_x, off_y)
EDGES = ("a view whose answer differs under the walk-order mistake", "rays that leave the map", "unknown > 0",
         "a view standing on an occupied cell", "a bad route", "a map with yw % 32 != 0")


def seeds():
    return range(int(os.environ.get("SLAM_HYP_EXAMPLES", "60")))


def random_map(rng, shape):
    pm = np.full(shape, 50, dtype=np.int8)
    pm[rng.random(shape) < rng.choice((0.5, 0.7, 0.9))] = 0
    pm[rng.random(shape) < rng.choice((0.03, 0.08, 0.15))] = 100
    return pm


def case_of(kind, seed):
    assert kind == "view"
    rng = np.random.default_rng(1000 + seed)
    shape = SHAPES[seed % len(SHAPES)]
    scale, off_x, off_y = RULES[(seed // len(SHAPES)) % len(RULES)]
    G = int(rng.integers(1, 4))
    pmaps = np.stack([random_map(rng, shape) for _ in range(G)])
    B = int(rng.integers(1, 6))
    maps = rng.integers(0, G, size=B).astype(np.int32)
    if rng.random() < 0.3:
        maps[rng.integers(0, B)] = rng.choice((-1, G, G + 5))
    cells = np.stack([rng.integers(0, shape[0], size=B), rng.integers(0, shape[1], size=B)], axis=1)
    if rng.random() < 0.35:                              # the first view stands on an occupied cell of its map
        g = maps[0] if 0 <= maps[0] < G else 0
        occ = np.argwhere(pmaps[g] == 100)
        if len(occ):
            cells[0] = occ[rng.integers(0, len(occ))]
    frac = rng.uniform(0.2, 0.8, size=(B, 2))
    poses = np.stack([(cells[:, 0] + frac[:, 0]) / scale - off_x, (cells[:, 1] + frac[:, 1]) / scale - off_y, rng.uniform(-3.2, 3.2, size=B)], axis=1)
    n = int(rng.choice((1, 7, 64, 90)))
    th = -np.pi + np.arange(n) * (2.0 * np.pi / n) + rng.uniform(0, 0.1)
    reach = float(rng.choice((4.0, 20.0, 90.0)))         # cells
    return dict(pmaps=pmaps, scale=scale, off_x=off_x, off_y=off_y, poses=np.ascontiguousarray(poses), maps=maps, ct=np.cos(th), st=np.sin(th),
                max_range=float(np.float32(reach / scale)), skip=int(rng.choice((0, 1, 1, 1, 3))))


def named(case):
    return (case["maps"] >= 0) & (case["maps"] < len(case["pmaps"]))


def answer(case, pmaps=None, rows=slice(None)):
    pm = case["pmaps"] if pmaps is None else pmaps
    return V.views(list(pm), case["scale"], case["off_x"], case["off_y"], case["poses"][rows], case["ct"], case["st"], case["max_range"],
                   case["skip"], gob=case["maps"][rows])


def edges_of(case, ans):
    out = set()
    pm, (xw, yw) = case["pmaps"], case["pmaps"].shape[1:]
    a = (case["scale"], case["off_x"], case["off_y"])
    if yw % 32:
        out.add(EDGES[5])
    if not named(case).all():
        out.add(EDGES[4])
    for b in np.flatnonzero(named(case)):
        g, pose = case["maps"][b], case["poses"][b]
        if ans[0][b, V.UNKNOWN] > 0:
            out.add(EDGES[2])
        start = (R.to_cell(pose[0], a[0], a[1]), R.to_cell(pose[1], a[0], a[2]))
        if pm[g][start] == 100:
            out.add(EDGES[3])
        pc = R.table_points(np.full(len(case["ct"]), np.float32(case["max_range"])), case["ct"], case["st"])
        _, ends = R._beams(pose, pc, *a)
        if any(e is not None and not (0 <= e[0] < xw and 0 <= e[1] < yw) for e in ends):
            out.add(EDGES[1])
        wrong = V.detail(pm[g], *a, pose, case["ct"], case["st"], case["max_range"], case["skip"], walk_order=True)
        if tuple(wrong["counts"]) != tuple(ans[0][b]):
            out.add(EDGES[0])
    return out
