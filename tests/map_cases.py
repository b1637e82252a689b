"""Seeded cases for the operators built on the map (test infrastructure only): the distance field, the window matcher,
global localisation, map frontiers, the two weighs, resampling, settle and the in-place map copy.

    case_of(kind, seed) -> dict     a pure function of (kind, seed): numpy.random.default_rng([KIND_ID[kind], seed]) is the
                                    only source of randomness, so a case is the same on every machine and in a bug report
    seeds()                         range(SLAM_HYP_EXAMPLES), default 60 (the variable tests/test_gpu_properties.py reads)

Sizes come from edge lists - the kernels' own edges: mask words of 32 cells, waves of 64, tiles of 32 x 64, segments of
1 024 cells, the 1 024 scan block and the 4 096 reduce run - mixed with uniform draws.  Seeds below 20 take every size
from the lower half of its list, so a failure tends to show first at a small case.  tests/test_map_cases.py (CPU) and
tests/test_gpu_map_properties.py (GPU) read the same cases; every assertion message there carries (kind, seed).

To reproduce a failure:  python -c "import map_cases as C; print(C.case_of('field', 17))"  from tests/."""
import math
import os

import numpy as np

import frontier_ref as FR
import gridslam_ref as G
import locate_ref as L
import match_ref as M
import mcl_ref as X
import raycast_ref as R

KINDS = ("field", "match", "locate", "frontiers", "weigh", "resample", "settle", "copy")
KIND_ID = {k: i + 1 for i, k in enumerate(KINDS)}
SMALL = 20                                  # seeds below this draw from the lower half of every list


def seeds():
    return range(int(os.environ.get("SLAM_HYP_EXAMPLES", "60")))


def rng_of(kind, seed):
    return np.random.default_rng([KIND_ID[kind], int(seed)])


def pick(rng, seed, values, p=None):
    """One entry of ``values``; a small seed takes it from the lower half (``p``: weights over the whole list)."""
    values = list(values)
    k = (len(values) + 1) // 2 if seed < SMALL else len(values)
    if p is not None:
        w = np.asarray(p[:k], dtype=np.float64)
        return values[int(rng.choice(k, p=w / w.sum()))]
    return values[int(rng.integers(k))]


def size(rng, seed, edges, lo, hi, p_edge=0.7):
    """An edge of the list or a uniform draw in lo .. hi (a small seed: the lower half of both)."""
    if rng.random() < p_edge:
        return int(pick(rng, seed, edges))
    return int(rng.integers(lo, (lo + hi) // 2 + 1 if seed < SMALL else hi + 1))


def reach(cap):
    """R = ceil(sqrt(cap)): how far the field's passes look."""
    return math.isqrt(int(cap) - 1) + 1


# ---------------------------------------------------------------- occupied cells of a map (field, match, weigh)
FIELD_SIDES = (1, 2, 31, 32, 33, 63, 64, 65, 190, 257, 300)
FIELD_CAPS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 32760, 32761, 32762, 32767)
FIELD_CELLS = 40000
OCCUPANCY = ("sparse", "ruler", "one", "row", "column", "none")
OCCUPANCY_P = (0.25, 0.42, 0.08, 0.09, 0.09, 0.07)
GAPS = ("R-1", "R", "R+1", "2R")


def word_edges(yw):
    """The y that sit at bit 0 or bit 31 of a mask word (rows are packed along y, 32 cells a word)."""
    return [y for y in range(yw) if y % 32 in (0, 31)]


def ruler(rng, xw, yw, cap):
    """Two occupied cells in one row (same x) or one column (same y), R - 1, R, R + 1 or 2 R apart, the first at bit 0 or
    bit 31 of a mask word; None when no such pair fits the map.  Returns (cells, gap name, axis)."""
    r = reach(cap)
    name = GAPS[int(rng.integers(4))]
    gap = {"R-1": r - 1, "R": r, "R+1": r + 1, "2R": 2 * r}[name]
    axes = ["row", "column"] if rng.random() < 0.5 else ["column", "row"]
    for axis in axes:
        if axis == "row":
            ys = [y for y in word_edges(yw) if y + gap < yw]
            if ys:
                x, y = int(rng.integers(xw)), ys[int(rng.integers(len(ys)))]
                return [(x, y), (x, y + gap)], name, axis
        elif gap < xw:
            ys = word_edges(yw)
            x, y = int(rng.integers(xw - gap)), ys[int(rng.integers(len(ys)))]
            return [(x, y), (x + gap, y)], name, axis
    return None


def occupancy(rng, xw, yw, cap):
    """(kind, cells, ruler gap or None) of one map."""
    kind = OCCUPANCY[int(rng.choice(len(OCCUPANCY), p=OCCUPANCY_P))]
    if kind == "ruler":
        got = ruler(rng, xw, yw, cap)
        if got is not None:
            return kind, got[0], (got[1], got[2])
        kind = "sparse"
    if kind == "none":
        return kind, [], None
    if kind == "one":
        return kind, [(int(rng.integers(xw)), int(rng.integers(yw)))], None
    if kind == "row":
        x = int(rng.integers(xw))
        return kind, [(x, y) for y in range(yw)], None
    if kind == "column":
        y = int(rng.integers(yw))
        return kind, [(x, y) for x in range(xw)], None
    k = int(rng.integers(1, 41))
    return kind, sorted({(int(x), int(y)) for x, y in zip(rng.integers(0, xw, k), rng.integers(0, yw, k))}), None


def field_maps(rng, seed, side=None):
    """G maps of one size, a cap and their occupied cells; ``side``: the largest axis allowed (None: up to 300, at most
    40 000 cells)."""
    G_ = int(rng.integers(1, 4))
    cap = int(pick(rng, seed, FIELD_CAPS))
    if side is None:
        xw, yw = size(rng, seed, FIELD_SIDES, 1, 300), size(rng, seed, FIELD_SIDES, 1, 300)
        if cap >= 32760 and rng.random() < 0.75:                      # R = 181 or 182 needs an axis that can hold it
            long = (190, 257, 300)[int(rng.integers(3))]
            xw, yw = (long, yw) if rng.random() < 0.5 else (xw, long)
        if xw * yw > FIELD_CELLS:
            xw, yw = (xw, FIELD_CELLS // xw) if xw >= yw else (FIELD_CELLS // yw, yw)
    else:
        edges = [s for s in FIELD_SIDES if s <= side]
        xw, yw = size(rng, seed, edges, 1, side), size(rng, seed, edges, 1, side)
    occ = [occupancy(rng, xw, yw, cap) for _ in range(G_)]
    return dict(G=G_, xw=xw, yw=yw, cap=cap, cells=[o[1] for o in occ], occupancy=[o[0] for o in occ],
                rulers=[o[2] for o in occ if o[2] is not None])


def pmaps_of_cells(case):
    """int8 [G, xw, yw]: 100 at the occupied cells, 50 elsewhere - what a grid gives whose hit counters alone were written."""
    pm = np.full((case["G"], case["xw"], case["yw"]), 50, dtype=np.int8)
    for gi, cs in enumerate(case["cells"]):
        for x, y in cs:
            pm[gi, x, y] = 100
    return pm


def case_field(rng, seed):
    c = field_maps(rng, seed)
    c.update(scale=1.0, off_x=0.0, off_y=0.0)
    return c


# ---------------------------------------------------------------- the window matcher
def routing(rng, B, G_, bad=True, none_ok=True):
    """A map entry per hypothesis: None (the operator's default), or int32 [B] with entries -1 and G among good ones."""
    if none_ok and rng.random() < 0.25:
        return None
    maps = rng.integers(0, G_, B).astype(np.int32)
    if bad:
        for b in range(B):
            u = rng.random()
            if u < 0.12:
                maps[b] = -1
            elif u < 0.24:
                maps[b] = G_
    return maps


def scan(rng, n, reach_, max_range, shape=None):
    """Beam tables over most of a circle and float32 ranges up to ``reach_``, with inf, NaN and >= max_range entries."""
    ang = np.linspace(-3.0, 3.1, n) if n > 1 else np.array([0.3])
    shape = (n,) if shape is None else shape
    r = rng.uniform(0.05 * reach_, reach_, shape).astype(np.float32)
    flat = r.reshape(-1)
    for v in (np.inf, np.nan, max_range, max_range * 1.5):
        if rng.random() < 0.6:
            flat[int(rng.integers(flat.size))] = v
    return np.cos(ang), np.sin(ang), r


def case_match(rng, seed):
    c = field_maps(rng, seed, side=64)
    G_, xw, yw = c["G"], c["xw"], c["yw"]
    scale = float(pick(rng, seed, (1.0, 20.0)))
    off_x, off_y = (0.0, 0.0) if scale == 1.0 else (xw / (2.0 * scale), yw / (2.0 * scale))
    B, K = int(rng.integers(1, 5)), int(rng.integers(1, 10))
    nx, ny = int(rng.integers(0, 5)), int(rng.integers(0, 5))
    n = int(pick(rng, seed, (1, 63, 64, 65, 130)))
    while K * (2 * nx + 1) * (2 * ny + 1) * n * B > 20000:             # the pure-Python restatement's budget
        if nx >= ny and nx > 0:
            nx -= 1
        elif ny > 0:
            ny -= 1
        elif K > 1:
            K -= 1
        elif B > 1:
            B -= 1
        else:
            n = 130 if n > 130 else 65
    step = float((1.0, 0.5, 1.7)[int(rng.integers(3))]) / scale
    max_range = 40.0 / scale
    centres = np.empty((B, 2))
    where = []
    for b in range(B):
        w = ("inside", "inside", "border", "outside", "nan")[int(rng.integers(5))] if b or B == 1 else "inside"
        u, v = rng.integers(0, xw) + rng.random(), rng.integers(0, yw) + rng.random()
        if w == "border":                                             # exactly on the first cell's edge, or in the last cell
            u, v = (0.0, v) if rng.random() < 0.5 else (u, float(yw - 1) + rng.random())
        elif w == "outside":
            u = float(xw) + 5.0 * rng.random() if rng.random() < 0.5 else -5.0 * rng.random() - 0.01
        centres[b] = (u / scale - off_x, v / scale - off_y)
        if w == "nan":
            centres[b, int(rng.integers(2))] = np.nan
        where.append(w)
    shared = bool(rng.random() < 0.4)
    ct, st, ranges = scan(rng, n, 30.0 / scale, max_range, None if shared else (B, n))
    theta = rng.uniform(-3.0, 3.0, B)
    rot = np.stack([np.stack([np.cos(t + (np.arange(K) - K // 2) * 0.03), np.sin(t + (np.arange(K) - K // 2) * 0.03)], axis=-1) for t in theta])
    c.update(scale=scale, off_x=off_x, off_y=off_y, B=B, K=K, nx=nx, ny=ny, n=n, step=step, max_range=max_range, centres=centres,
             where=where, ranges=ranges, cos_t=ct, sin_t=st, rot_cs=rot, maps=routing(rng, B, G_), costs=bool(rng.random() < 0.5))
    return c


# ---------------------------------------------------------------- global localisation
LOCATE_SIDES = (1, 2, 7, 8, 9, 16, 31, 32, 33, 48)
LOCATE_H_P = (0.2, 0.09, 0.09, 0.09, 0.09, 0.08, 0.08, 0.08, 0.2)     # the two ends weigh most: brute force, and the deepest pyramid


def case_locate(rng, seed):
    G_ = int(rng.integers(1, 4))
    xw, yw = size(rng, seed, LOCATE_SIDES, 1, 48), size(rng, seed, LOCATE_SIDES, 1, 48)
    cells = []
    for _ in range(G_):                                               # locate_ref.ragged_pmap's pattern: corners, a column, scattered cells
        cs = [(0, 0), (0, yw - 1), (xw - 1, 0), (xw - 1, yw - 1)] if rng.random() < 0.6 else []
        cs += [(x, yw - 1) for x in range(3, xw, 7)] if rng.random() < 0.4 else []
        k = int(rng.integers(0, 26))
        cs += [(int(x), int(y)) for x, y in zip(rng.integers(0, xw, k), rng.integers(0, yw, k))]
        cells.append(sorted(set(cs)))
    B = int(rng.integers(1, 7))
    H = int(pick(rng, seed, range(9), p=LOCATE_H_P))
    K = int(pick(rng, seed, (1, 2, 7, 8)))
    n = int(pick(rng, seed, (1, 17, 63, 65, 130)))
    cap = int((1, 9, 50, 32767 // n)[int(rng.integers(4))])
    scale = float((1.0, 2.0)[int(rng.integers(2))])
    far = bool(rng.random() < 0.25)                                   # one beam beyond 2^20 cells: it is used, and "off"
    max_range = float("inf") if far else 30.0 / scale
    shared = bool(rng.random() < 0.4)
    ct, st, ranges = scan(rng, n, 26.0 / scale, 30.0 / scale, None if shared else (B, n))
    if far:
        ranges.reshape(-1)[int(rng.integers(ranges.size))] = np.float32(3.0e6)
    th = rng.uniform(-np.pi, np.pi, K)
    rot = np.stack([np.cos(th), np.sin(th)], axis=-1)
    if rng.random() < 0.25:
        rot[int(rng.integers(K)), int(rng.integers(2))] = np.nan
    regions = None
    if rng.random() < 0.85:
        regions = np.empty((B, 4), dtype=np.int32)
        for b in range(B):
            ni, nj = (min(int(v), w) if v else w for v, w in ((pick(rng, seed, (1, 2, 3, 7, 8, 9, 0)), xw), (pick(rng, seed, (1, 2, 3, 7, 8, 9, 0)), yw)))
            if seed >= SMALL and rng.random() < 0.3:
                ni, nj = xw, yw
            regions[b] = (rng.integers(0, xw - ni + 1), rng.integers(0, yw - nj + 1), ni, nj)
    chunk = int(rng.integers(1, 4)) if seed % 3 == 2 else None           # a third of the cases, evenly spread
    return dict(G=G_, xw=xw, yw=yw, cells=cells, scale=scale, off_x=0.0, off_y=0.0, B=B, H=H, K=K, n=n, cap=cap, max_range=max_range,
                ranges=ranges, cos_t=ct, sin_t=st, rot_cs=rot, regions=regions, maps=routing(rng, B, G_), chunk_pairs=chunk)


def plan_query(name, a=0, b=0, c=0):
    """slam_plan_query of the built library: no context, no device."""
    import ctypes as C
    from conftest import pkg
    abi = pkg("_abi")
    out = C.c_int64()
    abi.check(abi.lib().slam_plan_query(name.encode(), int(a), int(b), int(c), -1, C.byref(out)))
    return int(out.value)


def locate_plan(case):
    """(locate_ws_mb or None, pairs per chunk) of the host form: the budget that lets exactly case["chunk_pairs"] of the
    call's (hypothesis, rotation) pairs into a chunk, from a pair's bytes as the library plans them for the largest region."""
    pairs = case["B"] * case["K"]
    if case["chunk_pairs"] is None or case["H"] == 0:                 # brute force keeps no list: nothing to cut
        return None, pairs
    reg = case["regions"]
    ni, nj = (case["xw"], case["yw"]) if reg is None else (int(reg[:, 2].max()), int(reg[:, 3].max()))
    pair = plan_query("locate_pair_bytes", ni, nj, case["H"]) + plan_query("locate_table_bytes", case["n"])
    return case["chunk_pairs"] * pair / 1048576.0, min(case["chunk_pairs"], pairs)


# ---------------------------------------------------------------- frontiers
FRONTIER_XW = (1, 31, 32, 33, 64, 65, 97, 140)
FRONTIER_YW = (1, 63, 64, 65, 128, 129, 140)


def smooth(rng, xw, yw):
    """A smooth random field [xw, yw]: coarse noise held over 12 x 12 cells, then a box blur twice."""
    s = 12
    coarse = rng.normal(size=(xw // s + 4, yw // s + 4))
    z = np.kron(coarse, np.ones((s, s)))
    for _ in range(2):
        for axis in (0, 1):
            c = np.cumsum(z, axis=axis)
            z = np.take(c, np.arange(s, c.shape[axis]), axis=axis) - np.take(c, np.arange(0, c.shape[axis] - s), axis=axis)
    ox, oy = int(rng.integers(0, s)), int(rng.integers(0, s))
    return z[ox:ox + xw, oy:oy + yw]


def blob_pmap(rng, xw, yw, salt):
    """Free, unknown and occupied regions as blobs several tiles wide, plus salt noise at density ``salt``."""
    z, w = smooth(rng, xw, yw), smooth(rng, xw, yw)
    pm = np.where(z < np.quantile(z, rng.uniform(0.35, 0.65)), 0, 50).astype(np.int8)
    pm[w > np.quantile(w, 0.88)] = 100
    noise = rng.random((xw, yw)) < salt
    pm[noise] = rng.choice(np.array([0, 50, 100], dtype=np.int8), size=(xw, yw))[noise]
    return pm


def case_frontiers(rng, seed):
    G_ = int(rng.integers(1, 4))
    xw, yw = int(pick(rng, seed, FRONTIER_XW)), int(pick(rng, seed, FRONTIER_YW))
    salt = float((0.0, 0.02, 0.2)[int(rng.integers(3))])
    pmaps = np.stack([blob_pmap(rng, xw, yw, salt) for _ in range(G_)])
    radius = int(pick(rng, seed, range(9)))
    full = (2 * radius + 1) ** 2
    # the window's centre is a free cell, so (2 r + 1)^2 unknown cells (and 1 at radius 0) leave no frontier at all: kept, but rare
    min_unknown = int((0, 1, radius + 1, full // 2, full)[int(rng.choice(5, p=(0.32, 0.25, 0.25, 0.15, 0.03)))])
    if radius == 0:                                                   # the ABI takes 0 .. (2 r + 1)^2: radius 0 takes 0 or 1
        min_unknown = min(min_unknown, 1) if rng.random() < 0.15 else 0
    cap = int((4, 16, 64)[int(rng.integers(3))])
    min_clear2 = int((0, 1, 4, cap)[int(rng.integers(4))])
    B = int(rng.integers(1, 7))
    maps = routing(rng, B, G_, none_ok=B <= G_)                       # without a table query b reads map b: B <= G
    chunk = int(rng.integers(1, 3)) if seed % 3 == 2 else None           # a third of the cases, evenly spread
    return dict(G=G_, xw=xw, yw=yw, pmaps=pmaps, salt=salt, B=B, maps=maps, radius=radius, min_unknown=min_unknown,
                min_size=int((1, 2, 5, 40)[int(rng.integers(4))]), M=int((0, 1, 3, 64, 512)[int(rng.integers(5))]),
                min_clear2=min_clear2, cap=cap, labels=bool(rng.random() < 0.6), chunk_queries=chunk)


def frontier_plan(case):
    """(frontier_ws_mb or None, queries per chunk): the budget that lets exactly case["chunk_queries"] queries into a chunk."""
    if case["chunk_queries"] is None:
        return None, case["B"]
    qb = plan_query("frontier_query_bytes", case["xw"], case["yw"])
    return case["chunk_queries"] * qb / 1048576.0, min(case["chunk_queries"], case["B"])


# ---------------------------------------------------------------- the weighs
WEIGH_P = (1, 15, 16, 17, 63, 64, 65, 255, 257, 300)
WEIGH_N = (1, 63, 64, 65, 111, 112, 113, 130)
WEIGH_CAPS = (1, 9, 64, 300, 32767)
MAX_RANGE = 19.0


def case_weigh(rng, seed):
    """slam_mcl_weigh (own_maps False) or slam_mcl_weigh_maps with a particle-to-map table, on 64 x 64 maps at scale 1.
    The launch shape and the operator cycle with the seed, so each combination comes round within six seeds."""
    G_ = int(rng.integers(1, 4))
    cells = []
    for _ in range(G_):
        if rng.random() < 0.5:
            cells.append(R.ring(8) + R.ring(16) if rng.random() < 0.5 else R.ring(12))
        else:
            cells.append(sorted({(int(x), int(y)) for x, y in rng.integers(4, 60, (30, 2))}))
    F = int(rng.integers(1, 6))
    ps = [p for p in WEIGH_P if F * p >= 64]
    P = int(pick(rng, seed, ps))
    n = int(pick(rng, seed, WEIGH_N))
    own = (seed // 3) % 2 == 1
    # poses: the middle of a cell plus an offset that stays clear of its edges; headings anywhere
    poses = np.concatenate([rng.integers(24, 41, (F, P, 2)) + 0.5 + rng.uniform(-0.45, 0.45, (F, P, 2)), rng.uniform(-3.0, 3.0, (F, P, 1))], axis=-1)
    for _ in range(int(rng.integers(0, 4))):                          # off the map, not finite, beyond 2^20 cells
        f, p = int(rng.integers(F)), int(rng.integers(P))
        poses[f, p, int(rng.integers(2))] = (-5.3, 70.2, np.nan, np.inf, float(1 << 21))[int(rng.integers(5))]
    if rng.random() < 0.2:
        poses[int(rng.integers(F)), int(rng.integers(P)), 2] = np.nan
    ct, st, ranges = scan(rng, n, 24.0, MAX_RANGE, (F, n))
    motion = noise = None
    if rng.random() < 0.6:
        motion = rng.uniform(-0.5, 0.5, (F, 3))
        if rng.random() < 0.6:
            noise = rng.normal(0.0, 0.1, (F, P, 3))
    acc_kind = ("absent", "zero", "high", "dead")[int(rng.integers(4))]
    acc = None
    if acc_kind != "absent":
        acc = np.zeros((F, P), dtype=np.int32)
        if acc_kind == "high":
            acc[:] = X.ACC_MAX - rng.integers(0, 2000, (F, P))
        if acc_kind == "dead":
            acc[:] = rng.integers(0, 5000, (F, P))
            acc[rng.random((F, P)) < 0.2] = X.DEAD
    if own:
        maps = rng.integers(0, G_, (F, P)).astype(np.int32)
        maps[rng.random((F, P)) < 0.03] = -1
        maps[rng.random((F, P)) < 0.03] = G_
    else:
        maps = routing(rng, F, G_)
    return dict(G=G_, xw=64, yw=64, cells=cells, scale=1.0, off_x=0.0, off_y=0.0, cap=int(pick(rng, seed, WEIGH_CAPS)), F=F, P=P, n=n,
                own_maps=own, mcl_shape=seed % 3 - 1, poses=poses, ranges=ranges, cos_t=ct, sin_t=st, max_range=MAX_RANGE, motion=motion,
                noise=noise, acc=acc, acc_kind=acc_kind, maps=maps)


# ---------------------------------------------------------------- resampling
RESAMPLE_P = (1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 5000)
RESAMPLE_P_P = (1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2)                   # the reduce run's far side weighs double
TABLES = ("weight_table", "constant", "steps", "zero", "first_only")


def case_resample(rng, seed):
    F = int(rng.integers(1, 5))
    P = int(pick(rng, seed, RESAMPLE_P, p=RESAMPLE_P_P)) if rng.random() < 0.8 else int(rng.integers(1, 2500 if seed < SMALL else 5001))
    T = int((1, 2, 64, 4096)[int(rng.integers(4))])
    shift = int((0, 1, 5, 12)[int(rng.integers(4))])
    kind = TABLES[int(rng.choice(5, p=(0.32, 0.15, 0.36, 0.07, 0.1)))]
    if kind == "weight_table":
        table = X.weight_table(float(rng.uniform(1.0, 8.0)), shift, T, floor=int(rng.integers(0, 2)))
    elif kind == "constant":
        table = np.full(T, int(rng.integers(1, X.W_MAX + 1)), dtype=np.uint32)
    elif kind == "steps":                                             # random, non-increasing, entries above 2^20 at the front
        table = np.sort(rng.integers(0, 3 << 20, T))[::-1].astype(np.uint32)
    elif kind == "zero":
        table = np.zeros(T, dtype=np.uint32)
    else:
        table = np.zeros(T, dtype=np.uint32)
        table[0] = int(rng.integers(1, X.W_MAX + 1))
    spread = int((3, 60, 5000, 1 << 20)[int(rng.integers(4))])
    acc = rng.integers(-spread // 4, spread, (F, P)).astype(np.int32)
    dead = float((0.0, 0.3, 1.0)[int(rng.choice(3, p=(0.55, 0.37, 0.08)))])
    acc[rng.random((F, P)) < dead] = X.DEAD
    u0 = np.array([(0.0, float(rng.random()), float(np.nextafter(1.0, 0.0)))[int(rng.integers(3))] for _ in range(F)])
    poses = rng.uniform(-5.0, 5.0, (F, P, 3))
    poses[..., 2] *= 40.0                                             # headings far outside +-pi
    return dict(F=F, P=P, T=T, shift=shift, table=table, table_kind=kind, acc=acc, dead=dead, u0=u0, poses=poses,
                ess_frac=float((0.0, 0.5, 1.0, np.inf)[int(rng.choice(4, p=(0.15, 0.2, 0.2, 0.45)))]))


# ---------------------------------------------------------------- settle and the map copy
SETTLE_P = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4096)
SETTLE_F = (1, 2, 3, 7, 20, 300)
SETTLE_CELLS = 300000


def ancestors(rng, F, P, kind):
    """int32 [F, P]: a real systematic resampling of random weights (some filters with half of them zero), all equal, or
    the identity."""
    if kind == "identity":
        return np.tile(np.arange(P, dtype=np.int32), (F, 1))
    if kind == "equal":
        return np.repeat(rng.integers(0, P, (F, 1)).astype(np.int32), P, axis=1)
    anc = np.empty((F, P), dtype=np.int32)
    for f in range(F):
        w = np.rint(X.W_MAX * rng.random(P) ** (1 + f % 7)).astype(np.int64) + 1
        if f % 3 == 1:
            w[rng.permutation(P)[:P // 2]] = 0
            w[int(rng.integers(P))] += 1
        anc[f] = X.resample_u64(w, float(rng.random()))
    return anc


def case_settle(rng, seed):
    P = int(pick(rng, seed, SETTLE_P))
    F = size(rng, seed, SETTLE_F, 1, 300, p_edge=0.8)
    F = max(1, min(F, SETTLE_CELLS // P, 40000 // P if seed < SMALL else F))
    kind = ("real", "real", "equal", "identity")[int(rng.integers(4))]
    anc = ancestors(rng, F, P, kind)
    return dict(F=F, P=P, ancestors=anc, anc_kind=kind, map0=int((0, 3)[int(rng.integers(2))]),
                poses=rng.normal(0.0, 1.0, (F, P, 3)) if rng.random() < 0.6 else None)


def case_copy(rng, seed):
    G_ = int(rng.integers(2, 10))
    xw, yw = pick(rng, seed, ((1, 1), (33, 35), (70, 33), (91, 91)))
    count = int(rng.integers(1, G_ + 1))
    first = int(rng.integers(0, G_ - count + 1))                       # maps before first and from first + count on stay untouched
    kind = ("identity", "one", "settle")[int(rng.integers(3))]
    if kind == "identity":
        src = first + np.arange(count)
    elif kind == "one":
        src = np.full(count, int(rng.integers(0, G_)))
    else:
        src = first + np.array(G.settle(ancestors(rng, 1, count, "real")[0]))
    src = src.astype(np.int32)
    for k in range(count):                                            # no map: the destination is kept
        if rng.random() < 0.1 and not np.any(src == first + k):
            src[k] = -1 if rng.random() < 0.5 else G_
    near = np.uint32(0xffffffff) - rng.integers(0, 3, (2, G_, xw, yw)).astype(np.uint32)
    cnt = rng.integers(0, 1 << 32, (2, G_, xw, yw), dtype=np.uint64).astype(np.uint32)
    cnt = np.where(rng.random((2, G_, xw, yw)) < 0.05, near, cnt)
    return dict(G=G_, xw=int(xw), yw=int(yw), first=first, count=count, src=src, src_kind=kind, pass_cnt=cnt[0], hit_cnt=cnt[1])


# ---------------------------------------------------------------- the restatement's answer to a case
def fields_of(pmaps, cap):
    return np.stack([M.field(p, cap) for p in pmaps])


def answer(case, pmaps=None):
    """What the restatements under tests/ say of the case; ``pmaps``: the maps read back from a device (None: the case's own)."""
    kind = case["kind"]
    c = case
    if pmaps is None and kind in ("field", "match", "locate", "weigh"):
        pmaps = pmaps_of_cells(c)
    if kind == "field":
        return fields_of(pmaps, c["cap"])
    if kind == "match":
        return M.match_batch(fields_of(pmaps, c["cap"]), c["scale"], c["off_x"], c["off_y"], c["ranges"], c["centres"], c["cos_t"], c["sin_t"],
                             c["rot_cs"], c["nx"], c["ny"], c["step"], c["max_range"], c["cap"], maps=c["maps"])
    if kind == "locate":
        return L.locate_batch(fields_of(pmaps, c["cap"]), c["scale"], c["ranges"], c["cos_t"], c["sin_t"], c["rot_cs"], c["H"], c["max_range"],
                              c["cap"], maps=c["maps"], regions=c["regions"], B=c["B"])
    if kind == "frontiers":
        pmaps = c["pmaps"] if pmaps is None else pmaps
        fields = fields_of(pmaps, c["cap"]) if c["min_clear2"] > 0 else None
        return FR.frontiers_batch(pmaps, maps=c["maps"], B=c["B"], fields=fields, radius=c["radius"], min_unknown=c["min_unknown"],
                                  min_size=c["min_size"], M=c["M"], min_clear2=c["min_clear2"])
    if kind == "weigh":
        return weigh_answer(c, fields_of(pmaps, c["cap"]), ulp=True)
    if kind == "resample":
        return X.resample(c["poses"], c["acc"], c["table"], c["shift"], c["u0"], c["ess_frac"])
    if kind == "settle":
        return G.settle_batch(c["ancestors"], c["poses"], map0=c["map0"])
    if kind == "copy":
        arrays = [c["pass_cnt"].astype(np.int64), c["hit_cnt"].astype(np.int64)]
        kinds = G.copy_maps(arrays, c["src"], c["first"])
        return dict(copied=kinds, pass_cnt=arrays[0], hit_cnt=arrays[1])
    raise KeyError(kind)


def weigh_answer(c, fields, ulp=False, moved=None):
    """mcl_ref.weigh of a weigh case; slam_mcl_weigh_maps is every particle as a filter of its own on its table entry's map."""
    geom = (c["scale"], c["off_x"], c["off_y"])
    if not c["own_maps"]:
        return X.weigh(fields, *geom, c["poses"], c["ranges"], c["cos_t"], c["sin_t"], c["max_range"], c["cap"], motion=c["motion"],
                       noise=c["noise"], maps=c["maps"], acc=c["acc"], ulp=ulp, moved=moved)
    import mcl_checks
    return mcl_checks.weigh_maps(fields, geom, c["poses"], c["ranges"], c["cos_t"], c["sin_t"], c["max_range"], c["cap"], c["maps"],
                                 motion=c["motion"], noise=c["noise"], acc=c["acc"], ulp=ulp, moved=moved)


MAKERS = dict(field=case_field, match=case_match, locate=case_locate, frontiers=case_frontiers, weigh=case_weigh, resample=case_resample,
              settle=case_settle, copy=case_copy)


def case_of(kind, seed):
    """The case of (kind, seed): a dict of plain Python values and NumPy arrays, with "kind" and "seed" in it."""
    c = MAKERS[kind](rng_of(kind, seed), int(seed))
    c.update(kind=kind, seed=int(seed))
    return c
