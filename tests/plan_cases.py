"""Seeded cases for the planners, the map ray cast and the landmark extraction (test infrastructure only): A* inflation,
A* search, DWA, slam_grid_raycast / slam_grid_scan_score and slam_landmarks.  The second sweep, in the shape of
tests/map_cases.py, whose helpers it uses.

    case_of(kind, seed) -> dict     a pure function of (kind, seed): numpy.random.default_rng([KIND_ID[kind], seed]) is the
                                    only source of randomness (helpers that take a seed of their own get one drawn from it)
    answer(case)                    what the restatements under tests/ say of the case

Sizes are the kernels' own edges - 64-column words of the trigger rows, the LDS ring of 32 768 bytes, search slots, the
12-row register chunk and the 64 / 512 lane window of the DWA, 32-cell mask words of the ray cast, waves of 64 and trips
of 256 lanes of the extraction - mixed with uniform draws; seeds below 20 take every size from the lower half of its list.
tests/test_plan_cases.py (CPU) and tests/test_gpu_plan_properties.py (GPU) read the same cases; every assertion message
there carries (kind, seed).

To reproduce a failure:  python -c "import plan_cases as P; print(P.case_of('inflate', 17))"  from tests/."""
import math

import numpy as np

import astar_ref as A
import dwa_ref as D
import raycast_cases as K
import raycast_ref as R
from map_cases import SMALL, pick, seeds, size  # noqa: F401  (seeds is re-exported for the two test files)

KINDS = ("inflate", "astar", "dwa", "raycast", "landmarks")
KIND_ID = {k: i + 101 for i, k in enumerate(KINDS)}     # map_cases.py has 1 .. 8


def rng_of(kind, seed):
    return np.random.default_rng([KIND_ID[kind], int(seed)])


def sub_seed(rng):
    """A seed for a helper that makes its own generator, drawn from the case's."""
    return int(rng.integers(1 << 31))


# ---------------------------------------------------------------- A* inflation
INFLATE_SPANS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257)
INFLATE_R = (0, 1, 2, 3, 31, 32, 33, 63, 64, 65)
INFLATE_DENSITY = (0.0, 0.005, 0.05, 0.3, 0.6, 1.0)
INFLATE_DENSITY_P = (0.05, 0.15, 0.2, 0.27, 0.25, 0.08)
INFLATE_OTHER = (0, 50, 99, 1, -2, 127, -128)
INFLATE_RING = (1152, 229)              # span, r: 229 * 18 words * 8 bytes = 32 976 > 32 768, the ring leaves the LDS
INFLATE_NO_TRIGGER = 0.06               # the share of cases left with span - r <= r: nothing triggers, no row walk


def global_ring(span, r):
    return span - r > r and r * ((span + 63) // 64) * 8 > 32768


def case_inflate(rng, seed):
    ring = seed >= SMALL and seed % 15 == 12                          # seeds 27, 42, 57 of the default 60
    if ring:
        span, r = INFLATE_RING
        G_, H, density, forced = 1, span, 0.0004, False
        W = H + int((0, 0, 48)[int(rng.integers(3))])
    else:
        span = size(rng, seed, INFLATE_SPANS, 1, 300)
        r = int(pick(rng, seed, INFLATE_R))
        if span - r <= r and rng.random() >= INFLATE_NO_TRIGGER:
            fit = [v for v in INFLATE_R if span - v > v] or [0]       # the larger radii that still leave a row
            r = int(fit[int(rng.integers(max(0, len(fit) - 3), len(fit)))])
        G_ = int(rng.integers(1, 4))
        H = span + int((0, 0, 1, 5, 64)[int(rng.integers(5))])       # in some cases span < H
        W = H + int((0, 0, 1, 5, 64)[int(rng.integers(5))])          # and H < W
        density = float(INFLATE_DENSITY[int(rng.choice(len(INFLATE_DENSITY), p=INFLATE_DENSITY_P))])
        forced = bool(rng.random() < 0.4)
    wire = bool(rng.random() < 0.5)
    lo, hi = r, span - r
    rows = np.array(INFLATE_OTHER, dtype=np.int8)[rng.integers(0, len(INFLATE_OTHER), (G_, H, W))]
    if ring:
        rows[:] = 0
    cand = rng.random((G_, H, W)) < (0.05 if density > 0 and not ring else 0.0)      # outside [lo, hi)^2: they must not trigger
    if hi > lo:
        cand[:, lo:hi, lo:hi] = rng.random((G_, hi - lo, hi - lo)) < density
        if forced:                                                    # the window's own edges and both sides of every word border
            edge = np.zeros((H, W), dtype=bool)
            cols = sorted({lo, hi - 1} | {j for j in range(lo, hi) if j % 64 in (0, 63)})
            edge[lo:hi, cols] = True
            edge[[lo, hi - 1], lo:hi] = True
            cand |= edge[None] & (rng.random((G_, H, W)) < 0.3)
    rows[cand] = np.where(rng.random(int(cand.sum())) < 0.7, 100, -1).astype(np.int8)
    maps = np.ascontiguousarray(rows if wire else rows.transpose(0, 2, 1))
    return dict(G=G_, H=H, W=W, span=span, r=r, wire=wire, density=density, forced=forced, maps=maps)


def rows_of(c):
    """The case's maps row-major, int8 [G][H][W]."""
    return c["maps"] if c["wire"] else c["maps"].transpose(0, 2, 1)


# ---------------------------------------------------------------- A* search
ASTAR_SIDES = (5, 9, 17, 31, 33, 64, 65, 100, 128, 129)
ASTAR_STYLES = ("dense", "sparse", "rooms", "box", "border")
ASTAR_BLOCKED = (100, -1, 50, 1, 99, -2, 127, -128)                     # a blocked cell holds any non-zero value
ASTAR_CAPS = (0, 1, 3, 8, 64, 512)
ASTAR_CAPS_P = (0.08, 0.06, 0.08, 0.1, 0.18, 0.5)
ASTAR_SHARES = dict(blocked=0.08, outside=0.06, same=0.05)              # of the queries; the rest go free cell to free cell
ASTAR_MAX_SLOTS, ASTAR_SLOT_BUDGET, ASTAR_SLOT_BYTES = 4096, 1 << 30, 25


def astar_slots(B, H, W):
    """The search slots of a call as astar_run computes them: query b runs in slot b % slots."""
    return max(1, min(B, ASTAR_MAX_SLOTS, ASTAR_SLOT_BUDGET // (ASTAR_SLOT_BYTES * H * W)))


def wall(m):
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = 100


def noise_map(rng, H, W, share, inflating):
    """``share`` of the cells blocked; ``inflating``: the share of those that hold 100 or -1."""
    m = np.zeros((H, W), dtype=np.int8)
    hit = rng.random((H, W)) < share
    infl = np.where(rng.random((H, W)) < 0.8, 100, -1)
    other = np.array(ASTAR_BLOCKED[2:], dtype=np.int64)[rng.integers(0, len(ASTAR_BLOCKED) - 2, (H, W))]
    m[hit] = np.where(rng.random((H, W)) < inflating, infl, other)[hit].astype(np.int8)
    return m


def rooms_map(rng, H, W):
    m = np.zeros((H, W), dtype=np.int8)
    pitch = int(rng.integers(4, 10))
    for i in range(pitch, H - 1, pitch):
        m[i, :] = 100
        for j0 in range(0, W, pitch):                                 # a door in every wall segment, two cells wide
            d = j0 + int(rng.integers(1, pitch))
            m[i, d:d + 2] = 0
    for j in range(pitch, W - 1, pitch):
        keep = m[:, j] == 0
        m[:, j] = 100
        for i0 in range(0, H, pitch):
            d = i0 + int(rng.integers(1, pitch))
            m[d:d + 2, j] = 0
        m[~keep, j] = 100
    return m


def astar_map(rng, style, H, W, r):
    """(map, box or None): box = (i0, i1, j0, j1), the rows and columns of a sealed wall around an inner region."""
    if style == "dense":
        m = noise_map(rng, H, W, rng.uniform(0.25, 0.40), 0.5)
    elif style == "rooms":
        m = rooms_map(rng, H, W)
    else:
        m = noise_map(rng, H, W, rng.uniform(0.02, 0.08 if r < 2 else 0.04), 0.8)
    box = None
    if style == "box" and min(H, W) >= 9:
        side = int(rng.integers(5, max(6, min(H, W, 48) - 3)))
        i0, j0 = int(rng.integers(1, H - side)), int(rng.integers(1, W - side))
        box = (i0, i0 + side - 1, j0, j0 + side - 1)
        inner = noise_map(rng, side, side, 0.03, 0.0)                 # a few cells that block and do not inflate
        m[i0:i0 + side, j0:j0 + side] = inner
        m[[box[0], box[1]], j0:j0 + side] = 50                        # the wall does not inflate either: the inside stays free
        m[i0:i0 + side, [box[2], box[3]]] = 50
    if style != "border":
        wall(m)
    return m, box


def case_astar(rng, seed):
    H, W = sorted(int(pick(rng, seed, ASTAR_SIDES)) for _ in range(2))
    style = ASTAR_STYLES[int(rng.integers(len(ASTAR_STYLES)))]
    r = {"dense": 0, "sparse": int(rng.integers(1, 3)), "rooms": int(rng.integers(0, 2)), "box": int(rng.integers(0, 2)),
         "border": int(rng.integers(0, 2))}[style]
    span = H if rng.random() < 0.8 else int(rng.integers(max(1, H // 2), H + 1))
    G_ = int(rng.integers(1, 5))
    wire = bool(rng.random() < 0.7)
    made = [astar_map(rng, style, H, W, r) for _ in range(G_)]
    rows = np.stack([m for m, _ in made])
    imaps = np.stack([A.inflate(m, span=span, r=r) for m in rows])
    floods = style in ("sparse", "box", "border")                     # long searches: fewer of them, for the restatement's time
    U = int(rng.integers(8, 17 if floods and H * W > 4500 else (33 if seed < SMALL or floods else 65)))
    tiled = seed % 5 == 0
    if tiled:                                                         # a period coprime to the slot count (below)
        while math.gcd(U, astar_slots(1 << 20, H, W)) != 1:
            U += 1
    moq = rng.integers(0, G_, U).astype(np.int32)
    starts, goals, what = np.empty((U, 2), np.int32), np.empty((U, 2), np.int32), []
    for u in range(U):
        im, box = imaps[moq[u]], made[moq[u]][1]
        free, shut = np.argwhere(im == 0), np.argwhere(im != 0)
        x = rng.random()
        p_b, p_o, p_s = (ASTAR_SHARES[k] for k in ("blocked", "outside", "same"))
        kind = "blocked" if x < p_b else "outside" if x < p_b + p_o else "same" if x < p_b + p_o + p_s else "free"
        inside = [] if box is None else [p for p in free if box[0] < p[0] < box[1] and box[2] < p[1] < box[3]]
        if len(free) == 0:
            kind = "blocked"
        if kind == "same" and H * W > 1500 and not inside:            # it floods its whole component: kept to small ones
            kind = "free"
        s = g = None
        if kind != "blocked" or len(shut) == 0:
            s, g = free[int(rng.integers(len(free)))], free[int(rng.integers(len(free)))]
        if kind == "blocked" and len(shut):
            bad = shut[int(rng.integers(len(shut)))]
            ok = free[int(rng.integers(len(free)))] if len(free) else bad
            s, g = (bad, ok) if rng.random() < 0.5 else (ok, bad)
        elif kind == "outside":
            out = np.array([(-1, 3), (H, 2), (2, -1), (1, W), (-5, -5), (H + 7, W + 7)][int(rng.integers(6))])
            s, g = (out, g) if rng.random() < 0.5 else (s, out)
        elif kind == "same":
            s = g = inside[int(rng.integers(len(inside)))] if inside else s
        elif inside and rng.random() < 0.5:                           # out of a sealed box (NO_PATH over its whole inside), or into it
            p = inside[int(rng.integers(len(inside)))]
            s, g = (p, g) if rng.random() < 0.7 else (s, p)
            kind = "box"
        starts[u], goals[u] = np.asarray(s) + 1, np.asarray(g) + 1   # as find_path receives them, before its -1
        what.append(kind)
    path_cap = int(ASTAR_CAPS[int(rng.choice(len(ASTAR_CAPS), p=ASTAR_CAPS_P))])
    B = U
    if tiled:
        slots = astar_slots(1 << 20, H, W)
        B = slots + U + 1 + int(rng.integers(0, U))
    return dict(G=G_, H=H, W=W, span=span, r=r, wire=wire, style=style, maps=np.ascontiguousarray(rows if wire else rows.transpose(0, 2, 1)),
                boxes=[b for _, b in made], U=U, B=B, tiled=tiled, starts=starts, goals=goals, map_of_query=moq, what=what,
                path_cap=path_cap)


def astar_batch(c):
    """(starts [B][2], goals [B][2], map_of_query [B], unique [B]): the case's query set tiled to B, query b being unique
    query b % U."""
    u = np.arange(c["B"]) % c["U"]
    return np.ascontiguousarray(c["starts"][u]), np.ascontiguousarray(c["goals"][u]), np.ascontiguousarray(c["map_of_query"][u]), u


# ---------------------------------------------------------------- DWA
DWA_STEPS = (1, 2, 11, 12, 13, 21, 24, 25, 37)                         # dwa_ref.n_steps: rows 2 .. 38 around the 12-row chunks
DWA_WINDOWS = {0: ((7, 9),), 1: ((1, 1),), 63: ((7, 9), (9, 7), (3, 21), (1, 63)), 64: ((8, 8), (4, 16), (64, 1)), 65: ((5, 13), (13, 5)),
               511: ((7, 73),), 512: ((16, 32), (32, 16)), 513: ((19, 27), (27, 19)), 1100: ((33, 33), (25, 44), (20, 55))}
DWA_WINDOW_KEYS = (0, 1, 63, 64, 65, 511, 512, 513, 1100)
DWA_OBSTACLES = (1, 2, 63, 64, 65, 200)
DWA_SAMPLES = 900                        # B * window of a case: the restatement takes about 64 us a sample
DWA_HALF_V, DWA_HALF_W = 0.1, 0.2        # max_accel * dt and max_dyawrate * dt of every config here


def case_dwa(rng, seed):
    steps = int(pick(rng, seed, DWA_STEPS))
    keys = DWA_WINDOW_KEYS[:5] if seed < SMALL else DWA_WINDOW_KEYS      # a uniform mix: the sizes take turns
    key = int(keys[seed % len(keys)])
    shapes = DWA_WINDOWS[key]
    nv, nw = shapes[int(rng.integers(len(shapes)))]
    dt = float((0.1, 0.05, 0.2)[int(rng.integers(3))])
    kind = {3: "flat", 6: "gain0"}.get(seed % 8, "plain")                # one case in eight each
    cfg = D.default_config(robot_type=int(rng.integers(2)), dt=dt, predict_time=(steps - 0.5) * dt, max_accel=DWA_HALF_V / dt,
                           max_dyawrate=DWA_HALF_W / dt, v_reso=2 * DWA_HALF_V / (nv - 0.5), yawrate_reso=2 * DWA_HALF_W / (nw - 0.5),
                           robot_radius=float(rng.uniform(0.2, 0.5)), robot_width=float(rng.uniform(0.2, 0.5)),
                           robot_length=float(rng.uniform(0.3, 0.8)), to_goal_cost_gain=float(rng.uniform(0.2, 1.5)),
                           speed_cost_gain=float(rng.uniform(0.05, 1.0)), obstacle_cost_gain=float(rng.uniform(0.3, 2.0)))
    if kind == "flat":
        cfg.update(to_goal_cost_gain=0.0, obstacle_cost_gain=0.0)
    if kind == "gain0":
        cfg.update(obstacle_cost_gain=0.0)
    B = max(1, min(int(rng.integers(1, 49 if seed >= SMALL else 25)), DWA_SAMPLES // max(nv * nw, 1)))
    M = int(pick(rng, seed, DWA_OBSTACLES))
    reach = 0.8 * steps * dt + 0.6
    states = np.zeros((B, 5))
    states[:, :2] = rng.uniform(-2.0, 2.0, (B, 2))
    states[:, 2] = rng.uniform(-math.pi, math.pi, B)
    states[:, 3] = rng.uniform(-0.5 + DWA_HALF_V, 0.8 - DWA_HALF_V, B)      # the whole window inside the speed limits
    states[:, 4] = rng.uniform(-1.5, 1.5, B)
    goals = states[:, :2] + rng.uniform(-3.0, 3.0, (B, 2))
    counts = rng.integers(1, M + 1, B).astype(np.int32)
    ob = states[:, None, :2] + rng.uniform(-reach, reach, (B, M, 2))
    what = []
    for b in range(B):
        x = rng.random()
        w = "plain"
        if (key == 0 and rng.random() < 0.6) or x < 0.07:                                     # above max_speed + max_accel dt: np.arange of a negative span
            states[b, 3] = rng.uniform(0.95, 1.2)
            w = "empty"
        elif x < 0.20:                                                # the window cut by a speed limit
            if rng.random() < 0.5:
                states[b, 3] = rng.uniform(0.72, 0.88) if rng.random() < 0.5 else rng.uniform(-0.58, -0.42)
            else:
                states[b, 4] = rng.uniform(1.6, 1.9) * (1 if rng.random() < 0.5 else -1)
            w = "clipped"
        elif x < 0.25:
            states[b, 3 + int(rng.integers(2))] = (np.inf, -np.inf, np.nan)[int(rng.integers(3))]
            w = "nonfinite"
        elif x < 0.30 and kind != "flat":
            goals[b, int(rng.integers(2))] = np.nan
            w = "nan_goal"
        elif x < 0.36 and kind != "flat":
            ob[b, int(rng.integers(counts[b]))] = states[b, :2]       # on the robot itself: row 0 of every sample collides
            w = "all_hit"
        if kind == "flat":                                            # nothing near: 0 * (1 / r) is 0 for every sample
            ob[b] = states[b, :2] + 50.0 + rng.uniform(0.0, 5.0, (M, 2))
        what.append(w)
    return dict(cfg=cfg, cfg_kind=kind, steps=steps, window=key, nv=nv, nw=nw, B=B, M=M, states=states, goals=goals, ob=ob, counts=counts,
                what=what)


def dwa_plan(c, b):
    """dwa_ref.plan of planner b, or None where the state's v or omega is not finite (the library plans an empty window
    there; the reference raises or leaves the window of its speed limits)."""
    if not np.all(np.isfinite(c["states"][b, 3:5])):
        return None
    return D.plan(c["states"][b], c["cfg"], c["goals"][b], c["ob"][b, :c["counts"][b]])


def dwa_margin(c, b, plan):
    """The smallest collision margin over the samples of planner b: |distance - radius|, or the rectangle's, over every
    (row, obstacle) pair of every sample - tests/test_gpu_dwa.py's collision_margin for all samples at once."""
    cfg, x, ob = c["cfg"], c["states"][b], c["ob"][b, :c["counts"][b]]
    dw = D.dynamic_window(x, cfg)
    vs, ws = D.arange(dw[0], dw[1], cfg["v_reso"]), D.arange(dw[2], dw[3], cfg["yawrate_reso"])
    best = np.inf
    for v in vs:
        for w in ws:
            tr = D.rollout(x, float(v), float(w), cfg, D.n_steps(cfg))
            dx, dy = np.abs(tr[:, 0] - ob[:, 0][:, None]), np.abs(tr[:, 1] - ob[:, 1][:, None])
            if int(cfg["robot_type"]) == D.RECTANGLE:
                m = np.min(np.abs(np.maximum(dx - cfg["robot_length"] / 2, dy - cfg["robot_width"] / 2)))
            else:
                m = np.min(np.abs(np.hypot(dx, dy) - cfg["robot_radius"]))
            best = min(best, float(m))
    return best


def dwa_flat(c):
    return c["cfg_kind"] == "flat"


def dwa_marked(c, b, plan):
    """Whether check_against_oracle's latitude applies to planner b, from the restatement alone: a sample whose collision
    margin is within 1e-12, or the two best finite costs within 1e-12 (relative to max(|cost|, 1)).  A flat planner's
    costs tie exactly in the reference, where the larger index wins: it is never marked."""
    if plan is None or dwa_flat(c):
        return False
    f = np.sort(plan["costs"][np.isfinite(plan["costs"])])
    if len(f) > 1 and f[1] - f[0] <= 1e-12 * max(abs(f[0]), 1.0):
        return True
    return len(plan["costs"]) > 0 and dwa_margin(c, b, plan) <= 1e-12


# ---------------------------------------------------------------- the map ray cast
RAY_SIDES = (1, 5, 31, 32, 33, 63, 64, 65, 95, 257)
RAY_N = (1, 37, 63, 64, 65, 100)
RAY_B = (1, 2, 63, 65, 300)
RAY_SKIPS = (0, 1, 2, 1 << 19)           # the last: longer than any path here
RAY_CELLS = 40000                        # B * n * cells of the longest line: the restatement walks them in Python


def case_raycast(rng, seed):
    xw, yw = int(pick(rng, seed, RAY_SIDES)), int(pick(rng, seed, RAY_SIDES))
    hit_inc = int(K.HIT_INCS[int(rng.integers(2))])
    G_ = int(rng.integers(1, 4))
    scale = float((1.0, 1.0, 2.5)[int(rng.integers(3))])
    ox, oy = (0.0, 0.0) if scale == 1.0 else (3.0, 7.0)
    maps = [K.draw_counters(xw, yw, hit_inc, sub_seed(rng))[:2] for _ in range(G_)]
    pmaps = [K.pmap_of(p, h, hit_inc) for p, h in maps]
    n, B = int(pick(rng, seed, RAY_N)), int(pick(rng, seed, RAY_B))
    long = max(xw, yw)
    max_range = float(np.float32(rng.uniform(0.3, 2.5) * max(long, 4) / scale))
    line = int(max_range * scale) + 2
    while B * n * line > RAY_CELLS:                                   # the restatement's budget: fewer beams, then fewer poses
        if n > 1 and (n >= B or B == 1):
            n = max(v for v in RAY_N if v < n)
        elif B > 1:
            B = max(v for v in RAY_B if v < B)
        else:
            max_range = float(np.float32(max_range / 2))
            line = int(max_range * scale) + 2
    ct, st = K.trig(n)
    poses, where = np.empty((B, 3)), []
    for b in range(B):
        w = ("inside", "inside", "inside", "border", "outside", "outside", "nan")[int(rng.integers(7))] if b or B == 1 else "inside"
        u, v = rng.integers(0, xw) + rng.random(), rng.integers(0, yw) + rng.random()
        if w == "border":                                             # exactly on the first cell's edge, or in the last cell
            u, v = (0.0, v) if rng.random() < 0.5 else (u, float(yw - 1) + rng.random())
        elif w == "outside":                                          # one to four cells outside, on any side
            d = 1.0 + 3.0 * rng.random()
            u, v = ((-d, v), (xw + d, v), (u, -d), (u, yw + d))[int(rng.integers(4))]
        poses[b] = (K.world(u, scale, ox), K.world(v, scale, oy), rng.uniform(-math.pi, math.pi))
        if w == "nan":
            poses[b, int(rng.integers(3))] = np.nan
        where.append(w)
    gob = rng.integers(0, G_, B).astype(np.int32)
    bad = gob.copy()                                                  # the device forms: entries that name no map
    for b in range(B):
        x = rng.random()
        if x < 0.2:
            bad[b] = -1 if x < 0.1 else G_
    shared = bool(rng.random() < 0.3)
    scan = rng.uniform(0.0, 1.2 * max_range, (n,) if shared else (B, n)).astype(np.float32)
    flat = scan.reshape(-1)
    for v in (np.inf, 0.0, 0.0):
        flat[int(rng.integers(flat.size))] = v
    skip = int(RAY_SKIPS[int(rng.integers(len(RAY_SKIPS)))])
    for _ in range(min(8, flat.size)):                                # a range that ends on the occupied cell its own beam finds
        b, i = int(rng.integers(B)), int(rng.integers(n))
        if not np.all(np.isfinite(poses[b])):
            continue
        r, _ = R.raycast(pmaps[gob[b]], scale, ox, oy, poses[b], ct[i:i + 1], st[i:i + 1], max_range, 1)
        if np.isfinite(r[0]):
            scan[i if shared else (b, i)] = r[0]
    return dict(G=G_, xw=xw, yw=yw, geom=(scale, ox, oy), hit_inc=hit_inc, maps=maps, pmaps=pmaps, n=n, B=B, ct=ct, st=st, poses=poses,
                where=where, gob=gob, gob_bad=bad, max_range=max_range, skip=skip, scan=scan)


def raycast_answer(c, gob=None):
    """(ranges, cells, counts, classes) of raycast_cases.ref_raycast / ref_score; ``gob``: another grid_of_batch."""
    gob = c["gob"] if gob is None else gob
    return K.ref_raycast(c["pmaps"], c["geom"], c["poses"], gob, c["ct"], c["st"], c["max_range"], c["skip"]) + \
        K.ref_score(c["pmaps"], c["geom"], c["poses"], gob, c["ct"], c["st"], c["scan"], c["skip"])


# ---------------------------------------------------------------- landmark extraction
LM_N = (3, 63, 64, 65, 130, 255, 256, 257, 360, 1080)
LM_N_P = (0.3, 1, 1, 1, 1, 1, 1, 1, 1, 1)  # three beams cannot close a cluster: kept, but rare
LM_RUNS = (1, 2, 3, 4, 63, 64, 65, 150)
LM_RUNS_P = (0.1, 0.1, 0.25, 0.2, 0.08, 0.08, 0.08, 0.11)
LM_S = (1, 3, 65)
LM_BEAMS = 24000                         # S * n of a case: the host class labels beam by beam
LM_UNIT = 2.0 ** -10                     # the grid of the line scans: every coordinate below 64 on it is a float32
LM_RT = (1.0, 0.5)                       # range_threshold and radius_max_th on that grid
LM_RM = (0.25, 0.125, 0.3125)
AMIN, AMAX = -3.14159, 3.14159


def line_scan(rng, n, rt, rm):
    """Ranges of a scan whose beams all point along +x (angle_min = angle_max = 0), so point i is (ranges[i], 0): runs of
    the listed lengths, each of an extent at, one grid unit below or above radius_max_th (or far from it), the gaps between
    them at, one unit below or above range_threshold (or far from it); some runs are +inf beams (30 m).  Returns the ranges
    and [(gap kind, extent kind, first, length)] of the runs."""
    u = LM_UNIT
    xs, runs, x, left = [], [], float(rng.integers(2048, 8192)) * u, n
    while left > 0:
        k = min(left, int(LM_RUNS[int(rng.choice(len(LM_RUNS), p=LM_RUNS_P))]))
        ext_kind = ("below", "at", "above", "small", "small", "wide")[int(rng.integers(6))]
        ext = {"below": rm - u, "at": rm, "above": rm + u, "small": rm / 4, "wide": min(3 * rm, rt - 2 * u)}[ext_kind]
        gap_kind = ("below", "at", "above", "far", "far", "far")[int(rng.integers(6))]
        gap = {"below": rt - u, "at": rt, "above": rt + u, "far": rt * float(rng.integers(2, 6))}[gap_kind]
        if xs:
            up = x + gap + ext < 60.0 and (rng.random() < 0.5 or x - gap - ext < 2.0)
            x = x + gap if up else x - gap - ext                      # the run after it climbs from x to x + ext
            if not up:
                gap_kind = "far"                                      # its first point is gap + ext away from the last one
        if k == 1:
            pts = [x]
        else:
            inner = np.sort(np.round(rng.uniform(0.0, ext, k - 2) / u) * u)
            pts = [x] + [x + float(v) for v in inner] + [x + ext]
        if rng.random() < 0.06:
            pts, ext_kind, gap_kind = [np.inf] * k, "inf", "inf"
        else:
            x = pts[-1]
        runs.append((gap_kind, ext_kind if k > 1 else "point", n - left, k))
        xs += pts
        left -= k
    return np.array(xs, dtype=np.float32), runs


def polar_scan(rng, n, rt):
    """Ranges over the whole circle: runs at a range of their own with a jitter of millimetres, a range_threshold or
    more apart from their neighbours; a few +inf beams."""
    out, left = [], n
    r0 = float(rng.uniform(1.0, 8.0))
    while left > 0:
        k = min(left, int(LM_RUNS[int(rng.choice(len(LM_RUNS), p=LM_RUNS_P))]))
        r0 = r0 + (1.0 if r0 < 5.0 else -1.0) * rt * float(rng.uniform(1.2, 3.0))
        out += list(r0 + rng.uniform(-0.002, 0.002, k))
        left -= k
    r = np.array(out, dtype=np.float32)
    r[rng.random(n) < 0.01] = np.inf
    return r


def case_landmarks(rng, seed):
    n = int(pick(rng, seed, LM_N, p=LM_N_P))
    S = int(pick(rng, seed, LM_S))
    while S * n > LM_BEAMS:
        S = max(v for v in LM_S if v < S)
    polar = bool(rng.random() < 0.3)
    rt, rm = float(LM_RT[int(rng.integers(len(LM_RT)))]), float(LM_RM[int(rng.integers(len(LM_RM)))])
    rows, runs = [], []
    for _ in range(S):
        if polar:
            rows.append(polar_scan(rng, n, rt))
            runs.append(None)
        else:
            row, rr = line_scan(rng, n, rt, rm)
            rows.append(row)
            runs.append(rr)
    amin, amax = (AMIN, AMAX) if polar else (0.0, 0.0)
    return dict(S=S, n=n, polar=polar, rt=rt, rm=rm, amin=amin, amax=amax, ranges=np.stack(rows), runs=runs, lm_cap=int(rng.integers(1, 9)))


def landmark_answer(c, extraction):
    """[(labels, landmark clusters)] per scan by ``extraction`` (the package's host class Extraction, its thresholds set
    here) on the points the library forms: cos / sin of linspace(amin, amax, n) times the range, +inf as 30 m."""
    ang = np.linspace(c["amin"], c["amax"], c["n"])
    ct, st = np.cos(ang), np.sin(ang)
    extraction.range_threshold, extraction.radius_max_th = c["rt"], c["rm"]
    out = []
    for row in c["ranges"]:
        r = row.astype(np.float64)
        r[np.isinf(r)] = 30.0
        out.append(extraction.labels(np.vstack([ct * r, st * r])))
    return out


# ---------------------------------------------------------------- the restatement's answer to a case
def answer(case):
    """What the restatements under tests/ (and, for the landmarks, the package's host class) say of the case.
    inflate: int64 [G][H][W]; astar: (inflated maps, [astar_ref.plan with counters per unique query]); dwa: [dwa_ref.plan
    or None per planner]; raycast: (ranges, cells, counts, classes); landmarks: [(labels, landmark clusters) per scan]."""
    kind, c = case["kind"], case
    if kind == "inflate":
        return np.stack([A.inflate(m, span=c["span"], r=c["r"]) for m in rows_of(c)])
    if kind == "astar":
        imaps = np.stack([A.inflate(m, span=c["span"], r=c["r"]) for m in rows_of(c)])
        return imaps, [A.plan(imaps[c["map_of_query"][u]], c["starts"][u], c["goals"][u], path_cap=c["path_cap"], counters=True)
                       for u in range(c["U"])]
    if kind == "dwa":
        return [dwa_plan(c, b) for b in range(c["B"])]
    if kind == "raycast":
        return raycast_answer(c)
    if kind == "landmarks":
        from conftest import pkg
        return landmark_answer(c, pkg("extraction").Extraction())
    raise KeyError(kind)


MAKERS = dict(inflate=case_inflate, astar=case_astar, dwa=case_dwa, raycast=case_raycast, landmarks=case_landmarks)


def case_of(kind, seed):
    """The case of (kind, seed): a dict of plain Python values and NumPy arrays, with "kind" and "seed" in it."""
    c = MAKERS[kind](rng_of(kind, seed), int(seed))
    c.update(kind=kind, seed=int(seed))
    return c
