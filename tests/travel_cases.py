"""Seeded cases of slam_grid_travel that the CPU and the GPU tests share (test infrastructure only), in the manner of
tests/map_cases.py:

    case_of('travel', seed)     one query: a pmap, sources, the rule's arguments, goals and a path_cap
    case_of('travel_batch', seed)  B queries routed over G maps of one shape - the 'travel' case's map of that seed, its
                                mirror and a fresh random map - with entries that name no map, a map queried twice and,
                                on a third of the seeds, a clearance; drawn from a generator of its own, so the 'travel'
                                cases stay what they were
    answer(case, pmap, field)   what tests/travel_ref.py says of it (the map read back from a device, or the case's own)
    seeds()                     range(SLAM_HYP_EXAMPLES), default 60

The maps come from the frontier patterns (tests/frontier_cases.py: serpentines, spirals, combs, blobs that touch
diagonally) and from random maps around the percolation threshold, at sizes from the edge list - one cell, one row, a
tile of 64 x 64, one more - and the arguments from their own edges; ``edges_of`` names the edges a case reaches and
tests/test_travel_cases.py asserts which ones the default seeds do."""
import os

import numpy as np

import frontier_cases as FC
import frontier_ref as F
import match_ref as M
import travel_ref as T

TILE = 64
SIZES = (1, 2, 7, 33, 63, 64, 65, 70, 130)
CAP = 16


def seeds():
    return range(int(os.environ.get("SLAM_HYP_EXAMPLES", "60")))


def random_map(rng, shape):
    """Free cells at a density around the threshold in unknown space, occupied cells at 5 to 15 %."""
    pm = FC.blank(shape)
    pm[rng.random(shape) < rng.choice((0.45, 0.6, 0.75, 0.9))] = 0
    pm[rng.random(shape) < rng.choice((0.05, 0.15))] = 100
    return pm


def spiral(xw, yw):
    """FC.spiral's walk, ended at the first leg that frees no new cell: at some sizes that walk ends in a loop over cells
    it has freed already.  The same map wherever that walk ends by itself."""
    pm = FC.blank((xw, yw))
    x, y, d = 0, 0, 0
    pm[0, 0] = 0
    inside = lambda i, j: 0 <= i < xw and 0 <= j < yw
    while True:
        dx, dy = ((0, 1), (1, 0), (0, -1), (-1, 0))[d]
        new = 0
        while inside(x + dx, y + dy) and not (inside(x + 2 * dx, y + 2 * dy) and pm[x + 2 * dx, y + 2 * dy] == 0):
            x, y = x + dx, y + dy
            new += pm[x, y] != 0
            pm[x, y] = 0
        if new == 0:
            return pm
        d = (d + 1) % 4


def rooms(rng, shape):
    """A free map cut by occupied walls with one door each, some of them closed: pockets nothing reaches."""
    pm = np.zeros(shape, dtype=np.int8)
    xw, yw = shape
    for x in range(int(rng.integers(2, 9)), xw - 1, int(rng.integers(5, 40))):
        pm[x, :] = 100
        if rng.random() < 0.7:
            pm[x, int(rng.integers(0, yw))] = 0
    pm[:, yw - 1][rng.random(xw) < 0.3] = 50
    return pm


def make(rng, seed):
    pick = lambda seq: seq[int(rng.integers(0, len(seq)))]
    family = ("random", "rooms", "serpentine", "spiral", "comb", "diagonal", "random")[seed % 7]
    small = seed < 14
    size = lambda: int(pick(SIZES[:5] if small else SIZES))
    if family == "serpentine":
        pm = FC.serpentine(max(size(), 3), max(size(), 3))
        pm = np.ascontiguousarray(pm.T) if rng.random() < 0.5 else pm
    elif family == "spiral":
        pm = spiral(size(), size())
    elif family == "comb":
        pm = FC.comb((size(), size()))
    elif family == "diagonal":
        pm = FC.diagonal_blobs()
    elif family == "rooms":
        pm = rooms(rng, (max(size(), 3), max(size(), 3)))
    else:
        pm = random_map(rng, (size(), size()))
    xw, yw = pm.shape
    free = np.argwhere(pm == 0)
    occupied = np.argwhere(pm == 100)
    S = int(pick((1, 1, 3, 64)))
    src = np.empty((S, 2), dtype=np.int32)
    for s in range(S):
        u = rng.random()
        if u < 0.15:
            src[s] = pick(((-1, 0), (xw, 0), (0, yw), (-5, -5), (xw + 3, yw - 1)))       # outside the map
        elif u < 0.3 and len(occupied):
            src[s] = pick(occupied)
        elif len(free):
            src[s] = pick(free)
        else:
            src[s] = (int(rng.integers(0, xw)), int(rng.integers(0, yw)))
    if family in ("serpentine", "spiral", "comb") and rng.random() < 0.7:
        src[0] = free[0]                                                                   # from one end: the longest way
    reps = F.frontiers(pm, radius=0, min_unknown=0, min_size=1, M=8)[1][:, 2:4]            # with its -1 padding
    extra = [pick(free) if len(free) else (0, 0) for _ in range(4)] + [src[0], (-1, -1), (xw, 0), (xw - 1, yw - 1)]
    goals = np.concatenate([reps, np.asarray(extra, dtype=np.int32).reshape(-1, 2)]).astype(np.int32)
    return dict(pmap=pm, sources=src, foot=int(pick((0, 0, 0, 1, 2, 8))), through_unknown=bool(rng.random() < 0.3),
                min_clear2=int(pick((0, 0, 0, 1, 2, 4))), cap=CAP, goals=goals, path_cap=min(int(pick((0, 1, 5, 40, 300))), xw * yw), family=family)


BATCH_CELLS = 40000      # B * cells of a batch case, but for every tenth seed


def ring_cells(T):
    """[n, 2]: the cells of T on the last or first row or column of their tile with a cell of T straight across the border."""
    xw, yw = T.shape
    out = np.zeros(T.shape, dtype=bool)
    xs, ys = np.indices(T.shape)
    out[:-1] |= T[:-1] & T[1:] & (xs[:-1] % TILE == TILE - 1)
    out[1:] |= T[1:] & T[:-1] & (xs[1:] % TILE == 0)
    out[:, :-1] |= T[:, :-1] & T[:, 1:] & (ys[:, :-1] % TILE == TILE - 1)
    out[:, 1:] |= T[:, 1:] & T[:, :-1] & (ys[:, 1:] % TILE == 0)
    return np.argwhere(out)


def make_batch(rng, seed):
    pick = lambda seq: seq[int(rng.integers(0, len(seq)))]
    one = make(np.random.default_rng([19, seed]), seed)
    pm0 = one["pmap"]
    xw, yw = pm0.shape
    G = int(rng.integers(1, 4))
    pmaps = np.stack([pm0, pm0[::-1], random_map(rng, pm0.shape)][:G])
    B = int(rng.integers(1, 7))
    if seed % 10:
        B = max(1, min(B, BATCH_CELLS // (xw * yw)))
    maps = rng.integers(0, G, B).astype(np.int32)
    if B >= 2 and rng.random() < 0.5:
        maps[int(rng.integers(1, B))] = maps[0]                                            # one map queried twice
    if rng.random() < 0.35:
        maps[int(rng.integers(0, B))] = pick((-1, G))                                      # entries that name no map
        if B >= 3:
            maps[int(rng.integers(0, B))] = pick((-1, G, G + 5))
    through, min_clear2 = bool(rng.random() < 0.3), int(pick((0, 0, 0, 0, 1, 4)))
    if min_clear2 > 0 and G >= 2 and rng.random() < 0.7:
        maps[0] = int(rng.integers(1, G))                                                  # query 0 under another map's field
    S = int(pick((1, 1, 2, 3, 64)))
    src = np.empty((B, S, 2), dtype=np.int32)
    goals = np.empty((B, 6, 2), dtype=np.int32)
    for b in range(B):
        pm = pmaps[min(max(int(maps[b]), 0), G - 1)]
        free, occupied = np.argwhere(pm == 0), np.argwhere(pm == 100)
        for s in range(S):
            u = rng.random()
            if u < 0.1:
                src[b, s] = pick(((-1, 0), (xw, 0), (0, yw), (xw + 3, yw - 1)))
            elif u < 0.2 and len(occupied):
                src[b, s] = pick(occupied)
            elif len(free):
                src[b, s] = pick(free)
            else:
                src[b, s] = (int(rng.integers(0, xw)), int(rng.integers(0, yw)))
        ring = ring_cells((pm == 0) | (through & (pm == 50)))
        if len(ring) and rng.random() < 0.5:
            src[b, 0] = pick(ring)                                                         # on a tile's border, with a way across it
        goals[b] = [pick(free) if len(free) else (0, 0) for _ in range(3)] + [src[b, 0], (-1, -1), (xw - 1, yw - 1)]
    return dict(pmaps=pmaps, maps=maps, sources=src, foot=int(pick((0, 0, 0, 1, 2, 8))), through_unknown=through,
                min_clear2=min_clear2, cap=CAP, goals=goals, path_cap=min(int(pick((0, 1, 5, 40, 300))), xw * yw), family=one["family"])


def case_of(kind, seed):
    """The case of (kind, seed): a dict of plain Python values and NumPy arrays, with "kind" and "seed" in it."""
    assert kind in ("travel", "travel_batch")
    if kind == "travel":
        c = make(np.random.default_rng([19, int(seed)]), int(seed))
    else:
        c = make_batch(np.random.default_rng([19, int(seed), 1]), int(seed))
    c.update(kind=kind, seed=int(seed))
    return c


def rule_of(case, **kw):
    """The rule's arguments of a case as keywords, for travel_ref.batch and grid_travel_host alike."""
    out = dict(foot=case["foot"], through_unknown=case["through_unknown"], min_clear2=case["min_clear2"], path_cap=case["path_cap"])
    out.update(kw)
    return out


def answer_batch(case, pmaps=None, fields=None, with_T=False):
    """tests/travel_ref.py on a 'travel_batch' case: the arrays of grid_travel_host, stacked over the queries; ``with_T``:
    also the list of each query's traversable set (None where it names no map)."""
    pm = case["pmaps"] if pmaps is None else pmaps
    if fields is None and case["min_clear2"] > 0:
        fields = np.stack([M.field(p, case["cap"]) for p in pm])
    out = T.batch(pm, case["sources"], maps=case["maps"], fields=fields, goals=case["goals"], **rule_of(case))
    if with_T:
        out["T"] = [T.traversable(pm[g], None if fields is None else fields[g], case["sources"][b], case["foot"], case["through_unknown"],
                                  case["min_clear2"]) if 0 <= g < len(pm) else None for b, g in enumerate(case["maps"])]
        out["fields"] = fields
    return out


def answer(case, pmap=None, field=None):
    """tests/travel_ref.py on the case; ``pmap`` / ``field``: the map and its field read back from a device."""
    if case["kind"] == "travel_batch":
        return answer_batch(case, pmap, field, with_T=True)
    pm = case["pmap"] if pmap is None else pmap
    if field is None and case["min_clear2"] > 0:
        field = M.field(pm, case["cap"])
    return T.answer(pm, field, case["sources"], case["foot"], case["through_unknown"], case["min_clear2"], case["goals"], case["path_cap"])


def tile_runs(cells):
    """The tiles a path visits, one entry per run of consecutive cells in the same tile."""
    runs = []
    for x, y in cells:
        t = (int(x) // TILE, int(y) // TILE)
        if not runs or runs[-1] != t:
            runs.append(t)
    return runs


def batch_edges_of(case, ans):
    """The names of the edges a 'travel_batch' case reaches (``ans``: answer_batch(case, with_T=True))."""
    pm, maps, src = case["pmaps"], case["maps"], case["sources"]
    G, (xw, yw) = len(pm), pm.shape[1:]
    named = [b for b, g in enumerate(maps) if 0 <= g < G]
    out = set()
    if len(named) < len(maps):
        out.add("a query that names no map")
    for i, b in enumerate(named):
        if any(maps[b] == maps[c] and not np.array_equal(src[b], src[c]) for c in named[:i]):
            out.add("one map queried twice")
    for b in named:
        g = int(maps[b])
        if case["min_clear2"] > 0 and g != b and b < G:
            other = T.traversable(pm[g], ans["fields"][b], src[b], case["foot"], case["through_unknown"], case["min_clear2"])
            if not np.array_equal(other, ans["T"][b]):
                out.add("a routed query under a clearance whose map's field differs from map b's")
        Tm = ans["T"][b]
        for x, y in T.valid_sources((xw, yw), src[b]):
            for dx, dy, on in ((1, 0, x % TILE == TILE - 1), (-1, 0, x % TILE == 0), (0, 1, y % TILE == TILE - 1), (0, -1, y % TILE == 0)):
                if on and 0 <= x + dx < xw and 0 <= y + dy < yw and Tm[x + dx, y + dy]:
                    out.add("a source on the last or first row or column of its tile with a traversable cell across the border")
    return out


def edges_of(case, ans):
    """The names of the edges this case reaches."""
    if case["kind"] == "travel_batch":
        return batch_edges_of(case, ans)
    pm, src = case["pmap"], case["sources"]
    xw, yw = pm.shape
    inside = [(x, y) for x, y in src if 0 <= x < xw and 0 <= y < yw]
    out = set()
    if any(pm[x, y] == 100 for x, y in inside):
        out.add("source on an occupied cell")
    if len(inside) < len(src):
        out.add("source outside the map")
    if not inside:
        out.add("no valid source")
    Tm, cost, d = ans["T"], ans["cost"], ans["dir"]
    ok = T.allowed(Tm)
    # a diagonal step between two reached cells of T that only the corner rule forbids
    for k, (dx, dy) in enumerate(T.MOVES[4:], start=4):
        P = np.zeros((xw + 2, yw + 2), dtype=bool)
        P[1:-1, 1:-1] = Tm & (cost >= 0)
        if np.any(Tm & (cost >= 0) & P[1 + dx:1 + dx + xw, 1 + dy:1 + dy + yw] & ~ok[k]):
            out.add("a diagonal wall")
    reps = case["goals"][:8]
    kept = reps[reps[:, 0] >= 0]
    if len(kept) and np.any(ans["goal_cost"][:8][reps[:, 0] >= 0] < 0):
        out.add("a goal that is unreachable while frontiers exist")
    # ties: more than one move leads back at the same cost
    P = np.full((xw + 2, yw + 2), -1, dtype=np.int64)
    P[1:-1, 1:-1] = cost
    n = np.zeros((xw, yw), dtype=np.int32)
    for k, (dx, dy) in enumerate(T.MOVES):
        nb = P[1 + dx:1 + dx + xw, 1 + dy:1 + dy + yw]
        n += ok[k] & (cost > 0) & (nb >= 0) & (nb + T.WEIGHTS[k] == cost)
    if np.any(n > 1):
        out.add("cost ties that dir must break")
    if np.any(ans["path_len"] > case["path_cap"]):
        out.add("a path longer than path_cap")
    for g in case["goals"]:
        runs = tile_runs(T.path(cost, d, g))
        if len(set(runs)) < len(runs):
            out.add("a tile re-activated after its neighbour improved")
    return out


# ------------------------------------------------------------------ the device side
KEYS = ("status", "cost", "dir", "goal_cost", "path_len", "path")
DTYPES = dict(status=np.int32, cost=np.int32, dir=np.int8, goal_cost=np.int32, path_len=np.int32, path=np.int32)


def same(got, want, tag=""):
    for k in KEYS:
        if k not in want:
            continue
        a, b = got[k], want[k]
        assert a.dtype == DTYPES[k] and a.shape == b.shape, (tag, k, a.dtype, a.shape, b.shape)
        assert np.array_equal(a, b), (tag, k, np.argwhere(a != b)[:5], a[a != b][:5], b[a != b][:5])


def check(slam, g, pmaps, sources, maps=None, fields=None, goals=None, path_cap=0, foot=0, through_unknown=False, min_clear2=0, cap=CAP):
    """The host form with every output against the restatement on the pmaps (and fields) read back; every named map
    answers with status 0."""
    src = np.asarray(sources, dtype=np.int32)
    want = T.batch(pmaps, src, maps=maps, fields=fields, goals=goals, path_cap=path_cap, foot=foot, through_unknown=through_unknown,
                   min_clear2=min_clear2)
    got = slam.grid_travel_host(g, src, grid_of_batch=maps, goals=goals, foot=foot, through_unknown=through_unknown, min_clear2=min_clear2,
                                cap=cap, path_cap=path_cap, cost=True, dirs=True)
    if goals is not None and path_cap == 0:
        got["path"] = np.full(want["path"].shape, -1, dtype=np.int32)
    same(got, want)
    named = np.array([0 <= gi < np.asarray(pmaps).shape[0] for gi in (range(src.shape[0]) if maps is None else maps)])
    assert np.array_equal(got["status"], np.where(named, 0, -1))
    return got
