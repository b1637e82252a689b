"""The seeded cases of tests/plan_cases.py without a device: every case builds and the restatement answers it in time,
two independent statements of the inflation and of the search agree, and the sweep reaches the edges it was written for.

The GPU file (tests/test_gpu_plan_properties.py) runs exactly these cases, so what is asserted here about the default 60
seeds - that enough of them block a trigger from another word, reuse a search slot after a long NO_PATH, tie a DWA window
exactly, find a cell in a row's last mask word, run a cluster across a trip of 256 lanes - is what that file can be trusted
to have exercised.  The thresholds are named constants, set from what the restatements report here, never from a device.
Every message carries (kind, seed): plan_cases.case_of(kind, seed) rebuilds the case."""
import functools
import time

import numpy as np
import pytest

import astar_ref as A
import dwa_ref as D
import plan_cases as P
import raycast_cases as K
import raycast_ref as R
from test_map_cases import same_case

DEFAULT = 60                                # the seeds over which the edge reach is asserted, whatever SLAM_HYP_EXAMPLES says
N = len(P.seeds())
KIND_SECONDS = 5.0 * max(N, DEFAULT) / DEFAULT     # a kind's restatement answers: 5 s per 60 seeds (scaled when soaking)
FILE_SECONDS = 60.0 * max(N, DEFAULT) / DEFAULT    # and a minute for the whole file
TRIVIAL = 0.15                              # at most this share of a kind's cases may be trivial (defined at each kind below)
_spent = []


@functools.lru_cache(maxsize=None)
def solved(kind, n):
    """(cases, answers, seconds the restatement took) of seeds 0 .. n - 1; each (kind, n) is worked out once."""
    cases = [P.case_of(kind, s) for s in range(n)]
    t = time.perf_counter()
    answers = [P.answer(c) for c in cases]
    return cases, answers, time.perf_counter() - t


def default(kind):
    cases, answers, _ = solved(kind, max(N, DEFAULT))
    return list(zip(cases[:DEFAULT], answers[:DEFAULT]))


def sweep(kind):
    cases, answers, _ = solved(kind, max(N, DEFAULT))
    return list(zip(cases[:N], answers[:N]))


def tag(c):
    return (c["kind"], c["seed"])


def count(kind, pred):
    return sum(1 for c, a in default(kind) if pred(c, a))


def show(name, value):
    print("reach %-28s %s" % (name, value))
    return value


@pytest.fixture(autouse=True)
def _clock():
    t = time.perf_counter()
    yield
    _spent.append(time.perf_counter() - t)


# ------------------------------------------------------------------ the cases build, and in time
@pytest.mark.parametrize("kind", P.KINDS)
def test_cases_build_and_the_restatement_answers_in_time(kind):
    cases, answers, seconds = solved(kind, max(N, DEFAULT))
    print("%s: %d restatement answers in %.2f s" % (kind, len(cases), seconds))
    assert len(cases) == len(answers) and seconds < KIND_SECONDS, (kind, seconds)
    for c in cases:
        assert c["kind"] == kind and P.case_of(kind, c["seed"]).keys() == c.keys(), tag(c)


def same_value(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same_value(a[k], b[k]) for k in a)
    if a is None or b is None:
        return a is b
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same_value(x, y) for x, y in zip(a, b))
    return same_case(a, b)


@pytest.mark.parametrize("kind", P.KINDS)
def test_a_case_is_a_pure_function_of_kind_and_seed(kind):
    for seed in (0, 7, 19, 20, 41, 57):
        a, b = P.case_of(kind, seed), P.case_of(kind, seed)
        assert all(same_value(a[k], b[k]) for k in a), (kind, seed)
    one, two = P.case_of(kind, 1), P.case_of(kind, 2)
    assert not all(same_value(one[k], two[k]) for k in one if k != "kind")


def test_kind_ids_are_apart_from_the_first_sweeps():
    import map_cases
    assert not set(P.KIND_ID.values()) & set(map_cases.KIND_ID.values()) and len(set(P.KIND_ID.values())) == len(P.KINDS)


def test_small_seeds_draw_small_shapes():
    """Seeds below 20 take every size from the lower half of its list (or of its range)."""
    for s in range(P.SMALL):
        c = P.case_of("inflate", s)
        assert c["span"] <= 150 and c["r"] <= 31 and c["W"] <= 150 + 128, tag(c)
        c = P.case_of("astar", s)
        assert c["W"] <= 33 and c["U"] <= 33, tag(c)
        c = P.case_of("dwa", s)
        assert c["steps"] <= 13 and c["nv"] * c["nw"] <= 65 and c["M"] <= 63 and c["B"] <= 24, tag(c)
        c = P.case_of("raycast", s)
        assert max(c["xw"], c["yw"]) <= 33 and c["n"] <= 63 and c["B"] <= 63, tag(c)
        c = P.case_of("landmarks", s)
        assert c["n"] <= 130 and c["S"] <= 3, tag(c)


# ------------------------------------------------------------------ the bounds the entry points document
def test_cases_stay_inside_their_bounds():
    for c, _ in sweep("inflate"):
        assert 1 <= c["G"] <= 3 and 1 <= c["span"] <= c["H"] <= c["W"] and c["r"] >= 0 and c["span"] <= 4096, tag(c)
        assert c["maps"].dtype == np.int8 and c["maps"].shape == ((c["G"], c["H"], c["W"]) if c["wire"] else (c["G"], c["W"], c["H"])), tag(c)
    for c, _ in sweep("astar"):
        assert 1 <= c["G"] <= 4 and 1 <= c["span"] <= c["H"] <= c["W"] <= 129 and c["H"] >= 5 and 0 <= c["r"] <= 2, tag(c)
        assert 8 <= c["U"] <= 67 and np.all((c["map_of_query"] >= 0) & (c["map_of_query"] < c["G"])), tag(c)
        assert c["B"] == c["U"] or (c["tiled"] and c["B"] > P.astar_slots(c["B"], c["H"], c["W"])), tag(c)
        assert c["B"] * max(c["path_cap"], 1) * 8 <= 1 << 26, tag(c)
    for c, _ in sweep("dwa"):
        assert 1 <= c["B"] <= 48 and 1 <= c["M"] <= 200 and np.all((c["counts"] >= 1) & (c["counts"] <= c["M"])), tag(c)
        assert c["B"] * c["nv"] * c["nw"] <= max(P.DWA_SAMPLES, c["nv"] * c["nw"]), tag(c)
        assert D.n_steps(c["cfg"]) == c["steps"] and all(np.isfinite(v) for v in c["cfg"].values()), tag(c)
    for c, _ in sweep("raycast"):
        assert 1 <= c["n"] <= 4096 and c["B"] >= 1 and 0 <= c["skip"] <= 1 << 20 and c["max_range"] > 0 and np.isfinite(c["max_range"]), tag(c)
        assert np.all((c["gob"] >= 0) & (c["gob"] < c["G"])) and c["scan"].shape in ((c["n"],), (c["B"], c["n"])), tag(c)
    for c, _ in sweep("landmarks"):
        assert c["ranges"].shape == (c["S"], c["n"]) and c["ranges"].dtype == np.float32 and not np.any(np.isnan(c["ranges"])), tag(c)
        assert 1 <= c["lm_cap"] <= 8 and c["S"] * c["n"] <= P.LM_BEAMS and c["n"] <= 1080, tag(c)


# ------------------------------------------------------------------ reference against reference
LITERAL_SPAN = 130      # the literal loops run where they are cheap: inflation up to this span,
LITERAL_SIDE = 40       # the list search on maps up to this side


def literal_inflate(m, span, r):
    """start_find's loop as it reads (:149-155), in place."""
    m = np.array(m, dtype=np.int64)
    for i in range(r, span - r):
        for j in range(r, span - r):
            if m[i][j] == 100 or m[i][j] == -1:
                m[i - r:i + r + 1, j - r:j + r + 1] = 99
    return m


def test_inflation_by_the_literal_loop_is_the_trigger_set():
    done = 0
    for c, a in sweep("inflate"):
        if c["span"] <= LITERAL_SPAN:
            for gi, m in enumerate(P.rows_of(c)):
                assert np.array_equal(literal_inflate(m, c["span"], c["r"]), a[gi]), tag(c) + (gi,)
            done += 1
    assert done >= N // 3


def literal_plan(imap, start, goal):
    """start_find's search as it reads (:157-223): lists, find_min_cost_f's scan, find_index, remove.  The rules that are
    the restatement's own are kept: a start or goal outside the map and the expansion of a border cell give EDGE (the
    reference wraps or raises there), an empty open list gives NO_PATH (the reference raises)."""
    H, W = imap.shape
    s, g = (int(start[0]) - 1, int(start[1]) - 1), (int(goal[0]) - 1, int(goal[1]) - 1)
    inside = lambda p: 0 <= p[0] < H and 0 <= p[1] < W
    if not inside(s):
        return A.EDGE, [], 0
    if imap[s] != 0:
        return A.INVALID_START, [], 0
    if not inside(g):
        return A.EDGE, [], 0
    if imap[g] != 0:
        return A.INVALID_GOAL, [], 0
    state = np.zeros((H, W), dtype=int)
    open_list, close_list = [], []

    def around(c, cost_g):
        if c[0] in (0, H - 1) or c[1] in (0, W - 1):
            return False
        for i in (-1, 0, 1):
            for j in (-1, 0, 1):
                if i == 0 and j == 0:
                    continue
                x, y = c[0] + i, c[1] + j
                if imap[x][y] == 0 and state[x][y] != 3:
                    node = dict(x=x, y=y, g=10 + cost_g, parent=c)
                    node["f"] = node["g"] + (abs(g[0] - x) + abs(g[1] - y)) * 10
                    if state[x][y] == 2:
                        k = next(k for k, o in enumerate(open_list) if o["x"] == x and o["y"] == y)
                        if open_list[k]["f"] > node["f"]:
                            open_list[k] = node
                    else:
                        state[x][y] = 2
                        open_list.append(node)
        return True

    if not around(s, 0):
        return A.EDGE, [], 0
    state[s] = 3
    close_list.append(dict(x=s[0], y=s[1], parent=None))
    while True:
        if not open_list:
            return A.NO_PATH, [], len(close_list)
        min_cost, k_min = 100000, 0
        for k, o in enumerate(open_list):
            if o["f"] < min_cost:
                min_cost, k_min = o["f"], k
        cur = open_list[k_min]
        if (cur["x"], cur["y"]) == g:
            path, node = [], cur
            while True:
                path.append((node["x"], node["y"]))
                if (node["x"], node["y"]) == s:
                    break
                node = next(o for o in close_list if (o["x"], o["y"]) == node["parent"])
            return A.OK, path[::-1], len(close_list)
        if not around((cur["x"], cur["y"]), cur["g"]):
            return A.EDGE, [], len(close_list)
        state[cur["x"]][cur["y"]] = 3
        close_list.append(cur)
        del open_list[k_min]                                          # remove(current_node): the object itself


def test_search_with_lists_is_search_with_a_heap():
    done = 0
    for c, (imaps, plans) in sweep("astar"):
        if c["W"] > LITERAL_SIDE:
            continue
        for u, p in enumerate(plans):
            st, path, closed = literal_plan(imaps[c["map_of_query"][u]], c["starts"][u], c["goals"][u])
            want = A.TRUNCATED if st == A.OK and len(path) > c["path_cap"] else st
            assert (want, len(path), closed) == (p["status"], p["length"], p["expansions"]), tag(c) + (u,)
            assert path == [tuple(v) for v in p["path"].tolist()], tag(c) + (u,)
        done += 1
    assert done >= N // 5


def test_counters_leave_the_answers_alone():
    for c, (imaps, plans) in sweep("astar")[:20]:
        stats = {}
        for gi, m in enumerate(P.rows_of(c)):
            assert np.array_equal(A.inflate(m, span=c["span"], r=c["r"], counters=stats), imaps[gi]), tag(c)
        for u in range(0, c["U"], 5):
            plain = A.plan(imaps[c["map_of_query"][u]], c["starts"][u], c["goals"][u], path_cap=c["path_cap"])
            assert set(plans[u]) - set(plain) == {"replacements", "max_open"}, tag(c)
            assert all(same_value(plain[k], plans[u][k]) for k in plain), tag(c) + (u,)


# ------------------------------------------------------------------ edge reach over the default 60 seeds: inflation
INFLATE_HEAVY = 6       # r >= 31 under 30 % candidates or more: long shifts of dense words, the `lim >= 63` shortcut
INFLATE_ABOVE = 30      # a candidate under the window of a trigger of an earlier row: the ring of dilated rows decides
INFLATE_FAR_LEFT = 10   # a candidate blocked by a trigger of its own row that lies in another 64-column word
INFLATE_NO_ROW = 1      # span - r <= r: nothing can trigger, the row walk is not launched (and at most 8 such cases)
INFLATE_RING = 3        # the ring of dilated rows in global memory
INFLATE_LAYOUT = 20     # of each of the two layouts
INFLATE_SHORT = 10      # span < H, and H < W: rows and columns the window must leave alone


@functools.lru_cache(maxsize=None)
def inflate_stats(seed):
    c = P.case_of("inflate", seed)
    total = dict(candidates=0, triggers=0, blocked_above=0, blocked_left=0, blocked_left_far=0)
    for m in P.rows_of(c):
        s = {}
        A.inflate(m, span=c["span"], r=c["r"], counters=s)
        total = {k: total[k] + s[k] for k in total}
    return total


def test_inflate_reach():
    st = lambda c: inflate_stats(c["seed"])
    assert show("inflate heavy", count("inflate", lambda c, a: c["r"] >= 31 and c["density"] >= 0.3 and st(c)["triggers"] > 0)) >= INFLATE_HEAVY
    assert show("inflate above", count("inflate", lambda c, a: st(c)["blocked_above"] > 0)) >= INFLATE_ABOVE
    assert show("inflate far left", count("inflate", lambda c, a: st(c)["blocked_left_far"] > 0)) >= INFLATE_FAR_LEFT
    assert INFLATE_NO_ROW <= show("inflate no row", count("inflate", lambda c, a: c["span"] - c["r"] <= c["r"])) <= 8
    assert show("inflate ring", count("inflate", lambda c, a: P.global_ring(c["span"], c["r"]))) >= INFLATE_RING
    for wire in (True, False):
        assert show("inflate wire %s" % wire, count("inflate", lambda c, a: c["wire"] == wire)) >= INFLATE_LAYOUT, wire
    assert show("inflate span < H", count("inflate", lambda c, a: c["span"] < c["H"])) >= INFLATE_SHORT
    assert show("inflate H < W", count("inflate", lambda c, a: c["H"] < c["W"])) >= INFLATE_SHORT
    # trivial: no cell triggers, so the output is the input
    assert show("inflate trivial", count("inflate", lambda c, a: st(c)["triggers"] == 0)) <= TRIVIAL * DEFAULT


# ------------------------------------------------------------------ A* search
ASTAR_STATUS = {A.OK: 35, A.INVALID_START: 20, A.INVALID_GOAL: 20, A.NO_PATH: 18, A.EDGE: 35, A.TRUNCATED: 18}   # cases with a query of it
ASTAR_REPLACED = 35     # cases with a query that replaces an open entry in place
ASTAR_OPEN_64 = 25      # cases with an open list past one wave's stride
ASTAR_OPEN_128 = 10     # and past two
ASTAR_LONG_NO_PATH = 5  # cases with a NO_PATH after 500 expansions or more: a large closed list for the slot's reset to walk
ASTAR_TILED = 12        # cases whose batch is longer than the search slots: every slot serves a second, different query
ASTAR_MAPS = 28         # cases with several maps and a map_of_query that is not sorted


def test_astar_reach():
    def has(c, a, pred):
        return any(pred(p) for p in a[1])

    for status, least in ASTAR_STATUS.items():
        assert show("astar " + A.STATUS_NAMES[status], count("astar", lambda c, a: has(c, a, lambda p: p["status"] == status))) >= least
    assert show("astar replaced", count("astar", lambda c, a: has(c, a, lambda p: p["replacements"] > 0))) >= ASTAR_REPLACED
    assert show("astar open > 64", count("astar", lambda c, a: has(c, a, lambda p: p["max_open"] > 64))) >= ASTAR_OPEN_64
    assert show("astar open > 128", count("astar", lambda c, a: has(c, a, lambda p: p["max_open"] > 128))) >= ASTAR_OPEN_128
    long_no_path = lambda p: p["status"] == A.NO_PATH and p["expansions"] >= 500
    assert show("astar long NO_PATH", count("astar", lambda c, a: has(c, a, long_no_path))) >= ASTAR_LONG_NO_PATH
    assert show("astar tiled", count("astar", lambda c, a: c["tiled"] and c["B"] > P.astar_slots(c["B"], c["H"], c["W"]))) >= ASTAR_TILED
    assert show("astar maps", count("astar", lambda c, a: c["G"] > 1 and bool(np.any(np.diff(c["map_of_query"]) < 0)))) >= ASTAR_MAPS
    # trivial: every inflated map all free or all blocked
    assert show("astar trivial", count("astar", lambda c, a: all(np.all(m == 0) or np.all(m != 0) for m in a[0]))) <= TRIVIAL * DEFAULT


def test_a_tiled_batch_hands_every_slot_a_different_query():
    for c, _ in sweep("astar"):
        if c["tiled"]:
            slots = P.astar_slots(c["B"], c["H"], c["W"])
            u = P.astar_batch(c)[3]
            assert c["B"] > slots and np.all(u[slots:] != u[:c["B"] - slots]), tag(c)


# ------------------------------------------------------------------ DWA
DWA_STEP_EDGE = 3       # cases at each of the row counts around the 12-row chunk
DWA_WINDOW_EDGE = 4     # cases at each window size around the 64 and 512 lanes
DWA_FLAT = 6            # cases whose planners' costs tie exactly across omega in the reference: the larger index must win
DWA_FLAT_TIES = 20      # flat planners with more than one omega sample, over all those cases
DWA_MARKED = 0.01       # check_against_oracle's latitude is a condition: at most this share of all planners may meet it
DWA_SPECIAL = 12        # planners of each special kind: NaN goal, non-finite speed, every sample colliding, a cut window


def test_dwa_reach():
    for steps in P.DWA_STEPS:
        assert show("dwa steps %d" % steps, count("dwa", lambda c, a: c["steps"] == steps)) >= DWA_STEP_EDGE, steps
    for key in P.DWA_WINDOW_KEYS:
        assert show("dwa window %d" % key, count("dwa", lambda c, a: c["window"] == key)) >= DWA_WINDOW_EDGE, key
    # the window the configuration was drawn for is the window the reference plans, on every planner whose speeds lie inside
    for c, a in default("dwa"):
        for b, p in enumerate(a):
            if c["what"][b] in ("plain", "nan_goal", "all_hit"):
                assert (p["nv"], p["nw"]) == (c["nv"], c["nw"]), tag(c) + (b,)
            if c["what"][b] == "empty":
                assert p["nv"] * p["nw"] == 0 and p["index"] == -1, tag(c) + (b,)
    for robot in (D.CIRCLE, D.RECTANGLE):
        assert show("dwa robot %d" % robot, count("dwa", lambda c, a: int(c["cfg"]["robot_type"]) == robot)) >= 20, robot
    assert show("dwa flat cases", count("dwa", lambda c, a: P.dwa_flat(c))) >= DWA_FLAT
    ties = 0
    for c, a in default("dwa"):
        if P.dwa_flat(c):
            for b, p in enumerate(a):
                if p is not None and p["nw"] > 1 and p["nv"] > 0:     # the best v's whole omega row ties, and its last sample wins
                    row = p["costs"][(p["nv"] - 1) * p["nw"]:]
                    assert np.all(row == row[0]) and p["index"] == p["nv"] * p["nw"] - 1, tag(c) + (b,)
                    ties += 1
    assert show("dwa flat ties", ties) >= DWA_FLAT_TIES
    for kind in ("nan_goal", "nonfinite", "all_hit", "clipped", "empty"):
        assert show("dwa " + kind, sum(c["what"].count(kind) for c, _ in default("dwa"))) >= DWA_SPECIAL, kind
    for c, a in default("dwa"):
        for b, p in enumerate(a):
            if c["what"][b] == "all_hit":                             # row 0 of every sample collides: inf, or 0 * inf
                assert np.all(np.isinf(p["costs"]) | np.isnan(p["costs"])), tag(c) + (b,)
    gain0 = lambda c, a: c["cfg_kind"] == "gain0" and any(p is not None and bool(np.any(np.isnan(p["costs"]))) for p in a)
    assert show("dwa gain 0 with collisions", count("dwa", gain0)) >= 2
    # trivial: no planner has a sample
    assert show("dwa trivial", count("dwa", lambda c, a: all(p is None or p["nv"] * p["nw"] == 0 for p in a))) <= TRIVIAL * DEFAULT


def test_the_restatement_is_sure_of_the_dwa_cases():
    planners = marked = 0
    for c, a in default("dwa"):
        for b, p in enumerate(a):
            planners += 1
            marked += P.dwa_marked(c, b, p)
    show("dwa marked planners", (marked, planners))
    assert marked <= DWA_MARKED * planners, (marked, planners)


# ------------------------------------------------------------------ the map ray cast
RAY_FLAGGED = 40        # cases with a cast line walked end -> start, and as many with one walked start -> end
RAY_CLASS = {R.EMPTY: 35, R.HIT: 20, R.BLOCKED: 22, R.FREE: 20, R.UNKNOWN: 28, R.OUT: 32, R.BAD: 14}   # cases with a beam of it
RAY_LAST_WORD = 8       # cases with a cell found in the last mask word of a row that has more than one
RAY_OUTSIDE = 15        # cases with a pose outside the map
RAY_SKIP = 8            # cases of each skip
RAY_MAPS = 8            # cases with several maps and a grid_of_batch that is not sorted
RAY_ON_CELL = 15        # cases with a scored range that ends on the occupied cell its own beam finds


def test_raycast_reach():
    def flagged(c):
        return K.flagged_of(c["poses"], c["ct"], c["st"], c["max_range"], c["geom"])

    def lines(c):
        return np.array([[bool(np.all(np.isfinite(p)))] * c["n"] for p in c["poses"]])

    assert show("ray flagged", count("raycast", lambda c, a: bool(np.any(flagged(c))))) >= RAY_FLAGGED
    assert show("ray unflagged", count("raycast", lambda c, a: bool(np.any(~flagged(c) & lines(c))))) >= RAY_FLAGGED
    for cls, least in RAY_CLASS.items():
        assert show("ray class %d" % cls, count("raycast", lambda c, a: bool(np.any(a[3] == cls)))) >= least, cls
    last_word = lambda c, a: c["yw"] > 32 and bool(np.any(a[1][..., 1] // 32 == (c["yw"] - 1) // 32))
    assert show("ray last word", count("raycast", last_word)) >= RAY_LAST_WORD
    assert show("ray outside", count("raycast", lambda c, a: "outside" in c["where"])) >= RAY_OUTSIDE
    for skip in P.RAY_SKIPS:
        assert show("ray skip %d" % skip, count("raycast", lambda c, a: c["skip"] == skip)) >= RAY_SKIP, skip
    for h in K.HIT_INCS:
        assert show("ray hit_inc %d" % h, count("raycast", lambda c, a: c["hit_inc"] == h)) >= 20, h
    assert show("ray maps", count("raycast", lambda c, a: c["G"] > 1 and bool(np.any(np.diff(c["gob"]) < 0)))) >= RAY_MAPS
    assert show("ray bad entries", count("raycast", lambda c, a: bool(np.any((c["gob_bad"] < 0) | (c["gob_bad"] >= c["G"]))))) >= 20
    on_cell = lambda c, a: bool(np.any((a[3] == R.HIT) & (np.broadcast_to(c["scan"], a[0].shape) == a[0])))
    assert show("ray on cell", count("raycast", on_cell)) >= RAY_ON_CELL
    # trivial: every map all occupied or without an occupied cell
    trivial = lambda c, a: all(bool(np.all(p == 100)) or not np.any(p == 100) for p in c["pmaps"])
    assert show("ray trivial", count("raycast", trivial)) <= TRIVIAL * DEFAULT


# ------------------------------------------------------------------ landmark extraction
LM_WAVE = 25            # cases with a closed cluster of three or more beams across a multiple of 64: two strides of a wave's lanes
LM_TRIP = 7             # cases with one across a multiple of 256: two trips of the workgroup's prefix count
LM_OVERFLOW = 12        # cases with a scan of more landmarks than lm_cap
LM_SIDES = 15           # cases with a gap (an extent) one unit below, at and one unit above its threshold, each
LM_LANDMARK = 25        # cases with a landmark at all


def closed_clusters(c, a):
    """[(first, last)] per scan of the clusters that a break closes with two earlier members - those whose extent is
    tested - from the gaps themselves; Extraction's labels give each of them one number."""
    out = []
    for row, (labels, _) in zip(c["ranges"], a):
        r = row.astype(np.float64)
        r[np.isinf(r)] = 30.0
        ang = np.linspace(c["amin"], c["amax"], c["n"])
        x, y = np.cos(ang) * r, np.sin(ang) * r
        brk = ~(np.sqrt((x[:-1] - x[1:]) ** 2 + (y[:-1] - y[1:]) ** 2) < c["rt"])
        cl, first = [], 0
        for i in np.flatnonzero(brk):
            if i - first >= 2:
                assert labels[first] == labels[i] >= 0, tag(c)
                cl.append((first, int(i)))
            first = int(i) + 1
        out.append(cl)
    return out


def test_landmark_reach():
    def across(c, a, step):
        return any(f // step != l // step for cl in closed_clusters(c, a) for f, l in cl)

    def sides(c, what, k):
        return not c["polar"] and any(run[what] == k and (what == 0 or run[3] >= 3) for runs in c["runs"] for run in runs)

    assert show("lm across 64", count("landmarks", lambda c, a: across(c, a, 64))) >= LM_WAVE
    assert show("lm across 256", count("landmarks", lambda c, a: across(c, a, 256))) >= LM_TRIP
    assert show("lm overflow", count("landmarks", lambda c, a: any(len(found) > c["lm_cap"] for _, found in a))) >= LM_OVERFLOW
    for k in ("below", "at", "above"):
        assert show("lm gap " + k, count("landmarks", lambda c, a: sides(c, 0, k))) >= LM_SIDES, ("gap", k)
        assert show("lm extent " + k, count("landmarks", lambda c, a: sides(c, 1, k))) >= LM_SIDES, ("extent", k)
    assert show("lm landmark", count("landmarks", lambda c, a: any(found for _, found in a))) >= LM_LANDMARK
    assert show("lm inf", count("landmarks", lambda c, a: bool(np.any(np.isinf(c["ranges"]))))) >= 15
    assert show("lm polar", count("landmarks", lambda c, a: c["polar"])) >= 10
    for s in P.LM_S:
        assert show("lm S %d" % s, count("landmarks", lambda c, a: c["S"] == s)) >= 8, s
    # trivial: no scan with a closed cluster of three beams or more
    assert show("lm trivial", count("landmarks", lambda c, a: not any(closed_clusters(c, a)))) <= TRIVIAL * DEFAULT


def test_line_scans_sit_on_their_thresholds():
    """An extent or a gap drawn at its threshold is exactly that in float64, and one grid unit to each side exactly that
    too: the float32 ranges hold every coordinate of a line scan."""
    for c, a in default("landmarks"):
        if c["polar"]:
            continue
        for row, runs in zip(c["ranges"], c["runs"]):
            for gap_kind, ext_kind, first, k in runs:
                if ext_kind in ("below", "at", "above"):
                    ext = float(row[first + k - 1]) - float(row[first])
                    assert ext == {"below": c["rm"] - P.LM_UNIT, "at": c["rm"], "above": c["rm"] + P.LM_UNIT}[ext_kind], tag(c)
                if gap_kind in ("below", "at", "above") and first > 0 and np.isfinite(row[first - 1]):
                    gap = abs(float(row[first]) - float(row[first - 1]))
                    assert gap == {"below": c["rt"] - P.LM_UNIT, "at": c["rt"], "above": c["rt"] + P.LM_UNIT}[gap_kind], tag(c)


# ------------------------------------------------------------------ the whole file's budget (runs last)
def test_zz_the_whole_file_stays_within_its_minute():
    total = sum(_spent)
    print("tests/test_plan_cases.py so far: %.1f s" % total)
    assert total < FILE_SECONDS, total
