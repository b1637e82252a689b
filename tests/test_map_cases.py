"""The seeded cases of tests/map_cases.py without a device: every case builds and the restatement answers it in time,
two independent restatements agree on it, and the sweep reaches the edges it was written for.

The GPU file (tests/test_gpu_map_properties.py) runs exactly these cases, so what is asserted here about the default 60
seeds - that enough of them cross a mask word at R, cut a call into chunks, span tiles and segments, gate a resample -
is what that file can be trusted to have exercised.  Every message carries (kind, seed): map_cases.case_of(kind, seed)
rebuilds the case."""
import functools
import time

import numpy as np
import pytest

import frontier_ref as FR
import gridslam_ref as G
import locate_ref as L
import map_cases as C
import match_ref as M
import mcl_ref as X

DEFAULT = 60                                # the seeds over which the edge reach is asserted, whatever SLAM_HYP_EXAMPLES says
N = len(C.seeds())
KIND_SECONDS = 5.0 * max(N, DEFAULT) / DEFAULT     # a kind's restatement answers: 5 s per 60 seeds (scaled when soaking)
FILE_SECONDS = 60.0 * max(N, DEFAULT) / DEFAULT    # and a minute for the whole file
_spent = []


@functools.lru_cache(maxsize=None)
def solved(kind, n):
    """(cases, answers, seconds the restatement took) of seeds 0 .. n - 1; each (kind, n) is worked out once."""
    cases = [C.case_of(kind, s) for s in range(n)]
    t = time.perf_counter()
    answers = [C.answer(c) if kind != "weigh" else C.weigh_answer(c, C.fields_of(C.pmaps_of_cells(c), c["cap"])) for c in cases]
    return cases, answers, time.perf_counter() - t


def default(kind):
    cases, answers, _ = solved(kind, max(N, DEFAULT))
    return list(zip(cases[:DEFAULT], answers[:DEFAULT]))


def sweep(kind):
    cases, answers, _ = solved(kind, max(N, DEFAULT))
    return list(zip(cases[:N], answers[:N]))


def tag(c):
    return (c["kind"], c["seed"])


@pytest.fixture(autouse=True)
def _clock():
    t = time.perf_counter()
    yield
    _spent.append(time.perf_counter() - t)


# ------------------------------------------------------------------ the cases build, and in time
@pytest.mark.parametrize("kind", C.KINDS)
def test_cases_build_and_the_restatement_answers_in_time(kind):
    cases, answers, seconds = solved(kind, max(N, DEFAULT))
    print("%s: %d restatement answers in %.2f s" % (kind, len(cases), seconds))
    assert len(cases) == len(answers) and seconds < KIND_SECONDS, (kind, seconds)
    for c in cases:
        assert c["kind"] == kind and C.case_of(kind, c["seed"]).keys() == c.keys(), tag(c)


def same_case(a, b):
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same_case(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and (a == b or (isinstance(a, float) and a != a and b != b))


@pytest.mark.parametrize("kind", C.KINDS)
def test_a_case_is_a_pure_function_of_kind_and_seed(kind):
    for seed in (0, 7, 19, 20, 41, 59):
        a, b = C.case_of(kind, seed), C.case_of(kind, seed)
        assert all(same_case(a[k], b[k]) for k in a), (kind, seed)
    assert not all(same_case(C.case_of(kind, 1)[k], C.case_of(kind, 2)[k]) for k in C.case_of(kind, 1) if k != "kind")


def test_small_seeds_draw_small_shapes():
    """Seeds below 20 take every size from the lower half of its list (or of its range)."""
    for s in range(C.SMALL):
        f = C.case_of("field", s)
        assert max(f["xw"], f["yw"]) <= 150 and f["cap"] <= 65, tag(f)
        assert max(C.case_of("match", s)[k] for k in ("xw", "yw")) <= 33 and C.case_of("locate", s)["H"] <= 4
        fr = C.case_of("frontiers", s)
        assert fr["xw"] <= 33 and fr["yw"] <= 65 and fr["radius"] <= 4, tag(fr)
        assert C.case_of("weigh", s)["P"] <= 65 and C.case_of("resample", s)["P"] <= 2500 and C.case_of("settle", s)["P"] <= 65
        assert C.case_of("copy", s)["xw"] <= 33


# ------------------------------------------------------------------ the bounds the issue sets on the shapes
def test_cases_stay_inside_their_bounds():
    for c, _ in sweep("field"):
        assert 1 <= c["G"] <= 3 and c["xw"] * c["yw"] <= 40000 and c["cap"] in C.FIELD_CAPS, tag(c)
    for c, _ in sweep("match"):
        assert max(c["xw"], c["yw"]) <= 64 and c["K"] * (2 * c["nx"] + 1) * (2 * c["ny"] + 1) * c["n"] * c["B"] <= 20000, tag(c)
        assert c["rot_cs"].shape == (c["B"], c["K"], 2) and c["ranges"].shape in ((c["n"],), (c["B"], c["n"])), tag(c)
    for c, _ in sweep("locate"):
        assert max(c["xw"], c["yw"]) <= 48 and 0 <= c["H"] <= 8 and c["n"] * c["cap"] < 2 ** 31, tag(c)
        if c["regions"] is not None:
            r = c["regions"]
            assert np.all(r[:, :2] >= 0) and np.all(r[:, 2:] >= 1) and np.all(r[:, 0] + r[:, 2] <= c["xw"]) and np.all(r[:, 1] + r[:, 3] <= c["yw"])
    for c, _ in sweep("frontiers"):
        assert 0 <= c["min_unknown"] <= (2 * c["radius"] + 1) ** 2 and c["min_clear2"] <= c["cap"], tag(c)
        assert c["maps"] is not None or c["B"] <= c["G"], tag(c)
    for c, _ in sweep("weigh"):
        assert c["F"] * c["P"] >= 64 and (c["noise"] is None or c["motion"] is not None), tag(c)
    for c, _ in sweep("settle"):
        assert c["F"] * c["P"] <= 300000 and c["ancestors"].min() >= 0 and c["ancestors"].max() < c["P"], tag(c)
    for c, a in sweep("copy"):
        assert 0 <= c["first"] and c["first"] + c["count"] <= c["G"] and not np.any(a["copied"] == -1), tag(c)


# ------------------------------------------------------------------ reference against reference
@pytest.mark.parametrize("kind", ["field", "match"])
def test_the_field_by_brute_force_is_the_field_by_two_passes(kind):
    for c, a in sweep(kind):
        f = a if kind == "field" else C.fields_of(C.pmaps_of_cells(c), c["cap"])
        pm = C.pmaps_of_cells(c)
        for gi in range(c["G"]):
            assert np.array_equal(f[gi], G.fast_field(pm[gi], c["cap"])), tag(c) + (gi,)


def searched(c, a):
    """The hypotheses of a locate case that a search ran for: a good map entry and a used beam."""
    return [b for b in range(c["B"]) if a[1][b] >= 0 and a[2][b] > 0]


def region_of(c, b):
    return (0, 0, c["xw"], c["yw"]) if c["regions"] is None else tuple(int(v) for v in c["regions"][b])


def test_locate_search_finds_what_brute_force_finds():
    for c, a in sweep("locate"):
        fields = C.fields_of(C.pmaps_of_cells(c), c["cap"])
        for b in range(c["B"]):
            gi = 0 if c["maps"] is None else int(c["maps"][b])
            if not 0 <= gi < c["G"]:
                assert a[0][b].tolist() == [-1, -1, -1] and a[1][b] == -1, tag(c) + (b,)
                continue
            r = c["ranges"] if c["ranges"].ndim == 1 else c["ranges"][b]
            best, cost, used = L.brute(fields[gi], c["scale"], r, c["cos_t"], c["sin_t"], c["rot_cs"], region_of(c, b), c["max_range"], c["cap"])
            assert a[0][b].tolist() == list(best) and a[1][b] == cost and a[2][b] == used, tag(c) + (b,)


def frontier_masks(c):
    """{map: frontier mask} of the maps that a frontier case's queries read."""
    maps = range(c["B"]) if c["maps"] is None else c["maps"]
    out = {}
    for gi in sorted({int(m) for m in maps if 0 <= int(m) < c["G"]}):
        fld = M.field(c["pmaps"][gi], c["cap"]) if c["min_clear2"] > 0 else None
        out[gi] = FR.mask(c["pmaps"][gi], c["radius"], c["min_unknown"], fld, c["min_clear2"])
    return out


def test_frontier_labels_are_the_flood_fills_components():
    for c, a in sweep("frontiers"):
        maps = list(range(c["B"])) if c["maps"] is None else [int(m) for m in c["maps"]]
        masks = frontier_masks(c)
        for gi, f in masks.items():
            b = maps.index(gi)
            assert np.array_equal(a[3][b] >= 0, f) and np.array_equal(a[3][b], FR.flood(f)), tag(c) + (gi,)


def test_resampling_with_python_integers_is_resampling_in_uint64():
    for c, a in sweep("resample"):
        for f in range(c["F"]):
            w = X.weights(c["acc"][f], c["table"], c["shift"])[0]
            if w.sum() > 0:
                ints = X.resample_ints(w, c["u0"][f])
                assert np.array_equal(ints, X.resample_u64(w, c["u0"][f])), tag(c) + (f,)
                if a["info"][f, 2]:
                    assert np.array_equal(a["ancestors"][f], ints), tag(c) + (f,)


def test_settle_keeps_every_survivor_in_its_slot():
    for c, a in sweep("settle"):
        P = c["P"]
        for f in range(c["F"]):
            anc, settled = c["ancestors"][f], a["settled"][f]
            alive = np.unique(anc)
            assert np.array_equal(settled[alive], alive), tag(c) + (f,)                       # every survivor keeps its slot
            assert a["moved"][f] == P - len(alive), tag(c) + (f,)                              # moved: exactly the free slots
            assert np.array_equal(np.bincount(settled, minlength=P), np.bincount(anc, minlength=P)), tag(c) + (f,)
        assert np.array_equal(a["map_src"], c["map0"] + np.arange(c["F"])[:, None] * P + a["settled"]), tag(c)


def test_copy_leaves_prefix_and_suffix_alone():
    for c, a in sweep("copy"):
        keep = np.ones(c["G"], dtype=bool)
        keep[c["first"]:c["first"] + c["count"]] = False
        assert np.array_equal(a["pass_cnt"][keep], c["pass_cnt"][keep]) and np.array_equal(a["hit_cnt"][keep], c["hit_cnt"][keep]), tag(c)
        for k in np.flatnonzero(a["copied"] == 1):
            assert np.array_equal(a["hit_cnt"][c["first"] + k], c["hit_cnt"][c["src"][k]]), tag(c)


# ------------------------------------------------------------------ the weigh's tolerance is a cap, not a measurement
UNSURE_SHARE = 0.01     # half of test_gpu_mcl.py's 2 %: the device may differ only on particles the restatement itself marks


def test_the_restatement_is_sure_of_the_weigh_cases():
    for c, a in sweep("weigh"):
        w = C.answer(c)                                                # with ulp=True
        assert np.array_equal(w["cost"], a["cost"]) and np.array_equal(w["used"], a["used"]), tag(c)
        assert w["unsure"].mean() <= UNSURE_SHARE, tag(c) + (int(w["unsure"].sum()),)


# ------------------------------------------------------------------ edge reach over the default 60 seeds
def count(kind, pred):
    return sum(1 for c, a in default(kind) if pred(c, a))


FIELD_WIDE = 6          # an axis above 256: rows of more than eight mask words
FIELD_FAR = 6           # cap >= 32760 (R = 181, 182) on an axis above 185, where a cell R away is inside the map
FIELD_RULER = 4         # of each of R - 1, R, R + 1: the last distance the passes must see, and the first they need not
FIELD_FLAT = 0.15       # at most this share with a field that is cap everywhere (it checks little)


def test_field_reach():
    assert count("field", lambda c, a: max(c["xw"], c["yw"]) > 256) >= FIELD_WIDE
    assert count("field", lambda c, a: c["cap"] >= 32760 and max(c["xw"], c["yw"]) > 185) >= FIELD_FAR
    for gap in ("R-1", "R", "R+1"):
        assert count("field", lambda c, a: any(r[0] == gap for r in c["rulers"])) >= FIELD_RULER, gap
    assert count("field", lambda c, a: bool(np.all(a == c["cap"]))) <= FIELD_FLAT * DEFAULT
    far = [c for c, _ in default("field") if c["cap"] >= 32760 and any(r[0] in ("R-1", "R", "R+1") for r in c["rulers"])]
    assert len(far) >= 1                                               # the ruler at R = 181 or 182 itself


LOCATE_SHARED = 10      # two hypotheses with different regions in one chunk: the sweep's mixed-wave path by design
LOCATE_CUT = 10         # more than one chunk: the lists are reset and refilled
LOCATE_ENDS = 5         # H = 0 (brute force through the same code) and H = 8 (the deepest pyramid), each
LOCATE_PRUNED = 0.5     # of the H > 0 cases: level-0 nodes below brute force's, so the bound did prune


def locate_chunks(c, a):
    """The hypotheses searched in every chunk of a locate case's sweep: pair p = b K + k, chunks of the planned size."""
    _, per = C.locate_plan(c)
    live = set(searched(c, a))
    pairs = c["B"] * c["K"]
    return [sorted({p // c["K"] for p in range(p0, min(p0 + per, pairs))} & live) for p0 in range(0, pairs, per)]


def test_locate_reach():
    def shared(c, a):
        return c["H"] > 0 and any(len({region_of(c, b) for b in ch}) > 1 for ch in locate_chunks(c, a))

    def pruned(c, a):
        live = searched(c, a)
        return sum(int(a[3][b][0]) for b in live) < sum(c["K"] * region_of(c, b)[2] * region_of(c, b)[3] for b in live)

    assert count("locate", shared) >= LOCATE_SHARED
    assert count("locate", lambda c, a: c["H"] > 0 and len(locate_chunks(c, a)) > 1) >= LOCATE_CUT
    assert count("locate", lambda c, a: c["H"] == 0) >= LOCATE_ENDS and count("locate", lambda c, a: c["H"] == 8) >= LOCATE_ENDS
    deep = count("locate", lambda c, a: c["H"] > 0 and len(searched(c, a)) > 0)
    assert count("locate", lambda c, a: c["H"] > 0 and len(searched(c, a)) > 0 and pruned(c, a)) >= LOCATE_PRUNED * deep


FRONTIER_SPAN = 15      # a cluster across two tiles and two segments: border unions and the segmented passes
FRONTIER_OVER = 8       # more kept clusters than M > 0 rows: the table is cut, the count is not
FRONTIER_CLEAR = 8      # min_clear2 removes a cell the plain rule keeps: the field decides
FRONTIER_WINDOW = 8     # radius >= 4 on two or more tiles: the window's halo crosses a tile border
FRONTIER_EMPTY = 0.15   # at most this share without any frontier cell


def valid_queries(c):
    maps = list(range(c["B"])) if c["maps"] is None else [int(m) for m in c["maps"]]
    return [(b, gi) for b, gi in enumerate(maps) if 0 <= gi < c["G"]]


def test_frontier_reach():
    def spans(c, a):
        for b, _ in valid_queries(c):
            lab = a[3][b]
            xs, ys = np.nonzero(lab >= 0)
            if not len(xs):
                continue
            key = lab[xs, ys]
            order = np.argsort(key, kind="stable")
            key, tile, seg = key[order], (xs // 32 * 1000 + ys // 64)[order], ((xs * c["yw"] + ys) // 1024)[order]
            for members in np.split(np.arange(len(key)), np.flatnonzero(np.diff(key)) + 1):
                if len(np.unique(tile[members])) > 1 and len(np.unique(seg[members])) > 1:
                    return True
        return False

    def cleared(c, a):
        if c["min_clear2"] == 0:
            return False
        return any(FR.mask(c["pmaps"][gi], c["radius"], c["min_unknown"]).sum() > f.sum() for gi, f in frontier_masks(c).items())

    tiles = lambda c: -(-c["xw"] // 32) * -(-c["yw"] // 64)
    assert count("frontiers", spans) >= FRONTIER_SPAN
    assert count("frontiers", lambda c, a: c["M"] > 0 and any(a[0][b][0] > c["M"] for b, _ in valid_queries(c))) >= FRONTIER_OVER
    assert count("frontiers", cleared) >= FRONTIER_CLEAR
    assert count("frontiers", lambda c, a: c["radius"] >= 4 and tiles(c) >= 2) >= FRONTIER_WINDOW
    assert count("frontiers", lambda c, a: not any(a[0][b][1] > 0 for b, _ in valid_queries(c))) <= FRONTIER_EMPTY * DEFAULT
    assert count("frontiers", lambda c, a: c["chunk_queries"] is not None and C.frontier_plan(c)[1] < c["B"]) >= 5


RESAMPLE_NO_WEIGHT = 5  # S = 0: no live particle, or a table that gives the live ones nothing
RESAMPLE_GATED = 5      # a filter with weight whose ESS gate says no: poses copied, acc kept, the identity
RESAMPLE_CLAMPED = 5    # a table entry above 2^20, which the device form clamps
RESAMPLE_LONG = 8       # P > 4096: past one reduce run, and the uint64 comparison
RESAMPLE_DONE = 24      # a filter that does resample - the operator's main path - in at least two cases of five


def test_resample_reach():
    assert count("resample", lambda c, a: bool(np.any(np.isnan(a["est"][:, 0])))) >= RESAMPLE_NO_WEIGHT
    assert count("resample", lambda c, a: bool(np.any(~np.isnan(a["est"][:, 0]) & (a["info"][:, 2] == 0)))) >= RESAMPLE_GATED
    assert count("resample", lambda c, a: int(c["table"].max()) > X.W_MAX) >= RESAMPLE_CLAMPED
    assert count("resample", lambda c, a: c["P"] > 4096) >= RESAMPLE_LONG
    assert count("resample", lambda c, a: bool(np.any(a["info"][:, 2] == 1))) >= RESAMPLE_DONE


WEIGH_SHAPE = 10        # of each launch shape: lanes over particles, a wave per particle, the library's choice
WEIGH_MAPS = 15         # slam_mcl_weigh_maps rather than slam_mcl_weigh


def test_weigh_reach():
    for shape in (-1, 0, 1):
        assert count("weigh", lambda c, a: c["mcl_shape"] == shape) >= WEIGH_SHAPE, shape
    assert count("weigh", lambda c, a: c["own_maps"]) >= WEIGH_MAPS
    assert count("weigh", lambda c, a: bool(np.any(a["cost"] > 0))) >= 50 and count("weigh", lambda c, a: bool(np.any(a["cost"] == -1))) >= 15


# ------------------------------------------------------------------ the whole file's budget (runs last)
def test_zz_the_whole_file_stays_within_its_minute():
    total = sum(_spent)
    print("tests/test_map_cases.py so far: %.1f s" % total)
    assert total < FILE_SECONDS, total
