"""The seeded cases of slam_grid_travel (tests/travel_cases.py) on the host: the same seed gives the same case, every case
answers, the restatement agrees with its Bellman-Ford twin on them, and the default seeds reach the edges that a
relaxation by tiles can get wrong; the batches of 'travel_batch' likewise, with the edges of routing."""
import numpy as np

import travel_cases as TC
import travel_ref as T

DEFAULT = 60
EDGES = ("source on an occupied cell", "source outside the map", "a diagonal wall", "a goal that is unreachable while frontiers exist",
         "cost ties that dir must break", "a path longer than path_cap", "a tile re-activated after its neighbour improved")
BATCH_EDGES = ("a routed query under a clearance whose map's field differs from map b's", "a query that names no map", "one map queried twice",
               "a source on the last or first row or column of its tile with a traversable cell across the border")


def test_cases_are_reproducible():
    for kind in ("travel", "travel_batch"):
        for seed in (0, 7, 41):
            a, b = TC.case_of(kind, seed), TC.case_of(kind, seed)
            assert a.keys() == b.keys()
            for k in a:
                assert np.array_equal(a[k], b[k]), (kind, seed, k)
    assert not np.array_equal(TC.case_of("travel", 1)["pmap"], TC.case_of("travel", 8)["pmap"])


def test_default_seeds_reach_the_edges():
    reached = {}
    for seed in range(DEFAULT):
        case = TC.case_of("travel", seed)
        ans = TC.answer(case)
        assert ans["cost"].shape == case["pmap"].shape and ans["path"].shape == (len(case["goals"]), case["path_cap"], 2), seed
        if seed % 3 == 0:
            assert np.array_equal(ans["cost"], T.costs_bellman_ford(ans["T"], case["sources"])), seed
        for e in TC.edges_of(case, ans):
            reached.setdefault(e, []).append(seed)
    for e in EDGES:
        assert len(reached.get(e, [])) >= 2, (e, reached.get(e))
    assert {TC.case_of("travel", s)["family"] for s in range(7)} == {"random", "rooms", "serpentine", "spiral", "comb", "diagonal"}


def test_default_batches_reach_the_edges_of_routing():
    reached, clearances, cells = {}, 0, []
    for seed in range(DEFAULT):
        case = TC.case_of("travel_batch", seed)
        pm, maps = case["pmaps"], case["maps"]
        assert np.array_equal(pm[0], TC.case_of("travel", seed)["pmap"]), seed          # the 'travel' case's own map, untouched
        assert 1 <= len(pm) <= 3 and 1 <= len(maps) <= 6 and case["sources"].shape[0] == len(maps) == case["goals"].shape[0], seed
        if len(pm) > 1:
            assert np.array_equal(pm[1], pm[0][::-1]), seed
        ans = TC.answer(case)
        B = len(maps)
        assert ans["cost"].shape == (B,) + pm.shape[1:] and ans["path"].shape == (B, case["goals"].shape[1], case["path_cap"], 2), seed
        named = (maps >= 0) & (maps < len(pm))
        assert np.array_equal(ans["status"], np.where(named, 0, -1)), seed
        if seed % 3 == 0:
            for b in np.flatnonzero(named):
                assert np.array_equal(ans["cost"][b], T.costs_bellman_ford(ans["T"][b], case["sources"][b])), (seed, b)
        clearances += case["min_clear2"] > 0
        if seed % 10:
            cells.append(B * pm[0].size)
        for e in TC.edges_of(case, ans):
            reached.setdefault(e, []).append(seed)
    for e in BATCH_EDGES:
        assert len(reached.get(e, [])) >= 2, (e, reached.get(e))
    assert DEFAULT // 5 <= clearances <= DEFAULT // 2 and max(cells) <= TC.BATCH_CELLS
