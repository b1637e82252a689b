"""The seeded cases of slam_grid_travel (tests/travel_cases.py) on the host: the same seed gives the same case, every case
answers, the restatement agrees with its Bellman-Ford twin on them, and the default seeds reach the edges that a
relaxation by tiles can get wrong."""
import numpy as np

import travel_cases as TC
import travel_ref as T

DEFAULT = 60
EDGES = ("source on an occupied cell", "source outside the map", "a diagonal wall", "a goal that is unreachable while frontiers exist",
         "cost ties that dir must break", "a path longer than path_cap", "a tile re-activated after its neighbour improved")


def test_cases_are_reproducible():
    for seed in (0, 7, 41):
        a, b = TC.case_of("travel", seed), TC.case_of("travel", seed)
        assert a.keys() == b.keys()
        for k in a:
            assert np.array_equal(a[k], b[k]), (seed, k)
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
