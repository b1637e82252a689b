"""The seeded cases of slam_grid_view_gain (tests/view_cases.py) on the host: the same seed gives the same case, every
case answers, and the default seeds reach the edges that a set union along reversed lines can get wrong."""
import numpy as np

import view_cases as VC
import view_ref as V

DEFAULT = 60


def test_cases_are_reproducible():
    for seed in (0, 7, 41):
        a, b = VC.case_of("view", seed), VC.case_of("view", seed)
        assert a.keys() == b.keys()
        for k in a:
            assert np.array_equal(a[k], b[k]), (seed, k)
    assert VC.case_of("view", 1)["pmaps"].shape != VC.case_of("view", 2)["pmaps"].shape


def test_default_seeds_reach_the_edges():
    reached = {}
    for seed in range(DEFAULT):
        case = VC.case_of("view", seed)
        counts, seen = VC.answer(case)
        B, (xw, yw) = len(case["poses"]), case["pmaps"].shape[1:]
        assert counts.shape == (B, 4) and seen.shape == (B, xw, (yw + 31) // 32), seed
        ok = VC.named(case)
        assert np.all(counts[~ok] == -1) and not seen[~ok].any() and np.all(counts[ok] >= 0), seed
        for b in np.flatnonzero(ok):
            assert int(counts[b, :3].sum()) == len(V.cells_of(seen[b], yw)), (seed, b)
        for e in VC.edges_of(case, (counts, seen)):
            reached.setdefault(e, []).append(seed)
    for e in VC.EDGES:
        assert len(reached.get(e, [])) >= 5, (e, reached.get(e))
