"""The seeded cases of slam_grid_travel (tests/travel_cases.py) on the device: every output of every case against the
restatement on the map and the field read back, with array_equal; SLAM_HYP_EXAMPLES turns the sweep into a soak run.
Every assertion message carries the seed."""
import numpy as np
import pytest

import frontier_cases as FC
import travel_cases as TC
from conftest import pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def slam():
    p = pkg()
    p._abi.default_context()   # fails loudly when there is no gfx950 device
    return p


@pytest.fixture(scope="module")
def ctx(slam):
    c = slam.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("lot", range(6))
def test_seeded_cases(slam, ctx, lot):
    seeds = [s for s in TC.seeds() if s % 6 == lot]
    for seed in seeds:
        case = TC.case_of("travel", seed)
        g, pm = FC.grid_of(slam, ctx, case["pmap"])
        field = slam.grid_distance_field_host(g, case["cap"])[0] if case["min_clear2"] > 0 else None
        want = TC.answer(case, pm[0], field)
        got = slam.grid_travel_host(g, case["sources"][None], goals=case["goals"][None], foot=case["foot"],
                                    through_unknown=case["through_unknown"], min_clear2=case["min_clear2"], cap=case["cap"],
                                    path_cap=case["path_cap"], dirs=True)
        if case["path_cap"] == 0:
            got["path"] = np.full((1,) + want["path"].shape, -1, dtype=np.int32)
        assert got["status"].tolist() == [0], seed
        TC.same({k: v[0] for k, v in got.items() if k != "status"}, {k: v for k, v in want.items() if k not in ("status", "T")}, tag=seed)
        g.close()
    ctx.check_status()
