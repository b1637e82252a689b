"""Seeded sweep of slam_track on the GPU: every case of tests/track_cases.py (30 by default, SLAM_HYP_EXAMPLES soaks it)
through the teacher-forced walk of test (A) - the host form on every seed, the device form on every third.  The cases run
on refine_cases' small maps under both index rules, S <= 6, L <= 3, gates from {0, small, +inf}, motion present or NULL;
tests/test_track_cases.py asserts which edges the default seeds reach."""
import pytest

import track_cases as C
from conftest import pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def slam():
    p = pkg()
    p._abi.default_context()   # fails loudly when there is no gfx950 device
    return p


@pytest.mark.parametrize("seed", C.seeds())
def test_seeded_walk(slam, seed):
    case = C.case_of(seed)
    for device in ((False, True) if seed % 3 == 0 else (False,)):
        grid, shadow = C.make_grids(slam, case)
        out = C.run(slam, grid, case, device=device)
        end = C.walk(slam, case, out, shadow)
        assert C.same(out["state"], end), (seed, device, out["state"], end)
        got, want = C.counters(grid), C.counters(shadow)
        assert C.same(got[0], want[0]) and C.same(got[1], want[1]), (seed, device)
        grid._ctx.check_status()
