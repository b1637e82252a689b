"""The NumPy A* oracle (tests/astar_ref.py) reproduces the reference's own global_planner.py on
the recorded cases of tests/golden/g12_astar.npz (tools/gen_astar_golden.py): inflated maps,
statuses, paths and len(close_list); and the package's GlobalPlanner turns the oracle's paths
into the reference's accumulated current_path."""
import numpy as np
import pytest

import astar_ref
from conftest import load_golden, pkg


@pytest.fixture(scope="module")
def g12():
    return load_golden("g12_astar.npz")


def map_of(g, k, key="maps"):
    return g[key][k, :g["map_h"][k], :g["map_w"][k]].astype(np.int64)


def test_golden_has_the_cases_the_spec_names(g12):
    names = [str(n) for n in g12["names"]]
    assert sum(n.startswith("course_") for n in names) >= 20
    st = dict(zip(names, g12["status"].tolist()))
    assert st["invalid_start"] == astar_ref.INVALID_START and st["invalid_goal"] == astar_ref.INVALID_GOAL
    assert st["start_is_goal"] == astar_ref.NO_PATH and st["unreachable"] == astar_ref.NO_PATH
    k = names.index("unreachable")
    assert g12["expansions"][k] > 1000          # len(close_list) when IndexError was raised
    # the serpentine: g past 100 000, so every open f is clamped by find_min_cost_f's initial 100 000
    k = names.index("serpentine")
    assert st["serpentine"] == astar_ref.OK and 10 * (g12["path_len"][k] - 1) > astar_ref.CLAMP
    maps = [str(n) for n in g12["map_names"]]
    assert maps[0] == "course" and (g12["map_h"][0], g12["map_w"][0]) == (129, 129)
    course = map_of(g12, 0)
    assert set(np.unique(course).tolist()) <= {-1, 0, 100}
    assert any(np.any(map_of(g12, i) == 50) for i in range(len(maps)))


def test_oracle_inflation_matches_the_reference(g12):
    for k in range(len(g12["map_names"])):
        got = astar_ref.inflate(map_of(g12, k), int(g12["span"]), int(g12["r"]))
        np.testing.assert_array_equal(got, map_of(g12, k, "inflated"), err_msg=str(g12["map_names"][k]))
        # a second pass changes nothing: the reference's re-inflation on every plan is a fixed point
        np.testing.assert_array_equal(astar_ref.inflate(got, int(g12["span"]), int(g12["r"])), got)


def test_inflation_is_not_a_dilation(g12):
    m = map_of(g12, 0)
    dil = m.copy()
    r, span = int(g12["r"]), int(g12["span"])
    for i, j in np.argwhere((m[r:span - r, r:span - r] == 100) | (m[r:span - r, r:span - r] == -1)) + r:
        dil[i - r:i + r + 1, j - r:j + r + 1] = 99
    assert np.sum(dil != map_of(g12, 0, "inflated")) > 100


def test_oracle_reproduces_every_query(g12):
    infl = [astar_ref.inflate(map_of(g12, k), int(g12["span"]), int(g12["r"])) for k in range(len(g12["map_names"]))]
    for k, name in enumerate(g12["names"]):
        o = astar_ref.plan(infl[g12["map_of_query"][k]], g12["starts"][k], g12["goals"][k])
        assert o["status"] == g12["status"][k], name
        assert o["expansions"] == g12["expansions"][k], name
        L = g12["path_len"][k]
        assert o["length"] == L, name
        np.testing.assert_array_equal(o["path"], g12["paths"][k, :L], err_msg=str(name))


def test_global_planner_world_path_of_two_plans(g12):
    """GlobalPlanner's world conversion and accumulation (no device call: the oracle plans)."""
    gp_mod = pkg("global_planner")
    assert gp_mod.STATUS_NAMES == astar_ref.STATUS_NAMES and (gp_mod.SPAN, gp_mod.R) == (129, 2)
    gp = gp_mod.GlobalPlanner()
    m = map_of(g12, 0)
    gp.map_callback(dict(data=m.reshape(-1), width=m.shape[1], height=m.shape[0],
                         resolution=float(g12["planner_resolution"]), origin=tuple(g12["planner_origin"]) + (0.0,)))
    sx, sy = g12["planner_start_xy"]
    start = gp.WorldTomap(sx, sy)
    infl = astar_ref.inflate(m)
    xy = []
    for k, (gx, gy) in enumerate(g12["planner_goals_xy"]):
        goal = gp.WorldTomap(gx, gy)
        o = astar_ref.plan(infl, start, goal)
        start = [start[0] - 1, start[1] - 1]                  # find_path shifts start_map_point in place
        assert start == g12["planner_start_map_point"][k].tolist()
        own = [gp.mapToWorld(c, r) for r, c in o["path"]]
        np.testing.assert_array_equal(np.array(own), astar_ref.world_path(o["path"], gp.resolution, gp.origin_x,
                                                                          gp.origin_y))
        xy += own
        assert len(xy) == g12["planner_counts"][k]
    np.testing.assert_array_equal(np.array(xy), g12["planner_path_xy"])
