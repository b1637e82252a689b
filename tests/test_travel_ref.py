"""The restatement of slam_grid_travel (tests/travel_ref.py) held against two independent things - a NumPy Bellman-Ford by
shifted arrays, and the definition checked cell by cell on every pattern - plus what needs no device of the operator
itself: plan_travel through slam_plan_query at its edges, and the new symbols in the header, the binding and the package."""
import ctypes as C

import numpy as np
import pytest

import frontier_cases as FC
import travel_ref as T
from conftest import pkg

PATTERNS = FC.patterns()


def sources_of(pm, k=2):
    free = np.argwhere(pm == 0)
    if len(free) == 0:
        return np.array([[0, 0]], dtype=np.int32)
    return free[[0, len(free) // 2][:k]].astype(np.int32)


def goals_of(pm):
    free = np.argwhere(pm == 0)
    xw, yw = pm.shape
    picks = free[:: max(len(free) // 6, 1)][:8] if len(free) else np.zeros((0, 2), dtype=np.int64)
    return np.concatenate([picks, [[-1, -1], [xw, 0], [xw - 1, yw - 1], [0, 0]]]).astype(np.int32)


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_dijkstra_is_bellman_ford_and_the_definition_cell_by_cell(name):
    pm = PATTERNS[name]
    xw, yw = pm.shape
    for through, foot in ((False, 0), (True, 1)):
        src = sources_of(pm)
        ans = T.answer(pm, None, src, foot=foot, through_unknown=through, goals=goals_of(pm), path_cap=xw * yw)
        Tm, cost, d = ans["T"], ans["cost"], ans["dir"]
        assert np.array_equal(cost, T.costs_bellman_ford(Tm, src)), name
        ok = T.allowed(Tm)
        assert np.all(cost[~Tm] == -1) and all(cost[x, y] == 0 and d[x, y] == -1 for x, y in src)
        P = np.full((xw + 2, yw + 2), -1, dtype=np.int64)
        P[1:-1, 1:-1] = cost
        best = np.full((xw, yw), 1 << 40, dtype=np.int64)
        for k, (dx, dy) in enumerate(T.MOVES):
            nb = P[1 + dx:1 + dx + xw, 1 + dy:1 + dy + yw]
            best = np.where(ok[k] & (nb >= 0), np.minimum(best, nb + T.WEIGHTS[k]), best)
            # no unreached cell of T has an allowed move to a reached one
            assert not np.any(ok[k] & (cost < 0) & (nb >= 0)), (name, k)
        inner = cost > 0
        assert np.array_equal(cost[inner], best[inner]), name                    # the minimum over the allowed moves
        assert np.all(best[cost == 0] >= 0) and np.all((d >= 0) == inner)
        for j, g in enumerate(goals_of(pm)):
            n = int(ans["path_len"][j])
            cells = ans["path"][j, :n]
            inside = 0 <= g[0] < xw and 0 <= g[1] < yw
            if not inside or cost[g[0], g[1]] < 0:
                assert n == 0 and ans["goal_cost"][j] == -1 and np.all(ans["path"][j] == -1)
                continue
            assert tuple(cells[-1]) == tuple(g) and cost[tuple(cells[0])] == 0 and np.all(ans["path"][j, n:] == -1)
            total = 0
            for u, v in zip(cells[1:], cells[:-1]):                              # from each cell the move back towards the source
                k = T.MOVES.index((int(v[0] - u[0]), int(v[1] - u[1])))
                assert ok[k, u[0], u[1]] and k == d[u[0], u[1]]
                total += T.WEIGHTS[k]
            assert total == ans["goal_cost"][j] == cost[g[0], g[1]]


def test_no_corner_cutting_and_the_foot():
    pm = np.zeros((5, 5), dtype=np.int8)
    pm[1, 2] = pm[2, 1] = 100                       # two occupied cells that touch diagonally are a wall
    cost = T.answer(pm, None, [[1, 1]])["cost"]
    # (2, 2) is reached round the wall: (0, 1), (0, 2), (0, 3), (1, 3), (2, 3), (2, 2) - every diagonal on the way is cut
    assert cost[1, 1] == 0 and cost[0, 0] == 14 and cost[0, 1] == 10 and cost[2, 2] == 60
    board = FC.checkerboard((9, 9))                 # no move exists at all
    cost = T.answer(board, None, [[4, 4]])["cost"]
    assert cost[4, 4] == 0 and (cost >= 0).sum() == 1
    pm = np.full((9, 9), 100, dtype=np.int8)        # the robot stands on occupied cells: its foot is traversable
    a = T.answer(pm, None, [[0, 0], [20, 20]], foot=2)
    assert (a["cost"] >= 0).sum() == 9 and a["cost"][2, 2] == 28 and a["cost"][3, 3] == -1
    assert np.all(T.answer(pm, None, [[-1, 0]], foot=8)["cost"] == -1)
    fld = np.full((9, 9), 4, dtype=np.int16)
    fld[:, 4] = 3
    free = np.zeros((9, 9), dtype=np.int8)
    assert (T.answer(free, fld, [[4, 0]], min_clear2=4)["cost"] >= 0).sum() == 36
    assert (T.answer(free, fld, [[4, 0]], min_clear2=3)["cost"] >= 0).sum() == 81


def query(name, a=0, b=0, c=0, guard=-1):
    abi = pkg("_abi")
    out = C.c_int64()
    abi.check(abi.lib().slam_plan_query(name.encode(), a, b, c, guard, C.byref(out)))
    return int(out.value)


def test_launch_shape_at_its_edges():
    t = query("kTravelTile")
    assert t == 64 == query("kWave") and query("kTravelThreads") == 1024 and query("kTravelTripsPerTile") == 4 * t + 6
    assert (query("kTravelMaxSources"), query("kTravelMaxFoot"), query("kTravelMaxGoals")) == (64, 8, 65536)
    ceil = lambda a, b: -(-a // b)
    for xw, yw in ((1, 1), (1, 70), (70, 1), (t, t), (t + 1, t), (t, t + 1), (t + 1, t + 1), (130, 67), (400, 400), (2000, 2000)):
        nx, ny = ceil(xw, t), ceil(yw, t)
        assert (query("travel_tiles_x", xw, yw), query("travel_tiles_y", xw, yw), query("travel_tiles", xw, yw)) == (nx, ny, nx * ny)
        assert query("travel_mask_words", xw, yw) == xw * ny and query("travel_trips", xw, yw) == nx * ny * (4 * t + 6)
        shared = xw * ny * 8 + ceil(nx * ny * 4, 8) * 8
        assert query("travel_query_bytes", xw, yw, 0) == shared and query("travel_query_bytes", xw, yw, 1) == shared + 4 * xw * yw
    assert query("travel_tiles", 0, 5) == 0 and query("travel_tiles", 5, -1) == 0
    halo = (t + 2) * (t + 2)
    want = halo * 4 + ceil(halo, 16) * 16 + 256
    assert query("travel_lds", guard=0) == want and query("travel_lds", guard=512) == want + 512 <= query("kLdsDefault")
    # chunks: as many queries as fit the budget, B at one chunk and one more; none (0) when one query does not fit
    qb = query("travel_query_bytes", 130, 67, 1)
    kib = ceil(7 * qb, 1024)
    assert query("travel_chunk_queries", 256 * 1024, qb, 7) == 7 and query("travel_chunks", 256 * 1024, qb, 7) == 1
    assert query("travel_chunk_queries", kib, qb, 7) == 7 and query("travel_chunks", kib, qb, 7) == 1
    assert query("travel_chunk_queries", kib, qb, 8) == 7 and query("travel_chunks", kib, qb, 8) == 2
    assert query("travel_chunk_queries", ceil(qb, 1024), qb, 7) == 1 and query("travel_chunks", ceil(qb, 1024), qb, 7) == 7
    assert query("travel_chunk_queries", qb // 1024, qb, 7) == 0 and query("travel_chunks", qb // 1024, qb, 7) == 0
    big = query("travel_query_bytes", 2000, 2000, 1)
    assert query("travel_chunk_queries", 256 * 1024, big, 64) == 256 * 1024 * 1024 // big == 16


def test_entry_points_are_declared_bound_and_exported():
    abi, slam = pkg("_abi"), pkg()
    declared = abi.header_symbols()
    for n in ("slam_grid_travel", "slam_grid_travel_dev"):
        assert n in declared and n in abi._SIGS and hasattr(abi.lib(), n), n
    assert abi._SIGS["slam_grid_travel"] == abi._SIGS["slam_grid_travel_dev"] and len(abi._SIGS["slam_grid_travel"][0]) == 19
    text = open(abi.HEADER_PATH).read()
    for n, v in (("SLAM_TRAVEL_STRAIGHT", 10), ("SLAM_TRAVEL_DIAGONAL", 14), ("SLAM_TRAVEL_TRIPS", 1)):
        assert "#define %s %d\n" % (n, v) in text
    assert (slam.TRAVEL_STRAIGHT, slam.TRAVEL_DIAGONAL, slam.TRAVEL_TRIPS) == (T.STRAIGHT, T.DIAGONAL, 1)
    for n in ("grid_travel_host", "TRAVEL_STRAIGHT", "TRAVEL_DIAGONAL", "TRAVEL_TRIPS"):
        assert n in slam.__all__ and hasattr(slam, n), n
    assert hasattr(slam.DeviceGrid, "travel") and hasattr(slam.Mapping, "travel_field") and hasattr(slam.Mapping, "travel_path")
    assert hasattr(slam.DeviceGridSLAM, "travel") and hasattr(slam.DeviceGridSLAM, "next_goals")
    assert abi.lib().slam_abi_version() == 1 and len(abi.K_NAMES) == 8
    fr = dict(point=np.zeros((3, 2)))
    from conftest import PKG
    import importlib
    travel_goal = importlib.import_module(PKG + ".replay").travel_goal
    assert travel_goal(fr, [-1, 30, 30]) == 1 and travel_goal(fr, [-1, -1, -1]) is None and travel_goal(dict(point=np.zeros((0, 2))), []) is None
