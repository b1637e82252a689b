"""Map frontiers on the CPU: the restatement (tests/frontier_ref.py) against an independent flood fill on every pattern
the GPU tests use, its statistics against their definition cell by cell, the four rows of the experiment that chose the
defaults on the 120-beam room and its 360-beam sibling, the launch shape at its edges through
slam_plan_query, and the entry points in the header, the binding and the package.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import frontier_cases as FC
import frontier_ref as F
import raycast_ref as R
from conftest import pkg

PATTERNS = FC.patterns()


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_restatement_is_a_flood_fill(name):
    pm = PATTERNS[name]
    for radius, min_unknown in ((0, 0), (1, 3), (2, 13)):
        f = F.mask(pm, radius, min_unknown)
        labels = F.label(f)
        assert np.array_equal(labels, F.flood(f)) and np.array_equal(labels >= 0, f)
        rows, sums = F.clusters_of(labels)
        assert np.all(np.diff(rows[:, 0]) > 0) and rows[:, 1].sum() == f.sum()
        for row, (sx, sy) in zip(rows, sums):
            xs, ys = np.nonzero(labels == row[0])
            assert row[0] == (xs * pm.shape[1] + ys).min() and row[1] == len(xs) and (sx, sy) == (xs.sum(), ys.sum())
            assert tuple(row[4:]) == (xs.min(), ys.min(), xs.max(), ys.max())
            assert labels[row[2], row[3]] == row[0]                      # the representative is a member
            cx, cy = (2 * sx + len(xs)) // (2 * len(xs)), (2 * sy + len(xs)) // (2 * len(xs))
            d2 = (xs - cx) ** 2 + (ys - cy) ** 2
            assert (row[2] - cx) ** 2 + (row[3] - cy) ** 2 == d2.min()
            near = np.flatnonzero(d2 == d2.min())
            assert row[2] * pm.shape[1] + row[3] == (xs[near] * pm.shape[1] + ys[near]).min()   # ties: the lowest flat index


def test_the_patterns_are_what_they_claim():
    count = lambda pm: len(F.clusters_of(F.label(F.mask(pm)))[0])
    for name in ("serpentine", "serpentine_t", "spiral_a", "spiral_b", "comb_a", "comb_b", "checker_a", "checker_b", "crescent"):
        assert count(PATTERNS[name]) == 1, name
    assert count(PATTERNS["u_a"]) == 17 and count(PATTERNS["u_b"]) == 32 and count(PATTERNS["diagonal"]) == 64
    serp = PATTERNS["serpentine"]                                        # all of the path but the corner (0, 64) is frontier
    assert np.argwhere((serp == 0) & ~F.mask(serp)).tolist() == [[0, 64]] and F.label(F.mask(serp)).max() == 0
    lat = FC.lattice(FC.A)
    assert count(lat) == 65 * 34 == int((lat == 0).sum())
    # the cell rule, clause by clause, on the hand-made map
    f = F.mask(PATTERNS["rules"])
    assert f[0, 0] and not f[8, 10] and f[3, 0] and f[5, 0] and f[8, 4] and f[8, 6] and f[7, 5]
    assert not (f[5, 2] or f[7, 4] or f[5, 4] or f[7, 2])               # a diagonal unknown neighbour is not enough
    assert f[2, 7] and f[3, 6] and f[3, 10] and not f[3, 8] and not f[2, 8]
    # the crescent's centroid is outside it; the tie goes to the lowest flat index
    rows, sums = F.clusters_of(F.label(F.mask(PATTERNS["crescent"])))
    cx, cy = (2 * sums[0] + rows[0, 1]) // (2 * rows[0, 1])
    assert PATTERNS["crescent"][cx, cy] == 50 and PATTERNS["crescent"][rows[0, 2], rows[0, 3]] == 0
    rows, _ = F.clusters_of(F.label(F.mask(PATTERNS["ties"])))
    assert rows[:, :4].tolist() == [[4 * 12 + 5, 4, 4, 5], [9 * 12 + 2, 2, 9, 3]]
    # the window's count is clipped at the map's edge
    pm = FC.blank((9, 9))
    assert F.unknown_count(pm, 8)[0, 0] == 81 and F.unknown_count(pm, 2)[0, 0] == 9 and F.unknown_count(pm, 2)[4, 4] == 25
    assert F.unknown_count(pm, 1)[0, 4] == 6 and F.unknown_count(pm, 0)[3, 3] == 1


def test_the_experiment_behind_the_defaults(syn):
    """The table of DESIGN.md section 18: (free cells, frontier cells, clusters, the five largest), and what the 5-cell
    minimum keeps."""
    want = {(120, 0, 0): (22669, 8672, 77, [3518, 2176, 1077, 544, 323]), (120, 2, 13): (22669, 500, 120, [39, 36, 32, 28, 25]),
            (360, 0, 0): (26652, 1342, 84, [117, 85, 73, 71, 70]), (360, 2, 13): (26652, 38, 15, [20, 2, 2, 2, 2])}
    for beams in (120, 360):
        if beams == 120:
            ranges, poses, _ = R.room(syn)
        else:
            rep = syn.make_replay(6, 360, seed=4)
            ranges, poses = np.asarray(rep.ranges, dtype=np.float32), np.asarray(rep.poses_true, dtype=np.float64)
        pm = R.room_pmap(ranges, poses)
        for radius, min_unknown in ((0, 0), (2, 13)):
            count, table, _, labels = F.frontiers(pm, radius, min_unknown, min_size=1, M=256)
            sizes = F.sizes_by_rank(labels)
            assert (int((pm == 0).sum()), int(count[1]), int(count[0]), sizes[:5]) == want[beams, radius, min_unknown]
            assert sorted(table[:count[0], 1].tolist(), reverse=True) == sizes
    count, table, _, _ = F.frontiers(pm)                                 # 360 beams, the defaults: one cluster of 20 cells
    assert count.tolist() == [1, 38] and table[0, 1] == 20 and np.all(table[1:] == -1)


def query(name, a=0, b=0, c=0, guard=-1):
    abi = pkg("_abi")
    out = C.c_int64()
    abi.check(abi.lib().slam_plan_query(name.encode(), int(a), int(b), int(c), int(guard), C.byref(out)))
    return int(out.value)


def test_launch_shape_at_its_edges():
    tx, ty, seg = query("kFrontierTileX"), query("kFrontierTileY"), query("kFrontierSeg")
    assert (tx, ty, seg) == (32, 64, 1024) and query("kFrontierThreads") == 256 and ty == query("kWave")
    assert query("kFrontierMaxRadius") == 8 and query("kFrontierMaxClusters") == 65536
    ceil = lambda a, b: -(-a // b)
    for xw, yw in ((1, 1), (1, 130), (130, 1), (tx, ty), (tx + 1, ty), (tx, ty + 1), (tx + 1, ty + 1), (130, 67), (400, 400), (2000, 2000)):
        nx, ny = ceil(xw, tx), ceil(yw, ty)
        assert (query("frontier_tiles_x", xw, yw), query("frontier_tiles_y", xw, yw), query("frontier_tiles", xw, yw)) == (nx, ny, nx * ny)
        assert query("frontier_border", xw, yw) == (nx - 1) * yw + (ny - 1) * xw         # a cell per tile border it lies on
        assert query("frontier_segs", xw, yw) == ceil(xw * yw, seg)
        assert query("frontier_query_bytes", xw, yw) == 4 * xw * yw + 8 * ceil(xw * yw, seg)
    assert query("frontier_border", tx, ty) == 0 and query("frontier_tiles", 1, 1) == 1
    assert query("frontier_tiles", 0, 5) == 0 and query("frontier_tiles", 5, -1) == 0
    # the tile's labels, its cell classes with a halo of max(radius, 1) and the window's row sums, then the guard
    for r in range(9):
        h = max(r, 1)
        want = ceil(tx * ty * 4 + (tx + 2 * h) * (ty + 2 * h) + (tx + 2 * h) * ty, 16) * 16
        assert query("frontier_lds", r, guard=0) == want and query("frontier_lds", r, guard=512) == want + 512
    assert query("frontier_lds", 8, guard=512) <= query("kLdsDefault") and query("frontier_lds", 9) == 0
    # chunks: as many queries as fit the budget, B at one chunk and one more; none (0) when one query does not fit
    qb = query("frontier_query_bytes", 130, 67)
    assert query("frontier_chunk_queries", 256 * 1024, qb, 7) == 7
    kib = ceil(7 * qb, 1024)
    assert query("frontier_chunk_queries", kib, qb, 7) == 7 and query("frontier_chunk_queries", kib, qb, 8) == 7
    assert query("frontier_chunk_queries", ceil(qb, 1024), qb, 7) == 1 and query("frontier_chunk_queries", qb // 1024, qb, 7) == 0
    big = query("frontier_query_bytes", 2000, 2000)
    assert query("frontier_chunk_queries", 256 * 1024, big, 64) == 256 * 1024 * 1024 // big == 16


def test_entry_points_are_declared_bound_and_exported():
    abi, slam = pkg("_abi"), pkg()
    declared = abi.header_symbols()
    for n in ("slam_grid_frontiers", "slam_grid_frontiers_dev"):
        assert n in declared and n in abi._SIGS and hasattr(abi.lib(), n), n
    assert abi._SIGS["slam_grid_frontiers"] == abi._SIGS["slam_grid_frontiers_dev"] and len(abi._SIGS["slam_grid_frontiers"][0]) == 14
    for n in ("grid_frontiers_host", "frontier_points"):
        assert n in slam.__all__ and hasattr(slam, n), n
    assert hasattr(slam.DeviceGrid, "frontiers") and hasattr(slam.Mapping, "frontiers") and hasattr(slam.Mapping, "next_goal")
    assert hasattr(slam.GridSLAM, "frontiers") and hasattr(slam.GridSLAM, "next_goal") and hasattr(slam.DeviceGridSLAM, "frontiers")
    assert abi.lib().slam_abi_version() == 1 and len(abi.K_NAMES) == 8
    pts = slam.frontier_points(np.array([[0, 0], [199, 3]]), 20.0, 10.0, 10.0)
    assert np.array_equal(pts, np.array([[0.5 / 20 - 10, 0.5 / 20 - 10], [199.5 / 20 - 10, 3.5 / 20 - 10]]))
