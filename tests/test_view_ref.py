"""The view gain without a GPU: the NumPy reference (tests/view_ref.py) and the inputs the GPU tests use have the
properties those tests rest on; the two entry points are declared, bound and exported; plan_view answers through
slam_plan_query at its edges; and the goal rule of next_goal(by="gain") on hand-made tables."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import raycast_ref as R
import view_ref as V
from conftest import ROOT, pkg
from oracle import oracle_np as O

SYMBOLS = ("slam_grid_view_gain", "slam_grid_view_gain_dev")


# ------------------------------------------------------------------ entry points
def test_header_declares_and_binding_covers_the_two_entry_points():
    abi = pkg("_abi")
    names = abi.header_symbols()
    for s in SYMBOLS:
        assert s in names, s
        assert s in abi._SIGS, s
        assert hasattr(abi.lib(), s), s
        assert len(abi._SIGS[s][0]) == 12, s
    assert abi._SIGS[SYMBOLS[0]] == abi._SIGS[SYMBOLS[1]] == abi._SIGS["slam_grid_raycast"]
    text = open(os.path.join(ROOT, "include", "slam_hip.h")).read()
    codes = dict(re.findall(r"#define SLAM_VIEW_([A-Z]+) (\d)", text))
    assert codes == {"UNKNOWN": "0", "FREE": "1", "OCCUPIED": "2", "OPEN": "3", "COUNTS": "4"}
    for word in ("gain_lds", "gain_ws_mb"):
        assert word in text, word
    slam = pkg()
    assert (slam.VIEW_UNKNOWN, slam.VIEW_FREE, slam.VIEW_OCCUPIED, slam.VIEW_OPEN, slam.VIEW_COUNTS) == \
        (V.UNKNOWN, V.FREE, V.OCCUPIED, V.OPEN, 4) == (0, 1, 2, 3, 4)
    for name in ("grid_view_gain_host", "view_poses", "view_tables", "gain_goal", "VIEW_UNKNOWN", "VIEW_COUNTS"):
        assert name in slam.__all__, name
    assert callable(slam.grid_view_gain_host) and callable(slam.view_poses) and callable(slam.gain_goal)
    assert callable(slam.Mapping.view_gain) and callable(slam.DeviceGrid.view_gain)
    assert callable(slam.GridSLAM.view_gain) and callable(slam.DeviceGridSLAM.view_gain)
    assert abi.lib().slam_abi_version() == 1 and len(abi.K_NAMES) == 8


def test_one_copy_of_trace_and_of_the_beam():
    """trace and the per-ray set-up live in the header both readers of the map include; neither kernel file has its own."""
    csrc = os.path.join(ROOT, pkg().__name__, "csrc")
    defs = {"trace": r"\bint trace\(", "beam_cells": r"\bvoid beam_cells\("}
    for f in ("raycast_kernels.hip", "view_kernels.hip"):
        text = open(os.path.join(csrc, f)).read()
        assert '#include "ray_trace.h"' in text and '#include "grid_walk.h"' in text, f
        for name, pat in list(defs.items()) + [("ray_setup", r"bool ray_setup\("), ("walk_step", r"bool walk_step\("), ("CellWalk", r"struct CellWalk \{")]:
            assert not re.search(pat, text), (f, name)
    text = open(os.path.join(csrc, "ray_trace.h")).read()
    for name, pat in defs.items():
        assert len(re.findall(pat, text)) == 1, name
    assert "view_kernels.hip" in open(os.path.join(csrc, "Makefile")).read()
    assert "asm" not in open(os.path.join(csrc, "view_kernels.hip")).read()


def test_view_poses_and_tables():
    slam = pkg()
    cells = np.array([[3, 4], [0, 0], [399, 17]])
    p = slam.view_poses(cells, 20.0, 10.0, 10.0)
    assert p.shape == (3, 3) and p.dtype == np.float64 and np.all(p[:, 2] == 0)
    assert np.array_equal(p[:, :2], slam.frontier_points(cells, 20.0, 10.0, 10.0))
    for c, q in zip(cells, p):                                     # a cell's centre is in that cell by the map's rule
        assert (R.to_cell(q[0], 20.0, 10.0), R.to_cell(q[1], 20.0, 10.0)) == tuple(c)
    assert slam.view_poses(cells.reshape(1, 3, 2), 20.0, 10.0, 10.0).shape == (1, 3, 3)
    ct, st = slam.view_tables(360)
    th = -np.pi + np.arange(360) * (2.0 * np.pi / 360)
    assert np.array_equal(ct, np.cos(th)) and np.array_equal(st, np.sin(th)) and ct.flags.c_contiguous
    import torch
    tp = slam.view_poses(torch.from_numpy(cells.astype(np.int32)), 20.0, 10.0, 10.0)
    assert tp.dtype == torch.float64 and np.array_equal(tp.numpy(), p)


# ------------------------------------------------------------------ launch shape
def query(name, a=0, b=0, c=0, guard=0):
    abi = pkg("_abi")
    out = C.c_int64(-1)
    abi.check(abi.lib().slam_plan_query(name.encode(), a, b, c, guard, C.byref(out)))
    return int(out.value)


def test_launch_shape_at_its_edges():
    bound = query("kViewLdsBytes")
    assert bound == 64 * 1024 and query("kViewThreads") == 256 and query("kViewMaxBlocks") == 16384
    # words per row at the word edge
    assert [query("view_row_words", yw) for yw in (1, 31, 32, 33, 64, 65)] == [1, 1, 1, 2, 2, 3]
    assert query("view_bytes", 400, 400) == 400 * 13 * 4 == 20800 and query("view_bytes", 5, 257) == 5 * 9 * 4
    # a box window of exactly the bound, and one word row more: 128 words a row, 128 rows fit, 129 do not
    rows = bound // 4 // 128
    assert rows * 128 * 4 == bound
    for mode in (-1, 1):
        assert query("view_engine", rows, 128, mode) == 1 and query("view_engine", rows + 1, 128, mode) == 0
    assert query("view_engine", rows, 128, 0) == 0 and query("view_engine", 1, 1, 0) == 0
    assert query("view_window_words", rows, 128) == bound // 4 and query("view_window_words", rows + 1, 128) == bound // 4 + 128
    assert query("view_lds_bytes", rows, 128, 0, 0) == bound and query("view_lds_bytes", rows, 128, 0, 512) == bound + 512
    assert query("view_lds_bytes", 3, 2, 0, 0) == 24
    # one word more in a row of 16 384: the same edge the other way round
    assert query("view_engine", 1, 16384, 1) == 1 and query("view_engine", 1, 16385, 1) == 0
    # chunking: budget for exactly B slots, for B + 1, for B - 1, for 1, and below one view
    vb = query("view_bytes", 300, 37)
    assert vb == 300 * 2 * 4
    kib = lambda views: -(-views * vb // 1024)
    B = 64
    assert vb * B % 1024 == 0
    assert (query("view_chunk_views", kib(B), vb, B), query("view_chunks", kib(B), vb, B)) == (B, 1)
    assert (query("view_chunk_views", kib(B), vb, B + 1), query("view_chunks", kib(B), vb, B + 1)) == (B, 2)
    assert (query("view_chunk_views", kib(B + 1), vb, B), query("view_chunks", kib(B + 1), vb, B)) == (B, 1)
    half = (vb * B // 2) // 1024
    assert (query("view_chunk_views", half, vb, B), query("view_chunks", half, vb, B)) == (B // 2, 2)
    assert (query("view_chunk_views", 3, vb, B), query("view_chunks", 3, vb, B)) == (1, B)          # 3 KiB: one slot of 2 400 bytes
    assert query("view_chunk_views", 2, vb, B) == 0 and query("view_chunks", 2, vb, B) == 0         # 2 KiB: below one view
    # never more slots than the block cap
    assert query("view_chunk_views", 1 << 20, 4, 1 << 20) == 16384 and query("view_chunks", 1 << 20, 4, 1 << 20) == 64


# ------------------------------------------------------------------ the goal rule
def fr_of(K):
    return dict(point=np.arange(2.0 * K).reshape(K, 2))


def test_gain_goal_rule():
    gain_goal = pkg().gain_goal
    # the larger unknown per (cost + bias) wins, not the nearer and not the larger count alone
    assert gain_goal(fr_of(3), [10, 100, 400], [5, 200, 210], bias=100) == 1
    assert gain_goal(fr_of(3), [10, 100, 400], [5, 200, 210], bias=100000) == 2       # a huge bias: the count alone
    # a tie on the ratio goes to the lower cost: 10 / (100 + 100) == 20 / (300 + 100)
    assert gain_goal(fr_of(2), [300, 100], [20, 10], bias=100) == 1
    assert gain_goal(fr_of(2), [100, 300], [10, 20], bias=100) == 0
    # a tie on the cost as well goes to the lower label
    assert gain_goal(fr_of(3), [-1, 50, 50], [9, 7, 7], bias=100) == 1
    # u == 0 everywhere, no reachable cluster, no cluster at all
    assert gain_goal(fr_of(3), [10, 20, 30], [0, 0, 0]) is None
    assert gain_goal(fr_of(3), [-1, -1, -1], [5, 6, 7]) is None
    assert gain_goal(fr_of(0), [], []) is None
    # the rows of a bad view (-1) and of an unreachable cluster are no candidates
    assert gain_goal(fr_of(3), [5, -1, 900], [-1, 1000, 1], bias=100) == 2
    # exact where floats would tie or flip: u / (c + bias) differ by 1 in 2^62
    big = 2 ** 31 // 14 - 1
    assert gain_goal(fr_of(2), [2 ** 31 - 3, 2 ** 31 - 2], [big, big], bias=1) == 0
    assert gain_goal(fr_of(2), [2 ** 31 - 2, 2 ** 31 - 3], [big, big], bias=1) == 1
    # only the kept clusters of fr count
    assert gain_goal(fr_of(1), [10, 10], [1, 50]) == 0
    with pytest.raises(ValueError):
        gain_goal(fr_of(1), [1], [1], bias=0)


# ------------------------------------------------------------------ the reference and the shared inputs
def run(pm, cell, ends, skip=1, **kw):
    ct, st = R.tables_to(ends, cell)
    return V.detail(pm, 1.0, 0.0, 0.0, V.pose_at(cell), ct, st, 1.0, skip, **kw)


def test_ring_map_is_a_union_and_keeps_path_order():
    pm = R.ring_pmap()
    d = run(pm, R.CENTRE, R.ring(24))
    print("ring(24):", d["counts"], "marks", d["marks"], "distinct", len(d["seen"]))
    assert d["marks"] > 4 * len(d["seen"])                                       # the beams share most of their cells
    assert d["counts"][V.UNKNOWN] == 0 and d["counts"][V.OPEN] == 0
    assert d["counts"][V.OCCUPIED] == len(R.ring(8)) == 64                       # every first hit: the whole inner ring
    assert d["counts"][V.FREE] == 15 * 15 - 1                                    # the disc inside it, without the robot's cell
    assert d["counts"][:3].sum() == len(d["seen"]) and R.CENTRE not in d["seen"]
    # counting marks instead of cells, or taking the walk-order find on the 96 reversed lines, gives other answers
    wrong = run(pm, R.CENTRE, R.ring(24), walk_order=True)
    print("walk order:", wrong["counts"])
    assert d["marks"] != len(d["seen"])
    assert tuple(wrong["counts"]) != tuple(d["counts"]) and wrong["counts"][V.OCCUPIED] == 64 + 64
    # skip 0 adds exactly the robot's own cell
    d0 = run(pm, R.CENTRE, R.ring(24), skip=0)
    assert d0["seen"] == d["seen"] | {R.CENTRE} and d0["counts"][V.FREE] == d["counts"][V.FREE] + 1
    # beams that end inside the inner ring find nothing
    d6 = run(pm, R.CENTRE, R.ring(6))
    assert tuple(d6["counts"]) == (0, 13 * 13 - 1, 0, len(R.ring(6)))
    # the words and the set say the same
    counts, words = V.view(pm, 1.0, 0.0, 0.0, R.RING_POSE, *R.tables_to(R.ring(24)), 1.0)
    assert V.cells_of(words, 64) == d["seen"] and np.array_equal(counts, d["counts"]) and words.shape == (64, 2)


def test_gap_map_sees_unknown_through_the_gap():
    pm = V.gap_pmap()
    assert int((pm == 100).sum()) == 64 + 128 - len(V.GAP_INNER) - len(V.GAP_OUTER)
    p, h = V.counters_of(pm)
    assert np.array_equal(np.where(h > 0, 100, np.where(p > 0, 0, 50)), pm)
    seq = [run(pm, R.CENTRE, R.ring(r))["counts"] for r in (24, 31, 40)]
    print("gap map, ring 24 / 31 / 40:", [tuple(int(v) for v in c) for c in seq])
    assert 0 < seq[0][V.UNKNOWN] < seq[1][V.UNKNOWN] < seq[2][V.UNKNOWN]         # unknown grows with range
    assert all(c[V.OPEN] > 0 for c in seq) and seq[0][V.OPEN] < seq[2][V.OPEN]
    # ring(40) ends outside the 64 x 64 map: the cells out there are seen by nobody
    d = run(pm, R.CENTRE, R.ring(40))
    assert all(0 <= x < 64 and 0 <= y < 64 for x, y in d["seen"])
    # through the inner gap the view sees cells of the outer ring, through the outer gap unknown cells beyond it
    occ = {c for c in d["seen"] if pm[c] == 100}
    assert any(max(abs(x - 32), abs(y - 32)) == 16 for x, y in occ) and len(occ) == d["counts"][V.OCCUPIED] < 64
    assert any(x > 48 and pm[x, y] == 50 for x, y in d["seen"])


def test_view_that_leaves_the_map():
    pm = V.gap_pmap()
    ends = R.ring(20, V.LEAVE_CELL)
    outside = sum(not (0 <= x < 64 and 0 <= y < 64) for x, y in ends)
    assert outside > len(ends) // 2                                              # most end cells are out of bounds
    d = run(pm, V.LEAVE_CELL, ends)
    print("leaving the map:", d["counts"])
    assert d["counts"][V.UNKNOWN] > 400 and d["counts"][V.OPEN] > outside // 2 and d["counts"][V.OCCUPIED] > 0
    assert all(0 <= x < 64 and 0 <= y < 64 for x, y in d["seen"])
    assert max(y for _, y in d["seen"]) == 63 and min(x for x, _ in d["seen"]) == 0     # up to the map's edges


def test_bad_views_and_beams():
    pm = R.ring_pmap()
    ct, st = R.tables_to(R.ring(24))
    for pose in ([np.nan, 32.5, 0.0], [32.5, np.inf, 0.0], [32.5, 32.5, np.nan], [2.0 ** 20, 32.5, 0.0]):
        counts, words = V.view(pm, 1.0, 0.0, 0.0, pose, ct, st, 1.0)
        assert np.all(counts == -1) and not words.any() and words.shape == (64, 2)
    assert np.all(V.view(None, 1.0, 0.0, 0.0, R.RING_POSE, ct, st, 1.0)[0] == -1)
    # a beam whose end the index rule rejects is skipped: not OPEN, nothing seen
    counts, words = V.view(pm, 1.0, 0.0, 0.0, R.RING_POSE, [1.0, 0.0], [0.0, 1.0], float(2 ** 21))
    assert tuple(counts) == (0, 0, 0, 0) and not words.any()
    # skip = Lp: nothing left to see, the beam still finds nothing
    counts, _ = V.view(pm, 1.0, 0.0, 0.0, R.RING_POSE, *R.tables_to([(56, 40)]), 1.0, skip=25)
    assert tuple(counts) == (0, 0, 0, 1)
    # identical cells: an empty path, OPEN
    assert tuple(V.view(pm, 1.0, 0.0, 0.0, R.RING_POSE, [0.0], [0.0], 1.0)[0]) == (0, 0, 0, 1)


def test_the_cast_sees_what_the_view_counts():
    """The cross-check the GPU test makes against slam_grid_raycast, on the references: the cast's cells are the seen
    occupied cells, its inf ranges the open beams."""
    pm = V.gap_pmap()
    ct, st = R.tables_to(R.ring(31))
    ranges, cells = R.raycast(pm, 1.0, 0.0, 0.0, R.RING_POSE, ct, st, 1.0)
    d = V.detail(pm, 1.0, 0.0, 0.0, R.RING_POSE, ct, st, 1.0)
    hit = {tuple(c) for c in cells if c[0] >= 0}
    assert hit == {c for c in d["seen"] if pm[c] == 100} and len(hit) == d["counts"][V.OCCUPIED]
    assert int(np.isinf(ranges).sum()) == d["counts"][V.OPEN]


def test_two_room_map_separates_the_goal_rules():
    """The slit is nearer by travel and in a straight line; the mouth reveals more per unit of travel."""
    import frontier_ref as F
    import travel_ref as T
    slam = pkg()
    pm = V.two_room_pmap()
    count, clusters, _, _ = F.frontiers(pm, M=16, **V.ROOM_FRONTIERS)
    assert count[0] == 2
    reps = clusters[:2, 2:4]
    assert [tuple(r) for r in reps] == [V.ROOM_SLIT, V.ROOM_MOUTH] and clusters[0, 1] < clusters[1, 1]
    cost = T.answer(pm, None, np.array([V.ROOM_ROBOT]), goals=reps)["goal_cost"]
    assert 0 <= cost[0] < cost[1]
    ct, st = slam.view_tables(360)
    counts, _ = V.views([pm], 1.0, 0.0, 0.0, slam.view_poses(reps, 1.0, 0.0, 0.0), ct, st, 30.0)
    u = counts[:, V.UNKNOWN]
    print("two rooms: cost", cost, "unknown in view", u)
    assert 0 < u[0] < u[1] and int(u[1]) * (int(cost[0]) + 100) > int(u[0]) * (int(cost[1]) + 100)
    fr = dict(point=slam.frontier_points(reps, 1.0, 0.0, 0.0))
    assert slam.replay.travel_goal(fr, cost) == 0 and slam.gain_goal(fr, cost, u, 100) == 1
    assert np.array_equal(slam.replay.nearest_goal(fr, V.pose_at(V.ROOM_ROBOT)), fr["point"][0])
