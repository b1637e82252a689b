"""Rays traced through a map, without a GPU: the NumPy reference (tests/raycast_ref.py) and the inputs the GPU tests
use (tests/test_gpu_raycast.py) have the properties those tests rest on, and the four entry points are declared
and bound."""
import os
import re

import numpy as np
import pytest

import raycast_ref as R
from conftest import ROOT, pkg
from oracle import oracle_np as O

SYMBOLS = ("slam_grid_raycast", "slam_grid_raycast_dev", "slam_grid_scan_score", "slam_grid_scan_score_dev")


def test_header_declares_and_binding_covers_the_four_entry_points():
    abi = pkg("_abi")
    names = abi.header_symbols()
    for s in SYMBOLS:
        assert s in names, s
        assert s in abi._SIGS, s
        assert hasattr(abi.lib(), s), s
    assert len(abi._SIGS["slam_grid_raycast"][0]) == len(abi._SIGS["slam_grid_raycast_dev"][0]) == 12
    assert len(abi._SIGS["slam_grid_scan_score"][0]) == len(abi._SIGS["slam_grid_scan_score_dev"][0]) == 13
    text = open(os.path.join(ROOT, "include", "slam_hip.h")).read()
    for ref in ("bresenham.py:2-58", "mapping.py:33-36", "slam_ekf.py:88-90", ":115-123", "raycast_lds"):
        assert ref in text, ref
    codes = dict(re.findall(r"SLAM_RAY_([A-Z]+) = (\d)", text))
    assert codes == {"EMPTY": "0", "HIT": "1", "BLOCKED": "2", "FREE": "3", "UNKNOWN": "4", "OUT": "5", "BAD": "6", "CLASSES": "7"}
    slam = pkg()
    assert (slam.RAY_EMPTY, slam.RAY_HIT, slam.RAY_BLOCKED, slam.RAY_FREE, slam.RAY_UNKNOWN, slam.RAY_OUT, slam.RAY_BAD) == \
        (R.EMPTY, R.HIT, R.BLOCKED, R.FREE, R.UNKNOWN, R.OUT, R.BAD) == tuple(range(7))
    assert callable(slam.grid_raycast_host) and callable(slam.grid_score_host)
    assert callable(slam.Mapping.raycast) and callable(slam.Mapping.score_scan)
    assert callable(slam.DeviceGrid.raycast) and callable(slam.DeviceGrid.score)


def test_one_copy_of_the_walk():
    """ray_setup, walk_step, CellWalk and to_cell are defined once, in the header both kernel files include."""
    csrc = os.path.join(ROOT, pkg().__name__, "csrc")
    defs = {"ray_setup": r"bool ray_setup\(", "walk_step": r"bool walk_step\(", "CellWalk": r"struct CellWalk \{", "to_cell": r"int to_cell\("}
    for f in ("grid_kernels.hip", "raycast_kernels.hip"):
        text = open(os.path.join(csrc, f)).read()
        assert '#include "grid_walk.h"' in text
        for name, pat in defs.items():
            assert not re.search(pat, text), (f, name)
    text = open(os.path.join(csrc, "grid_walk.h")).read()
    for name, pat in defs.items():
        assert len(re.findall(pat, text)) == 1, name


def test_ring_map_and_its_rays():
    pm = R.ring_pmap()
    assert int((pm == 100).sum()) == len(R.ring(8)) + len(R.ring(16)) == 64 + 128
    assert pm[R.CENTRE] == 0                                  # the origin cell was passed through, never hit
    ends = R.ring(24)
    assert len(ends) == 192 and sum(R.is_flagged(R.CENTRE, e) for e in ends) == 96
    ct, st = R.tables_to(ends)
    ranges, cells = R.raycast(pm, 1.0, 0.0, 0.0, R.RING_POSE, ct, st, 1.0, skip=1)
    for e, cell, r in zip(ends, cells, ranges):
        path = O.bresenham_path(R.CENTRE, e)
        assert path[0] == R.CENTRE and path[-1] == e          # the tables put the beam's end on the ring cell
        occ = [j for j, (x, y) in enumerate(path) if pm[x][y] == 100]
        assert len(occ) >= 2                                  # an early exit on a reversed walk has a second cell to find
        assert tuple(cell) == path[occ[0]] and max(abs(cell[0] - 32), abs(cell[1] - 32)) == 8
        assert r == np.float32(np.hypot(cell[0] - 32.0, cell[1] - 32.0))
    # a cast that took the first find in WALK order would answer the outer ring on the 96 reversed lines
    wrong = 0
    for e in ends:
        path = O.bresenham_path(R.CENTRE, e)
        walk = path[::-1] if R.is_flagged(R.CENTRE, e) else path
        first = next(c for c in walk if pm[c] == 100 and c != R.CENTRE)
        wrong += max(abs(first[0] - 32), abs(first[1] - 32)) != 8
    assert wrong == 96
    ties = R.near_tie_ends()
    assert len(ties) == 16 and len(set(ties)) == 16 and sum(R.is_flagged(R.CENTRE, e) for e in ties) == 8


def test_ring_scores():
    pm = R.ring_pmap()
    for r, want in ((24, R.BLOCKED), (8, R.HIT), (16, R.BLOCKED)):
        ends = R.ring(r)
        ct, st = R.tables_to(ends)
        counts, cls = R.score(pm, 1.0, 0.0, 0.0, R.RING_POSE, R.table_points(np.ones(len(ends), dtype=np.float32), ct, st))
        assert np.all(cls == want) and counts[want] == len(ends) == 8 * r and counts.sum() == len(ends)


def test_skip_and_empty():
    pm = R.ring_pmap().copy()
    pm[R.CENTRE] = 100
    e = (56, 40)
    assert R.trace(pm, R.CENTRE, e, 0)[:2] == (0, 25)
    j1 = R.trace(pm, R.CENTRE, e, 1)
    assert j1[0] == 8 and R.trace(pm, R.CENTRE, e, 3) == j1 and R.trace(pm, R.CENTRE, e, 9)[0] == 16
    assert R.trace(pm, R.CENTRE, e, 25) == (-1, 25, None)     # skip = Lp: nothing left
    assert R.trace(pm, R.CENTRE, R.CENTRE, 0) == (-1, 0, None)
    counts, cls = R.score(pm, 1.0, 0.0, 0.0, R.RING_POSE, R.table_points(np.zeros(3, dtype=np.float32), np.ones(3), np.zeros(3)))
    assert np.all(cls == R.EMPTY) and counts[R.EMPTY] == 3
    # infinite range -> 30 m; NaN range, NaN pose, an index beyond 2^20: BAD / NaN
    inf = R.table_points(np.array([np.inf], dtype=np.float32), [1.0], [0.0])
    assert inf[0, 0] == 30.0
    assert R.score(pm, 1.0, 0.0, 0.0, R.RING_POSE, R.table_points(np.array([np.nan], dtype=np.float32), [1.0], [0.0]))[1][0] == R.BAD
    assert R.score(pm, 1.0, 0.0, 0.0, [np.nan, 0.0, 0.0], inf)[1][0] == R.BAD
    r, c = R.raycast(pm, 1.0, 0.0, 0.0, R.RING_POSE, [1.0], [0.0], float(2 ** 20), skip=1)
    assert np.isnan(r[0]) and tuple(c[0]) == (-1, -1)
    assert R.to_cell(2.0 ** 20 - 0.5, 1.0, 0.0) == 2 ** 20 - 1 and R.to_cell(-0.9, 1.0, 0.0) == 0


@pytest.fixture(scope="module")
def room(syn):
    ranges, poses, hyp = R.room(syn)
    return ranges, poses, hyp, R.room_pmap(ranges, poses)


def test_room_true_pose_has_strictly_the_most_hits(room):
    ranges, poses, hyp, pm = room
    assert ranges.shape == (6, 120) and hyp.shape == (5, 3)
    pc = O.laser_to_numpy(ranges[-1], R.AMIN, R.AMAX, clip_inf=True)
    counts = np.stack([R.score(pm, 20.0, 10.0, 10.0, h, pc)[0] for h in hyp])
    print("room counts per hypothesis (empty hit blocked free unknown out bad):\n", counts)
    assert np.all(counts.sum(axis=1) == 120)
    assert np.all(counts[0, R.HIT] > counts[1:, R.HIT])
    assert counts[4, R.BAD] == 120 and counts[3, R.HIT] == 0
    assert R.to_cell(hyp[3, 0], 20.0, 10.0) < 0               # the fourth hypothesis stands outside the map ...
    r3, _ = R.raycast(pm, 20.0, 10.0, 10.0, hyp[3], *pkg("_abi").trig_tables(R.AMIN, R.AMAX, 120), 30.0)
    assert np.isfinite(r3).sum() > 0                          # ... and sees into it
    # the tables form of the points is laser_to_numpy's
    ct, st = pkg("_abi").trig_tables(R.AMIN, R.AMAX, 120)
    assert np.array_equal(R.table_points(ranges[-1], ct, st), pc)
