"""The NumPy reference of the distance field and the window matcher (tests/match_ref.py) pinned on the CPU: the
brute-force field against SciPy's exact Euclidean transform, and the reference's own answer to the recovery case the
GPU tests compare against.  Plus the pure helpers of the package and the header / binding of the four entry points."""
import numpy as np
import pytest

import match_ref as M
import raycast_ref as R
from conftest import pkg

SYMBOLS = ("slam_grid_distance_field", "slam_grid_distance_field_dev", "slam_grid_match", "slam_grid_match_dev")


def test_header_declares_and_binding_covers_the_four_entry_points():
    abi = pkg("_abi")
    names = abi.header_symbols()
    for s in SYMBOLS:
        assert s in names and s in abi._SIGS and hasattr(abi.lib(), s), s
    assert len(abi._SIGS["slam_grid_distance_field"][0]) == len(abi._SIGS["slam_grid_distance_field_dev"][0]) == 4
    assert len(abi._SIGS["slam_grid_match"][0]) == len(abi._SIGS["slam_grid_match_dev"][0]) == 21
    slam = pkg()
    for name in ("grid_distance_field_host", "grid_match_host", "match_pose"):
        assert callable(getattr(slam, name)), name
    for name in ("distance_field", "match"):
        assert callable(getattr(slam.DeviceGrid, name)), name
    for name in ("distance_field", "match_scan"):
        assert callable(getattr(slam.Mapping, name)), name


def test_brute_force_field_is_the_exact_euclidean_transform(syn):
    ndimage = pytest.importorskip("scipy.ndimage")
    case = M.room_case(syn)
    pm = case["pmap"]
    assert (pm == 100).sum() > 100
    edt2 = np.rint(ndimage.distance_transform_edt(pm != 100) ** 2).astype(np.int64)
    for cap in (1, 64, 32767):
        f = M.field(pm, cap)
        assert f.dtype == np.int16 and np.array_equal(f, np.minimum(edt2, cap))
    assert np.array_equal(case["field"], np.minimum(edt2, 64))
    # nothing occupied: cap everywhere
    assert np.all(M.field(np.full((5, 7), 50, dtype=np.int8), 9) == 9)
    # the ring map by hand: a cell of the inner ring, its neighbour, the centre (8 cells from the ring)
    f = M.field(R.ring_pmap(), 32767)
    assert f[24, 30] == 0 and f[25, 30] == 1 and f[32, 32] == 64 and f[0, 0] == 2 * 16 * 16


def test_reference_recovers_the_room_pose(syn):
    case = M.room_case(syn)
    best, cost, used, costs = case["ref"]
    a = M.ROOM_ARGS
    pose = M.pose_of(case["start"], case["thetas"], best, a["nx"], a["ny"], a["step"])
    assert np.allclose(case["true"], [0.8288, -1.3622, 0.4351], atol=5e-5)
    assert np.allclose(pose, [0.7988, -1.3422, 0.4351], atol=5e-5)
    assert abs(pose[0] - case["true"][0]) <= a["step"] + 1e-12 and abs(pose[1] - case["true"][1]) <= a["step"] + 1e-12
    assert abs(pose[2] - case["true"][2]) <= M.ROOM_ROT_STEP + 1e-12
    flat = np.sort(costs.reshape(-1))
    assert flat[0] == flat[1] == 51 and cost == 51           # a tie: the lowest flat index decides
    assert best == int(np.flatnonzero(costs.reshape(-1) == 51)[0]) and np.count_nonzero(costs == 51) >= 2
    assert used == int(np.sum(np.isfinite(case["scan"]) & (case["scan"] < 30.0))) and used > 0
    # the package's helper says the same pose
    slam = pkg()
    got = slam.match_pose(case["start"][None, :2], case["thetas"][None], [best], a["nx"], a["ny"], a["step"])
    assert got.shape == (1, 3) and np.array_equal(got[0], pose)
    th, rot = slam.match_rotations([case["start"][2]], M.ROOM_K, M.ROOM_ROT_STEP)
    assert np.array_equal(th[0], case["thetas"]) and np.array_equal(rot[0], case["rot_cs"])


def test_match_pose_rows():
    slam = pkg()
    ctr = np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]])
    th = np.array([[0.1, 0.2], [0.3, 0.4], [0.5, 0.6]])
    # nx = 1, ny = 2: 3 x 5 translations; flat = (k * 3 + i) * 5 + j
    got = slam.match_pose(ctr, th, [0, (1 * 3 + 2) * 5 + 4, -1], 1, 2, 0.5)
    assert np.array_equal(got[0], [0.5, 1.0, 0.1]) and np.array_equal(got[1], [3.5, 5.0, 0.4]) and np.all(np.isnan(got[2]))
    for b, best in enumerate((0, 29)):
        assert np.array_equal(got[b], M.pose_of(ctr[b], th[b], best, 1, 2, 0.5))


def test_reference_edges():
    fld = M.field(R.ring_pmap(), 64)
    ct, st = np.array([1.0, 0.0, -1.0]), np.array([0.0, 1.0, 0.0])
    rot = np.array([[1.0, 0.0]])
    kw = dict(nx=1, ny=0, step=1.0, max_range=10.0, cap=64)
    # beams of 8 cells from the middle of the ring's centre cell end on the inner ring: cost 0 at the centre
    best, cost, used, costs = M.match(fld, 1.0, 0.0, 0.0, np.full(3, 8.0, np.float32), (32.5, 32.5), ct, st, rot, **kw)
    assert (best, cost, used) == (1, 0, 3) and costs.shape == (1, 3, 1)
    # inf, NaN, at and above max_range are skipped
    r = np.array([np.inf, np.nan, 10.0], dtype=np.float32)
    assert M.match(fld, 1.0, 0.0, 0.0, r, (32.5, 32.5), ct, st, rot, **kw)[:3] == (0, 0, 0)
    # a NaN centre, a centre beyond 2^20 cells, no map
    for ctr, f in (((np.nan, 0.0), fld), ((2.0 ** 21, 0.0), fld), ((32.5, 32.5), None)):
        best, cost, used, costs = M.match(f, 1.0, 0.0, 0.0, np.full(3, 8.0, np.float32), ctr, ct, st, rot, **kw)
        assert (best, cost, used) == (-1, -1, 0) and np.all(costs == -1)
    # every end off the map: used * cap
    assert M.match(fld, 1.0, 0.0, 0.0, np.full(3, 8.0, np.float32), (500.5, 32.5), ct, st, rot, **kw)[:3] == (0, 192, 3)
