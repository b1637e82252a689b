"""A ``Mapping`` is a one-map ``DeviceGrid``: every one-map answer of ``Mapping`` equals, bit for bit, row 0 of the batched
host function on a ``DeviceGrid`` asked for the same map with ``grid_of_batch=[1]``.

The map is 70 x 45 cells of 0.2 m (not square, yw no multiple of 32) and holds three scans of 37 beams of the synthetic
room; the same scans go into map 1 of a two-map grid whose map 0 stays empty, so an answer read from the wrong map differs."""
import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

XW, YW, RESO, BEAMS = 70, 45, 0.2, 37
MAP = [1]


@pytest.fixture(scope="module")
def slam():
    p = pkg()
    p._abi.default_context()   # fails loudly when there is no gfx950 device
    return p


@pytest.fixture(scope="module")
def both(slam, syn):
    """(mapping, grid, ranges [3, 37], poses [3, 3], cos_t, sin_t) with the three scans in the mapping and in map 1 of the grid."""
    ctx = slam.Context(0)
    rep = syn.make_replay(3, BEAMS, seed=4)
    ranges, poses = np.asarray(rep.ranges, dtype=np.float32), np.asarray(rep.poses_true, dtype=np.float64)
    ct, st = pkg("_abi").trig_tables(syn.ANGLE_MIN, syn.ANGLE_MAX, BEAMS)
    m = slam.Mapping.metric(XW, YW, RESO, context=ctx)
    g = slam.DeviceGrid.metric(2, XW, YW, RESO, context=ctx)
    assert (m.index_scale, m.index_offset_x, m.index_offset_y) == (g.scale, g.off_x, g.off_y) == (5.0, 7.0, 4.5)
    m.update_scans(ranges, syn.ANGLE_MIN, syn.ANGLE_MAX, poses)
    for k in range(3):
        slam.grid_update_particles_host(g, ranges[k:k + 1], ct, st, poses[k].reshape(1, 1, 3), map0=1)
    yield m, g, ranges, poses, ct, st
    ctx.close()


def same(got, want):
    """Bit equality of two arrays (dtype and shape included), of two tuples of them, or of two plain numbers."""
    if isinstance(want, tuple):
        assert isinstance(got, tuple) and len(got) == len(want)
        for a, b in zip(got, want):
            same(a, b)
    elif isinstance(want, np.ndarray):
        assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape, (got, want)
        assert np.ascontiguousarray(got).tobytes() == np.ascontiguousarray(want).tobytes(), (got, want)
    else:
        assert type(got) is type(want) and got == want, (got, want)


def rows0(out):
    return tuple(o[0] for o in out) if isinstance(out, tuple) else out[0]


def test_the_maps_hold_the_same_evidence(slam, both):
    m, g, *_ = both
    got = g.read(1, want=("pass", "hit", "pmap"))
    same(m.counters(), (got["pass"], got["hit"]))
    assert got["hit"].any() and (got["pmap"] == 0).any() and not any(v.any() for v in g.read(0, want=("pass", "hit")).values())
    same(m.pmap.astype(np.int8), got["pmap"])
    same(m.occupancy_grid_data(), g.occupancy_grid_data(1))
    same(m.visits(), g.visits())
    assert m.visits() > 0


def test_raycast_and_score(slam, syn, both):
    m, g, ranges, poses, ct, st = both
    got = m.raycast(poses[2], syn.ANGLE_MIN, syn.ANGLE_MAX, BEAMS, return_cells=True)
    same(got, rows0(slam.grid_raycast_host(g, poses[2:3], ct, st, grid_of_batch=MAP, return_cells=True)))
    assert np.isfinite(got[0]).any()
    same(m.raycast(poses[2], syn.ANGLE_MIN, syn.ANGLE_MAX, BEAMS), got[0])
    same(m.score_scan(ranges[2], syn.ANGLE_MIN, syn.ANGLE_MAX, poses[2]),
         rows0(slam.grid_score_host(g, ranges[2], poses[2:3], ct, st, grid_of_batch=MAP)))
    with pytest.raises(ValueError):
        m.raycast(np.concatenate([poses[0], poses[1]]), syn.ANGLE_MIN, syn.ANGLE_MAX, BEAMS)      # six numbers are not two poses here


def test_distance_field_match_and_locate(slam, syn, both):
    m, g, ranges, poses, ct, st = both
    field = m.distance_field()
    same(field, slam.grid_distance_field_host(g)[1])
    assert field.min() == 0 and field.max() == 64
    pose, step = poses[2], 1.0 / g.scale
    th, rot = slam.match_rotations(pose[2:3], 3, 0.01)
    best, cost, used, vol = slam.grid_match_host(g, ranges[2], pose[None, :2], ct, st, rot, 2, 1, step, grid_of_batch=MAP, return_costs=True)
    assert vol.shape == (1, 3, 5, 3)
    same(m.match_scan(ranges[2], syn.ANGLE_MIN, syn.ANGLE_MAX, pose, window=(2, 1), n_rot=3, return_costs=True),
         (slam.match_pose(pose[None, :2], th, best, 2, 1, step)[0], int(cost[0]), int(used[0]), vol[0]))
    same(m.match_scan(ranges[2], syn.ANGLE_MIN, syn.ANGLE_MAX, pose, window=(2, 1), n_rot=3),
         (slam.match_pose(pose[None, :2], th, best, 2, 1, step)[0], int(cost[0]), int(used[0])))
    rot = slam.locate_rotations(8)[1]
    best, cost, used = slam.grid_locate_host(g, ranges[2], ct, st, rot, levels=2, grid_of_batch=MAP)
    assert best[0, 0] >= 0
    same(m.locate_scan(ranges[2], syn.ANGLE_MIN, syn.ANGLE_MAX, n_rot=8, levels=2),
         (slam.locate_pose(best, g.scale, g.off_x, g.off_y, rot)[0], int(cost[0]), int(used[0])))


def test_frontiers(slam, both):
    m, g, *_ = both
    got = m.frontiers(radius=1, min_unknown=2, min_size=1)
    count, clusters, sums = slam.grid_frontiers_host(g, MAP, radius=1, min_unknown=2, min_size=1)
    want = pkg("grid").frontier_dict(count[0], clusters[0], sums[0], g.scale, g.off_x, g.off_y)
    assert got["count"] > 0 and sorted(got) == sorted(want)
    for k in want:
        same(got[k], want[k])


def test_view_gain(slam, syn, both):
    m, g, ranges, poses, ct, st = both
    same(m.view_gain(poses[1], syn.ANGLE_MIN, syn.ANGLE_MAX, BEAMS, return_seen=True),
         rows0(slam.grid_view_gain_host(g, poses[1:2], ct, st, grid_of_batch=MAP, return_seen=True)))
    six = np.stack([poses, poses + [0.3, -0.2, 0.5]])                                             # [2, 3] poses
    got = m.view_gain(six, syn.ANGLE_MIN, syn.ANGLE_MAX, BEAMS, return_seen=True)
    same(got, slam.grid_view_gain_host(g, six.reshape(6, 3), ct, st, grid_of_batch=MAP * 6, return_seen=True))
    assert got[0].shape == (6, 4) and got[1].shape == (6, XW, 2) and (got[0] >= 0).all()
    same(m.view_gain(six, syn.ANGLE_MIN, syn.ANGLE_MAX, BEAMS), got[0])


def test_travel_field_and_path(slam, both):
    m, g, ranges, poses, ct, st = both
    grid = pkg("grid")
    src = np.array([[m.pose_cell(poses[2])]], dtype=np.int32)
    field = m.travel_field(poses[2])
    same(field, slam.grid_travel_host(g, src, MAP)["cost"][0])
    assert (field >= 0).sum() > 1
    goal = np.argwhere(field == field.max())[0].astype(np.int32)                                  # the reachable cell furthest to drive to
    want = slam.grid_travel_host(g, src, MAP, goals=goal.reshape(1, 1, 2), path_cap=256, cost=False)
    n = int(want["path_len"][0, 0])
    assert 1 < n <= 256
    same(m.travel_path(poses[2], grid.frontier_points(goal, g.scale, g.off_x, g.off_y)),
         (grid.frontier_points(want["path"][0, 0, :n], g.scale, g.off_x, g.off_y), int(want["goal_cost"][0, 0])))
