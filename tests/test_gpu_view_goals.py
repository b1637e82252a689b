"""Exploration goals by view gain on the GPU: Mapping.next_goal(by="gain") and DeviceGridSLAM.next_goals(by="gain")
on the two-room map of tests/view_ref.py - the nearer frontier is a slit into a small pocket, the farther one the mouth
of an unexplored hall - against the references (frontier_ref, travel_ref, view_ref) and the exact integer rule; and
by="distance" / by="travel" still answer what those references say."""
import numpy as np
import pytest

import frontier_cases as FC
import frontier_ref as F
import travel_ref as T
import view_ref as V
from conftest import pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def slam():
    p = pkg()
    p._abi.default_context()   # fails loudly when there is no gfx950 device
    return p


@pytest.fixture(scope="module", params=[0, 1], ids=["global", "lds"])
def ctx(request, slam):
    c = slam.Context(0)
    c.set_option("gain_lds", request.param)
    yield c
    c.close()


def test_mapping_next_goal_by_gain(slam, ctx):
    m = slam.Mapping(64, 64, 1.0, index_scale=1.0, index_offset=0.0, context=ctx)
    pm = FC.write(FC.MapGrid(m), V.two_room_pmap()[None])[0]
    pose = V.pose_at(V.ROOM_ROBOT)
    kw = dict(V.ROOM_FRONTIERS)
    slit, mouth = V.pose_at(V.ROOM_SLIT)[:2], V.pose_at(V.ROOM_MOUTH)[:2]
    fr = m.frontiers(**kw)
    assert fr["cell"].tolist() == [list(V.ROOM_SLIT), list(V.ROOM_MOUTH)]
    assert np.array_equal(m.next_goal(pose, **kw), slit) and np.array_equal(m.next_goal(pose, by="distance", **kw), slit)
    assert np.array_equal(m.next_goal(pose, by="travel", **kw), slit)
    assert np.array_equal(m.next_goal(pose, by="gain", **kw), mouth)
    # the pieces of the rule, against the references
    cost = T.answer(pm, None, np.array([V.ROOM_ROBOT]), goals=fr["cell"])["goal_cost"]
    ct, st = slam.view_tables(360)
    views = slam.view_poses(fr["cell"], 1.0, 0.0, 0.0)
    want = V.views([pm], 1.0, 0.0, 0.0, views, ct, st, 30.0)[0]
    got = slam.grid_view_gain_host(FC.MapGrid(m), views, ct, st, max_range=30.0)
    assert np.array_equal(got, want) and slam.gain_goal(fr, cost, want[:, V.UNKNOWN], 100) == 1
    # a bias far beyond the costs makes the count decide alone; a short range hides the hall: the slit's pocket wins
    assert np.array_equal(m.next_goal(pose, by="gain", bias=10 ** 6, **kw), mouth)
    near = V.views([pm], 1.0, 0.0, 0.0, views, ct, st, 3.0)[0][:, V.UNKNOWN]
    k = slam.gain_goal(fr, cost, near, 100)
    assert np.array_equal(m.next_goal(pose, by="gain", max_range=3.0, **kw), fr["point"][k])
    # the mouth walled off from the robot: only the slit can be reached
    closed = pm.copy()
    closed[25, 10:31] = 100
    FC.write(FC.MapGrid(m), closed[None])
    assert np.array_equal(m.next_goal(pose, by="gain", **kw), slit)
    # no frontier at all
    FC.write(FC.MapGrid(m), np.zeros((1, 64, 64), dtype=np.int8))
    assert m.next_goal(pose, by="gain", **kw) is None
    with pytest.raises(ValueError):
        m.next_goal(pose, by="bearing")


def test_device_gridslam_view_gain_and_next_goals_by_gain(slam, ctx):
    import torch
    from raycast_ref import AMAX, AMIN
    d = slam.DeviceGridSLAM(3, 2, 64, 64, 0.1, angle_min=AMIN, angle_max=AMAX, n=8, context=ctx, max_range=3.0)
    scale, ox, oy = d.grid.scale, d.grid.off_x, d.grid.off_y
    room, closed = V.two_room_pmap(), V.two_room_pmap()
    closed[25, 10:31] = 100
    free = np.zeros((64, 64), dtype=np.int8)
    pm = FC.write(d.grid, np.stack([free, room, free, free, closed, free]))
    at = lambda c: ((c[0] + 0.5) / scale - ox, (c[1] + 0.5) / scale - oy)
    poses = np.zeros((3, 2, 3))
    poses[0, 1, :2] = at(V.ROOM_ROBOT)
    poses[2, 0, :2] = at(V.ROOM_ROBOT)
    d.set_particles(poses)
    d.info[:, 0] = torch.tensor([1, -1, 0], dtype=torch.int32, device=d.dev)     # filter 1 has no live particle
    torch.cuda.synchronize()
    maps = [1, -1, 4]
    cells = np.array([[list(V.ROOM_ROBOT)], [[-1, -1]], [list(V.ROOM_ROBOT)]], dtype=np.int32)
    kw = dict(V.ROOM_FRONTIERS)
    M = 8
    reps = F.frontiers_batch(pm, maps=maps, M=M, **kw)[1][:, :, 2:4]
    cost = T.batch(pm, cells, maps=maps, goals=reps)["goal_cost"]
    ct, st = slam.view_tables(360)
    want = np.full((3, M, 4), -1, dtype=np.int32)
    for f, g in enumerate(maps):
        for k in range(M):
            if g >= 0 and reps[f, k, 0] >= 0:
                want[f, k] = V.view(pm[g], scale, ox, oy, slam.view_poses(reps[f, k], scale, ox, oy), ct, st, 3.0)[0]
    # view_gain on the table's representatives, device to device
    table = d.frontiers(max_clusters=M, **kw)[1]
    d.ctx.stream_order(d._torch_stream(), 0)
    counts = d.view_gain(table[:, :, 2:4].contiguous())
    ctx.synchronize()
    assert np.array_equal(counts.cpu().numpy(), want)
    # the goals
    cell, c, status, unknown = d.next_goals(by="gain", max_clusters=M, **kw)
    ctx.synchronize()
    assert status.cpu().tolist() == [0, -1, 0]
    for f in range(3):
        k = slam.gain_goal(dict(point=np.zeros((M, 2))), cost[f], want[f, :, V.UNKNOWN], 100)
        if k is None:
            assert cell[f].cpu().tolist() == [-1, -1] and c[f].item() == -1 and unknown[f].item() == -1, f
        else:
            assert cell[f].cpu().tolist() == reps[f, k].tolist() and c[f].item() == cost[f, k] and unknown[f].item() == want[f, k, 0], f
    assert cell[0].cpu().tolist() == list(V.ROOM_MOUTH) and cell[2].cpu().tolist() == list(V.ROOM_SLIT)
    # the default rule is still the travel rule, with its three return values
    out = d.next_goals(max_clusters=M, **kw)
    ctx.synchronize()
    assert len(out) == 3 and out[0][0].cpu().tolist() == list(V.ROOM_SLIT) and out[1][0].item() == cost[0, 0]
    assert out[0][1].cpu().tolist() == [-1, -1] and out[0][2].cpu().tolist() == list(V.ROOM_SLIT)
    with pytest.raises(ValueError):
        d.next_goals(by="bearing")
    ctx.check_status()
