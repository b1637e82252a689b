"""Global scan localisation on the device (slam_grid_locate) against the NumPy restatement (tests/locate_ref.py),
through the C ABI.  Everything is integer: best (k, i, j), cost, used beams and the search statistics - the nodes
evaluated per level and the incumbent U - compare with array_equal; in every case the restatement reads the pmap read
back from the device."""
import numpy as np
import pytest

import locate_cases as LC
import locate_ref as L
import raycast_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu

LEVELS = (0, 1, 3, 5, 8)


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


@pytest.fixture(scope="module")
def room(slam, ctx, syn):
    """The room map on the device and the restatement's answer (shared with the CPU tests)."""
    case = L.room_case(syn)
    abi = pkg("_abi")
    g = slam.DeviceGrid.metric(1, 400, 400, 0.05, context=ctx)
    abi.check(abi.lib().slam_grid_update_scans(ctx.handle, g._h, abi.ptr(case["ranges"]), abi.ptr(case["cos_t"]), abi.ptr(case["sin_t"]),
                                               abi.ptr(np.ascontiguousarray(case["poses"])), None, 6, 120))
    assert np.array_equal(g.read()["pmap"], case["pmap"])
    return g, case


def regions_of(xw, yw):
    """The whole map; 1 x 1 in a corner, on an edge and inside; one row, one column; odd sizes that leave partial nodes
    on both far edges; rectangles on every edge."""
    return np.array([(0, 0, xw, yw), (0, 0, 1, 1), (xw - 1, yw - 1, 1, 1), (xw - 1, 3, 1, 1), (5, 7, 1, 1), (4, 0, 1, yw),
                     (0, 9, xw, 1), (3, 2, 13, 11), (0, 5, 9, 7), (xw - 9, 4, 9, 5), (6, 0, 7, 10), (2, yw - 11, 19, 11)], dtype=np.int32)


# ------------------------------------------------------------------ shapes: maps, depths, rotations, beams, regions
@pytest.mark.parametrize("shape", L.RAGGED)
def test_ragged_maps_at_every_depth(slam, ctx, shape):
    xw, yw = shape
    g = LC.ragged_grid(slam, ctx, xw, yw)
    cap = 50
    fields = LC.fields_of(slam, g, cap)
    regs = regions_of(xw, yw)
    for H, K, n in ((0, 1, 1), (0, 64, 65), (1, 7, 63), (3, 64, 65), (3, 7, 4096), (5, 7, 120), (5, 1, 63), (8, 1, 4096), (8, 64, 120)):
        ct, st, ranges = L.ragged_scan(n, seed=n + K)
        if n > 4:
            ranges[n // 2], ranges[n // 3] = np.inf, 30.0
        else:
            ranges[:] = 7.5
        _, rot = L.rotations(K)
        best, cost, used, stats = LC.check(slam, g, fields, 1.0, ranges, ct, st, rot, H, 20.0, cap, regions=regs)
        assert np.all(best[:, 0] >= 0) and np.all(used == used[0]) and 0 < used[0] <= n
        assert np.array_equal(stats[:, H], K * -(-regs[:, 2] // (1 << H)) * -(-regs[:, 3] // (1 << H)))
        # the whole map without a region table is the same call
        whole = slam.grid_locate_host(g, ranges, ct, st, rot, levels=H, max_range=20.0, cap=cap, return_stats=True)
        LC.same(whole, [w[:1] for w in (best, cost, used, stats)])


# ------------------------------------------------------------------ degenerate scans and maps
def test_empty_map_is_the_full_frontier(slam, ctx):
    xw, yw, cap, K = 70, 33, 9, 3
    g = slam.DeviceGrid(1, xw, yw, 1.0, 0.0, 0.0, context=ctx)
    fields = LC.fields_of(slam, g, cap)
    assert np.all(fields == cap)
    ct, st, ranges = L.ragged_scan(17, seed=3)
    _, rot = L.rotations(K)
    regs = np.array([(0, 0, xw, yw), (7, 5, 21, 13)], dtype=np.int32)
    for H in LEVELS:
        best, cost, used, stats = LC.check(slam, g, fields, 1.0, ranges, ct, st, rot, H, 30.0, cap, regions=regs)
        assert best.tolist() == [[0, 0, 0], [0, 7, 5]] and cost.tolist() == [17 * cap] * 2       # everything ties: flat 0
        for b, reg in enumerate(regs):
            assert stats[b].tolist() == [K * -(-reg[2] // (1 << h)) * -(-reg[3] // (1 << h)) for h in range(H + 1)] + [17 * cap]


def test_skipped_beams_off_beams_and_nan_rotations(slam, ctx):
    xw, yw, cap = 70, 33, 9
    g = LC.ragged_grid(slam, ctx, xw, yw)
    fields = LC.fields_of(slam, g, cap)
    ct, st, ranges = L.ragged_scan(17, seed=3)
    _, rot = L.rotations(3)
    reg = np.array([(7, 5, 21, 13)], dtype=np.int32)
    scan = ranges.copy()
    scan[3], scan[10], scan[11], scan[5] = np.inf, np.nan, 12.0, np.nextafter(np.float32(12.0), np.float32(0))
    for H in (0, 3, 8):
        _, _, used, _ = LC.check(slam, g, fields, 1.0, scan, ct, st, rot, H, 12.0, cap)
        assert used[0] == int(np.sum(scan < np.float32(12.0))) and scan[5] < 12.0 and 0 < used[0] < 15
        # every beam unused: (0, i0, j0), cost 0, used 0, stats of 0; no search
        for dead in (np.full(17, np.inf, np.float32), np.full(17, np.nan, np.float32), np.full(17, 12.0, np.float32)):
            best, cost, used, stats = LC.check(slam, g, fields, 1.0, dead, ct, st, rot, H, 12.0, cap, regions=reg)
            assert best.tolist() == [[0, 7, 5]] and cost[0] == 0 and used[0] == 0 and not stats.any()
    # a range of 3 000 km and NaN rotation entries: off beams add cap to every candidate
    far = ranges.copy()
    far[2] = far[11] = 3.0e6
    nanrot = np.array([[np.nan, 0.0], [np.cos(0.3), np.sin(0.3)], [1.0, np.nan]])
    for r, rc in ((far, rot), (ranges, nanrot), (far, nanrot)):
        for H in (0, 3, 8):
            best, cost, used, _ = LC.check(slam, g, fields, 1.0, r, ct, st, rc, H, 4.0e6, cap)
            assert used[0] == 17 and (rc is rot or best[0, 0] == 1)
    allnan = np.full((2, 2), np.nan)
    best, cost, used, stats = LC.check(slam, g, fields, 1.0, ranges, ct, st, allnan, 3, 30.0, cap, regions=reg)
    assert best.tolist() == [[0, 7, 5]] and cost[0] == 17 * cap and used[0] == 17


# ------------------------------------------------------------------ routing
def test_routing_over_three_maps(slam, ctx):
    g = slam.DeviceGrid(3, 64, 64, 1.0, 0.0, 0.0, context=ctx)
    rng = np.random.default_rng(9)
    LC.occupy(g, [R.ring(8) + R.ring(16), R.ring(12), [(int(x), int(y)) for x, y in rng.integers(8, 56, (30, 2))]])
    cap, H, K, n, B = 100, 3, 7, 24, 7
    fields = LC.fields_of(slam, g, cap)
    ct, st, _ = L.ragged_scan(n, seed=5)
    _, rot = L.rotations(K)
    gob = np.array([2, 0, 1, 1, 0, 2, 0], dtype=np.int32)
    regs = np.array([(0, 0, 64, 64), (10, 3, 33, 21), (0, 0, 64, 64), (5, 5, 7, 50), (63, 63, 1, 1), (1, 0, 63, 64), (0, 0, 64, 64)],
                    dtype=np.int32)
    per = rng.uniform(4.0, 18.0, (B, n)).astype(np.float32)
    for ranges in (per[0], per):
        own = ranges.ndim == 2
        call = lambda idx: slam.grid_locate_host(g, ranges[idx] if own else ranges, ct, st, rot, levels=H, region=regs[idx],
                                                 max_range=17.0, cap=cap, grid_of_batch=gob[idx], return_stats=True)
        want = L.locate_batch(fields, 1.0, ranges, ct, st, rot, H, 17.0, cap, maps=gob, regions=regs)
        LC.same(call(np.arange(B)), want)
        LC.same(call(np.arange(B)[::-1]), [w[::-1] for w in want])
        for b in range(B):
            LC.same(call(np.array([b])), [w[b:b + 1] for w in want])
    assert len({want[0][b].tobytes() + want[3][b].tobytes() for b in range(B)}) >= B - 1
    # entries -1 and G between good neighbours: -1 / -1 / 0 and stats of 0, the neighbours unaffected
    bad = gob.copy()
    bad[1], bad[4] = -1, 3
    got = LC.check(slam, g, fields, 1.0, per, ct, st, rot, H, 17.0, cap, maps=bad, regions=regs)
    for b in (1, 4):
        assert got[0][b].tolist() == [-1, -1, -1] and got[1][b] == -1 and got[2][b] == 0 and not got[3][b].any()
    for b in (0, 2, 3, 5, 6):
        assert all(np.array_equal(a[b], w[b]) for a, w in zip(got, want))


# ------------------------------------------------------------------ the room, from nothing, through every surface
def test_room_recovered_on_the_device(slam, ctx, room):
    import torch
    g, case = room
    best, cost, used, stats = case["loc_ref"]
    rot, ct, st = case["loc_rot"], case["cos_t"], case["sin_t"]
    want = (np.array([best], dtype=np.int32), np.array([cost], dtype=np.int32), np.array([used], dtype=np.int32), stats[None])
    got = slam.grid_locate_host(g, case["scan"], ct, st, rot, levels=L.ROOM_H, return_stats=True, **L.ROOM_ARGS)
    print("room on the device: best", got[0][0], "cost", got[1][0], "used", got[2][0], "stats", got[3][0].tolist())
    LC.same(got, want)
    pose = slam.locate_pose(got[0], g.scale, g.off_x, g.off_y, rot)[0]
    assert np.array_equal(pose, L.pose_of(best, 20.0, 10.0, 10.0, rot))
    err = pose - case["true"]
    assert abs(err[0]) <= 0.05 and abs(err[1]) <= 0.05 and abs((err[2] + np.pi) % (2 * np.pi) - np.pi) <= 2 * np.pi / 256
    assert int(got[3][0, :6].sum()) < 0.01 * 256 * 400 * 400
    # brute force through the same code on a rectangle around the answer: the same cell
    reg = np.array([[best[1] - 20, best[2] - 17, 45, 38]], dtype=np.int32)
    b0 = slam.grid_locate_host(g, case["scan"], ct, st, rot, levels=0, region=reg, return_stats=True, **L.ROOM_ARGS)
    assert b0[0][0].tolist() == list(best) and b0[1][0] == cost and b0[3][0].tolist() == [256 * 45 * 38, cost]
    # DeviceGrid.locate on torch tensors, no synchronise inside
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d = g.locate(up(case["scan"]), up(ct), up(st), up(rot), levels=L.ROOM_H, return_stats=True, **L.ROOM_ARGS)
    ctx.synchronize()
    assert d[0].dtype == torch.int32 and d[3].dtype == torch.int64
    LC.same([t.cpu().numpy() for t in d], want)
    # Mapping.locate_scan on a map built by update_scans, and MCL.init_global around its answer
    m = slam.Mapping.metric(400, 400, 0.05, context=ctx)
    m.update_scans(case["ranges"], R.AMIN, R.AMAX, case["poses"])
    p2, c2, u2 = m.locate_scan(case["scan"], R.AMIN, R.AMAX)
    assert np.array_equal(p2, pose) and (c2, u2) == (cost, used)
    p3, c3, u3 = m.locate_scan(case["scan"], R.AMIN, R.AMAX, n_rot=256, levels=3, region=reg[0])
    assert np.array_equal(p3, pose) and (c3, u3) == (cost, used)
    f = slam.MCL(m, 64, np.random.default_rng(3))
    p4, c4, u4 = f.init_global(case["scan"], R.AMIN, R.AMAX, (0.1, 0.1, 0.05))
    assert np.array_equal(p4, pose) and (c4, u4) == (cost, used)
    assert f.particles.shape == (64, 3) and np.all(np.abs(f.particles - pose) <= np.array([0.1, 0.1, 0.05])) and not f.acc.any()
    est, _ = f.update(case["scan"], R.AMIN, R.AMAX)
    assert np.all(np.abs(est[:2] - case["true"][:2]) < 0.15)   # inside the spread plus the cell
