"""The distance field of the grid and the window matcher on it (slam_grid_distance_field / slam_grid_match) against
the NumPy reference (tests/match_ref.py), through the C ABI.  Everything is integer: fields, whole cost volumes,
best index, best cost and used beams compare with array_equal; in every case the reference reads the pmap read back
from the device."""
import numpy as np
import pytest

import match_ref as M
import raycast_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu


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


def occupy(g, cells):
    """Occupied cells written straight into the hit counters (one hit occupies): cells[gi] = [(x, y), ...]."""
    import torch
    g._ctx.synchronize()       # a reset before this has run: torch copies on a stream of its own
    _, h = g.counters_torch()
    hit = np.zeros((g.G, g.xw, g.yw), dtype=np.int32)
    for gi, cs in enumerate(cells):
        for x, y in cs:
            hit[gi, x, y] = 1
    h.copy_(torch.from_numpy(hit).to(h.device))
    torch.cuda.synchronize()
    pm = np.stack([g.read(gi)["pmap"] for gi in range(g.G)])
    assert np.array_equal(pm == 100, hit == 1)
    return pm


def ring_grid(slam, ctx):
    g = slam.DeviceGrid(1, 64, 64, 1.0, 0.0, 0.0, context=ctx)
    for ox, oy, cx, cy in R.ring_updates():
        g.update_host(ox, oy, cx, cy)
    return g


@pytest.fixture(scope="module")
def room(slam, ctx, syn):
    """The room map on the device, the recovery case and the reference's answer (shared with the CPU tests)."""
    case = M.room_case(syn)
    abi = pkg("_abi")
    g = slam.DeviceGrid.metric(1, 400, 400, 0.05, context=ctx)
    abi.check(abi.lib().slam_grid_update_scans(ctx.handle, g._h, abi.ptr(case["ranges"]), abi.ptr(case["cos_t"]), abi.ptr(case["sin_t"]),
                                               abi.ptr(np.ascontiguousarray(case["poses"])), None, 6, 120))
    assert np.array_equal(g.read()["pmap"], case["pmap"])
    return g, case


def same_match(got, want):
    for a, b in zip(got, want):
        assert a.dtype == np.int32 and np.array_equal(a, b)


# ------------------------------------------------------------------ the field
def test_field_ring_at_three_caps(slam, ctx):
    g = ring_grid(slam, ctx)
    pm = g.read()["pmap"]
    assert np.array_equal(pm, R.ring_pmap())
    for cap in (1, 64, 32767):
        f = slam.grid_distance_field_host(g, cap)
        assert f.dtype == np.int16 and f.shape == (1, 64, 64) and np.array_equal(f[0], M.field(pm, cap)), cap
    assert f[0, 32, 32] == 64 and f[0, 0, 0] == 512


def test_field_empty_corners_and_edge(slam, ctx):
    g = slam.DeviceGrid(1, 48, 40, 1.0, 0.0, 0.0, context=ctx)
    for cap in (1, 64, 32767):
        assert np.all(slam.grid_distance_field_host(g, cap) == cap)
    pm = occupy(g, [[(0, 0), (0, 39), (47, 0), (47, 39)]])
    for cap in (64, 32767):
        assert np.array_equal(slam.grid_distance_field_host(g, cap)[0], M.field(pm[0], cap)), cap
    g.reset()
    pm = occupy(g, [[(x, 39) for x in range(48)]])
    for cap in (64, 32767):
        f = slam.grid_distance_field_host(g, cap)[0]
        assert np.array_equal(f, M.field(pm[0], cap)), cap
    assert np.array_equal(f[7], (39 - np.arange(40)) ** 2)


@pytest.mark.parametrize("xw,yw,lys", [(70, 33, (0, 31, 32)), (40, 70, (63, 64, 69))])
def test_field_rows_that_end_inside_a_mask_word(slam, ctx, xw, yw, lys):
    g = slam.DeviceGrid(1, xw, yw, 1.0, 0.0, 0.0, context=ctx)
    for cells in ([(5 + 9 * k, ly) for k, ly in enumerate(lys)], [(xw - 1, lys[0])], [(3, lys[1])], [(xw // 2, lys[2])]):
        g.reset()
        pm = occupy(g, [cells])
        for cap in (1, 64, 32767):
            assert np.array_equal(slam.grid_distance_field_host(g, cap)[0], M.field(pm[0], cap)), (cells, cap)


def test_field_three_maps_and_every_surface(slam, ctx):
    import torch
    g = slam.DeviceGrid(3, 37, 45, 1.0, 0.0, 0.0, context=ctx)
    rng = np.random.default_rng(5)
    cells = [[(int(x), int(y)) for x, y in zip(rng.integers(0, 37, k), rng.integers(0, 45, k))] for k in (1, 6, 40)]
    pm = occupy(g, cells)
    for cap in (64, 3000):
        want = np.stack([M.field(pm[gi], cap) for gi in range(3)])
        assert len({want[gi].tobytes() for gi in range(3)}) == 3
        assert np.array_equal(slam.grid_distance_field_host(g, cap), want)
        d = g.distance_field(cap)
        ctx.synchronize()
        assert d.dtype == torch.int16 and np.array_equal(d.cpu().numpy(), want)
        out = torch.full((3, 37, 45), -7, dtype=torch.int16, device=d.device)
        torch.cuda.synchronize()
        assert g.distance_field(cap, out=out) is out
        ctx.synchronize()
        assert np.array_equal(out.cpu().numpy(), want)
    # Mapping.distance_field: the ring map through the drop-in class
    m = slam.Mapping(64, 64, 1.0, index_scale=1.0, index_offset=0.0, context=ctx)
    assert np.all(m.distance_field() == 64) and np.all(m.distance_field(cap=7) == 7)
    for ox, oy, cx, cy in R.ring_updates():
        m.update(ox, oy, cx, cy)
    f = m.distance_field(cap=200)
    assert f.shape == (64, 64) and f.dtype == np.int16 and np.array_equal(f, M.field(m.pmap.astype(np.int8), 200))
    assert np.array_equal(f, slam.grid_distance_field_host(ring_grid(slam, ctx), 200)[0])


# ------------------------------------------------------------------ the room: a whole volume, and the pose recovered
def test_room_volume_and_pose(slam, ctx, room):
    g, case = room
    a = M.ROOM_ARGS
    assert np.array_equal(slam.grid_distance_field_host(g, a["cap"])[0], case["field"])
    best, cost, used, costs = case["ref"]
    got = slam.grid_match_host(g, case["scan"], case["start"][None, :2], case["cos_t"], case["sin_t"], case["rot_cs"][None],
                               a["nx"], a["ny"], a["step"], max_range=a["max_range"], cap=a["cap"], return_costs=True)
    same_match(got, (np.array([best]), np.array([cost]), np.array([used]), costs[None]))
    assert cost == 51 and np.count_nonzero(costs == 51) >= 2          # the tie of the issue: lowest flat index
    pose = slam.match_pose(case["start"][None, :2], case["thetas"][None], got[0], a["nx"], a["ny"], a["step"])[0]
    assert np.allclose(pose, [0.7988, -1.3422, 0.4351], atol=5e-5)
    # the drop-in class on a map built by update_scans: the same pose, cost and volume
    m = slam.Mapping.metric(400, 400, 0.05, context=ctx)
    m.update_scans(case["ranges"], R.AMIN, R.AMAX, case["poses"])
    assert np.array_equal(m.pmap.astype(np.int8), case["pmap"])
    p2, c2, u2, v2 = m.match_scan(case["scan"], R.AMIN, R.AMAX, case["start"], window=(4, 4), step=None, n_rot=M.ROOM_K,
                                  rot_step=M.ROOM_ROT_STEP, max_range=30.0, cap=64, return_costs=True)
    assert np.array_equal(p2, pose) and (c2, u2) == (cost, used) and np.array_equal(v2, costs)
    p3, c3, u3 = m.match_scan(case["scan"], R.AMIN, R.AMAX, case["start"])
    assert np.array_equal(p3, pose) and (c3, u3) == (cost, used)


# ------------------------------------------------------------------ ties and skipped beams
def test_ties_and_skipped_beams(slam, ctx, room):
    g, case = room
    ct, st, rot = case["cos_t"], case["sin_t"], case["rot_cs"][None, 4:7]
    ctr = case["start"][None, :2]
    kw = dict(nx=1, ny=2, step=0.05, max_range=4.0, cap=64)
    scan = case["scan"].copy()
    assert np.sum(scan < 4.0) > 20 and np.sum(scan > 4.0) > 5
    scan[3], scan[10], scan[11], scan[50] = np.inf, np.nan, 4.0, np.nextafter(np.float32(4.0), np.float32(0))
    want = M.match_batch(case["field"][None], 20.0, 10.0, 10.0, scan, ctr, ct, st, rot, **kw)
    got = slam.grid_match_host(g, scan, ctr, ct, st, rot, kw["nx"], kw["ny"], kw["step"], max_range=4.0, cap=64, return_costs=True)
    same_match(got, want)
    assert 0 < got[2][0] < 120 - 3
    # every beam skipped: cost 0 everywhere, best 0, used 0
    for dead in (np.full(120, np.inf, np.float32), np.full(120, np.nan, np.float32), np.full(120, 4.0, np.float32)):
        b, c, u, v = slam.grid_match_host(g, dead, ctr, ct, st, rot, 1, 2, 0.05, max_range=4.0, cap=64, return_costs=True)
        assert (b[0], c[0], u[0]) == (0, 0, 0) and np.all(v == 0) and v.shape == (1, 3, 3, 5)
    # an empty map: every candidate costs used * cap, the lowest index wins
    e = slam.DeviceGrid.metric(1, 400, 400, 0.05, context=ctx)
    b, c, u, v = slam.grid_match_host(e, case["scan"], ctr, ct, st, rot, 1, 2, 0.05, max_range=30.0, cap=9, return_costs=True)
    assert b[0] == 0 and u[0] > 0 and c[0] == 9 * u[0] and np.all(v == 9 * u[0])


# ------------------------------------------------------------------ routing
def test_routing_over_three_maps(slam, ctx, room):
    _, case = room
    g = slam.DeviceGrid(3, 64, 64, 1.0, 0.0, 0.0, context=ctx)
    rng = np.random.default_rng(9)
    pm = occupy(g, [R.ring(8) + R.ring(16), R.ring(12), [(int(x), int(y)) for x, y in rng.integers(8, 56, (30, 2))]])
    cap = 100
    fields = slam.grid_distance_field_host(g, cap)
    assert np.array_equal(fields, np.stack([M.field(p, cap) for p in pm]))
    n, K, B = 24, 3, 7
    ang = np.linspace(-3.0, 3.0, n)
    ct, st = np.cos(ang), np.sin(ang)
    gob = np.array([2, 0, 1, 1, 0, 2, 0], dtype=np.int32)
    centres = 32.5 + rng.uniform(-2.0, 2.0, (B, 2))
    rot = np.stack([M.rotations(t, K, 0.05)[1] for t in rng.uniform(-1.0, 1.0, B)])
    per = rng.uniform(6.0, 18.0, (B, n)).astype(np.float32)
    kw = dict(nx=2, ny=1, step=1.0, max_range=17.0, cap=cap)
    for ranges in (per[0], per):
        want = M.match_batch(fields, 1.0, 0.0, 0.0, ranges, centres, ct, st, rot, maps=gob, **kw)
        call = lambda idx: slam.grid_match_host(g, ranges if ranges.ndim == 1 else ranges[idx], centres[idx], ct, st, rot[idx], 2, 1, 1.0,
                                                max_range=17.0, cap=cap, grid_of_batch=gob[idx], return_costs=True)
        same_match(call(np.arange(B)), want)
        same_match(call(np.arange(B)[::-1]), [w[::-1] for w in want])
        for b in range(B):
            same_match(call(np.array([b])), [w[b:b + 1] for w in want])
    assert len({want[3][b].tobytes() for b in range(B)}) == B


# ------------------------------------------------------------------ the device form
def test_device_form_back_to_back(slam, ctx, room):
    import torch
    g, case = room
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ct, st = case["cos_t"], case["sin_t"]
    centres = case["start"][None, :2] + np.array([[0.0, 0.0], [0.1, -0.1], [np.nan, 0.0]])
    rot = np.repeat(case["rot_cs"][None], 3, axis=0)
    scans = np.stack([case["scan"], case["ranges"][-2], case["scan"]])
    h1 = slam.grid_match_host(g, scans, centres, ct, st, rot, 4, 4, 0.05, return_costs=True)
    h2 = slam.grid_match_host(g, case["scan"], centres[:2], ct, st, rot[:2, 2:5], 1, 3, 0.03, max_range=5.0, cap=20)
    assert h1[0][2] == -1 and h1[0][0] == case["ref"][0] and np.array_equal(h1[3][0], case["ref"][3])
    d = dict(cos_t=up(ct), sin_t=up(st))
    a1 = (up(scans), up(centres), up(rot))
    a2 = (up(case["scan"]), up(centres[:2]), up(rot[:2, 2:5]))
    best2 = torch.full((2,), -5, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    # two _dev calls back to back without a synchronise: the second rebuilds the field the first one reads
    o1 = g.match(a1[0], a1[1], rot_cs=a1[2], nx=4, ny=4, step=0.05, return_costs=True, **d)
    o2 = g.match(a2[0], a2[1], rot_cs=a2[2], nx=1, ny=3, step=0.03, max_range=5.0, cap=20, best_out=best2, **d)
    ctx.synchronize()
    assert o2[0] is best2 and len(o1) == 4 and len(o2) == 3
    same_match([t.cpu().numpy() for t in o1], h1)
    same_match([t.cpu().numpy() for t in o2], h2)
