"""slam_grid_match at the edges of its arguments: windows that leave the map, hypotheses that have no answer, the
shapes at which the launch changes (beams around one wave, one candidate, more candidates than one pass of a
workgroup, more workgroups than 65 535) and every argument the library rejects.  Against tests/match_ref.py with
array_equal, through the C ABI."""
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


@pytest.fixture(scope="module")
def ring(slam, ctx):
    """The 64 x 64 ring map (scale 1, offsets 0), its pmap read back and its field at cap 64 and 32767."""
    g = slam.DeviceGrid(1, 64, 64, 1.0, 0.0, 0.0, context=ctx)
    for ox, oy, cx, cy in R.ring_updates():
        g.update_host(ox, oy, cx, cy)
    pm = g.read()["pmap"]
    assert np.array_equal(pm, R.ring_pmap())
    return g, {cap: M.field(pm, cap)[None] for cap in (64, 32767)}


@pytest.fixture(scope="module")
def room(slam, ctx, syn):
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


def tables(n, lo=-3.0, hi=3.0):
    ang = np.linspace(lo, hi, n)
    return np.cos(ang), np.sin(ang)


def check(slam, g, fields, scale, off, ranges, centres, ct, st, rot, nx, ny, step, max_range, cap, maps=None):
    want = M.match_batch(fields, scale, off, off, ranges, centres, ct, st, rot, nx, ny, step, max_range, cap, maps=maps)
    got = slam.grid_match_host(g, ranges, centres, ct, st, rot, nx, ny, step, max_range=max_range, cap=cap, grid_of_batch=maps,
                               return_costs=True)
    same_match(got, want)
    return got


# ------------------------------------------------------------------ outside the map
def test_window_that_leaves_the_map(slam, ring):
    g, fields = ring
    ct, st = tables(12)
    ranges = np.full(12, 3.0, dtype=np.float32)
    rot = M.rotations(0.3, 2, 0.2)[1][None]
    # the window runs from x = 50.5 to x = 82.5 in steps of 4: beams of 3 cells, so from 70.5 on every end is off the map
    best, cost, used, costs = check(slam, g, fields[64], 1.0, 0.0, ranges, np.array([[66.5, 32.5]]), ct, st, rot, 4, 1, 4.0, 10.0, 64)
    assert used[0] == 12 and np.all(costs[0, :, 5:, :] == 12 * 64) and np.any(costs[0, :, :2, :] < 12 * 64)
    # a whole window off the map, on the negative side (int() truncates -0.5 to cell 0: keep well away)
    best, cost, used, costs = check(slam, g, fields[64], 1.0, 0.0, ranges, np.array([[-40.5, -40.5]]), ct, st, rot, 1, 1, 1.0, 10.0, 64)
    assert best[0] == 0 and cost[0] == 12 * 64 and np.all(costs == 12 * 64)
    # beams whose end is NaN / beyond 2^20 cells cost cap as well: a rotation table with a NaN, a huge range
    rot_nan = rot.copy()
    rot_nan[0, 1, 0] = np.nan
    check(slam, g, fields[64], 1.0, 0.0, ranges, np.array([[32.5, 32.5]]), ct, st, rot_nan, 1, 1, 1.0, 10.0, 64)
    far = ranges.copy()
    far[4] = 3.0e6
    check(slam, g, fields[64], 1.0, 0.0, far, np.array([[32.5, 32.5]]), ct, st, rot, 1, 1, 1.0, np.inf, 64)


def test_hypotheses_without_an_answer(slam, ctx):
    g = slam.DeviceGrid(2, 64, 64, 1.0, 0.0, 0.0, context=ctx)
    for ox, oy, cx, cy in R.ring_updates():
        g.update_host(ox, oy, cx, cy, grid_of_batch=[1])
    pm = np.stack([g.read(gi)["pmap"] for gi in range(2)])
    assert np.all(pm[0] == 50) and np.array_equal(pm[1], R.ring_pmap())
    fields = np.stack([M.field(p, 64) for p in pm])
    ct, st = tables(12)
    ranges = np.full(12, 8.0, dtype=np.float32)
    centres = np.array([[32.5, 32.5], [np.nan, 32.5], [32.5, 32.5], [32.5, np.inf], [33.5, 31.5], [2.0 ** 21, 32.5], [32.5, 32.5],
                        [31.5, 32.5]])
    maps = np.array([1, 1, -1, 1, 1, 1, 2, 0], dtype=np.int32)
    rot = np.repeat(M.rotations(0.0, 3, 0.1)[1][None], 8, axis=0)
    best, cost, used, costs = check(slam, g, fields, 1.0, 0.0, ranges, centres, ct, st, rot, 1, 1, 1.0, 30.0, 64, maps=maps)
    for b in (1, 2, 3, 5, 6):
        assert (best[b], cost[b], used[b]) == (-1, -1, 0) and np.all(costs[b] == -1)
    for b in (0, 4, 7):
        assert best[b] >= 0 and used[b] == 12 and np.all(costs[b] >= 0)
    assert cost[7] == 12 * 64                                   # map 0 is empty
    # the neighbours are what they are alone
    for b in (0, 4, 7):
        alone = slam.grid_match_host(g, ranges, centres[b:b + 1], ct, st, rot[b:b + 1], 1, 1, 1.0, cap=64, grid_of_batch=maps[b:b + 1],
                                     return_costs=True)
        same_match(alone, (best[b:b + 1], cost[b:b + 1], used[b:b + 1], costs[b:b + 1]))
    # used_out and cost_out are optional
    abi = pkg("_abi")
    b2, c2 = np.empty(8, np.int32), np.empty(8, np.int32)
    abi.check(abi.lib().slam_grid_match(ctx.handle, g._h, abi.ptr(ranges), 1, abi.ptr(centres), 8, abi.ptr(maps), abi.ptr(ct), abi.ptr(st),
                                        12, abi.ptr(rot), 3, 1, 1, 1.0, 30.0, 64, abi.ptr(b2), abi.ptr(c2), None, None))
    assert np.array_equal(b2, best) and np.array_equal(c2, cost)


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize("n", [1, 63, 65, 120])
def test_beam_counts(slam, room, n):
    g, case = room
    ct, st = tables(n, R.AMIN, R.AMAX)
    idx = np.round(np.linspace(0, 119, n)).astype(int)
    scan = case["scan"][idx].copy()
    rot = case["rot_cs"][None, 3:8]
    check(slam, g, case["field"][None], 20.0, 10.0, scan, case["start"][None, :2], ct, st, rot, 2, 1, 0.05, 30.0, 64)


def test_window_shapes(slam, room):
    g, case = room
    ct, st, fld = case["cos_t"], case["sin_t"], case["field"][None]
    ctr = case["start"][None, :2]
    # one candidate
    best, cost, used, costs = check(slam, g, fld, 20.0, 10.0, case["scan"], ctr, ct, st, case["rot_cs"][None, 5:6], 0, 0, 0.05, 30.0, 64)
    assert best[0] == 0 and costs.shape == (1, 1, 1, 1) and cost[0] == costs[0, 0, 0, 0] == case["ref"][3][5, 4, 4]
    # nx != ny, both ways, and a step that is no multiple of the cell
    check(slam, g, fld, 20.0, 10.0, case["scan"], ctr, ct, st, case["rot_cs"][None, :4], 5, 1, 0.05, 30.0, 64)
    check(slam, g, fld, 20.0, 10.0, case["scan"], ctr, ct, st, case["rot_cs"][None, 9:], 0, 6, 0.05, 30.0, 64)
    check(slam, g, fld, 20.0, 10.0, case["scan"], ctr, ct, st, case["rot_cs"][None, 2:5], 3, 3, 0.03, 30.0, 64)
    # K alone beyond one workgroup's rotations: 40 rotations of one translation
    rot = M.rotations(case["start"][2], 40, 0.004)[1][None]
    check(slam, g, fld, 20.0, 10.0, case["scan"], ctr, ct, st, rot, 0, 0, 0.05, 30.0, 64)


def test_more_candidates_than_one_pass(slam, ring):
    g, fields = ring
    ct, st = tables(16)
    ranges = np.linspace(5.0, 12.0, 16).astype(np.float32)
    rot = M.rotations(0.2, 3, 0.3)[1][None]
    # 3 x 81 x 81 = 19 683 candidates over the whole ring map and past its border; cap 32767: no cost is capped
    best, cost, used, costs = check(slam, g, fields[32767], 1.0, 0.0, ranges, np.array([[32.5, 32.5]]), ct, st, rot, 40, 40, 1.0, 30.0,
                                    32767)
    assert costs.shape == (1, 3, 81, 81) and used[0] == 16 and len(np.unique(costs)) > 1000


def test_more_groups_than_65535(slam, ring):
    g, fields = ring
    B, n, period = 70000, 8, 36
    ct, st = tables(n)
    ranges = np.linspace(6.0, 9.5, n).astype(np.float32)
    rng = np.random.default_rng(3)
    c0 = np.concatenate([32.5 + rng.uniform(-6.0, 6.0, (period - 2, 2)), [[np.nan, 1.0], [90.5, 32.5]]])
    r0 = np.stack([M.rotations(t, 1, 0.0)[1] for t in rng.uniform(-3.0, 3.0, period)])
    w = M.match_batch(fields[64], 1.0, 0.0, 0.0, ranges, c0, ct, st, r0, 0, 0, 1.0, 30.0, 64)
    assert len(np.unique(w[1])) > 10 and w[0][period - 2] == -1 and w[1][period - 1] == 8 * 64
    rep = np.arange(B) % period
    got = slam.grid_match_host(g, ranges, c0[rep], ct, st, r0[rep], 0, 0, 1.0, max_range=30.0, cap=64, return_costs=True)
    same_match(got, [x[rep] for x in w])


# ------------------------------------------------------------------ errors
def test_rejected_arguments_leave_the_context_usable(slam, ctx, ring):
    g, fields = ring
    ct, st = tables(8)
    ranges = np.full(8, 8.0, dtype=np.float32)
    ctr = np.array([[32.5, 32.5]])
    rot = M.rotations(0.0, 2, 0.1)[1][None]
    good = dict(nx=1, ny=1, step=1.0, max_range=30.0, cap=64)

    def call(ranges=ranges, ct=ct, st=st, rot=rot, **kw):
        a = dict(good, **kw)
        return slam.grid_match_host(g, ranges, ctr, ct, st, rot, a["nx"], a["ny"], a["step"], max_range=a["max_range"], cap=a["cap"],
                                    return_costs=True)

    want = M.match_batch(fields[64], 1.0, 0.0, 0.0, ranges, ctr, ct, st, rot, **good)
    same_match(call(), want)
    big_ct, big_st = tables(70000)
    bad = [dict(cap=0), dict(cap=32768), dict(cap=-3), dict(nx=-1), dict(ny=-2), dict(step=0.0), dict(step=np.nan), dict(step=-1.0),
           dict(step=np.inf), dict(max_range=0.0), dict(max_range=-1.0), dict(max_range=np.nan),
           dict(rot=np.zeros((1, 0, 2))),                                          # K = 0
           dict(nx=2047, ny=2048),                                                 # 2 x 4095 x 4097 candidates > 2^24
           dict(nx=1 << 30, ny=1 << 30), dict(nx=(1 << 31) - 1),
           dict(ranges=np.full(70000, 8.0, np.float32), ct=big_ct, st=big_st, cap=32767)]     # n * cap >= 2^31
    assert 70000 * 32767 >= 2 ** 31 and 2 * 4095 * 4097 > 2 ** 24
    for kw in bad:
        with pytest.raises(slam.SlamError):
            call(**kw)
        same_match(call(), want)                                   # the context and the grid still work
    for cap in (0, 32768):
        with pytest.raises(slam.SlamError):
            slam.grid_distance_field_host(g, cap)
        assert np.array_equal(slam.grid_distance_field_host(g, 64), fields[64])
    ctx.check_status()                                             # nothing raised the sticky status
    # the candidate count is what is named
    with pytest.raises(slam.SlamError, match="2\\^24"):
        call(rot=np.zeros((1, 3, 2)), nx=2047, ny=2047)            # 3 x 4095 x 4095 > 2^24
