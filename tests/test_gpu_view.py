"""The view gain on the GPU (slam_grid_view_gain) against the NumPy reference (tests/view_ref.py), with every
bit window in the workspace ("gain_lds" 0, the global engine) and in LDS wherever it fits (1), each on a context of
its own.  Counts and seen words are compared bit-equal; in every case the reference reads the pmap read back from the
device."""
import ctypes as C

import numpy as np
import pytest

import raycast_ref as R
import view_ref as V
from conftest import pkg
from test_gpu_raycast import ring_grid, same, three_maps

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


def up(a):
    import torch
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(torch.device("cuda", 0))      # (a copy: a reversed row of one keeps its negative stride)


def grid_of(slam, ctx, pmaps, scale=1.0, off_x=0.0, off_y=0.0):
    """A DeviceGrid whose maps finalize to ``pmaps``: their (pass, hit) counters written straight into the device arrays,
    and the pmaps read back checked."""
    import torch
    pmaps = [np.asarray(p) for p in pmaps]
    g = slam.DeviceGrid(len(pmaps), pmaps[0].shape[0], pmaps[0].shape[1], scale, off_x, off_y, context=ctx)
    ctx.synchronize()                                  # the new grid's reset is on the context's stream, the copies on torch's
    p, h = g.counters_torch()
    cnt = [V.counters_of(pm) for pm in pmaps]
    p.copy_(up(np.stack([c[0] for c in cnt])))
    h.copy_(up(np.stack([c[1] for c in cnt])))
    torch.cuda.synchronize()
    for i, pm in enumerate(pmaps):
        assert same(g.read(i)["pmap"], pm.astype(np.int8)), i
    return g


def check(got, want, what=""):
    """counts [B, 4] and seen [B, xw, wpr] bit-equal, with the first difference named."""
    (gc, gs), (wc, ws) = got, want
    assert gc.dtype == np.int32 and gs.dtype == np.uint32
    if not same(gc, wc):
        b = int(np.argwhere((gc != wc).any(axis=1))[0][0])
        raise AssertionError("%s: counts of view %d: %s against %s" % (what, b, gc[b], wc[b]))
    if not same(gs, ws):
        b, x, w = (int(v) for v in np.argwhere(gs != ws)[0])
        raise AssertionError("%s: seen word [%d][%d][%d]: %08x against %08x (%d words differ)" % (what, b, x, w, gs[b, x, w], ws[b, x, w], int((gs != ws).sum())))


def host(slam, g, poses, ct, st, max_range=1.0, skip=1, gob=None):
    return slam.grid_view_gain_host(g, poses, ct, st, max_range=max_range, skip=skip, grid_of_batch=gob, return_seen=True)


def dev(g, ctx, poses, ct, st, max_range=1.0, skip=1, gob=None):
    import torch
    d = [up(np.asarray(poses, dtype=np.float64).reshape(-1, 3)), up(np.asarray(ct, dtype=np.float64)), up(np.asarray(st, dtype=np.float64))]
    dg = None if gob is None else up(np.asarray(gob, dtype=np.int32))
    torch.cuda.synchronize()
    counts, seen = g.view_gain(*d, max_range=max_range, skip=skip, grid_of_batch=dg, return_seen=True)
    ctx.synchronize()
    return counts.cpu().numpy(), seen.cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------ 1. the three shared inputs
def test_ring_map(slam, ctx):
    g = ring_grid(slam, ctx)
    pm = g.read()["pmap"]
    assert same(pm, R.ring_pmap())
    for ends, skip in ((R.ring(24), 1), (R.ring(24), 0), (R.ring(6), 1)):
        ct, st = R.tables_to(ends)
        want = V.views([pm], 1.0, 0.0, 0.0, R.RING_POSE[None], ct, st, 1.0, skip)
        check(host(slam, g, R.RING_POSE[None], ct, st, skip=skip), want, "host")
        check(dev(g, ctx, R.RING_POSE[None], ct, st, skip=skip), want, "dev")
    counts = slam.grid_view_gain_host(g, R.RING_POSE[None], *R.tables_to(R.ring(24)), max_range=1.0)
    wrong = V.detail(pm, 1.0, 0.0, 0.0, R.RING_POSE, *R.tables_to(R.ring(24)), 1.0, walk_order=True)
    assert counts[0, V.OCCUPIED] == 64 and tuple(counts[0]) != tuple(wrong["counts"])
    ctx.check_status()


def test_gap_map_and_leaving_the_map(slam, ctx):
    g = grid_of(slam, ctx, [V.gap_pmap()])
    pm = g.read()["pmap"]
    unknown = []
    for r in (24, 31, 40):
        ct, st = R.tables_to(R.ring(r))
        want = V.views([pm], 1.0, 0.0, 0.0, R.RING_POSE[None], ct, st, 1.0)
        got = host(slam, g, R.RING_POSE[None], ct, st)
        check(got, want, "ring %d" % r)
        check(dev(g, ctx, R.RING_POSE[None], ct, st), want, "ring %d dev" % r)
        unknown.append(int(got[0][0, V.UNKNOWN]))
        assert got[0][0, V.OPEN] > 0
    assert 0 < unknown[0] < unknown[1] < unknown[2]
    ct, st = R.tables_to(R.ring(20, V.LEAVE_CELL), V.LEAVE_CELL)
    want = V.views([pm], 1.0, 0.0, 0.0, V.LEAVE_POSE[None], ct, st, 1.0)
    check(host(slam, g, V.LEAVE_POSE[None], ct, st), want, "leaving")
    check(dev(g, ctx, V.LEAVE_POSE[None], ct, st), want, "leaving dev")
    assert want[0][0, V.UNKNOWN] > 400 and want[0][0, V.OPEN] > 50
    ctx.check_status()


# ------------------------------------------------------------------ 2. the near-tie lines in all eight octants
def test_near_tie_octants(slam, ctx):
    g = ring_grid(slam, ctx)
    pm = g.read()["pmap"]
    ends = R.near_tie_ends()
    ct, st = R.tables_to(ends)
    want = V.views([pm], 1.0, 0.0, 0.0, R.RING_POSE[None], ct, st, 1.0)
    check(host(slam, g, R.RING_POSE[None], ct, st), want, "sixteen beams")
    for i in range(len(ends)):                          # and each line alone: a seen set is that line's cells
        want = V.views([pm], 1.0, 0.0, 0.0, R.RING_POSE[None], ct[i:i + 1], st[i:i + 1], 1.0)
        check(host(slam, g, R.RING_POSE[None], ct[i:i + 1], st[i:i + 1]), want, "line %d" % i)
    ctx.check_status()


# ------------------------------------------------------------------ 3. skip
def test_skip(slam, ctx):
    g = ring_grid(slam, ctx, extra=[(np.array([32.5]), np.array([32.5]), 20.5, 20.5)])     # a hit on the origin cell
    pm = g.read()["pmap"]
    assert pm[32, 32] == 100
    ct, st = R.tables_to(R.ring(24))
    for skip in (0, 1, 3, 25):                          # Lp = 25 for every one of these rays
        want = V.views([pm], 1.0, 0.0, 0.0, R.RING_POSE[None], ct, st, 1.0, skip)
        got = host(slam, g, R.RING_POSE[None], ct, st, skip=skip)
        check(got, want, "skip %d" % skip)
        check(dev(g, ctx, R.RING_POSE[None], ct, st, skip=skip), want, "skip %d dev" % skip)
    assert tuple(got[0][0]) == (0, 0, 0, 192) and not got[1].any()         # skip = Lp: nothing seen, nothing found
    ctx.check_status()


# ------------------------------------------------------------------ 4. routing
GOB = np.array([2, 0, 2, 2, 0], dtype=np.int32)       # neither monotone nor covering: map 1 is read by nobody


def routed(slam, ctx):
    g = three_maps(slam, ctx)
    pms = [g.read(i)["pmap"] for i in range(3)]
    poses = np.array([[32.5, 32.5, 0.0], [30.5, 35.5, 0.3], [20.5, 20.5, 1.0], [32.5, 32.5, 2.0], [45.5, 12.5, -1.0]])
    ct, st = R.tables_to(R.ring(24))
    return g, pms, poses, ct, st


def test_routing_and_batch_invariance(slam, ctx):
    g, pms, poses, ct, st = routed(slam, ctx)
    want = V.views(pms, 1.0, 0.0, 0.0, poses, ct, st, 1.0, gob=GOB)
    assert len({tuple(c) for c in want[0]}) == 5       # five different answers
    check(host(slam, g, poses, ct, st, gob=GOB), want, "batch")
    check(dev(g, ctx, poses, ct, st, gob=GOB), want, "batch dev")
    perm = np.array([3, 0, 4, 2, 1])
    check(host(slam, g, poses[perm], ct, st, gob=GOB[perm]), (want[0][perm], want[1][perm]), "permuted")
    for b in range(5):
        check(host(slam, g, poses[b:b + 1], ct, st, gob=GOB[b:b + 1]), (want[0][b:b + 1], want[1][b:b + 1]), "alone %d" % b)
    # no grid_of_batch: every view reads map 0
    check(host(slam, g, poses, ct, st), V.views(pms, 1.0, 0.0, 0.0, poses, ct, st, 1.0), "map 0")
    ctx.check_status()


def test_bad_map_entry_in_both_forms(slam, ctx):
    g, pms, poses, ct, st = routed(slam, ctx)
    for bad in (3, -1):
        gob = GOB.copy()
        gob[1] = bad
        with pytest.raises(slam.SlamError, match="grid_of_batch"):
            host(slam, g, poses, ct, st, gob=gob)
        want = V.views(pms, 1.0, 0.0, 0.0, poses, ct, st, 1.0, gob=gob)
        assert np.all(want[0][1] == -1) and not want[1][1].any()
        check(dev(g, ctx, poses, ct, st, gob=gob), want, "entry %d" % bad)
    ctx.check_status()                                  # a bad entry does not raise the sticky status


def test_bad_poses_leave_the_status_clean(slam, ctx):
    g = ring_grid(slam, ctx)
    pm = g.read()["pmap"]
    ct, st = R.tables_to(R.ring(24))
    poses = np.array([[np.nan, 32.5, 0.0], [32.5, 32.5, 0.0], [float(2 ** 20), 32.5, 0.0], [32.5, np.inf, 0.0], [32.5, 32.5, np.nan],
                      [float(2 ** 20) - 1.0, 32.5, 0.0]])
    want = V.views([pm], 1.0, 0.0, 0.0, poses, ct, st, 1.0)
    assert [bool(np.all(c == -1)) for c in want[0]] == [True, False, True, True, True, False]
    check(host(slam, g, poses, ct, st), want, "host")
    check(dev(g, ctx, poses, ct, st), want, "dev")
    # beams whose END the index rule rejects are skipped, not counted as open
    far = host(slam, g, R.RING_POSE[None], [1.0, 0.0, -1.0], [0.0, 1.0, 0.0], max_range=float(2 ** 21))
    check(far, V.views([pm], 1.0, 0.0, 0.0, R.RING_POSE[None], [1.0, 0.0, -1.0], [0.0, 1.0, 0.0], float(2 ** 21)), "far ends")
    assert tuple(far[0][0]) == (0, 0, 0, 0)
    ctx.check_status()


# ------------------------------------------------------------------ 5. bounds of the call
def test_beam_count_bounds(slam, ctx):
    g = ring_grid(slam, ctx)
    pm = g.read()["pmap"]
    want = V.views([pm], 1.0, 0.0, 0.0, R.RING_POSE[None], [24.0], [7.0], 1.0)
    check(host(slam, g, R.RING_POSE[None], [24.0], [7.0]), want, "n = 1")
    ends = (R.ring(24) * 22)[:4096]
    ct, st = R.tables_to(ends)
    got = host(slam, g, R.RING_POSE[None], ct, st)
    want = V.views([pm], 1.0, 0.0, 0.0, R.RING_POSE[None], *R.tables_to(R.ring(24)), 1.0)
    assert same(got[1], want[1]) and same(got[0][0, :3], want[0][0, :3])         # the same set from 4 096 beams
    counts = np.full((1, 4), 77, dtype=np.int32)
    seen = np.full((1, 64, 2), 0x5a5a5a5a, dtype=np.uint32)
    abi = pkg("_abi")
    ct1, st1 = R.tables_to((R.ring(24) * 22)[:4097])
    pose = np.ascontiguousarray(R.RING_POSE[None])
    call = lambda n, mr, skip, B=1: abi.lib().slam_grid_view_gain(ctx.handle, g._h, abi.ptr(pose), B, None, abi.ptr(ct1), abi.ptr(st1), n, mr, skip,
                                                                   abi.ptr(counts), abi.ptr(seen))
    for args in ((4097, 1.0, 1), (0, 1.0, 1), (4, 0.0, 1), (4, float("inf"), 1), (4, float("nan"), 1), (4, 1.0, -1), (4, 1.0, 2 ** 20 + 1), (4, 1.0, 1, 0)):
        assert call(*args) == abi.ERR_INVALID, args
        assert np.all(counts == 77) and np.all(seen == 0x5a5a5a5a), args           # outputs untouched
    assert call(4, 1.0, 2 ** 20) == abi.SLAM_OK
    ctx.check_status()


def test_seen_is_optional_and_outputs_end_where_they_should(slam, ctx):
    g, pms, poses, ct, st = routed(slam, ctx)
    want = V.views(pms, 1.0, 0.0, 0.0, poses, ct, st, 1.0, gob=GOB)
    only = slam.grid_view_gain_host(g, poses, ct, st, max_range=1.0, grid_of_batch=GOB)
    assert same(only, want[0])
    # guard words behind both host outputs
    abi = pkg("_abi")
    counts = np.full(5 * 4 + 16, 0x7b7b7b7b, dtype=np.int32)
    seen = np.full(5 * 64 * 2 + 16, 0xa5a5a5a5, dtype=np.uint32)
    p = np.ascontiguousarray(poses)
    abi.check(abi.lib().slam_grid_view_gain(ctx.handle, g._h, abi.ptr(p), 5, abi.ptr(GOB), abi.ptr(ct), abi.ptr(st), len(ct), 1.0, 1,
                                            abi.ptr(counts), abi.ptr(seen)))
    assert same(counts[:20].reshape(5, 4), want[0]) and np.all(counts[20:] == 0x7b7b7b7b)
    assert same(seen[:640].reshape(5, 64, 2), want[1]) and np.all(seen[640:] == 0xa5a5a5a5)
    ctx.check_status()


# ------------------------------------------------------------------ 6. the device form on the stream
def test_back_to_back_into_given_tensors_and_an_update_between(slam, ctx):
    import torch
    g = ring_grid(slam, ctx)
    pm0 = g.read()["pmap"]
    ct, st = R.tables_to(R.ring(24))
    poses = np.array([[32.5, 32.5, 0.0], [30.5, 35.5, 0.3]])
    dp, dct, dst = up(poses), up(ct), up(st)
    c1 = torch.full((2, 4), 99, dtype=torch.int32, device=dp.device)
    c2, c3 = c1.clone(), c1.clone()
    s1 = torch.full((2, 64, 2), 0x55555555, dtype=torch.int32, device=dp.device)
    s2 = s1.clone()
    torch.cuda.synchronize()
    before = (g.read(want=("pass", "hit", "pmap")), g.visits())
    out1 = g.view_gain(dp, dct, dst, max_range=1.0, counts_out=c1, seen_out=s1)
    out2 = g.view_gain(dp, dct, dst, max_range=1.0, skip=0, counts_out=c2, seen_out=s2)
    assert out1[0] is c1 and out1[1] is s1 and out2[0] is c2
    ctx.synchronize()
    check((c1.cpu().numpy(), s1.cpu().numpy().view(np.uint32)), V.views([pm0], 1.0, 0.0, 0.0, poses, ct, st, 1.0, 1), "first")
    check((c2.cpu().numpy(), s2.cpu().numpy().view(np.uint32)), V.views([pm0], 1.0, 0.0, 0.0, poses, ct, st, 1.0, 0), "second")
    # the call changes nothing in the grid
    after = (g.read(want=("pass", "hit", "pmap")), g.visits())
    assert before[1] == after[1] and all(same(before[0][k], after[0][k]) for k in ("pass", "hit", "pmap"))
    # an update enqueued between two calls is seen by the second: a wall of hits inside the inner ring
    wall = [(36, y) for y in range(28, 37)]
    g.update_host(np.array([x + 0.5 for x, _ in wall]), np.array([y + 0.5 for _, y in wall]), 32.5, 32.5)
    g.view_gain(dp, dct, dst, max_range=1.0, counts_out=c3)
    ctx.synchronize()
    pm1 = g.read()["pmap"]
    assert not same(pm0, pm1)
    want = V.views([pm1], 1.0, 0.0, 0.0, poses, ct, st, 1.0)
    assert same(c3.cpu().numpy(), want[0]) and not same(want[0], c1.cpu().numpy())
    ctx.check_status()


# ------------------------------------------------------------------ 7. against the cast
def test_the_cast_sees_the_occupied_cells_of_the_view(slam, ctx):
    g = grid_of(slam, ctx, [V.gap_pmap()])
    pm = g.read()["pmap"]
    poses = np.array([[32.5, 32.5, 0.0], [36.5, 30.5, 0.7], [3.5, 60.5, 0.0]])
    ct, st = R.tables_to(R.ring(31))
    counts, seen = host(slam, g, poses, ct, st)
    ranges, cells = slam.grid_raycast_host(g, poses, ct, st, max_range=1.0, return_cells=True)
    for b in range(3):
        hit = {(int(x), int(y)) for x, y in cells[b] if x >= 0}
        occ = {c for c in V.cells_of(seen[b], 64) if pm[c] == 100}
        assert hit == occ and len(hit) == counts[b, V.OCCUPIED], b
        assert int(np.isinf(ranges[b]).sum()) == counts[b, V.OPEN], b
    ctx.check_status()


# ------------------------------------------------------------------ 8. a real map, and the Mapping method
def test_room(slam, ctx, syn):
    ranges, poses, hyp = R.room(syn)
    abi = pkg("_abi")
    ct, st = abi.trig_tables(R.AMIN, R.AMAX, 120)
    g = slam.DeviceGrid.metric(1, 400, 400, 0.05, context=ctx)
    abi.check(abi.lib().slam_grid_update_scans(ctx.handle, g._h, abi.ptr(ranges), abi.ptr(ct), abi.ptr(st),
                                               abi.ptr(np.ascontiguousarray(poses)), None, 6, 120))
    pm = g.read()["pmap"]
    want = V.views([pm], 20.0, 10.0, 10.0, hyp, ct, st, 30.0)
    print("room counts per view (unknown free occupied open):\n", want[0])
    assert np.all(want[0][4] == -1) and want[0][0, V.UNKNOWN] > 0 and want[0][3, V.OCCUPIED] > 0
    check(host(slam, g, hyp, ct, st, max_range=30.0), want, "room")
    check(dev(g, ctx, hyp, ct, st, max_range=30.0), want, "room dev")
    ctx.check_status()


def test_mapping_view_gain(slam, ctx):
    m = slam.Mapping(64, 64, 1.0, index_scale=1.0, index_offset=0.0, context=ctx)
    for ox, oy, cx, cy in R.ring_updates():
        m.update(ox, oy, cx, cy)
    pmm = m.pmap.astype(np.int8)
    ct, st = pkg("_abi").trig_tables(R.AMIN, R.AMAX, 90)
    counts, seen = m.view_gain(R.RING_POSE, R.AMIN, R.AMAX, 90, max_range=30.0, return_seen=True)
    wc, ws = V.view(pmm, 1.0, 0.0, 0.0, R.RING_POSE, ct, st, 30.0)
    assert same(counts, wc) and same(seen, ws) and counts.shape == (4,)
    two = m.view_gain(np.stack([R.RING_POSE, [20.5, 20.5, 0.5]]), R.AMIN, R.AMAX, 90)
    assert two.shape == (2, 4) and same(two[0], wc) and same(two[1], V.view(pmm, 1.0, 0.0, 0.0, [20.5, 20.5, 0.5], ct, st, 30.0)[0])
    assert same(m.pmap.astype(np.int8), pmm)
