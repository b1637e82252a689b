"""Rays traced through a map on the GPU (slam_grid_raycast / slam_grid_scan_score) against the NumPy reference
(tests/raycast_ref.py), with the mask words read from global memory ("raycast_lds" 0) and from LDS (1), each on a
context of its own.  Cells, classes and counts bit-equal, ranges equal as float32; in every case the reference
reads the pmap read back from the device."""
import ctypes as C

import numpy as np
import pytest

import raycast_ref as R
from conftest import pkg
from oracle import oracle_np as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def slam():
    p = pkg()
    p._abi.default_context()   # fails loudly when there is no gfx950 device
    return p


@pytest.fixture(scope="module", params=[0, 1], ids=["direct", "staged"])
def ctx(request, slam):
    c = slam.Context(0)
    c.set_option("raycast_lds", request.param)
    yield c
    c.close()


def ring_grid(slam, ctx, extra=()):
    g = slam.DeviceGrid(1, 64, 64, 1.0, 0.0, 0.0, context=ctx)
    for ox, oy, cx, cy in list(R.ring_updates()) + list(extra):
        g.update_host(ox, oy, cx, cy)
    return g


def same(a, b):
    """equal as bits of their type (NaN == NaN, inf == inf)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def ref_raycast(pm, scale, ox, oy, poses, ct, st, max_range, skip=1):
    out = [R.raycast(pm, scale, ox, oy, p, ct, st, max_range, skip) for p in poses]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


# ------------------------------------------------------------------ 1. all directions
def test_all_directions(slam, ctx):
    g = ring_grid(slam, ctx)
    pm = g.read()["pmap"]
    assert same(pm, R.ring_pmap())
    for ends in (R.ring(24), R.near_tie_ends()):
        ct, st = R.tables_to(ends)
        r, cells = slam.grid_raycast_host(g, R.RING_POSE[None], ct, st, max_range=1.0, return_cells=True)
        rr, rc = ref_raycast(pm, 1.0, 0.0, 0.0, R.RING_POSE[None], ct, st, 1.0)
        assert same(cells, rc) and same(r, rr)
        assert np.all(np.max(np.abs(cells[0] - 32), axis=1) == 8)     # every first hit lies on the inner ring


# ------------------------------------------------------------------ 2. early exit on flagged rays
def test_flagged_rays_keep_path_order(slam, ctx):
    g = ring_grid(slam, ctx)
    pm = g.read()["pmap"]
    for r, want in ((24, R.BLOCKED), (8, R.HIT), (16, R.BLOCKED)):
        ends = R.ring(r)
        ct, st = R.tables_to(ends)
        ranges = np.ones(len(ends), dtype=np.float32)
        counts, cls = slam.grid_score_host(g, ranges, R.RING_POSE[None], ct, st, return_classes=True)
        rcounts, rcls = R.score(pm, 1.0, 0.0, 0.0, R.RING_POSE, R.table_points(ranges, ct, st))
        assert same(cls[0], rcls) and same(counts[0], rcounts)
        assert np.all(cls == want) and counts[0, want] == 8 * r


# ------------------------------------------------------------------ 3. skip
def test_skip(slam, ctx):
    # a hit on the origin cell (32, 32), put there by a ray that ends in it
    g = ring_grid(slam, ctx, extra=[(np.array([32.5]), np.array([32.5]), 20.5, 20.5)])
    pm = g.read()["pmap"]
    assert pm[32, 32] == 100
    ends = R.ring(24)
    ct, st = R.tables_to(ends)
    for skip, radius in ((0, 0), (1, 8), (3, 8), (9, 16), (25, None)):        # Lp = 25 for every one of these rays
        r, cells = slam.grid_raycast_host(g, R.RING_POSE[None], ct, st, max_range=1.0, skip=skip, return_cells=True)
        rr, rc = ref_raycast(pm, 1.0, 0.0, 0.0, R.RING_POSE[None], ct, st, 1.0, skip)
        assert same(cells, rc) and same(r, rr), skip
        if radius is None:
            assert np.all(np.isinf(r)) and np.all(cells == -1)
        else:
            assert np.all(np.max(np.abs(cells[0] - 32), axis=1) == radius), skip
    # one cell from the wall at x = 40, skip past it
    pose = np.array([[39.5, 32.5, 0.0]])
    for skip in (1, 2):
        r, cells = slam.grid_raycast_host(g, pose, [20.0], [0.0], max_range=1.0, skip=skip, return_cells=True)
        rr, rc = ref_raycast(pm, 1.0, 0.0, 0.0, pose, [20.0], [0.0], 1.0, skip)
        assert same(cells, rc) and same(r, rr)
        assert tuple(cells[0, 0]) == ((40, 32) if skip == 1 else (48, 32))
    # the end cell is the origin cell: EMPTY
    counts, cls = slam.grid_score_host(g, np.zeros(3, dtype=np.float32), R.RING_POSE[None], np.ones(3), np.zeros(3), return_classes=True)
    assert np.all(cls == R.EMPTY) and counts[0, R.EMPTY] == 3 and counts.sum() == 3
    # the Mapping methods: one pose, linspace tables
    m = slam.Mapping(64, 64, 1.0, index_scale=1.0, index_offset=0.0, context=ctx)
    for ox, oy, cx, cy in R.ring_updates():
        m.update(ox, oy, cx, cy)
    abi = pkg("_abi")
    ct, st = abi.trig_tables(R.AMIN, R.AMAX, 90)
    pmm = m.pmap.astype(np.int8)
    r, cells = m.raycast(R.RING_POSE, R.AMIN, R.AMAX, 90, max_range=30.0, return_cells=True)
    rr, rc = R.raycast(pmm, 1.0, 0.0, 0.0, R.RING_POSE, ct, st, 30.0)
    assert same(r, rr) and same(cells, rc) and np.all(np.isfinite(r))
    scan = np.full(90, 8.0, dtype=np.float32)
    assert same(m.score_scan(scan, R.AMIN, R.AMAX, R.RING_POSE), R.score(pmm, 1.0, 0.0, 0.0, R.RING_POSE, R.table_points(scan, ct, st))[0])


# ------------------------------------------------------------------ 4. a real map
def test_room(slam, ctx, syn):
    ranges, poses, hyp = R.room(syn)
    abi = pkg("_abi")
    ct, st = abi.trig_tables(R.AMIN, R.AMAX, 120)
    g = slam.DeviceGrid.metric(1, 400, 400, 0.05, context=ctx)
    abi.check(abi.lib().slam_grid_update_scans(ctx.handle, g._h, abi.ptr(ranges), abi.ptr(ct), abi.ptr(st),
                                               abi.ptr(np.ascontiguousarray(poses)), None, 6, 120))
    pm = g.read()["pmap"]
    assert same(pm, R.room_pmap(ranges, poses))
    counts, cls = slam.grid_score_host(g, ranges[-1], hyp, ct, st, return_classes=True)
    pc = O.laser_to_numpy(ranges[-1], R.AMIN, R.AMAX, clip_inf=True)
    ref = [R.score(pm, 20.0, 10.0, 10.0, h, pc) for h in hyp]
    assert same(counts, np.stack([c for c, _ in ref])) and same(cls, np.stack([k for _, k in ref]))
    assert np.all(counts[0, R.HIT] > counts[1:, R.HIT])
    # per-hypothesis ranges instead of the shared scan: the same answer
    counts2 = slam.grid_score_host(g, np.tile(ranges[-1], (5, 1)), hyp, ct, st)
    assert same(counts2, counts)
    r, cells = slam.grid_raycast_host(g, hyp, ct, st, max_range=30.0, return_cells=True)
    rr, rc = ref_raycast(pm, 20.0, 10.0, 10.0, hyp, ct, st, 30.0)
    assert same(cells, rc) and same(r, rr)
    assert np.all(np.isnan(r[4])) and np.isfinite(r[3]).sum() > 0


# ------------------------------------------------------------------ 5. bounds and routing
def three_maps(slam, ctx):
    g = slam.DeviceGrid(3, 64, 64, 1.0, 0.0, 0.0, context=ctx)
    ups = R.ring_updates()
    g.update_host(np.stack([ups[0][0][:60], ups[1][0][:60], ups[1][0][60:120]]), np.stack([ups[0][1][:60], ups[1][1][:60], ups[1][1][60:120]]),
                  [32.5] * 3, [32.5] * 3, grid_of_batch=[0, 1, 2])
    return g


def test_routing(slam, ctx):
    g = three_maps(slam, ctx)
    pms = [g.read(k)["pmap"] for k in range(3)]
    ends = R.ring(24)[::3]
    ct, st = R.tables_to(ends)
    gob = np.array([2, 0, 0, 2, 2, 0, 2], dtype=np.int32)             # neither monotone nor covering
    poses = np.array([[32.5, 32.5, 0.0], [30.5, 33.5, 0.0], [32.5, 32.5, 0.0], [34.5, 31.5, 0.0], [32.5, 32.5, 0.0],
                      [20.5, 40.5, 0.0], [32.5, 30.5, 0.0]])
    scan = np.linspace(0.2, 1.0, len(ends)).astype(np.float32)
    r, cells = slam.grid_raycast_host(g, poses, ct, st, max_range=1.0, grid_of_batch=gob, return_cells=True)
    counts, cls = slam.grid_score_host(g, scan, poses, ct, st, grid_of_batch=gob, return_classes=True)
    for b in range(len(gob)):
        r1, c1 = slam.grid_raycast_host(g, poses[b:b + 1], ct, st, max_range=1.0, grid_of_batch=gob[b:b + 1], return_cells=True)
        n1, k1 = slam.grid_score_host(g, scan, poses[b:b + 1], ct, st, grid_of_batch=gob[b:b + 1], return_classes=True)
        assert same(r[b], r1[0]) and same(cells[b], c1[0]) and same(counts[b], n1[0]) and same(cls[b], k1[0]), b
        rr, rc = R.raycast(pms[gob[b]], 1.0, 0.0, 0.0, poses[b], ct, st, 1.0)
        assert same(r[b], rr) and same(cells[b], rc), b
        assert same(counts[b], R.score(pms[gob[b]], 1.0, 0.0, 0.0, poses[b], R.table_points(scan, ct, st))[0]), b
    # a permuted batch: the same rows
    perm = np.array([3, 6, 0, 5, 1, 4, 2])
    assert same(slam.grid_score_host(g, scan, poses[perm], ct, st, grid_of_batch=gob[perm]), counts[perm])
    # a bad entry: the host form rejects it, the device form gives that hypothesis BAD / NaN rows
    bad = gob.copy()
    bad[3] = 3
    with pytest.raises(slam.SlamError, match="grid_of_batch"):
        slam.grid_score_host(g, scan, poses, ct, st, grid_of_batch=bad)
    with pytest.raises(slam.SlamError, match="grid_of_batch"):
        slam.grid_raycast_host(g, poses, ct, st, grid_of_batch=bad)
    import torch
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    torch.cuda.synchronize()
    d = dict(poses=up(poses), cos_t=up(ct), sin_t=up(st), grid_of_batch=up(bad))
    # two _dev calls back to back without a synchronise, into caller-given outputs
    counts_d = torch.full((len(gob), 7), -5, dtype=torch.int32, device=dev)
    cls_d = torch.full((len(gob), len(ends)), -5, dtype=torch.int8, device=dev)
    torch.cuda.synchronize()
    out = g.score(up(scan), counts_out=counts_d, class_out=cls_d, **d)
    r_d, cells_d = g.raycast(max_range=1.0, return_cells=True, **d)
    ctx.synchronize()
    assert out[0] is counts_d and out[1] is cls_d
    want_counts, want_cls = counts.copy(), cls.copy()
    want_counts[3], want_cls[3] = [0, 0, 0, 0, 0, 0, len(ends)], R.BAD
    assert same(counts_d.cpu().numpy(), want_counts) and same(cls_d.cpu().numpy(), want_cls)
    want_r, want_c = r.copy(), cells.copy()
    want_r[3], want_c[3] = np.nan, -1
    assert same(r_d.cpu().numpy(), want_r) and same(cells_d.cpu().numpy(), want_c)
    ctx.check_status()                                                 # the sticky status is left untouched


def test_more_hypotheses_than_a_grid_dimension(slam, ctx):
    g = ring_grid(slam, ctx)
    five = np.array([[32.5, 32.5, 0.0], [30.5, 33.5, 0.3], [12.5, 50.5, 1.0], [40.5, 40.5, -2.0], [np.inf, 1.0, 0.0]])
    ct, st = pkg("_abi").trig_tables(R.AMIN, R.AMAX, 8)
    B = 70000
    poses = five[np.arange(B) % 5]
    scan = np.array([3.0, 8.0, 9.5, 20.0, np.inf, 0.0, 11.5, 16.0], dtype=np.float32)
    r5, c5 = slam.grid_raycast_host(g, five, ct, st, max_range=40.0, return_cells=True)
    n5, k5 = slam.grid_score_host(g, scan, five, ct, st, return_classes=True)
    pm = g.read()["pmap"]
    rr, rc = ref_raycast(pm, 1.0, 0.0, 0.0, five, ct, st, 40.0)
    assert same(r5, rr) and same(c5, rc)
    assert same(n5, np.stack([R.score(pm, 1.0, 0.0, 0.0, p, R.table_points(scan, ct, st))[0] for p in five]))
    r, cells = slam.grid_raycast_host(g, poses, ct, st, max_range=40.0, return_cells=True)
    counts, cls = slam.grid_score_host(g, scan, poses, ct, st, return_classes=True)
    idx = np.arange(B) % 5                                             # equal poses give equal rows, past row 65 535 too
    assert same(r, r5[idx]) and same(cells, c5[idx]) and same(counts, n5[idx]) and same(cls, k5[idx])


def test_beam_count_bounds(slam, ctx):
    g = ring_grid(slam, ctx)
    pm = g.read()["pmap"]
    pose = np.array([[31.5, 33.5, 0.4]])
    for n in (1, 4096):
        ct, st = pkg("_abi").trig_tables(R.AMIN, R.AMAX, n)
        r, cells = slam.grid_raycast_host(g, pose, ct, st, max_range=25.0, return_cells=True)
        rr, rc = ref_raycast(pm, 1.0, 0.0, 0.0, pose, ct, st, 25.0)
        assert same(r, rr) and same(cells, rc), n
        scan = np.linspace(0.0, 30.0, n).astype(np.float32)
        assert same(slam.grid_score_host(g, scan, pose, ct, st)[0], R.score(pm, 1.0, 0.0, 0.0, pose[0], R.table_points(scan, ct, st))[0]), n
    ct, st = pkg("_abi").trig_tables(R.AMIN, R.AMAX, 4097)
    with pytest.raises(slam.SlamError, match="4096"):
        slam.grid_raycast_host(g, pose, ct, st)
    with pytest.raises(slam.SlamError, match="4096"):
        slam.grid_score_host(g, np.ones(4097, dtype=np.float32), pose, ct, st)
    ct, st = np.ones(4), np.zeros(4)
    for kw in (dict(skip=-1), dict(skip=2 ** 20 + 1), dict(max_range=0.0), dict(max_range=np.inf)):
        with pytest.raises(slam.SlamError):
            slam.grid_raycast_host(g, pose, ct, st, **kw)
    with pytest.raises(slam.SlamError, match="B < 1"):
        slam.grid_raycast_host(g, np.zeros((0, 3)), ct, st)
    # B * n = 2^31: rejected before anything is read or written (the buffers here are far too small for it)
    abi, big = pkg("_abi"), pkg("_abi").trig_tables(R.AMIN, R.AMAX, 4096)
    out = np.full(16, 7.0, dtype=np.float32)
    assert abi.lib().slam_grid_raycast(ctx.handle, g._h, abi.ptr(pose), 2 ** 19, None, abi.ptr(big[0]), abi.ptr(big[1]), 4096,
                                       C.c_float(30.0), 1, abi.ptr(out), None) == abi.ERR_INVALID
    assert b"2^31" in abi.lib().slam_last_error() and np.all(out == 7.0)
    # a cell index that reaches 2^20: NaN / BAD, and the context's status stays clean
    r, cells = slam.grid_raycast_host(g, R.RING_POSE[None], ct, st, max_range=float(2 ** 20), return_cells=True)
    assert np.all(np.isnan(r)) and np.all(cells == -1)
    counts = slam.grid_score_host(g, np.full(4, 2.0 ** 20, dtype=np.float32), R.RING_POSE[None], ct, st)
    assert counts[0, R.BAD] == 4 and counts.sum() == 4
    ctx.check_status()


def test_a_map_too_large_for_lds(slam, ctx):
    """2 000 x 2 000: 504 KB of mask - the staged engine does not apply under option 1 and the call still returns
    the reference's bits."""
    g = slam.DeviceGrid(1, 2000, 2000, 1.0, 0.0, 0.0, context=ctx)
    rng = np.random.default_rng(3)
    ox, oy = rng.uniform(5, 1995, 400), rng.uniform(5, 1995, 400)
    g.update_host(ox, oy, 1000.5, 1000.5)
    pm = g.read()["pmap"]
    poses = np.array([[1000.5, 1000.5, 0.0], [300.5, 1700.5, 2.0], [-50.5, 1000.5, 0.0]])
    ct, st = pkg("_abi").trig_tables(R.AMIN, R.AMAX, 24)
    r, cells = slam.grid_raycast_host(g, poses, ct, st, max_range=1500.0, return_cells=True)
    rr, rc = ref_raycast(pm, 1.0, 0.0, 0.0, poses, ct, st, 1500.0)
    assert same(r, rr) and same(cells, rc)
    scan = rng.uniform(0.0, 1200.0, 24).astype(np.float32)
    counts, cls = slam.grid_score_host(g, scan, poses, ct, st, return_classes=True)
    ref = [R.score(pm, 1.0, 0.0, 0.0, p, R.table_points(scan, ct, st)) for p in poses]
    assert same(counts, np.stack([c for c, _ in ref])) and same(cls, np.stack([k for _, k in ref]))


def test_guard_bytes_behind_every_host_output(slam, ctx):
    g = ring_grid(slam, ctx)
    L, abi = pkg("_abi").lib(), pkg("_abi")
    B, n = 3, 37
    ct, st = abi.trig_tables(R.AMIN, R.AMAX, n)
    poses = np.ascontiguousarray(np.array([[32.5, 32.5, 0.1], [33.5, 30.5, 0.0], [10.5, 10.5, 1.0]]))
    scan = np.full(n, 9.0, dtype=np.float32)

    def guarded(count, dtype):
        return np.full(count * np.dtype(dtype).itemsize + 64, 0x5A, dtype=np.uint8)

    r, cells = guarded(B * n, np.float32), guarded(B * n * 2, np.int32)
    counts, cls = guarded(B * 7, np.int32), guarded(B * n, np.int8)
    abi.check(L.slam_grid_raycast(ctx.handle, g._h, abi.ptr(poses), B, None, abi.ptr(ct), abi.ptr(st), n, C.c_float(30.0), 1,
                                  abi.ptr(r), abi.ptr(cells)))
    abi.check(L.slam_grid_scan_score(ctx.handle, g._h, abi.ptr(scan), 1, abi.ptr(poses), B, None, abi.ptr(ct), abi.ptr(st), n, 1,
                                     abi.ptr(counts), abi.ptr(cls)))
    for buf in (r, cells, counts, cls):
        assert np.all(buf[-64:] == 0x5A)
    want_r, want_c = slam.grid_raycast_host(g, poses, ct, st, return_cells=True)
    want_n, want_k = slam.grid_score_host(g, scan, poses, ct, st, return_classes=True)
    assert r[:-64].tobytes() == want_r.tobytes() and cells[:-64].tobytes() == want_c.tobytes()
    assert counts[:-64].tobytes() == want_n.tobytes() and cls[:-64].tobytes() == want_k.tobytes()
    # a rejected call leaves its outputs untouched
    before = r.copy()
    assert L.slam_grid_raycast(ctx.handle, g._h, abi.ptr(poses), B, None, abi.ptr(ct), abi.ptr(st), n, C.c_float(30.0), -1,
                               abi.ptr(r), abi.ptr(cells)) == abi.ERR_INVALID
    assert np.array_equal(r, before)


def test_second_call_sees_an_update(slam, ctx):
    g = slam.DeviceGrid(1, 64, 64, 1.0, 0.0, 0.0, context=ctx)
    g.live_pmap()                                                     # with a live pmap the update below leaves it stale
    ox, oy, cx, cy = R.ring_updates()[1]
    g.update_host(ox, oy, cx, cy)
    ends = R.ring(24)
    ct, st = R.tables_to(ends)
    r1, c1 = slam.grid_raycast_host(g, R.RING_POSE[None], ct, st, max_range=1.0, return_cells=True)
    assert np.all(np.max(np.abs(c1[0] - 32), axis=1) == 16)
    ox, oy, cx, cy = R.ring_updates()[0]
    g.update_host(ox, oy, cx, cy)
    r2, c2 = slam.grid_raycast_host(g, R.RING_POSE[None], ct, st, max_range=1.0, return_cells=True)
    assert np.all(np.max(np.abs(c2[0] - 32), axis=1) == 8)
    pm = g.read()["pmap"]
    rr, rc = ref_raycast(pm, 1.0, 0.0, 0.0, R.RING_POSE[None], ct, st, 1.0)
    assert same(r2, rr) and same(c2, rc)


# ------------------------------------------------------------------ 6. the map is not disturbed
def test_the_map_is_not_disturbed(slam, ctx, g2):
    g = ring_grid(slam, ctx)
    before, visits = g.read(want=("pass", "hit", "pmap")), g.visits()
    ct, st = R.tables_to(R.ring(24))
    slam.grid_raycast_host(g, R.RING_POSE[None], ct, st, max_range=1.0)
    slam.grid_score_host(g, np.ones(192, dtype=np.float32), R.RING_POSE[None], ct, st)
    after = g.read(want=("pass", "hit", "pmap"))
    for k in ("pass", "hit", "pmap"):
        assert same(before[k], after[k]), k
    assert g.visits() == visits
    # Mapping.update of g2 with ray casts in between still ends on g2's pmap
    m = slam.Mapping(200, 200, 0.1, context=ctx)
    for i in range(10):
        c = g2["demo120_c"][i]
        p = m.update(g2["demo120_ox"][i], g2["demo120_oy"][i], c[0], c[1])
        r = m.raycast([c[0], c[1], 0.1 * i], R.AMIN, R.AMAX, 120)
        assert r.shape == (120,) and not np.any(np.isnan(r))
        m.score_scan(np.full(120, 3.0, dtype=np.float32), R.AMIN, R.AMAX, [c[0], c[1], 0.0])
        assert np.array_equal(p.astype(np.int8), g2["demo120_pmap_steps"][i]), i
    assert np.array_equal(m._fetch_pmap().astype(np.int8), g2["demo120_pmap_steps"][9])
