"""slam_grid_frontiers at the edges of its arguments and its workspace: the label budget ("frontier_ws_mb") cut to one,
two and many queries a chunk, the query that fits no budget, one 2 000 x 2 000 map as a single query, every argument set
the library rejects - each followed by a good call - and the context: the device form back to back, a call enqueued
right behind an update, the counters before and after, the sticky status.  Against tests/frontier_ref.py with
array_equal, through the C ABI."""
import ctypes as C

import numpy as np
import pytest

import frontier_cases as FC
import frontier_ref as F
import raycast_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu

PATTERNS = FC.patterns()
KW = dict(radius=1, min_unknown=2, min_size=2, M=48)


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
def case(slam, ctx):
    """Three maps of 130 x 67 and seven queries routed over them, one of them without a map."""
    names = ["random_130x67_0.5", "spiral_a", "random_130x67_0.6"]
    g, pm = FC.grid_of(slam, ctx, np.stack([PATTERNS[n] for n in names]))
    maps = np.array([2, 0, 1, 1, -1, 0, 2], dtype=np.int32)
    return dict(g=g, pm=pm, maps=maps, want=F.frontiers_batch(pm, maps=maps, **KW))


def call(slam, c, **kw):
    a = dict(grid_of_batch=c["maps"], radius=KW["radius"], min_unknown=KW["min_unknown"], min_size=KW["min_size"],
             max_clusters=KW["M"], labels=True)
    a.update(kw)
    return slam.grid_frontiers_host(c["g"], **a)


def query(name, a=0, b=0, c=0):
    abi = pkg("_abi")
    out = C.c_int64()
    abi.check(abi.lib().slam_plan_query(name.encode(), int(a), int(b), int(c), -1, C.byref(out)))
    return int(out.value)


# ------------------------------------------------------------------ chunks
def test_chunks_change_nothing(slam, ctx, case):
    FC.same(call(slam, case), case["want"])                              # the default budget: one chunk
    qb = query("frontier_query_bytes", 130, 67)
    try:
        for per_chunk in (1, 2, 3, 6):                                   # 7, 4, 3 and 2 chunks
            kib = -(-per_chunk * (qb + 256) // 1024)
            assert query("frontier_chunk_queries", kib, qb, 7) == per_chunk
            ctx.set_option("frontier_ws_mb", kib / 1024.0)
            FC.same(call(slam, case), case["want"])
    finally:
        ctx.set_option("frontier_ws_mb", 256)


def test_a_query_over_the_budget_is_rejected(slam, ctx, case):
    qb = query("frontier_query_bytes", 130, 67)
    try:
        ctx.set_option("frontier_ws_mb", (qb - 1) / 1048576.0)
        with pytest.raises(slam.SlamError, match="frontier_ws_mb"):
            call(slam, case)
        ctx.set_option("frontier_ws_mb", qb / 1048576.0)
        FC.same(call(slam, case), case["want"])                          # exactly one query fits
    finally:
        ctx.set_option("frontier_ws_mb", 256)
    for v in (0, -1, float("nan"), 2 ** 20 + 1):
        with pytest.raises(slam.SlamError, match="frontier_ws_mb"):
            ctx.set_option("frontier_ws_mb", v)
    FC.same(call(slam, case), case["want"])


def test_one_map_of_2000_x_2000(slam, ctx, syn):
    """The room scaled onto 2 000 x 2 000 cells, a single query: 63 x 32 tiles, 3 907 segments."""
    ranges, poses, _ = R.room(syn)
    big = np.kron(R.room_pmap(ranges, poses), np.ones((5, 5), dtype=np.int8))
    g, pm = FC.grid_of(slam, ctx, big)
    for kw in (dict(radius=0, min_unknown=0, min_size=1, M=256), dict(radius=2, min_unknown=13, min_size=5, M=256)):
        count = FC.check(slam, g, pm, **kw)[0]
        assert count[0, 1] > 2000                                        # 985 clusters under the plain rule: beyond the table
    g.close()


# ------------------------------------------------------------------ rejected arguments
def test_every_rejected_argument_set_and_a_good_call_after_each(slam, ctx, case):
    abi = pkg("_abi")
    g, B, Mx = case["g"], 7, KW["M"]
    count, table, sums = np.empty((B, 2), np.int32), np.empty((B, Mx, 8), np.int32), np.empty((B, Mx, 2), np.int64)
    labels = np.empty((B, 130, 67), np.int32)
    base = dict(B=B, gob=case["maps"], radius=1, min_unknown=2, min_clear2=0, cap=64, min_size=2, M=Mx, count=count, table=table,
                sums=sums, labels=labels)

    def raw(**kw):
        a = dict(base)
        a.update(kw)
        return abi.lib().slam_grid_frontiers(ctx.handle, g._h, a["B"], abi.ptr(a["gob"]), a["radius"], a["min_unknown"], a["min_clear2"],
                                             a["cap"], a["min_size"], a["M"], abi.ptr(a["count"]), abi.ptr(a["table"]),
                                             abi.ptr(a["sums"]), abi.ptr(a["labels"]))

    assert raw() == 0
    FC.same((count, table, sums, labels), case["want"])
    bad = [dict(B=0), dict(B=-1), dict(radius=-1), dict(radius=9), dict(min_unknown=-1), dict(min_unknown=10), dict(radius=0, min_unknown=2),
           dict(min_clear2=-1), dict(min_clear2=1, cap=0), dict(min_clear2=1, cap=32768), dict(min_clear2=65, cap=64), dict(min_size=0),
           dict(min_size=-3), dict(M=-1), dict(M=65537), dict(count=None), dict(table=None), dict(sums=None),
           dict(gob=None),                                               # B = 7 > G = 3 without routing
           dict(B=1 << 16, M=1 << 15)]                                   # B * M >= 2^31
    for kw in bad:
        count[:], table[:], sums[:], labels[:] = -7, -7, -7, -7
        assert raw(**kw) == abi.ERR_INVALID, kw
        assert abi.lib().slam_last_error()
        assert np.all(count == -7) and np.all(table == -7) and np.all(labels == -7), kw
        assert raw() == 0, kw
        FC.same((count, table, sums, labels), case["want"])
    ctx.check_status()                                                   # the sticky status is untouched
    # what is NOT rejected: the limits themselves, labels absent, NULL tables with M = 0, cap ignored without a clearance
    assert raw(radius=8, min_unknown=289, labels=None) == 0 and raw(radius=0, min_unknown=1) == 0
    assert raw(M=0, table=None, sums=None) == 0 and raw(cap=0) == 0 and raw(cap=-5, min_clear2=0) == 0
    assert raw(min_clear2=64, cap=64) == 0 and raw(min_clear2=1, cap=32767) == 0 and raw(min_size=2 ** 31 - 1) == 0
    assert raw(B=3, gob=None) == 0
    FC.same(call(slam, case), case["want"])


# ------------------------------------------------------------------ the context
def test_device_form_back_to_back_behind_an_update_and_counters_untouched(slam, ctx, case, syn):
    import torch
    g = case["g"]
    dev = torch.device("cuda", 0)
    maps = torch.from_numpy(case["maps"]).to(dev)
    p, h = FC.counters(g)
    before = (p.clone(), h.clone())
    other = F.frontiers_batch(case["pm"], B=3, radius=0, min_unknown=0, min_size=1, M=16)
    torch.cuda.synchronize()
    # two _dev calls back to back without a synchronise: the second reuses the workspace of the first
    o1 = g.frontiers(maps, radius=KW["radius"], min_unknown=KW["min_unknown"], min_size=KW["min_size"], max_clusters=KW["M"], labels=True)
    o2 = g.frontiers(radius=0, min_unknown=0, min_size=1, max_clusters=16, labels=True)
    ctx.synchronize()
    FC.same(tuple(t.cpu().numpy() for t in o1), case["want"])
    FC.same(tuple(t.cpu().numpy() for t in o2), other)
    assert torch.equal(p, before[0]) and torch.equal(h, before[1])       # the call changes nothing in the grid
    ctx.check_status()
    # a call enqueued right behind an update sees it
    abi = pkg("_abi")
    rep = syn.make_replay(3, 120, seed=4)
    m = slam.DeviceGrid.metric(1, 400, 400, 0.05, context=ctx)
    ct, st = abi.trig_tables(R.AMIN, R.AMAX, 120)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).to(dev)
    d_r, d_c, d_s, d_p = up(rep.ranges, np.float32), up(ct, np.float64), up(st, np.float64), up(rep.poses_true, np.float64)
    torch.cuda.synchronize()
    empty = m.frontiers(radius=0, min_unknown=0, min_size=1, max_clusters=64)
    abi.check(abi.lib().slam_grid_update_scans_dev(ctx.handle, m._h, abi.ptr(d_r), abi.ptr(d_c), abi.ptr(d_s), abi.ptr(d_p), None, 3, 120))
    seen = m.frontiers(radius=0, min_unknown=0, min_size=1, max_clusters=64, labels=True)
    ctx.synchronize()
    assert empty[0].cpu().numpy().tolist() == [[0, 0]]
    pm = FC.pmaps_of(m)
    FC.same(tuple(t.cpu().numpy() for t in seen), F.frontiers_batch(pm, radius=0, min_unknown=0, min_size=1, M=64))
    assert seen[0][0, 1].item() > 1000
    ctx.check_status()
