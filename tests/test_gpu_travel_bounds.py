"""slam_grid_travel at the edges of its arguments and its workspace: batches routed, alone, reversed and with entries that
name no map; NULL routing; the budget ("travel_ws_mb") cut to one, two and three queries a chunk and the query that fits
no budget; every argument set the library rejects - each followed by a good call - and the context: the device form back
to back, a call enqueued right behind an update, the counters before and after, the sticky status; the routed batch under a
clearance - whole, in chunks, with its costs in the workspace and in the device form around a call without one; more
queries than a launch has workgroups, so that the kernels take their grid-stride loops; and the map whose costs
could overflow.  Against tests/travel_ref.py with array_equal, through the C ABI."""
import ctypes as C

import numpy as np
import pytest

import frontier_cases as FC
import match_ref as M
import raycast_ref as R
import travel_cases as TC
import travel_ref as T
from conftest import pkg

pytestmark = pytest.mark.gpu

PATTERNS = FC.patterns()
KW = dict(foot=1, through_unknown=False, path_cap=6)
SHAPE = (130, 67)


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
    """Three maps of 130 x 67 and seven queries routed over them, -1 and G among the entries."""
    names = ["random_130x67_0.6", "spiral_a", "comb_a"]
    g, pm = FC.grid_of(slam, ctx, np.stack([PATTERNS[n] for n in names]))
    maps = np.array([2, 0, 1, 1, -1, 3, 0], dtype=np.int32)
    rng = np.random.default_rng(11)
    src = np.stack([rng.integers(0, SHAPE, (2, 2)) for _ in maps]).astype(np.int32)
    src[2, 0] = src[3, 1] = (0, 0)
    goals = np.stack([rng.integers(-2, (132, 69), (5, 2)) for _ in maps]).astype(np.int32)
    goals[:, 0] = src[:, 0]
    want = T.batch(pm, src, maps=maps, goals=goals, **KW)
    return dict(g=g, pm=pm, maps=maps, src=src, goals=goals, want=want)


def call(slam, c, **kw):
    a = dict(grid_of_batch=c["maps"], goals=c["goals"], dirs=True, **KW)
    a.update(kw)
    return slam.grid_travel_host(c["g"], c["src"], **a)


def query(name, a=0, b=0, c=0):
    abi = pkg("_abi")
    out = C.c_int64()
    abi.check(abi.lib().slam_plan_query(name.encode(), int(a), int(b), int(c), -1, C.byref(out)))
    return int(out.value)


# ------------------------------------------------------------------ batches
def test_batches_routed_alone_reversed_and_entries_without_a_map(slam, ctx, case):
    batch = call(slam, case)
    TC.same(batch, case["want"])
    assert batch["status"].tolist() == [0, 0, 0, 0, -1, -1, 0]
    for b in (4, 5):                                                     # every output of such a query is -1, the lengths 0
        assert np.all(batch["cost"][b] == -1) and np.all(batch["dir"][b] == -1) and np.all(batch["goal_cost"][b] == -1)
        assert np.all(batch["path_len"][b] == 0) and np.all(batch["path"][b] == -1)
    rev = slam.grid_travel_host(case["g"], case["src"][::-1].copy(), grid_of_batch=case["maps"][::-1].copy(), goals=case["goals"][::-1].copy(),
                                dirs=True, **KW)
    TC.same({k: v[::-1] for k, v in rev.items()}, batch)
    for b, gi in enumerate(case["maps"]):
        alone = slam.grid_travel_host(case["g"], case["src"][b:b + 1], grid_of_batch=[gi], goals=case["goals"][b:b + 1], dirs=True, **KW)
        TC.same(alone, {k: v[b:b + 1] for k, v in batch.items()}, tag=b)
    null = slam.grid_travel_host(case["g"], case["src"][[1, 2, 0]], goals=case["goals"][[1, 2, 0]], dirs=True, **KW)   # NULL routing: B = G
    TC.same(null, {k: v[[1, 2, 0]] for k, v in batch.items()})
    TC.same(slam.grid_travel_host(case["g"], case["src"][[1, 2]], goals=case["goals"][[1, 2]], dirs=True, **KW),      # B = 2 < G
            {k: v[[1, 2]] for k, v in batch.items()})
    with pytest.raises(slam.SlamError, match="B > G"):
        slam.grid_travel_host(case["g"], case["src"][:4])                # B = G + 1
    TC.same(call(slam, case), case["want"])
    ctx.check_status()


# ------------------------------------------------------------------ chunks
@pytest.mark.parametrize("own", (0, 1), ids=("in_cost_out", "in_the_workspace"))
def test_chunks_change_nothing(slam, ctx, case, own):
    kw = dict(cost=not own)
    want = {k: v for k, v in case["want"].items() if own == 0 or k != "cost"}
    TC.same(call(slam, case, **kw), want)                                # the default budget: one chunk
    qb = query("travel_query_bytes", *SHAPE, own)
    try:
        for per_chunk in (1, 2, 3):                                      # 7, 4 and 3 chunks
            kib = -(-per_chunk * (qb + 256) // 1024)
            assert query("travel_chunk_queries", kib, qb, 7) == per_chunk
            ctx.set_option("travel_ws_mb", kib / 1024.0)
            TC.same(call(slam, case, **kw), want)
    finally:
        ctx.set_option("travel_ws_mb", 256)


def test_a_query_over_the_budget_is_rejected(slam, ctx, case):
    qb = query("travel_query_bytes", *SHAPE, 0)
    try:
        ctx.set_option("travel_ws_mb", (qb - 1) / 1048576.0)
        with pytest.raises(slam.SlamError, match="travel_ws_mb"):
            call(slam, case)
        ctx.set_option("travel_ws_mb", qb / 1048576.0)
        TC.same(call(slam, case), case["want"])                          # exactly one query fits
        with pytest.raises(slam.SlamError, match="travel_ws_mb"):
            call(slam, case, cost=False)                                 # its costs in the workspace: it no longer does
    finally:
        ctx.set_option("travel_ws_mb", 256)
    for v in (0, -1, float("nan"), 2 ** 20 + 1):
        with pytest.raises(slam.SlamError, match="travel_ws_mb"):
            ctx.set_option("travel_ws_mb", v)
    TC.same(call(slam, case), case["want"])


# ------------------------------------------------------------------ rejected arguments
def test_every_rejected_argument_set_and_a_good_call_after_each(slam, ctx, case):
    abi = pkg("_abi")
    g, B, Q, P = case["g"], 7, 5, KW["path_cap"]
    out = dict(status=np.empty(B, np.int32), cost=np.empty((B,) + SHAPE, np.int32), dir=np.empty((B,) + SHAPE, np.int8),
               goal_cost=np.empty((B, Q), np.int32), path_len=np.empty((B, Q), np.int32), path=np.empty((B, Q, P, 2), np.int32))
    base = dict(B=B, gob=case["maps"], src=case["src"], S=2, foot=KW["foot"], through=0, min_clear2=0, cap=64, goals=case["goals"], Q=Q,
                path_cap=P, **out)

    def raw(**kw):
        a = dict(base)
        a.update(kw)
        return abi.lib().slam_grid_travel(ctx.handle, g._h, a["B"], abi.ptr(a["gob"]), abi.ptr(a["src"]), a["S"], a["foot"], a["through"],
                                          a["min_clear2"], a["cap"], abi.ptr(a["goals"]), a["Q"], a["path_cap"], abi.ptr(a["status"]),
                                          abi.ptr(a["cost"]), abi.ptr(a["dir"]), abi.ptr(a["goal_cost"]), abi.ptr(a["path_len"]),
                                          abi.ptr(a["path"]))

    assert raw() == 0
    TC.same(out, case["want"])
    bad = [dict(B=0), dict(B=-1), dict(S=0), dict(S=65), dict(foot=-1), dict(foot=9), dict(min_clear2=-1), dict(min_clear2=1, cap=0),
           dict(min_clear2=1, cap=32768), dict(min_clear2=65, cap=64), dict(Q=-1), dict(Q=65537), dict(path_cap=-1),
           dict(path_cap=130 * 67 + 1), dict(status=None), dict(src=None), dict(goal_cost=None), dict(path_len=None), dict(path=None),
           dict(cost=None, dir=None, goals=None), dict(cost=None, dir=None, Q=0),     # no output asked for
           dict(gob=None),                                               # B = 7 > G = 3 without routing
           dict(B=1 << 16, Q=1 << 15, path_cap=1)]                       # B * Q * path_cap >= 2^31
    for kw in bad:
        for v in out.values():
            v[:] = -7
        assert raw(**kw) == abi.ERR_INVALID, kw
        assert abi.lib().slam_last_error()
        assert all(np.all(v == -7) for v in out.values()), kw
        assert raw() == 0, kw
        TC.same(out, case["want"])
    ctx.check_status()                                                   # the sticky status is untouched
    # what is NOT rejected: the limits themselves, outputs absent, cap ignored without a clearance, goals without paths
    assert raw(foot=8) == 0 and raw(cap=0) == 0 and raw(cap=-5, min_clear2=0) == 0 and raw(min_clear2=64, cap=64) == 0
    assert raw(min_clear2=1, cap=32767) == 0 and raw(cost=None) == 0 and raw(dir=None) == 0 and raw(cost=None, dir=None) == 0
    assert raw(goals=None, goal_cost=None, path_len=None, path=None) == 0 and raw(Q=0, goal_cost=None, path_len=None, path=None) == 0
    assert raw(path_cap=0, path=None) == 0 and raw(B=3, gob=None) == 0
    wide = np.zeros((B, 64, 2), np.int32)
    assert raw(src=wide, S=64) == 0
    TC.same(call(slam, case), case["want"])


# ------------------------------------------------------------------ the context
def test_device_form_back_to_back_behind_an_update_and_counters_untouched(slam, ctx, case, syn):
    import torch
    g = case["g"]
    dev = torch.device("cuda", 0)
    up = lambda a, dt=np.int32: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).to(dev)
    maps, src, goals = up(case["maps"]), up(case["src"]), up(case["goals"])
    p, h = FC.counters(g)
    before = (p.clone(), h.clone())
    src2 = np.array([[[0, 0]], [[5, 5]], [[129, 66]]], dtype=np.int32)
    d_src2 = up(src2)
    other = T.batch(case["pm"], src2, through_unknown=True)
    torch.cuda.synchronize()
    # two _dev calls back to back without a synchronise: the second reuses the workspace of the first
    o1 = g.travel(src, maps, goals=goals, dirs=True, **KW)
    o2 = g.travel(d_src2, through_unknown=True, dirs=True)
    ctx.synchronize()
    TC.same({k: v.cpu().numpy() for k, v in o1.items()}, case["want"])
    TC.same({k: v.cpu().numpy() for k, v in o2.items()}, other)
    assert torch.equal(p, before[0]) and torch.equal(h, before[1])       # the call changes nothing in the grid
    ctx.check_status()
    # a call enqueued right behind an update sees it
    abi = pkg("_abi")
    rep = syn.make_replay(3, 120, seed=4)
    m = slam.DeviceGrid.metric(1, 400, 400, 0.05, context=ctx)
    ct, st = abi.trig_tables(R.AMIN, R.AMAX, 120)
    d_r, d_c, d_s, d_p = up(rep.ranges, np.float32), up(ct, np.float64), up(st, np.float64), up(rep.poses_true, np.float64)
    pose = np.asarray(rep.poses_true, dtype=np.float64)[2]
    cell = np.array([[[int(m.scale * (pose[0] + m.off_x)), int(m.scale * (pose[1] + m.off_y))]]], dtype=np.int32)
    d_cell = up(cell)
    torch.cuda.synchronize()
    empty = m.travel(d_cell)
    abi.check(abi.lib().slam_grid_update_scans_dev(ctx.handle, m._h, abi.ptr(d_r), abi.ptr(d_c), abi.ptr(d_s), abi.ptr(d_p), None, 3, 120))
    seen = m.travel(d_cell, foot=1, dirs=True)
    ctx.synchronize()
    assert (empty["cost"].cpu().numpy() >= 0).sum() == 1                  # nothing is known: the robot's own cell alone
    pm = FC.pmaps_of(m)
    TC.same({k: v.cpu().numpy() for k, v in seen.items()}, T.batch(pm, cell, foot=1))
    assert (seen["cost"] >= 0).sum().item() > 1000
    ctx.check_status()
    m.close()


# ------------------------------------------------------------------ routing, chunks and the workspace with a clearance
CLEAR_CAP = 16


@pytest.fixture(scope="module")
def cleared(slam, case):
    """The module's case under min_clear2 = 1 and 4: the fields of the three maps read back, and the restatement on them."""
    fields = np.stack([M.field(p, CLEAR_CAP) for p in case["pm"]])
    assert np.array_equal(slam.grid_distance_field_host(case["g"], CLEAR_CAP), fields)
    want = {c2: T.batch(case["pm"], case["src"], maps=case["maps"], fields=fields, goals=case["goals"], min_clear2=c2, **KW) for c2 in (1, 4)}
    return dict(fields=fields, want=want)


@pytest.mark.parametrize("c2", (1, 4))
def test_clearance_routed_in_chunks_in_the_workspace_and_back_to_back(slam, ctx, case, cleared, c2):
    import torch
    pm, maps, fields, want = case["pm"], case["maps"], cleared["fields"], cleared["want"][c2]
    # the field must be the MAP's, not the query's: under map b's field some routed query would see another T
    other = [b for b, gi in enumerate(maps) if 0 <= gi < 3 and b < 3 and gi != b
             and not np.array_equal(T.traversable(pm[gi], fields[gi], case["src"][b], KW["foot"], False, c2),
                                    T.traversable(pm[gi], fields[b], case["src"][b], KW["foot"], False, c2))]
    assert other, "the maps' fields do not tell routing by query from routing by map"
    assert (c2 == 1) == np.array_equal(want["cost"], case["want"]["cost"])   # 1 closes no free cell under its own map's field, 4 does
    kw = dict(min_clear2=c2, cap=CLEAR_CAP)
    got = call(slam, case, **kw)
    TC.same(got, want)
    assert got["status"].tolist() == [0, 0, 0, 0, -1, -1, 0]
    no_cost = {k: v for k, v in want.items() if k != "cost"}
    TC.same(call(slam, case, cost=False, **kw), no_cost)                  # the costs in the workspace, beside the field
    try:
        for own in (0, 1):
            qb = query("travel_query_bytes", *SHAPE, own)
            for per_chunk in (1, 2, 3):
                kib = -(-per_chunk * (qb + 256) // 1024)
                assert query("travel_chunk_queries", kib, qb, 7) == per_chunk
                ctx.set_option("travel_ws_mb", kib / 1024.0)
                TC.same(call(slam, case, cost=not own, **kw), no_cost if own else want)
    finally:
        ctx.set_option("travel_ws_mb", 256)
    # the device form twice, a call WITHOUT a clearance and with its costs in the workspace in between: the field is
    # rebuilt and the arena carved at another layout, all three enqueued without a synchronise
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    d_maps, d_src, d_goals = up(maps), up(case["src"]), up(case["goals"])
    torch.cuda.synchronize()
    o1 = case["g"].travel(d_src, d_maps, goals=d_goals, dirs=True, **kw, **KW)
    o2 = case["g"].travel(d_src, d_maps, goals=d_goals, dirs=True, cost=False, **KW)
    o3 = case["g"].travel(d_src, d_maps, goals=d_goals, dirs=True, **kw, **KW)
    ctx.synchronize()
    host = lambda o: {k: v.cpu().numpy() for k, v in o.items()}
    TC.same(host(o1), want)
    TC.same(host(o2), {k: v for k, v in case["want"].items() if k != "cost"})
    TC.same(host(o3), want)
    ctx.check_status()


# ------------------------------------------------------------------ past the block cap
def pocket_room():
    """17 x 16, free, with a wall that closes the rows behind it off, a stub of a wall and a few unknown cells."""
    pm = np.zeros((17, 16), dtype=np.int8)
    pm[10, :] = 100
    pm[0:6, 5] = 100
    pm[3:5, 9:12] = 50
    pm[13, 2:7] = 50
    return pm


def test_more_queries_than_the_block_cap_in_one_chunk(slam, ctx):
    """B = kTravelMaxBlocks + 3 queries in ONE chunk: k_travel_classes and k_travel_relax take their grid-stride loops, and
    with 272 cells a query k_travel_finish does at 256 cells a block (k_travel_paths, a lane per goal at 256 a block, would
    need 2^28 goals in a chunk; here it only runs past 2^21 rows).  The queries cycle through 7
    combinations of (map, sources, goals), one of them without a map; 7 does not divide the cap, so a workgroup's second
    query differs from its first.  Compared on the device, combination by combination."""
    import torch
    if torch.cuda.mem_get_info(0)[0] < 6 << 30:
        pytest.skip("needs 6 GB of free device memory")
    cap = query("kTravelMaxBlocks")
    B, K, S, Q, P = cap + 3, 7, 2, 2, 4
    assert cap % K != 0 and B * 17 * 16 > 256 * cap
    g, pm = FC.grid_of(slam, ctx, np.stack([FC.random_map((17, 16), 0.8, 23), pocket_room()]))
    free = np.argwhere(T.answer(pm[0], None, [[0, 0]], foot=1)["cost"] > 0)       # what (0, 0) reaches on the random map
    cmaps = np.array([0, 1, -1, 1, 0, 1, 0], dtype=np.int32)
    csrc = np.array([[[0, 0], [16, 15]], [[2, 2], [2, 2]], [[1, 1], [3, 3]], [[14, 3], [20, 3]], [free[3], free[-2]], [[9, 9], [11, 9]],
                     [[16, 0], [0, 15]]], dtype=np.int32)
    cgoals = np.array([[[8, 8], [3, 12]], [[16, 15], [0, 15]], [[1, 1], [2, 2]], [[12, 12], [2, 2]], [free[0], [-1, -1]], [[16, 0], [0, 0]],
                       [free[len(free) // 2], [17, 0]]], dtype=np.int32)
    kw = dict(foot=1, path_cap=P)
    want = T.batch(pm, csrc, maps=cmaps, goals=cgoals, **kw)
    assert len({want["cost"][k].tobytes() for k in range(K)}) == K and len(free) > 100
    assert np.all((want["goal_cost"] >= 0).sum(axis=1)[cmaps >= 0] >= 1) and (want["goal_cost"] < 0).any() and want["path_len"].max() > P
    assert query("travel_chunks", 256 * 1024, query("travel_query_bytes", 17, 16, 0), B) == 1
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    which = torch.arange(B, device=dev) % K
    maps, src, goals = up(cmaps)[which].contiguous(), up(csrc)[which].contiguous(), up(cgoals)[which].contiguous()
    torch.cuda.synchronize()
    out = g.travel(src, maps, goals=goals, dirs=True, **kw)
    ctx.synchronize()
    assert sorted(out) == sorted(TC.KEYS) and out["cost"].shape == (B, 17, 16) and out["path"].shape == (B, Q, P, 2)
    for key in TC.KEYS:
        for k in range(K):
            rows, w = out[key][k::K], up(want[key][k])
            assert rows.dtype == w.dtype and bool((rows == w).all()), (key, k, torch.nonzero((rows != w).reshape(rows.shape[0], -1).any(1))[:4].flatten().tolist())
    # the last queries alone, in the host form: the same rows
    tail = np.arange(B - 5, B) % K
    alone = slam.grid_travel_host(g, csrc[tail], grid_of_batch=cmaps[tail], goals=cgoals[tail], dirs=True, **kw)
    TC.same(alone, {k: v[B - 5:].cpu().numpy() for k, v in out.items()})
    TC.same(alone, {k: v[tail] for k, v in want.items()})
    ctx.check_status()
    del out, maps, src, goals, which, rows, w
    g.close()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ the overflow rejection
def test_a_map_whose_costs_could_overflow_is_rejected_and_one_cell_row_less_is_not(slam, ctx):
    """14 * xw * yw >= 2^31 at 12 386 x 12 385 cells and not at 12 385 x 12 385.  The smaller grid is not relaxed: with the
    budget at 1 MB it is refused by the LATER clause, which shows that the overflow clause let it pass."""
    import torch
    if torch.cuda.mem_get_info(0)[0] < 4 << 30:
        pytest.skip("needs 4 GB of free device memory")
    abi = pkg("_abi")
    assert 14 * 12386 * 12385 >= 2 ** 31 > 14 * 12385 * 12385
    src, goals = np.array([[[5, 5]]], dtype=np.int32), np.array([[[7, 7]]], dtype=np.int32)
    out = [np.full(1, -7, np.int32) for _ in range(3)]                   # status, goal_cost, path_len

    def raw(g):
        return abi.lib().slam_grid_travel(ctx.handle, g._h, 1, None, abi.ptr(src), 1, 0, 0, 0, 64, abi.ptr(goals), 1, 0, abi.ptr(out[0]), None,
                                          None, abi.ptr(out[1]), abi.ptr(out[2]), None)

    g = slam.DeviceGrid(1, 12386, 12385, 1.0, 0.0, 0.0, context=ctx)
    try:
        assert raw(g) == abi.ERR_INVALID
        assert "overflow" in abi.lib().slam_last_error().decode() and all(v[0] == -7 for v in out)
        with pytest.raises(slam.SlamError, match="overflow"):
            slam.grid_travel_host(g, src, goals=goals, cost=False)
        ctx.check_status()
    finally:
        g.close()
    g = slam.DeviceGrid(1, 12385, 12385, 1.0, 0.0, 0.0, context=ctx)
    try:
        ctx.set_option("travel_ws_mb", 1)
        assert raw(g) == abi.ERR_INVALID
        assert "travel_ws_mb" in abi.lib().slam_last_error().decode() and all(v[0] == -7 for v in out)
        with pytest.raises(slam.SlamError, match="travel_ws_mb"):
            slam.grid_travel_host(g, src, goals=goals, cost=False)
        ctx.check_status()
    finally:
        ctx.set_option("travel_ws_mb", 256)
        g.close()
    torch.cuda.empty_cache()
