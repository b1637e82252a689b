"""slam_grid_locate at the edges of its arguments and its workspace: the list budget ("locate_ws_mb") cut so small that a
call takes many chunks, the request that fits no budget, every argument set the library rejects - each followed by a good
call - the device form back to back, and a region the device form finds outside the map.  Against tests/locate_ref.py
with array_equal, through the C ABI."""
import numpy as np
import pytest

import locate_cases as LC
import locate_ref as L
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
def case(slam, ctx):
    """The 70 x 33 ragged map, a 65-beam scan, K = 64, three hypotheses with regions of their own."""
    g = LC.ragged_grid(slam, ctx, 70, 33)
    cap = 50
    fields = LC.fields_of(slam, g, cap)
    ct, st, ranges = L.ragged_scan(65, seed=8)
    _, rot = L.rotations(64)
    regs = np.array([(0, 0, 70, 33), (3, 2, 41, 27), (60, 0, 10, 33)], dtype=np.int32)
    per = np.stack([ranges, ranges[::-1], np.roll(ranges, 7)])
    return dict(g=g, cap=cap, fields=fields, ct=ct, st=st, rot=rot, regs=regs, per=per)


def call(slam, c, H=3, **kw):
    a = dict(levels=H, region=c["regs"], max_range=20.0, cap=c["cap"], return_stats=True)
    a.update(kw)
    return slam.grid_locate_host(c["g"], c["per"], c["ct"], c["st"], c["rot"], **a)


def query(name, a=0, b=0, c=0):
    import ctypes as C
    abi = pkg("_abi")
    out = C.c_int64()
    abi.check(abi.lib().slam_plan_query(name.encode(), int(a), int(b), int(c), -1, C.byref(out)))
    return int(out.value)


# ------------------------------------------------------------------ chunks
def test_chunks_change_nothing(slam, ctx, case):
    want = L.locate_batch(case["fields"], 1.0, case["per"], case["ct"], case["st"], case["rot"], 3, 20.0, case["cap"], regions=case["regs"])
    LC.same(call(slam, case), want)                                  # the default budget: one chunk
    pair = query("locate_pair_bytes", 70, 33, 3) + query("locate_table_bytes", 65)     # a pair's lists and its row of offsets
    assert query("locate_chunk_pairs", 64 * 1024, pair, 192) == 192
    try:
        for kib in (20, 7, 100):                                     # 2 pairs, 1 pair, 14 pairs a chunk: 96, 192, 14 chunks
            assert query("locate_chunk_pairs", kib, pair, 192) == kib * 1024 // pair < 192 // 4
            ctx.set_option("locate_ws_mb", kib / 1024.0)
            LC.same(call(slam, case), want)
        for H in (1, 5, 8):
            ctx.set_option("locate_ws_mb", 0.05)
            small = call(slam, case, H=H)
            ctx.set_option("locate_ws_mb", 64)
            LC.same(small, call(slam, case, H=H))
    finally:
        ctx.set_option("locate_ws_mb", 64)


def test_a_request_over_the_budget_is_rejected(slam, ctx, case):
    pair = query("locate_pair_bytes", 70, 33, 3) + query("locate_table_bytes", 65)
    good = call(slam, case)
    try:
        ctx.set_option("locate_ws_mb", (pair - 1) / 1048576.0)
        with pytest.raises(slam.SlamError, match="locate_ws_mb"):
            call(slam, case)
        LC.same(call(slam, case, H=0), call(slam, case, H=0))        # brute force keeps no list: it still runs
        small = np.array([(0, 0, 9, 9)] * 3, dtype=np.int32)
        assert call(slam, case, region=small)[0].shape == (3, 3)      # and so does a region whose lists fit
        ctx.set_option("locate_ws_mb", pair / 1048576.0)
        LC.same(call(slam, case), good)                              # exactly one pair fits
    finally:
        ctx.set_option("locate_ws_mb", 64)
    for v in (0, -1, float("nan"), 2 ** 20 + 1):
        with pytest.raises(slam.SlamError, match="locate_ws_mb"):
            ctx.set_option("locate_ws_mb", v)
    LC.same(call(slam, case), good)


# ------------------------------------------------------------------ rejected arguments
def test_every_rejected_argument_set_and_a_good_call_after_each(slam, ctx, case):
    abi = pkg("_abi")
    g = case["g"]
    good = call(slam, case)
    n, K, B = 65, 64, 3
    best, cost, used = np.empty((B, 3), np.int32), np.empty(B, np.int32), np.empty(B, np.int32)
    stats = np.empty((B, 5), np.int64)
    base = dict(ranges=case["per"], shared=0, B=B, gob=None, ct=case["ct"], st=case["st"], n=n, rot=case["rot"], K=K, region=case["regs"],
                levels=3, max_range=20.0, cap=50, best=best, cost=cost, used=used, stats=stats)

    def raw(**kw):
        a = dict(base)
        a.update(kw)
        return abi.lib().slam_grid_locate(ctx.handle, g._h, abi.ptr(a["ranges"]), a["shared"], a["B"], abi.ptr(a["gob"]), abi.ptr(a["ct"]),
                                          abi.ptr(a["st"]), a["n"], abi.ptr(a["rot"]), a["K"], abi.ptr(a["region"]), a["levels"],
                                          a["max_range"], a["cap"], abi.ptr(a["best"]), abi.ptr(a["cost"]), abi.ptr(a["used"]),
                                          abi.ptr(a["stats"]))

    assert raw() == 0
    LC.same((best, cost, used, stats), good)
    reg = lambda *r: np.array([r] * B, dtype=np.int32)
    big_rot = np.zeros((1 << 20, 2))
    bad = [dict(B=0), dict(B=-1), dict(K=0), dict(n=0), dict(n=4097), dict(cap=0), dict(cap=32768), dict(max_range=0.0),
           dict(max_range=-1.0), dict(max_range=float("nan")), dict(levels=-1), dict(levels=9),
           dict(ranges=None), dict(ct=None), dict(st=None), dict(rot=None), dict(best=None), dict(cost=None),
           dict(region=reg(-1, 0, 5, 5)), dict(region=reg(0, -1, 5, 5)), dict(region=reg(0, 0, 0, 5)), dict(region=reg(0, 0, 5, 0)),
           dict(region=reg(66, 0, 5, 5)), dict(region=reg(0, 29, 5, 5)), dict(region=reg(0, 0, 71, 33)), dict(region=reg(0, 0, 70, 34)),
           dict(region=reg(2 ** 31 - 1, 0, 2, 2)),
           dict(rot=big_rot, K=1 << 20, region=None, levels=0),               # K * ni * nj >= 2^31 on the whole map
           dict(rot=big_rot, K=1 << 20, B=2048, shared=1, region=np.array([(0, 0, 1, 1)] * 2048, dtype=np.int32), levels=0)]   # B * K >= 2^31 alone
    for kw in bad:
        best[:], cost[:], used[:], stats[:] = -7, -7, -7, -7
        assert raw(**kw) == abi.ERR_INVALID, kw
        assert abi.lib().slam_last_error()
        assert np.all(best == -7) and np.all(cost == -7) and np.all(stats == -7), kw
        assert raw() == 0, kw
        LC.same((best, cost, used, stats), good)
    ctx.check_status()                                               # the sticky status is untouched
    # what is NOT rejected: +inf max_range, used_out and stats_out absent, the limits themselves
    assert raw(max_range=float("inf"), used=None, stats=None) == 0
    assert raw(cap=32767, levels=8, stats=np.empty((B, 10), np.int64)) == 0 and raw(cap=1, levels=0, stats=np.empty((B, 2), np.int64)) == 0
    wide_ct, wide_st, wide_r = L.ragged_scan(4096, seed=1)
    assert raw(n=4096, ct=wide_ct, st=wide_st, ranges=wide_r, shared=1) == 0
    LC.same(call(slam, case), good)


# ------------------------------------------------------------------ the device form
def test_device_form_back_to_back_and_a_region_outside_the_map(slam, ctx, case):
    import torch
    g = case["g"]
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    h1 = call(slam, case)
    h2 = slam.grid_locate_host(g, case["per"][1], case["ct"], case["st"], case["rot"][5:12], levels=5, max_range=15.0, cap=20,
                               return_stats=True)
    d = dict(cos_t=up(case["ct"]), sin_t=up(case["st"]))
    r1, r2, rot1, rot2, regs = up(case["per"]), up(case["per"][1]), up(case["rot"]), up(case["rot"][5:12]), up(case["regs"])
    best2 = torch.full((1, 3), -5, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    # two _dev calls back to back without a synchronise: the second rebuilds the field, the pyramid and the lists of the first
    o1 = g.locate(r1, rot_cs=rot1, levels=3, region=regs, max_range=20.0, cap=case["cap"], return_stats=True, **d)
    o2 = g.locate(r2, rot_cs=rot2, levels=5, max_range=15.0, cap=20, best_out=best2, return_stats=True, **d)
    ctx.synchronize()
    assert o2[0] is best2
    LC.same([t.cpu().numpy() for t in o1], h1)
    LC.same([t.cpu().numpy() for t in o2], h2)
    # device memory the host cannot check: a region that is empty or leaves the map costs its hypothesis its answer,
    # as a map entry outside [0, G) does; its neighbours are unaffected
    odd = case["regs"].copy()
    odd[1] = (66, 0, 5, 5)
    want = L.locate_batch(case["fields"], 1.0, case["per"], case["ct"], case["st"], case["rot"], 3, 20.0, case["cap"], regions=odd)
    assert want[0][1].tolist() == [-1, -1, -1] and want[0][0].tolist() == h1[0][0].tolist()
    o3 = g.locate(r1, rot_cs=rot1, levels=3, region=up(odd), max_range=20.0, cap=case["cap"], return_stats=True, **d)
    ctx.synchronize()
    LC.same([t.cpu().numpy() for t in o3], want)
    for empty in ((5, 5, 0, 3), (5, 5, 3, -2), (-1, 5, 3, 3)):
        odd[1] = empty
        o4 = g.locate(r1, rot_cs=rot1, levels=3, region=up(odd), max_range=20.0, cap=case["cap"], return_stats=True, **d)
        ctx.synchronize()
        LC.same([t.cpu().numpy() for t in o4], want)
    ctx.check_status()
