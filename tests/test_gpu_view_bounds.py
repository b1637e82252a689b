"""The view gain on the GPU at the edges of its launch shapes: ragged maps whose last word of a row is partial, boxes
at the LDS bound, views per map across a change of map, one view past the block cap, and window slots for 1, 2 and
B - 1 views under the global engine.  Counts and seen words bit-equal to tests/view_ref.py under "gain_lds" 0 and 1."""
import ctypes as C

import numpy as np
import pytest

import raycast_ref as R
import view_ref as V
from conftest import pkg
from test_gpu_raycast import same
from test_gpu_view import check, dev, grid_of, host, up

pytestmark = pytest.mark.gpu

MODE = {}                                                # "gain_lds" of a context of this module


@pytest.fixture(scope="module")
def slam():
    p = pkg()
    p._abi.default_context()   # fails loudly when there is no gfx950 device
    return p


@pytest.fixture(scope="module", params=[0, 1], ids=["global", "lds"])
def ctx(request, slam):
    c = slam.Context(0)
    c.set_option("gain_lds", request.param)
    MODE[id(c)] = request.param
    yield c
    c.close()


def query(name, a=0, b=0, c=0, guard=0):
    abi = pkg("_abi")
    out = C.c_int64(-1)
    abi.check(abi.lib().slam_plan_query(name.encode(), a, b, c, guard, C.byref(out)))
    return int(out.value)


def random_pmap(xw, yw, seed, occupied=0.04):
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([50, 0, 100], dtype=np.int8), size=(xw, yw), p=[0.35, 0.65 - occupied, occupied])


def spokes(cell, reach, step):
    """Beam tables from the middle of `cell` to every step-th cell of the ring of Chebyshev radius `reach` around it."""
    return R.tables_to(R.ring(reach, cell)[::step], cell)


# ------------------------------------------------------------------ A. ragged maps
SHAPES = [(37, 300), (300, 37), (5, 257), (1, 70), (65, 33)]


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_ragged_maps(slam, ctx, shape):
    xw, yw = shape
    pm = random_pmap(xw, yw, seed=xw * 1000 + yw)
    pm[xw - 1, max(yw - 40, 0):] = 0                     # the end of the last row is free: it can be seen from inside it
    cells = [(xw - 1, yw - 1), (0, 0), (xw // 2, yw // 2), (xw - 1, max(yw - 40, 0))]
    for cell in cells:
        pm[cell] = 0
    g = grid_of(slam, ctx, [pm])
    reach = max(xw, yw) // 2 + 3
    poses = np.array([[c[0] + 0.5, c[1] + 0.5, th] for c, th in zip(cells, (0.0, 0.4, -2.0, 0.0))])
    ct, st = R.tables_to(R.ring(reach, (0, 0))[::5] + [(reach, 0), (-reach, 0), (0, reach), (0, -reach)], (0, 0))
    want = V.views([pm], 1.0, 0.0, 0.0, poses, ct, st, 1.0)
    last_word = (yw - 1) >> 5
    assert want[1][:, xw - 1, last_word].any()           # seen cells in the last, partial word of the last row
    assert yw % 32 == 0 or not (want[1][:, :, last_word] >> np.uint32(yw % 32)).any()
    check(host(slam, g, poses, ct, st), want, "%dx%d" % shape)
    check(dev(g, ctx, poses, ct, st), want, "%dx%d dev" % shape)
    ctx.check_status()


# ------------------------------------------------------------------ B. boxes at the LDS bound
@pytest.mark.parametrize("rows", [-1, 0, 1], ids=["one-row-below", "on", "one-row-above"])
def test_box_at_the_lds_bound(slam, ctx, rows):
    bound = query("kViewLdsBytes")
    yw = 4096                                            # 128 words a row
    fit = bound // 4 // 128
    R_ = fit + rows
    assert query("view_engine", R_, 128, 1) == (1 if rows <= 0 else 0)
    xw = fit + 3
    pm = random_pmap(xw, yw, seed=11 + rows, occupied=0.0005)
    pm[0, 0] = 0
    g = grid_of(slam, ctx, [pm])
    # the box of this view: rows 0 .. R_ - 1, all 128 words of each
    ends = [(R_ - 1, yw - 1), (R_ - 1, 0), (0, yw - 1), (R_ // 2, yw - 70), (R_ - 1, yw // 2), (3, 1000)]
    ct, st = R.tables_to(ends, (0, 0))
    pose = np.array([[0.5, 0.5, 0.0]])
    want = V.views([pm], 1.0, 0.0, 0.0, pose, ct, st, 1.0)
    assert want[0][0, :3].sum() > 1000
    check(host(slam, g, pose, ct, st), want, "rows %d" % R_)
    # a second view with a small box beside it: the two engines share a batch
    poses = np.array([[0.5, 0.5, 0.0], [xw - 1.5, 40.5, 0.0], [0.5, 0.5, 0.0]])
    check(dev(g, ctx, poses, ct, st), V.views([pm], 1.0, 0.0, 0.0, poses, ct, st, 1.0), "rows %d, three views" % R_)
    ctx.check_status()


# ------------------------------------------------------------------ C. views per map across a change of map
def test_views_per_map_across_a_change_of_map(slam, ctx):
    pms = [random_pmap(40, 50, seed=s) for s in (1, 2, 3)]
    for pm in pms:
        pm[20, 25] = 0
    g = grid_of(slam, ctx, pms)
    ct, st = spokes((0, 0), 30, 3)
    rng = np.random.default_rng(5)
    for gob in ([0], [1, 1], [2, 2, 2], [0, 1, 1, 2, 2, 2], [2, 2, 2, 0, 1, 1, 0]):
        poses = np.stack([[20.5 + rng.integers(-3, 4), 25.5 + rng.integers(-3, 4), rng.uniform(-3, 3)] for _ in gob])
        want = V.views(pms, 1.0, 0.0, 0.0, poses, ct, st, 1.0, gob=gob)
        check(host(slam, g, poses, ct, st, gob=gob), want, str(gob))
        check(dev(g, ctx, poses, ct, st, gob=gob), want, str(gob) + " dev")
    ctx.check_status()


# ------------------------------------------------------------------ D. one view past the block cap
def test_one_view_past_the_block_cap(slam, ctx):
    import torch
    cap = query("kViewMaxBlocks")
    B = cap + 1
    pm = random_pmap(3, 40, seed=9, occupied=0.1)
    g = grid_of(slam, ctx, [pm])
    kinds = np.array([[0.5, 0.5, 0.0], [1.5, 20.5, 0.0], [2.5, 39.5, 3.14], [2.5, 10.5, 1.5], [np.nan, 0.5, 0.0]])
    ct, st = [17.0], [1.0]
    wc, ws = V.views([pm], 1.0, 0.0, 0.0, kinds, ct, st, 1.0)
    assert len({tuple(c) for c in wc}) == 5
    idx = (np.arange(B) * 7) % 5
    idx[-1] = 3                                          # the one view of the second pass
    d_poses, d_ct, d_st = up(kinds[idx]), up(np.array(ct)), up(np.array(st))
    torch.cuda.synchronize()
    counts, seen = g.view_gain(d_poses, d_ct, d_st, max_range=1.0, return_seen=True)
    ctx.synchronize()
    d_idx = up(idx)
    assert bool((counts == up(wc)[d_idx]).all())
    assert bool((seen == up(ws.view(np.int32))[d_idx]).all())
    assert same(counts[-1].cpu().numpy(), wc[3])
    ctx.check_status()


# ------------------------------------------------------------------ E. window slots of the global engine
def test_window_slots_and_a_budget_below_one_view(slam, ctx):
    abi = pkg("_abi")
    xw, yw, B = 37, 300, 6
    pm = random_pmap(xw, yw, seed=21)
    pm[18, 150] = 0
    g = grid_of(slam, ctx, [pm])
    vb = query("view_bytes", xw, yw)
    assert vb == 37 * 10 * 4
    rng = np.random.default_rng(6)
    poses = np.stack([[18.5 + rng.integers(-10, 11), 150.5 + rng.integers(-100, 101), rng.uniform(-3, 3)] for _ in range(B)])
    ct, st = spokes((0, 0), 120, 9)
    want = V.views([pm], 1.0, 0.0, 0.0, poses, ct, st, 1.0)
    try:
        for slots in (1, 2, B - 1, B):
            ctx.set_option("gain_ws_mb", (slots * vb + 0.5) / 1048576.0)
            check(host(slam, g, poses, ct, st), want, "%d slots" % slots)
            check(dev(g, ctx, poses, ct, st), want, "%d slots dev" % slots)
        # below one view: the global engine has no slot to work in
        ctx.set_option("gain_ws_mb", (vb - 1 + 0.5) / 1048576.0)
        counts = np.full((B, 4), 77, dtype=np.int32)
        seen = np.full((B, xw, 10), 0x5a5a5a5a, dtype=np.uint32)
        p, c, s = np.ascontiguousarray(poses), np.ascontiguousarray(ct), np.ascontiguousarray(st)
        rc = abi.lib().slam_grid_view_gain(ctx.handle, g._h, abi.ptr(p), B, None, abi.ptr(c), abi.ptr(s), len(c), 1.0, 1, abi.ptr(counts), abi.ptr(seen))
        if MODE[id(ctx)] == 0:
            assert rc == abi.ERR_INVALID and b"gain_ws_mb" in abi.lib().slam_last_error()
            assert np.all(counts == 77) and np.all(seen == 0x5a5a5a5a)             # nothing enqueued, outputs untouched
            import torch
            d = [up(p), up(c), up(s)]
            torch.cuda.synchronize()
            with pytest.raises(slam.SlamError, match="gain_ws_mb"):
                g.view_gain(*d, max_range=1.0)
        else:                                            # every box of this map fits LDS: no slot is needed
            assert rc == abi.SLAM_OK
            check((counts, seen), want, "LDS without a slot")
    finally:
        ctx.set_option("gain_ws_mb", 256)
    ctx.check_status()
