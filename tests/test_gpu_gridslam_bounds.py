"""The bounds and rejections of the grid FastSLAM entry points: every refused call answers SLAM_ERR_INVALID with a message,
enqueues nothing and is followed by a good call on the same context; a chain of copies is refused by the host form and
marked -1 by the device form; one copy call takes 70 000 maps, past 65 535 workgroups."""
import numpy as np
import pytest

import gridslam_ref as G
import mcl_ref as X
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


def refused(slam, what, fn, *args, **kw):
    with pytest.raises(slam.SlamError, match=what):
        fn(*args, **kw)


def counters(g, ctx):
    import torch
    ctx.synchronize()
    p, h = g.counters_torch()
    out = p.cpu().numpy().astype(np.int64), h.cpu().numpy().astype(np.int64)
    torch.cuda.synchronize()
    return out


def fill(g, ctx, p, h):
    import torch
    ctx.synchronize()
    tp, th = g.counters_torch()
    tp.copy_(torch.from_numpy(p.astype(np.int32)).to(tp.device))
    th.copy_(torch.from_numpy(h.astype(np.int32)).to(th.device))
    torch.cuda.synchronize()


def test_weigh_maps_rejections(slam, ctx):
    g = slam.DeviceGrid(5, 64, 64, 1.0, 0.0, 0.0, context=ctx)
    k = X.ring_case(2, 3, 24, 1)
    args = (g, k["poses"], k["ranges"], k["cos_t"], k["sin_t"])
    refused(slam, "F \\* P > G", slam.mcl_weigh_host, *args, own_maps=True)                    # NULL with F * P = 6 > G = 5
    pm = np.array([[0, 1, 2], [3, 4, 0]], dtype=np.int32)
    good = slam.mcl_weigh_host(*args, grid_of_particle=pm, max_range=19.0)                      # the same shape with maps named
    assert np.all(good[1] >= 0)
    refused(slam, "cap outside", slam.mcl_weigh_host, *args, grid_of_particle=pm, cap=0)
    refused(slam, "noise without motion", slam.mcl_weigh_host, *args, grid_of_particle=pm, noise=k["noise"])
    with pytest.raises(ValueError):
        slam.mcl_weigh_host(*args, grid_of_particle=pm, grid_of_filter=[0, 1])
    again = slam.mcl_weigh_host(*args, grid_of_particle=pm, max_range=19.0)
    assert np.array_equal(again[1], good[1])


def test_settle_rejections_each_followed_by_a_good_call(slam, ctx):
    abi = pkg("_abi")
    L = abi.lib()
    anc = np.array([[0, 0, 2]], dtype=np.int32)
    want = G.settle_batch(anc)["settled"]
    out = np.empty((1, 3), dtype=np.int32)

    def good():
        s, _, _, m = slam.mcl_settle_host(ctx, anc)
        assert np.array_equal(s, want) and m.tolist() == [1]

    good()
    for bad, msg in (([[0, 3, 1]], "ancestor outside"), ([[0, -1, 1]], "ancestor outside")):
        refused(slam, msg, slam.mcl_settle_host, ctx, np.array(bad, dtype=np.int32))
        good()
    refused(slam, "map0", slam.mcl_settle_host, ctx, anc, map0=-1)
    good()
    refused(slam, "map0", slam.mcl_settle_host, ctx, anc, map0=2 ** 31 - 2)
    good()
    big = np.zeros((1, 4097), dtype=np.int32)
    refused(slam, "P outside", slam.mcl_settle_host, ctx, big)
    good()
    assert L.slam_mcl_settle(ctx.handle, abi.ptr(anc), None, 0, 3, 0, abi.ptr(out), None, None, None) == abi.ERR_INVALID
    assert b"F < 1" in L.slam_last_error()
    assert L.slam_mcl_settle(ctx.handle, abi.ptr(anc), None, 1, 3, 0, None, None, None, None) == abi.ERR_INVALID
    assert L.slam_mcl_settle(ctx.handle, None, None, 1, 3, 0, abi.ptr(out), None, None, None) == abi.ERR_INVALID
    poses = np.zeros((1, 3, 3))
    assert L.slam_mcl_settle(ctx.handle, abi.ptr(anc), abi.ptr(poses), 1, 3, 0, abi.ptr(out), abi.ptr(poses), None, None) == abi.ERR_INVALID
    assert b"must not be poses_src" in L.slam_last_error()
    assert L.slam_mcl_settle(ctx.handle, abi.ptr(anc), None, 1, 3, 0, abi.ptr(out), abi.ptr(poses), None, None) == abi.ERR_INVALID
    good()
    at_cap = slam.mcl_settle_host(ctx, np.zeros((2, 4096), dtype=np.int32))                     # the largest P
    assert at_cap[3].tolist() == [4095, 4095] and not at_cap[0].any()


def test_copy_rejections_and_chains(slam, ctx):
    import torch
    abi = pkg("_abi")
    G_, xw, yw = 5, 33, 35
    g = slam.DeviceGrid(G_, xw, yw, 1.0, 0.0, 0.0, context=ctx)
    rng = np.random.default_rng(2)
    p, h = rng.integers(0, 1 << 30, (G_, xw, yw)), rng.integers(0, 9, (G_, xw, yw))
    fill(g, ctx, p, h)

    def unchanged():
        gp, gh = counters(g, ctx)
        assert np.array_equal(gp, p) and np.array_equal(gh, h)

    for first, src, msg in ((0, [1, 2, 2], "itself a destination"),           # 0 <- 1 while 1 <- 2: a chain
                            (0, [1, 0], "itself a destination"),              # a swap
                            (-1, [0], "first < 0"), (4, [0, 0], "first \\+ count > G"), (5, [0], "first \\+ count > G")):
        refused(slam, msg, slam.grid_copy_maps_host, g, src, first)
        unchanged()
        assert slam.grid_copy_maps_host(g, [3], 3).tolist() == [0]             # a good call afterwards
    refused(slam, "count < 1", slam.grid_copy_maps_host, g, [], 0)
    assert abi.lib().slam_grid_copy_maps(ctx.handle, g._h, None, 0, 1, None) == abi.ERR_INVALID
    unchanged()
    # the device form: the destination whose source is a destination is left alone and marked -1, the rest is done
    dev = torch.device("cuda", ctx.device)
    src = np.array([1, 2, 2, 2, -1], dtype=np.int32)
    want = G.copy_maps([p, h], src, 0)
    assert want.tolist() == [-1, 1, 0, 1, 0]
    t_src, t_self, t_four = (torch.from_numpy(np.array(v, dtype=np.int32)).to(dev) for v in (src, [0], [4]))
    torch.cuda.synchronize()                                                   # the context's stream is not torch's
    out = g.copy_maps(t_src)
    ctx.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    unchanged()                                                                # (p, h now hold the restatement's result)
    assert np.array_equal(p[1], p[2]) and np.array_equal(p[3], p[2]) and not np.array_equal(p[0], p[1])
    none = g.copy_maps(t_self, first=0)
    abi.check(abi.lib().slam_grid_copy_maps_dev(ctx.handle, g._h, abi.ptr(t_four), 0, 1, None))   # copied_out may be absent
    ctx.synchronize()
    assert none.cpu().numpy().tolist() == [0]
    p[0], h[0] = p[4], h[4]
    unchanged()


def test_copy_70000_maps_in_one_call(slam, ctx):
    G_, xw, yw = 70000, 3, 5
    g = slam.DeviceGrid(G_, xw, yw, 1.0, 0.0, 0.0, context=ctx)
    p = (np.arange(G_ * 15, dtype=np.int64) * 7919 % (1 << 30)).reshape(G_, xw, yw)
    h = (np.arange(G_ * 15, dtype=np.int64) % 11).reshape(G_, xw, yw)
    fill(g, ctx, p, h)
    k = np.arange(G_)
    src = np.where(k % 3 == 0, k, k - k % 3).astype(np.int32)                  # every source keeps itself
    src[5], src[G_ - 1] = -1, G_
    want = G.copy_maps([p, h], src, 0)
    got = slam.grid_copy_maps_host(g, src, 0)
    assert np.array_equal(got, want) and (want == 1).sum() > 46000
    gp, gh = counters(g, ctx)
    assert np.array_equal(gp, p) and np.array_equal(gh, h)


def test_update_particles_rejections(slam, ctx, syn):
    g = slam.DeviceGrid(4, 200, 200, 10.0, 10.0, 10.0, context=ctx)
    rep = syn.make_replay(2, 120, seed=4)
    ang = np.linspace(rep.angle_min, rep.angle_max, 120)
    ct, st = np.cos(ang), np.sin(ang)
    ranges = np.asarray(rep.ranges, dtype=np.float32)
    poses = np.tile(np.asarray(rep.poses_true)[:2, None], (1, 2, 1))
    refused(slam, "map0 \\+ F \\* P > G", slam.grid_update_particles_host, g, ranges, ct, st, poses, map0=1)
    refused(slam, "map0 < 0", slam.grid_update_particles_host, g, ranges, ct, st, poses, map0=-1)
    gp, gh = counters(g, ctx)
    assert not gp.any() and not gh.any()
    slam.grid_update_particles_host(g, ranges, ct, st, poses, map0=0)
    gp, gh = counters(g, ctx)
    assert all(gh[i].sum() > 100 for i in range(4)) and np.array_equal(gp[0], gp[1]) and not np.array_equal(gp[0], gp[2])
    abi = pkg("_abi")
    assert abi.lib().slam_grid_update_particles(ctx.handle, g._h, abi.ptr(ranges), abi.ptr(ct), abi.ptr(st), abi.ptr(poses), None, 2, 2,
                                                65536, 0) == abi.ERR_INVALID
    assert abi.lib().slam_grid_update_particles(ctx.handle, g._h, None, abi.ptr(ct), abi.ptr(st), abi.ptr(poses), None, 2, 2, 120,
                                                0) == abi.ERR_INVALID
    ctx.check_status()


def test_update_particles_past_65535_particles(slam, ctx):
    """One call, 70 000 particles: the launches split at 65 535 particles, and a particle behind the split still reads its
    own filter's scan, its own pose and its own map."""
    abi = pkg("_abi")
    F, P, n, xw, yw = 2, 35000, 8, 8, 16
    g = slam.DeviceGrid(F * P, xw, yw, 1.0, 0.0, 0.0, context=ctx)
    rng = np.random.default_rng(6)
    ang = np.linspace(-3.0, 3.0, n)
    ct, st = np.cos(ang), np.sin(ang)
    ranges = rng.uniform(1.0, 6.0, (F, n)).astype(np.float32)
    poses = np.concatenate([rng.uniform(2.0, 6.0, (F, P, 1)), rng.uniform(4.0, 12.0, (F, P, 1)), rng.uniform(-3.0, 3.0, (F, P, 1))], axis=-1)
    acc = np.zeros((F, P), dtype=np.int32)
    acc[1, 65537 - P] = X.DEAD
    slam.grid_update_particles_host(g, ranges, ct, st, poses, acc=acc)
    gp, gh = counters(g, ctx)
    one = slam.DeviceGrid(1, xw, yw, 1.0, 0.0, 0.0, context=ctx)
    for l in (0, 1, P - 1, P, 65534, 65535, 65536, 65537, 65538, F * P - 1):
        f, p = divmod(l, P)
        if acc[f, p] == X.DEAD:
            assert not gp[l].any() and not gh[l].any()
            continue
        one.reset()
        abi.check(abi.lib().slam_grid_update_scans(ctx.handle, one._h, abi.ptr(ranges[f]), abi.ptr(ct), abi.ptr(st),
                                                   abi.ptr(np.ascontiguousarray(poses[f, p])), None, 1, n))
        r = one.read(0, want=("pass", "hit"))
        assert np.array_equal(gp[l], r["pass"]) and np.array_equal(gh[l], r["hit"]), l
        assert r["pass"].sum() > 0
    touched = (gp.reshape(F * P, -1).sum(axis=1) + gh.reshape(F * P, -1).sum(axis=1)) > 0
    assert touched.sum() == F * P - 1
