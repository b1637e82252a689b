"""Grid FastSLAM on the device (slam_mcl_weigh_maps / slam_mcl_settle / slam_grid_copy_maps / slam_grid_update_particles,
DeviceGridSLAM, GridSLAM) through the C ABI.  The weigh is held against the EXISTING slam_mcl_weigh (bit equality), the map
update against the existing slam_grid_update_scans (every counter), settle, copy and the whole step against the restatement
(tests/gridslam_ref.py).  Integers compare with array_equal, poses and estimates at 1e-9."""
import numpy as np
import pytest

import gridslam_ref as G
import mcl_ref as X
from conftest import pkg

pytestmark = pytest.mark.gpu

PS = (1, 2, 63, 64, 65, 1000, 4096)


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


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def set_counters(g, ctx, pass_, hit):
    import torch
    ctx.synchronize()
    p, h = g.counters_torch()
    p.copy_(torch.from_numpy(np.ascontiguousarray(pass_).astype(np.int32)).to(p.device))
    h.copy_(torch.from_numpy(np.ascontiguousarray(hit).astype(np.int32)).to(h.device))
    torch.cuda.synchronize()


def get_counters(g, ctx):
    import torch
    ctx.synchronize()
    p, h = g.counters_torch()
    out = p.cpu().numpy().astype(np.int64), h.cpu().numpy().astype(np.int64)
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------ weigh: against the existing entry, bit for bit
def random_maps(slam, ctx, G_, seed):
    """G_ different 64 x 64 maps (scale 1): 40 occupied cells each, written into the hit counters."""
    g = slam.DeviceGrid(G_, 64, 64, 1.0, 0.0, 0.0, context=ctx)
    rng = np.random.default_rng(seed)
    hit = np.zeros((G_, 64, 64), dtype=np.int32)
    for gi in range(G_):
        xy = rng.integers(4, 60, (40, 2))
        hit[gi, xy[:, 0], xy[:, 1]] = 1
    set_counters(g, ctx, np.zeros_like(hit), hit)
    return g


def weigh_both(slam, g, k, acc, pmaps=None, own=True, field=None, cap=64, max_range=19.0):
    """slam_mcl_weigh_maps, and slam_mcl_weigh run as F * P filters of one particle on the same maps."""
    F, P, _ = k["poses"].shape
    got = slam.mcl_weigh_host(g, k["poses"], k["ranges"], k["cos_t"], k["sin_t"], motion=k["motion"], noise=k["noise"], max_range=max_range,
                              cap=cap, field=field, acc=acc, grid_of_particle=pmaps, own_maps=own)
    maps = np.arange(F * P, dtype=np.int32) if pmaps is None else np.asarray(pmaps, dtype=np.int32).reshape(-1)
    ref = slam.mcl_weigh_host(g, k["poses"].reshape(F * P, 1, 3), np.repeat(k["ranges"], P, axis=0), k["cos_t"], k["sin_t"],
                              motion=np.repeat(k["motion"], P, axis=0), noise=k["noise"].reshape(F * P, 1, 3), max_range=max_range, cap=cap,
                              field=field, acc=None if acc is None else acc.reshape(F * P, 1), grid_of_filter=maps)
    assert same_bits(got[0], ref[0].reshape(F, P, 3))                          # the moved poses, bit for bit
    assert got[1].dtype == np.int32 and np.array_equal(got[1], ref[1].reshape(F, P))
    if acc is not None:
        assert np.array_equal(got[2], ref[2].reshape(F, P))
    assert np.array_equal(got[3], ref[3].reshape(F, P)[:, 0])
    return got


@pytest.mark.parametrize("P", [1, 63, 65])
@pytest.mark.parametrize("n", [1, 65, 120])
def test_weigh_maps_is_the_existing_weigh_per_particle(slam, ctx, P, n):
    F = 2
    g = random_maps(slam, ctx, F * P + 1, 100 + P)
    k = X.ring_case(F, P, n, 7 * P + n)
    acc = np.random.default_rng(P + n).integers(0, 1000, (F, P)).astype(np.int32)
    if P > 2:
        acc[1, 2] = X.DEAD                                                     # a dead particle stays dead
    outs = []
    for shape in (-1, 0, 1):                                                   # both launch shapes and the automatic choice
        ctx.set_option("mcl_shape", shape)
        outs.append(weigh_both(slam, g, k, acc))
    ctx.set_option("mcl_shape", -1)
    for o in outs[1:]:
        assert all(same_bits(a, b) for a, b in zip(o, outs[0]))
    cost, acc_out = outs[0][1], outs[0][2]
    assert np.all(cost[acc != X.DEAD] >= 0) and (P < 8 or len(np.unique(cost)) > 4)   # maps that differ give costs that differ
    if P > 2:
        assert cost[1, 2] == -1 and acc_out[1, 2] == X.DEAD
    # the field given against the field rebuilt
    fld = slam.grid_distance_field_host(g, 64)
    given = weigh_both(slam, g, k, acc, field=fld)
    assert all(same_bits(a, b) for a, b in zip(given, outs[0]))
    # an explicit grid_of_particle, entries -1 and G between good neighbours
    G_ = F * P + 1
    pm = np.random.default_rng(n).integers(0, G_, (F, P)).astype(np.int32)
    if P > 2:
        pm[0, 1], pm[1, P - 2] = -1, G_
    ex = weigh_both(slam, g, k, acc, pmaps=pm, own=False)
    if P > 2:
        assert ex[1][0, 1] == -1 and ex[1][1, P - 2] == -1 and ex[2][0, 1] == X.DEAD
        assert ex[1][0, 0] >= 0 and ex[1][0, 2] >= 0 and ex[1][1, P - 1] >= 0
    # no acc, no motion: nothing written back
    got = slam.mcl_weigh_host(g, k["poses"], k["ranges"], k["cos_t"], k["sin_t"], max_range=19.0, own_maps=True)
    assert same_bits(got[0], np.ascontiguousarray(k["poses"])) and got[2] is None and np.all(got[1] >= 0)


# ------------------------------------------------------------------ settle: against the restatement
def real_ancestors(F, P, seed):
    rng = np.random.default_rng(seed)
    anc = np.empty((F, P), dtype=np.int32)
    for f in range(F):
        w = np.rint(X.W_MAX * rng.random(P) ** (1 + f % 7)).astype(np.int64) + 1
        if f % 3 == 1:
            w[rng.permutation(P)[:P // 2]] = 0
            w[rng.integers(P)] += 1
        anc[f] = X.resample_u64(w, rng.uniform())
    return anc


@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("F", [1, 300])
def test_settle_against_the_restatement(slam, ctx, F, P):
    anc = real_ancestors(F, P, 1000 * F + P)
    if F > 5:                                                                  # the identity, all equal, reversed, not monotone
        anc[0], anc[1], anc[2], anc[3] = np.arange(P), P // 2, np.arange(P)[::-1], (np.arange(P) * 7 + 3) % P
        anc[4] = np.minimum(np.arange(P) // 3 * 3 + 2, P - 1)
    poses = np.random.default_rng(P).normal(0.0, 1.0, (F, P, 3))
    ref = G.settle_batch(anc, poses, map0=3)
    settled, out, map_src, moved = slam.mcl_settle_host(ctx, anc, poses, map0=3)
    assert settled.dtype == np.int32 and np.array_equal(settled, ref["settled"])
    assert same_bits(out, ref["poses"]) and np.array_equal(map_src, ref["map_src"]) and np.array_equal(moved, ref["moved"])
    if F > 5:
        assert np.array_equal(settled[0], np.arange(P)) and moved[0] == 0 and moved[2] == 0 and moved[1] == P - 1
    assert P < 63 or moved.max() > 0
    only, none, _, _ = slam.mcl_settle_host(ctx, anc)                          # every optional output absent but the counts
    assert np.array_equal(only, ref["settled"]) and none is None
    for f in range(min(F, 6)):                                                 # (a): no source is a destination
        src = np.unique(settled[f])
        assert np.array_equal(settled[f][src], src)


def test_settle_dev_clamps_out_of_range_ancestors(slam, ctx):
    import torch
    abi = pkg("_abi")
    dev = torch.device("cuda", ctx.device)
    F, P = 3, 65
    anc = real_ancestors(F, P, 5)
    anc[1, 4], anc[1, 9], anc[2, 0] = -7, P, 2 ** 31 - 1
    t = torch.from_numpy(anc).to(dev)
    settled = torch.full((F, P), -9, dtype=torch.int32, device=dev)
    moved = torch.full((F,), -9, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    abi.check(abi.lib().slam_mcl_settle_dev(ctx.handle, abi.ptr(t), None, F, P, 0, abi.ptr(settled), None, None, abi.ptr(moved)))
    ctx.synchronize()
    ref = G.settle_batch(anc, clamp=True)
    assert np.array_equal(settled.cpu().numpy(), ref["settled"]) and np.array_equal(moved.cpu().numpy(), ref["moved"])
    assert settled.min().item() >= 0 and settled.max().item() < P


# ------------------------------------------------------------------ copy: every counter of every map
def distinct_maps(G_, xw, yw):
    cells = xw * yw
    p = (np.arange(G_ * cells, dtype=np.int64) * 2654435761 % (1 << 31)).reshape(G_, xw, yw)
    h = ((np.arange(G_ * cells, dtype=np.int64) * 40503 + 17) % 3 == 0).astype(np.int64).reshape(G_, xw, yw)
    h += np.arange(G_)[:, None, None] * 4
    return p, h


@pytest.mark.parametrize("xw,yw", [(1, 1), (33, 35), (70, 33), (200, 200)])
def test_copy_maps_every_counter(slam, ctx, xw, yw):
    G_ = 5
    g = slam.DeviceGrid(G_, xw, yw, 1.0, 0.0, 0.0, context=ctx)
    for first, src in [(0, [1, 1, 3, 3, 3]), (0, [4, 4, 4, 4, 4]), (1, [0, 0, 0, 4]), (2, [-1, G_, 4]), (0, [0, 1, 2, 3, 4]), (3, [1])]:
        p, h = distinct_maps(G_, xw, yw)
        set_counters(g, ctx, p, h)
        want = G.copy_maps([p, h], src, first)
        assert not np.any(want == -1)
        got = slam.grid_copy_maps_host(g, src, first)
        assert got.dtype == np.int32 and np.array_equal(got, want)
        gp, gh = get_counters(g, ctx)
        assert np.array_equal(gp, p % (1 << 32)) and np.array_equal(gh, h)      # copies and untouched maps alike


def test_copy_maps_keeps_a_live_pmap_current(slam, ctx):
    G_, xw, yw = 5, 33, 35
    g = slam.DeviceGrid(G_, xw, yw, 1.0, 0.0, 0.0, context=ctx)
    g.live_pmap()
    rng = np.random.default_rng(3)
    p = rng.integers(0, 3, (G_, xw, yw)) * rng.integers(0, 2, (G_, xw, yw)) * 600
    h = (rng.random((G_, xw, yw)) < 0.1).astype(np.int64)
    set_counters(g, ctx, p, h)
    before = np.stack([g.read(gi)["pmap"] for gi in range(G_)])               # refreshes the live pmap: it is current now
    assert np.array_equal(before, G.pmap_of(p, h)) and len(np.unique(before)) == 3
    want = G.copy_maps([p, h], [2, 2, 2, 4, 4], 0)
    assert np.array_equal(slam.grid_copy_maps_host(g, [2, 2, 2, 4, 4], 0), want)
    after = np.stack([g.read(gi)["pmap"] for gi in range(G_)])
    assert np.array_equal(after, G.pmap_of(p, h)) and not np.array_equal(after, before)
    fresh = slam.DeviceGrid(G_, xw, yw, 1.0, 0.0, 0.0, context=ctx)           # a fresh finalize of the same counters
    set_counters(fresh, ctx, p, h)
    assert np.array_equal(after, np.stack([fresh.read(gi)["pmap"] for gi in range(G_)]))


# ------------------------------------------------------------------ update: slam_grid_update_scans per particle
GEOM = (10.0, 10.0, 10.0)


def scans_ref(slam, ctx, ranges, ct, st, pose):
    """(pass, hit, pmap) of slam_grid_update_scans of one scan into a one-map grid of its own; the error it raised."""
    abi = pkg("_abi")
    one = slam.DeviceGrid(1, 200, 200, *GEOM, context=ctx)
    err = None
    try:
        abi.check(abi.lib().slam_grid_update_scans(ctx.handle, one._h, abi.ptr(np.ascontiguousarray(ranges, dtype=np.float32)), abi.ptr(ct),
                                                   abi.ptr(st), abi.ptr(np.ascontiguousarray(pose, dtype=np.float64)), None, 1, len(ct)))
    except (ValueError, OverflowError) as e:
        err = type(e)
    r = one.read(0, want=("pmap", "pass", "hit"))
    one.close()
    return r["pass"].astype(np.int64), r["hit"].astype(np.int64), r["pmap"], err


def update_case(syn, F, P, seed):
    rep = syn.make_replay(F + 1, 120, seed=seed)
    ranges = np.asarray(rep.ranges, dtype=np.float32)[:F].copy()
    ranges[0, 5], ranges[F - 1, 17] = np.inf, np.inf                           # inf -> 30 m: a ray that leaves the map
    ang = np.linspace(rep.angle_min, rep.angle_max, 120)
    rng = np.random.default_rng(seed)
    poses = np.asarray(rep.poses_true)[:F, None, :] + rng.normal(0.0, 1.0, (F, P, 3)) * np.array([0.5, 0.5, 0.3])
    return ranges, np.cos(ang), np.sin(ang), poses


@pytest.mark.parametrize("P,map0,live", [(1, 0, False), (65, 0, True), (3, 2, False)])
def test_update_particles_is_update_scans_per_particle(slam, ctx, syn, P, map0, live):
    F = 2
    ranges, ct, st, poses = update_case(syn, F, P, 11 + P)
    G_ = map0 + F * P
    g = slam.DeviceGrid(G_, 200, 200, *GEOM, context=ctx)
    if live:
        g.live_pmap()
    acc = np.zeros((F, P), dtype=np.int32)
    if P > 2:
        acc[1, 1] = X.DEAD
        poses[1, 1] = np.nan                                                   # a dead particle's pose may hold anything
    for rounds in range(2):                                                    # a second scan on top of the first
        slam.grid_update_particles_host(g, ranges, ct, st, poses, acc=acc, map0=map0)
    ctx.check_status()                                                         # the dead particle raised nothing
    gp, gh = get_counters(g, ctx)
    assert not gp[:map0].any() and not gh[:map0].any()
    for f in range(F):
        for p in range(P):
            gi = map0 + f * P + p
            if acc[f, p] == X.DEAD:
                assert not gp[gi].any() and not gh[gi].any()
                continue
            rp, rh, rpm, err = scans_ref(slam, ctx, ranges[f], ct, st, poses[f, p])
            assert err is None
            assert np.array_equal(gp[gi], 2 * rp) and np.array_equal(gh[gi], 2 * rh), (f, p)
            if p % 16 == 0:
                assert np.array_equal(g.read(gi)["pmap"], G.pmap_of(2 * rp, 2 * rh))
                assert np.array_equal(G.pmap_of(rp, rh), rpm)
    assert gh.sum() > 100 * F * (P - (P > 2))


def test_update_particles_nan_beam_as_update_scans_treats_it(slam, ctx, syn):
    F, P = 2, 2
    ranges, ct, st, poses = update_case(syn, F, P, 40)
    ranges[1, 60] = np.nan                                                     # filter 1: the scan stops at beam 60 and raises
    g = slam.DeviceGrid(F * P, 200, 200, *GEOM, context=ctx)
    with pytest.raises(ValueError):
        slam.grid_update_particles_host(g, ranges, ct, st, poses)
    gp, gh = get_counters(g, ctx)
    for f in range(F):
        for p in range(P):
            rp, rh, _, err = scans_ref(slam, ctx, ranges[f], ct, st, poses[f, p])
            assert (err is ValueError) == (f == 1)
            assert np.array_equal(gp[f * P + p], rp) and np.array_equal(gh[f * P + p], rh)
    ctx.check_status()                                                         # reported once, then clean
    slam.grid_update_particles_host(g, ranges[:1].repeat(2, axis=0), ct, st, poses)   # a good call afterwards


# ------------------------------------------------------------------ the step
STEP = dict(F=2, P=16, n=120, xw=200, yw=200, reso=0.1, scans=6)


def step_inputs(syn, F=2):
    import torch
    k = STEP
    rep = syn.make_replay(k["scans"], k["n"], seed=4)
    ranges, true = np.asarray(rep.ranges, dtype=np.float32), np.asarray(rep.poses_true, dtype=np.float64)
    ang = np.linspace(rep.angle_min, rep.angle_max, k["n"])
    rng = np.random.default_rng(8)
    S, P = k["scans"], k["P"]
    motion = np.zeros((S, 2, 3))
    motion[1:] = np.stack([X.odometry(true[i], true[i + 1]) for i in range(S - 1)])[:, None]
    noise = rng.normal(0.0, 1.0, (S, 2, P, 3)) * np.array([0.05, 0.05, 0.03])
    noise[:, 1] = 0.0                                                          # filter 1: identical particles, it never resamples
    u0 = rng.uniform(0.0, 1.0, (S, 2))
    scans = np.stack([ranges, ranges], axis=1)                                 # [S, 2, n]
    sel = slice(0, F)
    return dict(scans=np.ascontiguousarray(scans[:, sel]), motion=np.ascontiguousarray(motion[:, sel]),
                noise=np.ascontiguousarray(noise[:, sel]), u0=np.ascontiguousarray(u0[:, sel]), cos_t=np.cos(ang), sin_t=np.sin(ang),
                start=true[0], torch=torch)


def make_dev(slam, ctx, inp, F):
    k = STEP
    d = slam.DeviceGridSLAM(F, k["P"], k["xw"], k["yw"], k["reso"], cos_t=inp["cos_t"], sin_t=inp["sin_t"], context=ctx,
                            table=X.weight_table(2.0, 0, 4096))
    d.set_particles(inp["start"])
    return d


def on_dev(inp, d, name, s=None):
    a = inp[name] if s is None else inp[name][s]
    return inp["torch"].from_numpy(np.ascontiguousarray(a)).to(d.dev)


def test_every_step_against_the_restatement(slam, ctx, syn):
    k = STEP
    F, P = k["F"], k["P"]
    inp = step_inputs(syn)
    d = make_dev(slam, ctx, inp, F)
    geom = (10.0, 10.0, 10.0)
    table = X.weight_table(2.0, 0, 4096)
    resampled = []
    for s in range(k["scans"]):
        state = d.results()
        poses0, acc0 = state["poses"].copy(), state["acc"].copy()
        pass_, hit = get_counters(d.grid, ctx)
        d.step(on_dev(inp, d, "scans", s), on_dev(inp, d, "motion", s), on_dev(inp, d, "noise", s), on_dev(inp, d, "u0", s))
        got = d.results()
        moved_poses = X.move(poses0, inp["motion"][s], inp["noise"][s])
        cost = got["cost"].astype(np.int64)
        assert np.all(cost >= 0)
        acc1 = np.minimum(acc0.astype(np.int64) + cost, X.ACC_MAX).astype(np.int32)   # the device's costs, the header's accumulation
        ref = G.step_after_costs(pass_, hit, geom, moved_poses, acc1, table, 0, inp["u0"][s], 0.5, inp["scans"][s], inp["cos_t"],
                                 inp["sin_t"], make=G.c_mapping)
        for name in ("ancestors", "settled", "map_src", "moved", "acc", "info"):
            assert got[name].dtype == np.int32 and np.array_equal(got[name], ref[name]), (s, name)
        assert np.array_equal(got["copied"], ref["copied"]), s
        assert np.allclose(got["poses"], ref["poses"], rtol=0.0, atol=1e-9) and np.allclose(got["est"], ref["est"], rtol=0.0, atol=1e-9)
        gp, gh = get_counters(d.grid, ctx)
        assert np.array_equal(gp, pass_) and np.array_equal(gh, hit), s
        resampled.append(got["info"][:, 2].tolist())
        b = int(got["info"][0, 0])                                             # (b): best still names its pose after the step
        assert got["settled"][0, b] == b and np.array_equal(got["poses"][0, b], d.best(0)[1])
    r = np.array(resampled)
    assert r[:, 0].any() and not r[:, 1].any()                                 # one filter resamples, the other never does
    assert np.array_equal(d.best_map(0), d.grid.read(int(d.info[0, 0].item()))["pmap"])


def run_all(slam, ctx, inp, F, how):
    d = make_dev(slam, ctx, inp, F)
    args = [on_dev(inp, d, n) for n in ("scans", "motion", "noise", "u0")]
    if how == "run":
        d.run(*args)
    else:
        for s in range(STEP["scans"]):
            d.step(*(a[s] for a in args))                                      # back to back, no host synchronise between them
            if how == "synced":
                d.results()
    out = d.results()
    out["pass"], out["hit"] = get_counters(d.grid, ctx)
    if how == "run":
        assert np.array_equal(out["est_hist"][-1], out["est"]) and np.array_equal(out["moved_hist"][-1], out["moved"])
        assert d.trajectory.shape == (STEP["scans"], F, 3)
    return out


KEYS = ("poses", "acc", "est", "info", "moved", "ancestors", "settled", "map_src", "copied", "cost", "used", "pass", "hit")


def test_run_is_the_same_steps_and_a_filter_does_not_depend_on_its_batch(slam, ctx, syn):
    inp = step_inputs(syn)
    a, b, c = (run_all(slam, ctx, inp, 2, how) for how in ("run", "steps", "synced"))
    for name in KEYS:
        assert same_bits(a[name], b[name]) and same_bits(a[name], c[name]), name
    assert a["moved_hist"][:, 0].max() > 0 and not a["moved_hist"][:, 1].any()
    alone = run_all(slam, ctx, step_inputs(syn, F=1), 1, "run")
    P = STEP["P"]
    for name in ("poses", "acc", "est", "info", "moved", "ancestors", "settled", "cost", "used", "est_hist", "info_hist", "moved_hist"):
        full = a[name][:, :1] if name.endswith("hist") else a[name][:1]
        assert same_bits(np.ascontiguousarray(full), alone[name]), name
    assert np.array_equal(a["pass"][:P], alone["pass"]) and np.array_equal(a["hit"][:P], alone["hit"])
    assert np.array_equal(a["copied"][:P], alone["copied"])


def test_gridslam_class_against_the_device_class(slam, ctx, syn):
    k = STEP
    inp = step_inputs(syn, F=1)
    dev = run_all(slam, ctx, inp, 1, "run")
    gs = slam.GridSLAM(k["xw"], k["yw"], k["reso"], k["P"], np.random.default_rng(0), context=ctx)
    gs.init(inp["start"])
    for s in range(k["scans"]):
        pose, ess = gs.update(inp["scans"][s, 0], -3.14159, 3.14159, u=inp["motion"][s, 0], noise=inp["noise"][s, 0], u0=inp["u0"][s, 0])
        assert np.array_equal(pose, dev["est_hist"][s, 0, :3]) and ess == dev["est_hist"][s, 0, 3]
        assert gs.moved == dev["moved_hist"][s, 0]
    assert same_bits(gs.particles, dev["poses"][0]) and np.array_equal(gs.acc, dev["acc"][0])
    gp, gh = get_counters(gs.grid, ctx)
    assert np.array_equal(gp, dev["pass"]) and np.array_equal(gh, dev["hit"])
    assert np.array_equal(gs.pmap, G.pmap_of(gp, gh)[gs.best])


# ------------------------------------------------------------------ it maps better than odometry
def test_it_maps_better_than_odometry(slam, ctx, syn):
    """The case of test_gridslam_ref.py (bias (0.015 m, 0, 0.01 rad) per step, dead reckoning 0.2260 m off at the end; the
    restatement's best particle ends 0.0362 m / 0.0144 rad from the truth) through DeviceGridSLAM and through GridSLAM."""
    import torch
    k, case = G.SLAM, G.slam_case(syn)
    dead = X.pose_error(case["dead"][-1], case["true"][-1])
    assert dead[0] >= 4 * 0.05
    S, P = k["scans"], k["P"]
    motion = np.concatenate([np.zeros((1, 3)), case["motion"]])[:, None]
    noise = np.concatenate([np.zeros((1, P, 3)), case["noise"]])[:, None]
    d = slam.DeviceGridSLAM(1, P, k["xw"], k["yw"], 0.05, cos_t=case["cos_t"], sin_t=case["sin_t"], context=ctx, table=case["table"],
                            cap=k["cap"], max_range=k["max_range"], ess_frac=k["ess_frac"])
    d.set_particles(case["true"][0])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d.dev)
    d.run(up(case["scans"][:, None]), up(motion), up(noise), up(case["u0"][:, None]))
    out = d.results()
    _, best = d.best(0)
    gs = slam.GridSLAM(k["xw"], k["yw"], 0.05, P, np.random.default_rng(0), cap=k["cap"], max_range=k["max_range"],
                       sigma_cells=k["sigma_cells"], ess_frac=k["ess_frac"], context=ctx)
    gs.init(case["true"][0])
    for s in range(S):
        gs.update(case["scans"][s], -3.14159, 3.14159, u=motion[s, 0], noise=noise[s, 0], u0=case["u0"][s])
    for name, pose, moved in (("device", best, out["moved_hist"][:, 0]), ("numpy", gs.best_pose, None)):
        err = X.pose_error(pose, case["true"][-1])
        print(name, "best particle", err, "dead reckoning", dead)
        assert err[0] <= G.SLAM_BOUND[0] and err[1] <= G.SLAM_BOUND[1]
        assert err[0] < 0.5 * dead[0]
        if moved is not None:
            assert np.any((out["info_hist"][:, 0, 2] == 1) & (moved > 0))
    assert same_bits(gs.particles, out["poses"][0])
    pm = d.best_map(0)
    assert (pm == 100).sum() > 100 and (pm == 0).sum() > 1000
