"""DWA local planner (k_dwa) at the bounds of its launch shape, against the NumPy oracle
(tests/dwa_ref.py): obstacle sets past one LDS tile (kDwaTile = 4 096), the scans form filling
that tile, windows wider than one 512-lane pass, planners past the kDwaMaxGroups = 2^20 grid
stride, a map-fed planner at real map size, and the small contracts of the device form.

The oracle is slow at thousands of obstacles (seconds per planner with the default window), so
the large-M cases use a 5 x 5 window and check a handful of planners each; what they stress is
the obstacle walk, which does not depend on the window size."""
import numpy as np
import pytest

import dwa_ref
from conftest import pkg
from test_gpu_dwa import check_against_oracle, random_batch

pytestmark = pytest.mark.gpu

TILE = 4096                  # kDwaTile
MAX_GROUPS = 1 << 20         # kDwaMaxGroups
RTS = [dwa_ref.RECTANGLE, dwa_ref.CIRCLE]


@pytest.fixture(scope="module")
def slam():
    return pkg()


def bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float64:
        return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))
    return np.array_equal(a, b)


def assert_same(r, q, rows=slice(None), q_rows=slice(None), keys=("u", "cost", "index", "counts", "costs", "traj")):
    """Bit-equal outputs; of `costs` only each row's nv * nw window samples (the rest is not written)."""
    for k in keys:
        if k not in r:
            continue
        a, b = r[k][rows], q[k][q_rows]
        if k == "costs":
            n = r["counts"][rows]
            keep = np.arange(a.shape[-1]) < (n[..., 0] * n[..., 1])[..., None]
            a, b = np.where(keep, a, 0.0), np.where(keep, b, 0.0)
        assert bits_equal(a, b), k


def to_np(out):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def far_fill(rng, n):
    """Obstacles 20-40 m away: past any trajectory's reach, never the nearest."""
    r, a = rng.uniform(20.0, 40.0, n), rng.uniform(-np.pi, np.pi, n)
    return np.stack([r * np.cos(a), r * np.sin(a)], 1)


def annulus(rng, n):
    """Obstacles 1.5-4 m away: the nearest in any tile, and collisions for the farthest-reaching samples."""
    r, a = rng.uniform(1.5, 4.0, n), rng.uniform(-np.pi, np.pi, n)
    return np.stack([r * np.cos(a), r * np.sin(a)], 1)


def ahead(x, c):
    """A point 0.1 m past the end of the fastest straight-on sample: some samples of the window
    collide with it and the rest pass it, for both robot types."""
    tr = dwa_ref.rollout(np.asarray(x, dtype=np.float64), 0.6, float(x[4]), c, dwa_ref.n_steps(c))
    return tr[-1, :2] + 0.1 * np.array([np.cos(tr[-1, 2]), np.sin(tr[-1, 2])])


# ---- 1. explicit obstacle lists past one tile --------------------------------------------

def tiled_config(rt, **over):
    # 25 rows: three 12-row register chunks, so every tile is re-staged per chunk
    return dwa_ref.default_config(robot_type=rt, predict_time=2.4, v_reso=0.04, yawrate_reso=0.07, **over)


def tiled_sets(rng, M, states, c):
    """One obstacle set per planner, each of which a wrong tile loop answers differently:
    0 random in an annulus (the nearest obstacle in any tile);
    1 only the last obstacle (the last, partial tile) within reach;
    2 a colliding obstacle only in tile 2 or 3, one near non-colliding obstacle in tile 1;
    3 a colliding obstacle in tile 1 and a NaN obstacle in the last tile."""
    later = min(M - 1, 2 * TILE + 3 if M > 2 * TILE else TILE + 7)
    ob = np.empty((4, M, 2))
    ob[0] = annulus(rng, M)
    for k in (1, 2, 3):
        ob[k] = far_fill(rng, M)
    ob[1, M - 1] = ahead(states[1], c)
    ob[2, 5] = (-1.0, 1.0)
    ob[2, later] = ahead(states[2], c)
    ob[3, 5] = ahead(states[3], c)
    ob[3, M - 1] = (np.nan, 0.5)
    return ob


@pytest.mark.parametrize("rt", RTS)
@pytest.mark.parametrize("M", [4095, 4096, 4097, 8192, 8193, 12300])
def test_obstacle_tiles_vs_oracle(slam, M, rt):
    rng = np.random.default_rng(M + 7 * rt)
    c = tiled_config(rt)
    assert slam.dwa.shape(c)[0] == 25
    states = np.zeros((4, 5))
    states[:, 3] = 0.5
    states[:, 4] = (0.1, 0.0, 0.2, -0.2)
    goals = rng.uniform(-3, 3, (4, 2))
    ob = tiled_sets(rng, M, states, c)
    r = slam.dwa_batch_host(states, goals, c, ob=ob, want_costs=True)
    for b in range(4):
        check_against_oracle(r, b, states[b], c, goals[b], ob[b])
    S = r["counts"][:, 0] * r["counts"][:, 1]
    costs = [r["costs"][b, :S[b]] for b in range(4)]
    # the inputs mean what they say: collisions and misses side by side, NaN wherever nothing collides
    for b in (0, 1, 2):
        assert 0 < np.sum(np.isinf(costs[b])) < S[b] and not np.any(np.isnan(costs[b])), b
    assert 0 < np.sum(np.isinf(costs[3])) < S[3] and np.all(np.isinf(costs[3]) | np.isnan(costs[3]))
    # the nearest obstacle of planner 1 is its last one: cost 1 / min r over it alone where nothing collides
    alone = dwa_ref.plan(states[1], c, goals[1], ob[1, M - 1:])["costs"]
    assert np.array_equal(np.isinf(costs[1]), np.isinf(alone))
    # one shared set: the same answers as that set given to every planner
    sh = slam.dwa_batch_host(states, goals, c, ob=ob[0], shared=True, want_costs=True)
    rep = slam.dwa_batch_host(states, goals, c, ob=np.repeat(ob[:1], 4, 0), want_costs=True)
    assert_same(sh, rep)
    assert_same(sh, r, 0, 0)


@pytest.mark.parametrize("rt", RTS)
def test_counts_straddle_the_tile_in_one_launch(slam, rt):
    """One- and multi-tile planners side by side; every obstacle past a planner's count is NaN,
    so reading one changes the answer."""
    rng = np.random.default_rng(40 + rt)
    c = dwa_ref.default_config(robot_type=rt, v_reso=0.04, yawrate_reso=0.07)
    M = 12300
    counts = np.array([4095, 4096, 4097, 8192, 8193, 12300, 100, 1, 4096 + 2048, 12299], np.int32)
    B = len(counts)
    states = np.zeros((B, 5))
    states[:, 3] = 0.5
    states[:, 4] = rng.uniform(-0.3, 0.3, B)
    goals = rng.uniform(-3, 3, (B, 2))
    ob = np.full((B, M, 2), np.nan)
    for b, n in enumerate(counts):
        ob[b, :n] = annulus(rng, n)
        ob[b, n - 1] = ahead(states[b], c)               # within reach, in the planner's last tile
    r = slam.dwa_batch_host(states, goals, c, ob=ob, counts=counts, want_costs=True)
    for b in range(B):
        want = check_against_oracle(r, b, states[b], c, goals[b], ob[b, :counts[b]])
        assert not np.any(np.isnan(want["costs"])) and np.any(np.isinf(want["costs"])), b


# ---- 2. scans form at its bound ----------------------------------------------------------

@pytest.mark.parametrize("rt", RTS)
def test_scans_fill_one_tile(slam, rt):
    """4 095 beams, all below the threshold: the sentinel and every beam fill the 4 096-obstacle
    tile (64 KB of LDS) exactly."""
    rng = np.random.default_rng(50 + rt)
    n, B = 4095, 4
    c = dwa_ref.default_config(robot_type=rt, v_reso=0.04, yawrate_reso=0.07)
    thr = c["max_speed"] * c["predict_time"]
    am, inc = -np.pi, 2 * np.pi / n
    scans = rng.uniform(0.75, 1.55, (B, n)).astype(np.float32)
    assert np.all(scans < thr)
    states = np.zeros((B, 5))
    states[:, 3] = rng.uniform(0.0, 0.3, B)              # slow: some samples clear of the ring
    states[:, 4] = rng.uniform(-0.5, 0.5, B)
    goals = rng.uniform(-3, 3, (B, 2))
    r = slam.dwa_batch_host(states, goals, c, scans=scans, angle_min=am, angle_increment=inc, want_costs=True)
    for b in range(B):
        ob = dwa_ref.scan_obstacles(scans[b], am, inc, thr)
        assert len(ob) == TILE
        check_against_oracle(r, b, states[b], c, goals[b], ob)
    sh = slam.dwa_batch_host(states, goals, c, scans=scans[1], shared=True, angle_min=am, angle_increment=inc,
                             want_costs=True)
    rep = slam.dwa_batch_host(states, goals, c, scans=np.repeat(scans[1:2], B, 0), angle_min=am, angle_increment=inc,
                              want_costs=True)
    assert_same(sh, rep)
    assert_same(sh, r, 1, 1)


# ---- 3. windows wider than one pass of 512 lanes -------------------------------------------

@pytest.mark.parametrize("rt", RTS)
def test_windows_wider_than_512_lanes(slam, rt):
    rng = np.random.default_rng(60 + rt)
    c = dwa_ref.default_config(robot_type=rt, v_reso=0.0025, yawrate_reso=0.0044)
    _, nvc, nwc = slam.dwa.shape(c)
    assert nvc * nwc > 12 * 512
    B, M = 3, 50
    states, goals, ob, counts = random_batch(rng, B, M)
    states[0, 3:] = (0.3, 0.1)
    ob[0, 0] = states[0, :2]                              # every sample collides: the last one wins
    counts[0] = max(counts[0], 1)
    r = slam.dwa_batch_host(states, goals, c, ob=ob, counts=counts, want_costs=True)
    assert r["counts"][0, 0] * r["counts"][0, 1] > 12 * 512
    for b in range(B):
        check_against_oracle(r, b, states[b], c, goals[b], ob[b, :counts[b]])
    assert r["index"][0] == r["counts"][0, 0] * r["counts"][0, 1] - 1 and np.isinf(r["cost"][0])


@pytest.mark.parametrize("rt", RTS)
@pytest.mark.parametrize("g", [0.1, -0.1, 0.0])
def test_window_near_2_20_samples(slam, g, rt):
    """About 10^6 samples, 2 000 lane passes.  With the goal and obstacle gains 0 and one far
    obstacle every cost is (0 + g * (max_speed - v)) + 0, exactly; the winner is the last sample
    for g >= 0 (ties to the larger index, across passes) and the last of the slowest row for
    g < 0 (an early pass beating every later one)."""
    c = dwa_ref.default_config(robot_type=rt, v_reso=0.0002, yawrate_reso=0.349e-3, to_goal_cost_gain=0.0,
                               obstacle_cost_gain=0.0, speed_cost_gain=g)
    _, nvc, nwc = slam.dwa.shape(c)
    assert nvc * nwc <= MAX_GROUPS
    x = np.array([0.0, 0.0, 0.0, 0.2, 0.0])
    dw = dwa_ref.dynamic_window(x, c)
    vs, ws = dwa_ref.arange(dw[0], dw[1], c["v_reso"]), dwa_ref.arange(dw[2], dw[3], c["yawrate_reso"])
    nv, nw = len(vs), len(ws)
    S = nv * nw
    assert min(nv, nw) >= 1000 and nv <= nvc and nw <= nwc
    r = slam.dwa_batch_host(x[None], np.array([[1.0, 2.0]]), c, ob=np.array([[[50.0, 50.0]]]), want_costs=True)
    assert tuple(r["counts"][0]) == (nv, nw)
    want = np.repeat((0.0 + g * (c["max_speed"] - vs)) + 0.0, nw)
    assert bits_equal(r["costs"][0, :S], want)
    win = nw - 1 if g < 0 else S - 1
    assert r["index"][0] == win and bits_equal(r["cost"][0], want[win])
    assert bits_equal(r["u"][0], np.array([vs[win // nw], ws[win % nw]]))
    if g == 0.0:
        assert np.all(r["costs"][0, :S] == 0.0)


# ---- 4. grid stride past 2^20 planners -----------------------------------------------------

def test_grid_stride_past_2_20_planners(slam):
    """Workgroup g plans g and g + 2^20 in turn: the second must see its own obstacles, count
    and state, not what the first left in LDS."""
    rng = np.random.default_rng(70)
    extra, K = 40, 8
    B = MAX_GROUPS + extra
    states, goals, _, _ = random_batch(rng, B, 1)
    ob = rng.uniform(-2.5, 2.5, (B, K, 2))
    counts = rng.integers(4, K + 1, B).astype(np.int32)
    hi = np.arange(MAX_GROUPS, B)
    lo = hi - MAX_GROUPS
    counts[hi] = 4 + (counts[lo] - 4 + rng.integers(1, K - 3, extra)) % (K - 3)
    assert np.all(counts[hi] != counts[lo])
    c = dwa_ref.default_config()
    r = slam.dwa_batch_host(states, goals, c, ob=ob, counts=counts)      # no costs: 2^20 rows of them
    spread = np.linspace(extra, MAX_GROUPS - 1, 12).astype(np.int64)
    idx = np.concatenate([hi, lo, spread])
    small = slam.dwa_batch_host(states[idx], goals[idx], c, ob=ob[idx], counts=counts[idx], want_costs=True)
    assert_same(r, small, idx, keys=("u", "cost", "index", "counts"))
    for j in list(range(extra + 6)) + list(range(2 * extra, len(idx))):   # every planner past 2^20, a spread below
        b = idx[j]
        check_against_oracle(small, j, states[b], c, goals[b], ob[b, :counts[b]])


# ---- 5. map-fed planning at real map size ------------------------------------------------

def test_map_fed_at_real_map_size(slam):
    """slam_map_obstacles_dev -> slam_dwa_dev on a 160 x 160 map of walls and an unknown strip:
    some 9 300 obstacles, three tiles, listed in atomic-append order."""
    torch = pytest.importorskip("torch")
    L = slam._abi.lib()
    ctx = slam.default_context()
    W = H = 160
    res, ox0, oy0 = 0.05, -4.0, -4.0
    rng = np.random.default_rng(80)
    grid = np.zeros((W, H), np.int8)                          # [x][y], as Mapping.pmap
    grid[[0, -1], :] = 100
    grid[:, [0, -1]] = 100
    grid[60:100, 110] = 100                                   # a wall 1.5 m ahead of the robots
    grid[:, 1:56] = -1                                        # unknown cells count as obstacles too
    xs, ys = rng.integers(50, 110, 400), rng.integers(60, 110, 400)
    far = np.hypot(xs - 80, ys - 80) >= 14                    # scattered cells, none on the start poses
    grid[xs[far], ys[far]] = 100
    oxs, oys = np.nonzero((grid > 20) | (grid < -0.5))
    host_ob = np.stack([oxs * res + ox0, oys * res + oy0], 1)
    assert len(host_ob) > 2 * TILE
    dev = torch.device("cuda", ctx.device)
    g = torch.from_numpy(grid.reshape(-1)).to(dev)
    cap = W * H
    obuf = torch.zeros(2 * cap, dtype=torch.float64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    slam._abi.check(L.slam_map_obstacles_dev(ctx.handle, g.data_ptr(), W, H, 0, res, ox0, oy0, obuf.data_ptr(),
                                             obuf.data_ptr() + 8 * cap, cap, cnt.data_ptr()))
    n = int(cnt.item())
    assert n == len(host_ob)
    perm = torch.from_numpy(rng.permutation(n)).to(dev)
    shuf = obuf.view(2, cap).clone()
    shuf[:, :n] = obuf.view(2, cap)[:, perm]
    B = 32
    states = np.zeros((B, 5))
    states[:, :2] = rng.uniform(-0.3, 0.3, (B, 2))
    states[:, 2] = rng.uniform(-np.pi, np.pi, B)
    states[:, 3] = rng.uniform(-0.3, 0.7, B)
    states[:, 4] = rng.uniform(-1.0, 1.0, B)
    goals = rng.uniform(-3, 3, (B, 2))
    st, go = torch.from_numpy(states).to(dev), torch.from_numpy(goals).to(dev)
    for rt in RTS:
        c = dwa_ref.default_config(robot_type=rt)
        dd = slam.DeviceDWA(c, ctx=ctx)
        r = to_np(dd.run(st, go, obuf.view(2, cap), counts=cnt, shared=True, want_costs=True, want_traj=True))
        q = to_np(dd.run(st, go, shuf, counts=cnt, shared=True, want_costs=True, want_traj=True))
        assert_same(r, q)
        assert np.any(np.isinf(r["costs"])) and np.any(np.isfinite(r["costs"]))
        for b in (rt, 2 + rt):
            check_against_oracle(r, b, states[b], c, goals[b], host_ob)


# ---- 6. small contracts -------------------------------------------------------------------

def test_device_counts_below_one_and_above_M(slam):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(90)
    M = TILE + 1
    c = tiled_config(dwa_ref.RECTANGLE)
    B = 5
    states = np.zeros((B, 5))
    states[:, 3] = 0.5
    states[:, 4] = rng.uniform(-0.3, 0.3, B)
    goals = rng.uniform(-3, 3, (B, 2))
    ob = np.empty((B, M, 2))
    for b in range(B):
        ob[b] = annulus(rng, M)
        ob[b, M - 1] = ahead(states[b], c)                # within reach, alone in tile 2
    dd = slam.DeviceDWA(c)
    st, go = torch.from_numpy(states).to(dd.dev), torch.from_numpy(goals).to(dd.dev)
    soa = torch.from_numpy(np.ascontiguousarray(np.swapaxes(ob, 1, 2))).to(dd.dev)
    k = torch.tensor([0, -3, M + 1, 1 << 30, M], dtype=torch.int32, device=dd.dev)
    r = to_np(dd.run(st, go, soa, counts=k, want_costs=True, want_traj=True))
    full = to_np(dd.run(st, go, soa, counts=torch.full((B,), M, dtype=torch.int32, device=dd.dev), want_costs=True,
                        want_traj=True))
    for b in (0, 1):                                      # a count < 1: nothing to plan against
        assert r["index"][b] == -1 and np.isposinf(r["cost"][b]), b
        assert np.array_equal(r["u"][b], [0.0, 0.0]) and np.array_equal(r["counts"][b], [0, 0]), b
        assert bits_equal(r["traj"][b, 0], states[b]) and np.all(np.isnan(r["traj"][b, 1:])), b
    assert_same(r, full, slice(2, 5), slice(2, 5))        # a count > M is M
    check_against_oracle(full, 2, states[2], c, goals[2], ob[2])


def test_costs_rows_shorter_than_window(slam):
    """s_cap below the window: samples s >= s_cap are not written, and nothing past B * s_cap."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(95)
    B, M, s_cap = 6, 300, 100
    states, goals, ob, counts = random_batch(rng, B, M)
    c = dwa_ref.default_config()
    dd = slam.DeviceDWA(c)
    st, go = torch.from_numpy(states).to(dd.dev), torch.from_numpy(goals).to(dd.dev)
    soa = torch.from_numpy(np.ascontiguousarray(np.swapaxes(ob, 1, 2))).to(dd.dev)
    k = torch.from_numpy(counts).to(dd.dev)
    full = to_np(dd.run(st, go, soa, counts=k, want_costs=True))
    assert np.all(full["counts"][:, 0] * full["counts"][:, 1] > s_cap)
    f = dict(dtype=torch.float64, device=dd.dev)
    u, cost = torch.empty((B, 2), **f), torch.empty(B, **f)
    idx, cnt = torch.empty(B, dtype=torch.int32, device=dd.dev), torch.empty((B, 2), dtype=torch.int32, device=dd.dev)
    buf = torch.full((B * s_cap + 333,), float("nan"), **f)
    p = slam._abi.ptr
    slam._abi.check(slam._abi.lib().slam_dwa_dev(dd.ctx.handle, p(st), p(go), p(soa), p(k), M, 0, p(dd.cfg), B, p(u),
                                                 p(cost), p(idx), p(cnt), p(buf), s_cap, None))
    r = to_np(dict(u=u, cost=cost, index=idx, counts=cnt, costs=buf))
    assert bits_equal(r["costs"][:B * s_cap].reshape(B, s_cap), full["costs"][:, :s_cap])
    assert np.all(np.isnan(r["costs"][B * s_cap:]))
    assert_same(r, full, keys=("u", "cost", "index", "counts"))


@pytest.mark.parametrize("pt,rows", [(1.0, 12), (1.1, 13), (2.3, 24), (2.4, 25)])
def test_rows_at_register_chunk_edges(slam, pt, rows):
    rt = dwa_ref.CIRCLE if rows % 2 else dwa_ref.RECTANGLE
    c = dwa_ref.default_config(robot_type=rt, predict_time=pt)
    assert slam.dwa.shape(c)[0] == rows
    rng = np.random.default_rng(rows)
    B = 4
    states, goals, _, _ = random_batch(rng, B, 1)
    ob = far_fill(rng, 30)
    ob[:4] = rng.uniform(0.6, 1.2, (4, 2)) * np.array([1.0, -1.0])
    r = slam.dwa_batch_host(states, goals, c, ob=np.repeat(ob[None], B, 0), want_costs=True, want_traj=True)
    assert r["traj"].shape == (B, rows, 5)
    compared = 0
    for b in range(B):
        want = check_against_oracle(r, b, states[b], c, goals[b], ob)
        assert len(want["traj"]) in (1, rows)
        if r["index"][b] == want["index"] >= 0:
            assert np.max(np.abs(r["traj"][b] - want["traj"])) < 1e-12, b
            compared += 1
    assert compared >= B - 1
