"""A* global planner on the MI355X (slam_astar, global_planner.py) against the reference's
recorded results (tests/golden/g12_astar.npz) and the NumPy oracle (tests/astar_ref.py)."""
import numpy as np
import pytest

import astar_ref
from conftest import load_golden, pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g12():
    return load_golden("g12_astar.npz")


@pytest.fixture(scope="module")
def slam():
    return pkg()


def map_of(g, k, key="maps"):
    return g[key][k, :g["map_h"][k], :g["map_w"][k]]


def padded_maps(g):
    """Every golden map in one [G][H][W] stack: 129-cell maps padded with 50 (neither obstacle nor free)."""
    H, W = int(g["map_h"].max()), int(g["map_w"].max())
    out = np.full((len(g["map_names"]), H, W), 50, np.int8)
    for k in range(len(out)):
        out[k, :g["map_h"][k], :g["map_w"][k]] = map_of(g, k)
    return out


def check_query(o, g, k, b=None, name=""):
    b = k if b is None else b
    assert o["status"][b] == g["status"][k], name
    assert o["expansions"][b] == g["expansions"][k], name
    L = int(g["path_len"][k])
    assert o["path_len"][b] == L, name
    np.testing.assert_array_equal(np.asarray(o["path"][b])[:L], g["paths"][k, :L], err_msg=name)


def test_golden_queries_one_call_over_every_map(g12, slam):
    maps = padded_maps(g12)
    o = slam.astar_host(maps, g12["starts"], g12["goals"], map_of_query=g12["map_of_query"], span=129, r=2,
                        path_cap=int(g12["path_len"].max()), want_inflated=True)
    for k, name in enumerate(g12["names"]):
        check_query(o, g12, k, name=str(name))
    for k in range(len(maps)):
        np.testing.assert_array_equal(o["inflated"][k, :g12["map_h"][k], :g12["map_w"][k]], map_of(g12, k, "inflated"))


def test_golden_queries_per_map_and_inflate_alone(g12, slam):
    for k in range(len(g12["map_names"])):
        m = map_of(g12, k)
        np.testing.assert_array_equal(slam.inflate_host(m), map_of(g12, k, "inflated"))
        sel = np.nonzero(g12["map_of_query"] == k)[0]
        o = slam.astar_host(m, g12["starts"][sel], g12["goals"][sel], path_cap=int(g12["path_len"].max()))
        for b, q in enumerate(sel):
            check_query(o, g12, q, b, str(g12["names"][q]))


def test_find_path_drop_in(g12, slam):
    for k, name in enumerate(g12["names"]):
        mi = g12["map_of_query"][k]
        m = np.array(map_of(g12, mi), dtype=object)          # map_callback's object array of ints
        start, goal = g12["starts"][k].tolist(), g12["goals"][k].tolist()
        fp = slam.find_path(m, start, goal)
        assert start == (g12["starts"][k] - 1).tolist() and goal == (g12["goals"][k] - 1).tolist(), name
        st = g12["status"][k]
        if st == astar_ref.NO_PATH:
            with pytest.raises(IndexError):
                fp.start_find()
        else:
            got = fp.start_find()
            if st == astar_ref.OK:
                L = g12["path_len"][k]
                assert got == g12["paths"][k, :L][::-1].tolist(), name       # goal -> start
            else:
                assert got == "None", name
        np.testing.assert_array_equal(np.asarray(m, dtype=np.int64), map_of(g12, mi, "inflated"), err_msg=str(name))


def test_global_planner_two_plans(g12, slam):
    published = []
    gp = slam.GlobalPlanner(publish=published.append)
    m = map_of(g12, 0)
    gp.map_callback(dict(data=m.reshape(-1), width=m.shape[1], height=m.shape[0],
                         resolution=float(g12["planner_resolution"]), origin=tuple(g12["planner_origin"]) + (0.0,)))
    gp.init_pose_callback(*g12["planner_start_xy"])
    own = []
    for k, (gx, gy) in enumerate(g12["planner_goals_xy"]):
        own.append(gp.goal_pose_callback(gx, gy))
        assert len(gp.current_path) == g12["planner_counts"][k]
        assert gp.start_map_point == g12["planner_start_map_point"][k].tolist()
        np.testing.assert_array_equal(gp.map, map_of(g12, 0, "inflated"))
    np.testing.assert_array_equal(np.array(gp.current_path), g12["planner_path_xy"])
    np.testing.assert_array_equal(np.concatenate(own), g12["planner_path_xy"])
    np.testing.assert_array_equal(published[-1], g12["planner_path_xy"])
    # plan(): this plan's own path, from a fresh start point
    p = gp.plan(g12["planner_start_xy"], g12["planner_goals_xy"][0])
    np.testing.assert_array_equal(p, g12["planner_path_xy"][:g12["planner_counts"][0]])


def test_device_astar_on_torch_tensors(g12, slam):
    import torch
    maps = padded_maps(g12)
    G, H, W = maps.shape
    da = slam.DeviceAStar(H, W, G=G, span=129, r=2)
    dev = da.dev
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
    tm, ts, tg, tq = t(maps), t(g12["starts"]), t(g12["goals"]), t(g12["map_of_query"])
    torch.cuda.synchronize()
    o = da.run(ts, tg, maps=tm, map_of_query=tq, path_cap=int(g12["path_len"].max()), want_inflated=True)
    infl = da.inflate(tm)
    da.ctx.synchronize()
    o = {k: v.cpu().numpy() for k, v in o.items()}
    for k, name in enumerate(g12["names"]):
        check_query(o, g12, k, name=str(name))
    np.testing.assert_array_equal(infl.cpu().numpy(), o["inflated"])


def random_pairs(imap, n, rng):
    free = np.argwhere(imap == 0)
    a = free[rng.integers(0, len(free), n)] + 1
    b = free[rng.integers(0, len(free), n)] + 1
    return a.astype(np.int32), b.astype(np.int32)


def test_ten_thousand_pairs_on_the_course_map(g12, slam):
    m = map_of(g12, 0)
    imap = map_of(g12, 0, "inflated").astype(np.int64)
    rng = np.random.default_rng(7)
    s, g = random_pairs(imap, 10000, rng)
    s[:50] = rng.integers(1, 130, (50, 2))                  # some starts on walls or inflated cells
    o = slam.astar_host(m, s, g, path_cap=512)
    for b in range(len(s)):
        r = astar_ref.plan(imap, s[b], g[b], path_cap=512)
        assert o["status"][b] == r["status"] and o["expansions"][b] == r["expansions"], b
        assert o["path_len"][b] == r["length"], b
        np.testing.assert_array_equal(o["path"][b, :r["length"]], r["path"], err_msg=str(b))
    assert np.sum(o["status"] == astar_ref.OK) > 9000


def test_g_maps_with_map_of_query(g12, slam):
    rng = np.random.default_rng(8)
    base = map_of(g12, 0)
    maps = np.stack([base] + [np.where(rng.random(base.shape) < 0.01, 100, base).astype(np.int8) for _ in range(5)])
    infl = [astar_ref.inflate(mm) for mm in maps]
    B = 600
    moq = rng.integers(0, len(maps), B).astype(np.int32)
    s, g = random_pairs(infl[0], B, rng)
    o = slam.astar_host(maps, s, g, map_of_query=moq, path_cap=512, want_inflated=True)
    for k in range(len(maps)):
        np.testing.assert_array_equal(o["inflated"][k], infl[k])
    for b in range(B):
        r = astar_ref.plan(infl[moq[b]], s[b], g[b])
        assert (o["status"][b], o["expansions"][b], o["path_len"][b]) == (r["status"], r["expansions"], r["length"]), b
        np.testing.assert_array_equal(o["path"][b, :r["length"]], r["path"])
    # one map per query without map_of_query (G == B)
    o2 = slam.astar_host(maps, s[:6], g[:6], path_cap=512)
    for b in range(6):
        r = astar_ref.plan(infl[b], s[b], g[b])
        assert (o2["status"][b], o2["expansions"][b], o2["path_len"][b]) == (r["status"], r["expansions"], r["length"])


def test_slam_live_pmap_device_to_device(slam):
    """A replay's live pmap (layout [x][y], 50 for unknown cells) planned on with span = min(H, W)."""
    import torch
    rep = slam.synthetic.make_replay(24, 120, seed=4)
    grid = slam.DeviceGrid(1, 200, 200, 10.0, 10.0, 10.0)
    slam.replay_host(rep.ranges, rep.angle_min, rep.angle_max, grid=grid)
    pmap = grid.read(0)["pmap"]                              # [x][y]
    rows = pmap.T.astype(np.int64)                           # row = y, column = x
    assert np.any(rows == 50) and np.any(rows == 0)
    imap = astar_ref.inflate(rows, span=200, r=2)
    rng = np.random.default_rng(9)
    s, g = random_pairs(imap, 256, rng)
    da = slam.DeviceAStar.from_grid(grid)
    assert (da.H, da.W, da.span, da.wire_layout) == (200, 200, 200, False)
    ts, tg = torch.from_numpy(s).to(da.dev), torch.from_numpy(g).to(da.dev)
    torch.cuda.synchronize()
    o = da.run(ts, tg, path_cap=1024, want_inflated=True)
    da.ctx.synchronize()
    o = {k: v.cpu().numpy() for k, v in o.items()}
    np.testing.assert_array_equal(o["inflated"][0], imap)
    for b in range(len(s)):
        r = astar_ref.plan(imap, s[b], g[b])
        assert (o["status"][b], o["expansions"][b], o["path_len"][b]) == (r["status"], r["expansions"], r["length"]), b
        np.testing.assert_array_equal(o["path"][b, :r["length"]], r["path"])
    assert np.sum(o["status"] == astar_ref.OK) > 100


def test_path_into_local_planner(g12, slam):
    """GlobalPlanner's path fed to LocalPlanner.pathCallback, then planOnce steps: the same as
    with the oracle's path."""
    m = map_of(g12, 0)
    res, org = float(g12["planner_resolution"]), tuple(g12["planner_origin"])
    gp = slam.GlobalPlanner()
    gp.map_callback(dict(data=m.reshape(-1), width=129, height=129, resolution=res, origin=org + (0.0,)))
    start_xy, goal_xy = g12["planner_start_xy"], g12["planner_goals_xy"][0]
    path_xy = gp.plan(start_xy, goal_xy)
    s0, g0 = gp.WorldTomap(*start_xy), gp.WorldTomap(*goal_xy)
    want = astar_ref.world_path(astar_ref.plan(astar_ref.inflate(m), s0, g0)["path"], res, org[0], org[1])
    np.testing.assert_array_equal(path_xy, want)
    runs = []
    for p in (path_xy, want):
        lp = slam.LocalPlanner()
        pose = (float(p[0, 0]), float(p[0, 1]), 0.3)
        lp.pathCallback(p, pose=pose)
        runs.append([lp.planOnce(pose) for _ in range(4)])
    assert runs[0] == runs[1]
    assert any(v != 0.0 for v in np.ravel(runs[0]))
