"""DWA local planner on the MI355X (slam_dwa / slam_dwa_scans, dwa.py, local_planner.py)
against the reference's recorded results (tests/golden/g11_dwa.npz) and the NumPy oracle
(tests/dwa_ref.py)."""
import ctypes as C
import math

import numpy as np
import pytest

import dwa_ref
from conftest import load_golden, pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g11():
    return load_golden("g11_dwa.npz")


@pytest.fixture(scope="module")
def slam():
    return pkg()


def cfg_of(row):
    return dict(zip(dwa_ref.FIELDS, (float(v) for v in row)))


def close_costs(got, want, rel=1e-12):
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(np.isposinf(got), np.isposinf(want))
    f = np.isfinite(want)
    assert np.all(np.abs(got[f] - want[f]) <= rel * np.maximum(np.abs(want[f]), 1.0))


def test_golden_cases_through_slam_dwa(g11, slam):
    for k, name in enumerate(g11["names"]):
        c = cfg_of(g11["configs"][k])
        ob = g11["ob"][k, :g11["ob_count"][k]]
        r = slam.dwa_batch_host(g11["states"][k][None], g11["goals"][k][None], c, ob=ob[None], want_costs=True,
                                want_traj=True)
        nv, nw = int(g11["nv"][k]), int(g11["nw"][k])
        assert tuple(r["counts"][0]) == (nv, nw), name
        assert r["index"][0] == g11["index"][k], name
        assert np.array_equal(r["u"][0], g11["u"][k]), name               # an arange value: bit-equal
        close_costs(r["costs"][0, :nv * nw], g11["costs"][k, :nv * nw])
        rows = int(g11["traj_rows"][k])
        if g11["index"][k] >= 0:
            assert np.max(np.abs(r["traj"][0] - g11["traj"][k, :rows])) < 1e-12, name
        else:
            assert np.array_equal(r["traj"][0, 0], g11["states"][k]) and np.all(np.isnan(r["traj"][0, 1:])), name
        # the scans form of the cases recorded from a scan
        if g11["has_scan"][k]:
            s = slam.dwa_batch_host(g11["states"][k][None], g11["goals"][k][None], c, scans=g11["scans"][k][None],
                                    angle_min=float(g11["angle_min"]), angle_increment=float(g11["angle_increment"]),
                                    want_costs=True)
            assert s["index"][0] == g11["index"][k] and np.array_equal(s["u"][0], g11["u"][k]), name
            close_costs(s["costs"][0, :nv * nw], g11["costs"][k, :nv * nw])


def test_edge_cases(g11, slam):
    names = [str(n) for n in g11["names"]]
    k = names.index("edge_own_cell")                      # every sample collides: the last one wins
    c = cfg_of(g11["configs"][k])
    r = slam.dwa_batch_host(g11["states"][k][None], g11["goals"][k][None], c, ob=g11["ob"][k, :2][None])
    assert r["index"][0] == g11["nv"][k] * g11["nw"][k] - 1 and np.isinf(r["cost"][0])
    for e in ("edge_nan_goal", "edge_empty_window", "edge_obgain0_all_hit"):
        k = names.index(e)
        c = cfg_of(g11["configs"][k])
        ob = g11["ob"][k, :g11["ob_count"][k]]
        u, tr = slam.dwa_control(list(g11["states"][k]), c, g11["goals"][k], ob)
        assert u == [0.0, 0.0] and tr.shape == (1, 5), e
        r = slam.dwa_batch_host(g11["states"][k][None], g11["goals"][k][None], c, ob=ob[None], want_costs=True)
        assert r["index"][0] == -1 and np.isinf(r["cost"][0]), e
        if e == "edge_obgain0_all_hit":                   # 0 * inf = NaN, and NaN never wins
            assert np.all(np.isnan(r["costs"][0, :r["counts"][0, 0] * r["counts"][0, 1]]))


def random_batch(rng, B, M_max):
    states = np.zeros((B, 5))
    states[:, 3] = rng.uniform(-0.6, 0.9, B)
    states[:, 4] = rng.uniform(-1.9, 1.9, B)
    goals = rng.uniform(-3, 3, (B, 2))
    counts = rng.integers(1, M_max + 1, B).astype(np.int32)
    ob = rng.uniform(-2.5, 2.5, (B, M_max, 2))
    return states, goals, ob, counts


def collision_margin(x, c, s, nw, ob):
    dw = dwa_ref.dynamic_window(x, c)
    v = dwa_ref.arange(dw[0], dw[1], c["v_reso"])[s // nw]
    w = dwa_ref.arange(dw[2], dw[3], c["yawrate_reso"])[s % nw]
    tr = dwa_ref.rollout(np.asarray(x, dtype=np.float64), float(v), float(w), c, dwa_ref.n_steps(c))
    dx = np.abs(tr[:, 0] - ob[:, 0][:, None])
    dy = np.abs(tr[:, 1] - ob[:, 1][:, None])
    if int(c["robot_type"]) == dwa_ref.RECTANGLE:
        return np.min(np.abs(np.maximum(dx - c["robot_length"] / 2, dy - c["robot_width"] / 2)))
    return np.min(np.abs(np.hypot(dx, dy) - c["robot_radius"]))


def check_against_oracle(r, b, x, c, goal, ob):
    want = dwa_ref.plan(x, c, goal, ob)
    nv, nw = want["nv"], want["nw"]
    assert tuple(r["counts"][b]) == (nv, nw)
    got = r["costs"][b, :nv * nw]
    w = want["costs"]
    # the collision pattern may differ only at a margin of 1e-12 (sqrt of the squared distance vs hypot)
    diff = np.isinf(got) != np.isinf(w)
    for s in np.flatnonzero(diff):
        m = collision_margin(x, c, s, nw, ob)
        assert m <= 1e-12, (b, s, m)
    keep = ~diff
    close_costs(got[keep], w[keep])
    if r["index"][b] != want["index"]:
        f = np.sort(w[np.isfinite(w)])
        assert len(f) > 1 and f[1] - f[0] <= 1e-12 * max(abs(f[0]), 1.0), (b, r["index"][b], want["index"])
    else:
        assert np.array_equal(r["u"][b], want["u"])
    return want


@pytest.mark.parametrize("rt", [dwa_ref.RECTANGLE, dwa_ref.CIRCLE])
def test_random_batches_vs_oracle(slam, rt):
    rng = np.random.default_rng(20 + rt)
    B = 256
    states, goals, ob, counts = random_batch(rng, B, 1081)
    configs = [dwa_ref.default_config(robot_type=rt),
               dwa_ref.default_config(robot_type=rt, predict_time=1.0, to_goal_cost_gain=0.5, robot_radius=0.3),
               dwa_ref.default_config(robot_type=rt, dt=0.05, v_reso=0.02, robot_width=0.5, robot_length=0.4)]
    for ci, c in enumerate(configs):
        r = slam.dwa_batch_host(states, goals, c, ob=ob, counts=counts, want_costs=True)
        for b in range(ci, B, 7):                         # a third of the planners per config: oracle time
            check_against_oracle(r, b, states[b], c, goals[b], ob[b, :counts[b]])


def test_scans_form_vs_oracle_preprocessing(slam, syn):
    rng = np.random.default_rng(5)
    B, n = 64, 360
    world = syn.World.room(0.45)
    poses = np.stack([rng.uniform(-1.6, 1.6, B), rng.uniform(-1.2, 1.2, B), rng.uniform(-np.pi, np.pi, B)], 1)
    scans = syn.scans_from_poses(world, poses, n, seed=5)
    scans[::3, ::17] = np.inf
    scans[1::3, 5::23] = np.nan
    am, inc = syn.ANGLE_MIN, (syn.ANGLE_MAX - syn.ANGLE_MIN) / (n - 1)
    states, goals, _, _ = random_batch(rng, B, 1)
    c = dwa_ref.default_config()
    r = slam.dwa_batch_host(states, goals, c, scans=scans, angle_min=am, angle_increment=inc, want_costs=True)
    for b in range(B):
        ob = dwa_ref.scan_obstacles(scans[b], am, inc, c["max_speed"] * c["predict_time"])
        check_against_oracle(r, b, states[b], c, goals[b], ob)
    # one shared scan
    rs = slam.dwa_batch_host(states, goals, c, scans=scans[0], shared=True, angle_min=am, angle_increment=inc)
    r0 = slam.dwa_batch_host(states, goals, c, scans=np.repeat(scans[:1], B, 0), angle_min=am, angle_increment=inc)
    assert np.array_equal(rs["index"], r0["index"]) and np.array_equal(rs["u"], r0["u"])


def test_batch_past_65535_planners(slam):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(9)
    B = 70000
    states, goals, _, _ = random_batch(rng, B, 1)
    ob = rng.uniform(-1.5, 1.5, (24, 2))
    c = dwa_ref.default_config()
    dd = slam.DeviceDWA(c)
    dev = dd.dev
    soa = torch.from_numpy(np.ascontiguousarray(ob.T)).to(dev)
    out = dd.run(torch.from_numpy(states).to(dev), torch.from_numpy(goals).to(dev), soa, shared=True, want_costs=True)
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in out.items()}
    for b in list(range(0, B, 997)) + [B - 1]:
        check_against_oracle(r, b, states[b], c, goals[b], ob)


def test_device_to_device_from_map_obstacles(slam):
    torch = pytest.importorskip("torch")
    L = slam._abi.lib()
    ctx = slam.default_context()
    W = H = 40
    rng = np.random.default_rng(2)
    grid = np.zeros((W, H), np.int8)
    grid[rng.integers(0, W, 60), rng.integers(0, H, 60)] = 100
    grid[:3, :] = -1                                          # unknown cells count as obstacles too
    dev = torch.device("cuda", ctx.device)
    g = torch.from_numpy(grid.reshape(-1)).to(dev)
    cap = W * H
    obuf = torch.zeros(2 * cap, dtype=torch.float64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    res, ox0, oy0 = 0.1, -2.0, -2.0
    slam._abi.check(L.slam_map_obstacles_dev(ctx.handle, g.data_ptr(), W, H, 0, res, ox0, oy0, obuf.data_ptr(),
                                             obuf.data_ptr() + 8 * cap, cap, cnt.data_ptr()))
    B = 32
    states, goals, _, _ = random_batch(rng, B, 1)
    c = dwa_ref.default_config(robot_type=dwa_ref.CIRCLE)
    dd = slam.DeviceDWA(c, ctx=ctx)
    out = dd.run(torch.from_numpy(states).to(dev), torch.from_numpy(goals).to(dev), obuf.view(2, cap), counts=cnt,
                 shared=True, want_costs=True)
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in out.items()}
    xs, ys = np.nonzero((grid > 20) | (grid < -0.5))
    ob = np.stack([xs * res + ox0, ys * res + oy0], 1)
    assert int(cnt.item()) == len(ob)
    for b in range(B):
        check_against_oracle(r, b, states[b], c, goals[b], ob)


def test_dwa_control_drop_in_and_config(slam, g11):
    d = slam.dwa
    c = d.Config()
    assert (c.max_speed, c.min_speed, c.max_accel, c.dt, c.predict_time, c.robot_type) == (0.8, -0.5, 1, 0.1, 2, d.RobotType.rectangle)
    assert c.v_reso == 1 * 0.1 / 10.0 and c.yawrate_reso == (100.0 * math.pi / 180.0) * 0.1 / 10.0
    with pytest.raises(TypeError, match="robot_type must be an instance of RobotType"):
        c.robot_type = 1
    assert d.calc_dynamic_window([0, 0, 0, 0.75, -1.7], c) == dwa_ref.dynamic_window([0, 0, 0, 0.75, -1.7], dwa_ref.default_config())
    names = [str(n) for n in g11["names"]]
    k = names.index("scan_rt1_s1_g0")
    u, tr = d.dwa_control(list(g11["states"][k]), c, g11["goals"][k], g11["ob"][k, :g11["ob_count"][k]])
    assert isinstance(u, list) and tr.shape == (21, 5)
    assert u == list(g11["u"][k])
    assert np.max(np.abs(tr - g11["traj"][k, :21])) < 1e-12


def test_local_planner_sequence_matches_oracle(slam, syn):
    world = syn.World.room(0.45)
    n = 360
    am, inc = syn.ANGLE_MIN, (syn.ANGLE_MAX - syn.ANGLE_MIN) / (n - 1)
    t = np.linspace(0, 1, 40)
    path = np.stack([-1.8 + 3.6 * t, 0.9 * np.sin(3 * t)], 1)
    rng = np.random.default_rng(8)
    poses = np.stack([path[:, 0][np.linspace(0, 39, 50).astype(int)] + rng.normal(0, 0.05, 50),
                      path[:, 1][np.linspace(0, 39, 50).astype(int)] + rng.normal(0, 0.05, 50),
                      rng.uniform(-0.4, 0.4, 50)], 1)
    scans = syn.scans_from_poses(world, poses, n, seed=8)
    sent = []
    lp = slam.LocalPlanner(publish=lambda vx, vw: sent.append((vx, vw)))
    ref = dwa_ref.LocalPlannerRef()
    lp.pathCallback(path, pose=poses[0])
    ref.path_callback(path, pose=poses[0])
    for i in range(50):
        lp.laserCallback(syn.LaserScan(ranges=tuple(float(v) for v in scans[i]), angle_min=am, angle_increment=inc))
        ref.laser_callback(scans[i], am, inc)
        got = lp.planOnce(poses[i])
        want = ref.plan_once(poses[i])
        assert abs(got[0] - want[0]) <= 1e-12 and abs(got[1] - want[1]) <= 1e-12, (i, got, want)
        assert lp.goal_index == ref.goal_index
    assert len(sent) == 50 and sent[-1] == (lp.vx, lp.vw)


def test_invalid_arguments_are_rejected(slam):
    L = slam._abi.lib()
    ctx = slam.default_context()
    ERR = slam._abi.ERR_INVALID
    x = np.zeros(5)
    g = np.ones(2)
    ob = np.array([1.0, 1.0])
    cfg = slam.dwa.config_array(dwa_ref.default_config())
    u, cost, idx = np.empty(2), np.empty(1), np.empty(1, np.int32)
    p = slam._abi.ptr

    def call(cfg=cfg, ob=ob, counts=None, M=1, B=1, states=x, u_=u):
        return L.slam_dwa(ctx.handle, p(states), p(g), p(ob), p(counts), M, 0, p(cfg), B, p(u_), p(cost), p(idx),
                          None, None, 0, None)

    assert call() == 0
    for field, bad in (("dt", 0.0), ("v_reso", -0.01), ("yawrate_reso", 0.0), ("robot_type", 2.0),
                       ("predict_time", -1.0), ("dt", float("nan")), ("v_reso", 1e-9)):
        c2 = cfg.copy()
        c2[dwa_ref.FIELDS.index(field)] = bad
        assert call(cfg=c2) == ERR, field
    assert call(M=0) == ERR
    assert call(counts=np.array([0], np.int32)) == ERR
    assert call(counts=np.array([2], np.int32)) == ERR
    assert call(B=0) == ERR
    assert call(states=None) == ERR
    assert call(u_=None) == ERR
    assert L.slam_dwa_scans(ctx.handle, p(x), p(g), p(np.zeros(4096, np.float32)), 4096, 0, p(np.zeros(4096)),
                            p(np.zeros(4096)), 1.6, p(cfg), 1, p(u), p(cost), p(idx), None, None, 0, None) == ERR
    rows, nv, nw = C.c_int(), C.c_int(), C.c_int()
    assert L.slam_dwa_shape(p(cfg), C.byref(rows), C.byref(nv), C.byref(nw)) == 0 and rows.value == 21
    with pytest.raises(slam.SlamError):
        c = slam.dwa.Config()
        c.dt = 0.0
        slam.dwa_control([0, 0, 0, 0, 0], c, [1, 0], [[1.0, 1.0]])
