"""The batched W9 node (``slam_loc_replay``: DeviceLocalizationReplay / loc_replay_host) against the reference's
own run of the node (tests/golden/g5_map_observation.npz, ``node9_*``), the CPU oracle chain (tests/loc_ref.py)
and the host class ``Localization.laserCallback`` on the same numbers.

Bars: iteration counts and statuses exact; poses, transforms and P within 1e-9; the target
points of every step bit-equal to ``slam_virtual_scan`` + ``slam_scan_to_points_f64`` at that step's xEst; a
trajectory alone and in a batch bit-equal."""
import types

import numpy as np
import pytest

import loc_ref
from conftest import load_golden, pkg
from loc_cases import AMAX, AMIN, GUARD, make_stream, pick, same_bits
from oracle import oracle_np as on

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def slam():
    p = pkg()
    p._abi.default_context()
    return p


@pytest.fixture(scope="module")
def g5():
    return load_golden("g5_map_observation.npz")


@pytest.fixture(scope="module")
def wall(g5):
    return np.ascontiguousarray(g5["obs_wall"])


def scan_msg(slam, ranges, n):
    return slam.LaserScan(ranges=tuple(float(v) for v in ranges), angle_min=AMIN, angle_max=AMAX,
                          angle_increment=(AMAX - AMIN) / (n - 1))


def host_class_run(slam, ranges, obstacle, pose0):
    """Localization.laserCallback fed every scan as a processed one -> per-step lists; stops where it raises."""
    loc = slam.Localization()
    loc.obstacle = np.asarray(obstacle, dtype=np.float64)
    loc.xEst, loc.xOdom = [float(v) for v in pose0], [float(v) for v in pose0]
    out = {"xest": [], "xodom": [], "P": [np.eye(3)], "raised_at": None}
    for s, r in enumerate(ranges):
        loc.laser_count = 5
        try:
            loc.laserCallback(scan_msg(slam, r, len(r)))
        except np.linalg.LinAlgError:
            out["raised_at"] = s
            break
        out["xest"].append(np.array(loc.xEst, dtype=float))
        out["xodom"].append(np.array(loc.xOdom, dtype=float))
        out["P"].append(np.array(loc.PEst))
    return out


def operator_target_points(slam, obstacle, pose, n, angle_increment=None):
    """slam_virtual_scan + slam_scan_to_points_f64 at one pose -> [2, n]; ``angle_increment``: the caller's own."""
    loc = slam.Localization()
    loc.obstacle = np.asarray(obstacle, dtype=np.float64).reshape(2, -1)
    msg = types.SimpleNamespace(ranges=[0.0] * n, angle_min=AMIN, angle_max=AMAX,
                                angle_increment=(AMAX - AMIN) / (n - 1) if angle_increment is None else angle_increment)
    r = loc.virtual_ranges(msg, np.asarray(pose, dtype=np.float64).reshape(1, 3))[0]
    return loc.laserToNumpy(types.SimpleNamespace(ranges=r, angle_min=AMIN, angle_max=AMAX))[:2], r


def check_targets(slam, o, maps, map_of_traj, pose0, n, angle_increment=None):
    """Every step's target points == the existing operators at the xEst the step started from (bit for bit)."""
    L, n_scan = o["xest"].shape[:2]
    for l in range(L):
        for s in range(n_scan):
            if s and not np.all(np.isfinite(o["xest"][l, s - 1])):
                break
            pose = pose0[l] if s == 0 else o["xest"][l, s - 1]
            want, _ = operator_target_points(slam, maps[map_of_traj[l]], pose, n, angle_increment)
            assert np.array_equal(o["tar_pts"][l, s], want), (l, s)


# ---- 1. the reference's own run -----------------------------------------------------------------

def test_reference_golden(slam, g5, wall):
    r = g5["node9_ranges"][g5["node9_steps"]]
    assert r.shape == (6, 120)
    o = slam.loc_replay_host(r, AMIN, AMAX, wall)
    assert o["status"].tolist() == [slam.loc_replay.LOC_OK]
    assert np.max(np.abs(o["xest"][0] - g5["node9_xest"])) < 1e-9
    assert np.max(np.abs(o["xodom"][0] - g5["node9_xodom"])) < 1e-9
    assert np.max(np.abs(o["P"][0] - g5["node9_P"])) < 1e-9


# ---- 2. the CPU oracle chain ----------------------------------------------------------------------

@pytest.mark.parametrize("n,seed", [(120, 2), (120, 4), (361, 2), (361, 4)])
def test_against_oracle_chain(slam, syn, wall, n, seed):
    r, p0 = make_stream(syn, seed, n)
    ref, worst = loc_ref.stable(r, wall, AMIN, AMAX, p0)
    print("n %d seed %d: worst deviation of the nudged oracle runs %.3e" % (n, seed, worst))
    assert worst < 1e-10                                   # the inputs sit away from the chain's discontinuities
    o = slam.loc_replay_host(r, AMIN, AMAX, wall, pose0=p0)
    assert o["status"].tolist() == [0]
    assert o["iters_obs"][0].tolist() == ref["iters_obs"].tolist()
    for k in ("xest", "xodom", "P", "T_obs", "T_odom"):
        d = float(np.max(np.abs(o[k][0] - ref[k])))
        print("  %s: %.3e" % (k, d))
        assert d < 1e-9, k


# ---- 3. the host class ----------------------------------------------------------------------------

def test_against_host_class_streams_and_maps(slam, syn, wall):
    n = 120
    streams = [make_stream(syn, seed, n, steps=6) for seed in (2, 4, 7)]
    r = np.stack([s[0] for s in streams])
    p0 = np.stack([s[1] for s in streams])
    maps = [wall, np.ascontiguousarray(wall[:, ::2])]
    mot = [0, 1, 0]
    o = slam.loc_replay_host(r, AMIN, AMAX, maps, pose0=p0, map_of_traj=mot, target_points=True)
    assert o["status"].tolist() == [0, 0, 0]
    for l in range(3):
        h = host_class_run(slam, r[l], maps[mot[l]], p0[l])
        assert h["raised_at"] is None
        assert np.max(np.abs(o["xest"][l] - np.array(h["xest"]))) < 1e-9, l
        assert np.max(np.abs(o["xodom"][l] - np.array(h["xodom"]))) < 1e-9, l
        assert np.max(np.abs(o["P"][l] - h["P"][-1])) < 1e-9, l
    # iteration counts of the map observation: the host class's third solve of every step
    for l in range(3):
        loc = slam.Localization()
        loc.obstacle = maps[mot[l]]
        for s in range(6):
            loc.xEst = [float(v) for v in (p0[l] if s == 0 else o["xest"][l, s - 1])]
            msg = scan_msg(slam, r[l, s], n)
            _, it = loc.map_observation_batch(msg, loc._poses(loc.xEst), src_pc=loc.laserToNumpy(msg))
            assert o["iters_obs"][l, s] == it[0], (l, s)
    check_targets(slam, o, maps, mot, p0, n)


# ---- 4. batch invariance and routing --------------------------------------------------------------

def test_batch_invariance_permutation_and_maps(slam, syn, wall):
    n, L = 120, 257
    r, p = make_stream(syn, 2, n, steps=4)
    rng = np.random.default_rng(11)
    p0 = p + rng.uniform(-1, 1, size=(L, 3)) * np.array([0.3, 0.3, 0.1])
    sot = np.zeros(L, dtype=np.int32)
    o = slam.loc_replay_host(r, AMIN, AMAX, wall, pose0=p0, stream_of_traj=sot)
    assert np.all(o["status"] == 0) and np.all(np.isfinite(o["xest"]))
    for l in (0, 128, 256):
        solo = slam.loc_replay_host(r, AMIN, AMAX, wall, pose0=p0[l:l + 1])
        assert same_bits(solo, pick(o, slice(l, l + 1))), l
    perm = rng.permutation(L)
    op = slam.loc_replay_host(r, AMIN, AMAX, wall, pose0=p0[perm], stream_of_traj=sot)
    assert same_bits(op, pick(o, perm))
    # two maps in one call == two single-map calls
    maps = [wall, np.ascontiguousarray(wall[:, ::3])]
    mot = (np.arange(L) % 2).astype(np.int32)
    both = slam.loc_replay_host(r, AMIN, AMAX, maps, pose0=p0, stream_of_traj=sot, map_of_traj=mot)
    for m in (0, 1):
        idx = np.nonzero(mot == m)[0]
        one = slam.loc_replay_host(r, AMIN, AMAX, maps[m], pose0=p0[idx], stream_of_traj=sot[idx])
        assert same_bits(one, pick(both, idx)), m


# ---- 5. edges of the projection -------------------------------------------------------------------

@pytest.mark.parametrize("K", [0, 1, 255, 256, 257, 1025])
def test_obstacle_counts(slam, syn, wall, K):
    """Lists shorter and longer than a workgroup; with 1 025 obstacles into 120 bins the minimum wins in every bin."""
    n = 120
    r, p0 = make_stream(syn, 4, n, steps=2)
    rng = np.random.default_rng(K)
    obs = np.tile(wall, (1, 3))[:, :K] + (rng.uniform(-0.02, 0.02, size=(2, K)) if K else np.zeros((2, 0)))
    o = slam.loc_replay_host(r, AMIN, AMAX, obs, pose0=p0, target_points=True)
    ct, st = slam._abi.trig_tables(AMIN, AMAX, n)
    want = np.array(on.laser_estimation(obs, p0, AMIN, (AMAX - AMIN) / (n - 1), n))
    got = np.hypot(o["tar_pts"][0, 0, 0], o["tar_pts"][0, 0, 1])
    assert np.array_equal(np.abs(got - 100.0) < 1e-9, want == 100.0)            # same bins filled
    assert np.max(np.abs(got - want)) < 1e-9
    if K == 0:
        assert np.array_equal(o["tar_pts"][0, 0], np.vstack([ct * 100.0, st * 100.0]))
    check_targets(slam, o, [obs], [0], p0[None], n)


def test_empty_map_beside_a_full_one(slam, syn, wall):
    n = 120
    r, p0 = make_stream(syn, 4, n, steps=3)
    maps = [np.zeros((2, 0)), wall, np.zeros((2, 0))]
    o = slam.loc_replay_host(r, AMIN, AMAX, maps, pose0=np.stack([p0] * 3), stream_of_traj=[0, 0, 0], map_of_traj=[0, 1, 2],
                             target_points=True)
    ct, st = slam._abi.trig_tables(AMIN, AMAX, n)
    assert np.array_equal(o["tar_pts"][0, 0], np.vstack([ct * 100.0, st * 100.0]))
    assert same_bits(pick(o, slice(0, 1)), pick(o, slice(2, 3)))
    solo = slam.loc_replay_host(r, AMIN, AMAX, wall, pose0=p0)
    assert same_bits(solo, pick(o, slice(1, 2)))
    check_targets(slam, o, maps, [0, 1, 2], np.stack([p0] * 3), n)


def test_pose_on_an_obstacle_and_headings_of_several_turns(slam, syn, wall):
    """Distance 0 with atan2(0, 0); quotients far outside [0, n) on both sides: truncation toward zero, then wrap."""
    n = 16
    obs = np.array([[1.0, 2.0, -1.0, 200.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 0.0, 3.0]])
    p0 = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 7.0], [0.0, 0.0, -7.0], [0.0, 0.0, 40.0], [0.0, 0.0, -40.0], [1.0, 0.0, 0.3]])
    r = np.full((1, 1, n), 2.0, dtype=np.float32)
    o = slam.loc_replay_host(r, AMIN, AMAX, obs, pose0=p0, stream_of_traj=np.zeros(6, dtype=np.int32), target_points=True)
    inc = (AMAX - AMIN) / (n - 1)
    for l in range(6):
        want = on.laser_estimation(obs, p0[l], AMIN, inc, n)
        got = np.hypot(o["tar_pts"][l, 0, 0], o["tar_pts"][l, 0, 1])
        assert np.array_equal(np.abs(got - 100.0) < 1e-9, want == 100.0), l
        assert np.max(np.abs(got - want)) < 1e-9, l
    assert np.hypot(o["tar_pts"][0, 0, 0], o["tar_pts"][0, 0, 1]).min() == 0.0
    assert np.hypot(o["tar_pts"][5, 0, 0], o["tar_pts"][5, 0, 1]).min() == 0.0
    check_targets(slam, o, [obs], [0] * 6, p0, n)


def test_sizes_and_rejections(slam, syn, wall):
    # n = 4096 with one step, one trajectory (n_scan = 1 and L = 1 as well)
    n = 4096
    r, p0 = make_stream(syn, 4, n, steps=1)
    o = slam.loc_replay_host(r, AMIN, AMAX, wall, pose0=p0, target_points=True)
    assert o["xest"].shape == (1, 1, 3) and o["status"].tolist() == [0]
    check_targets(slam, o, [wall], [0], p0[None], n)
    h = host_class_run(slam, r, wall, p0)
    assert np.max(np.abs(o["xest"][0] - np.array(h["xest"]))) < 1e-9 and np.max(np.abs(o["P"][0] - h["P"][-1])) < 1e-9
    with pytest.raises(slam.SlamError, match="4096"):
        slam.loc_replay_host(np.ones((1, 1, 4097), dtype=np.float32), AMIN, AMAX, wall)
    # S != L without stream_of_traj
    r2 = np.ones((2, 2, 16), dtype=np.float32)
    with pytest.raises(slam.SlamError, match="S must equal L"):
        slam.loc_replay_host(r2, AMIN, AMAX, wall, pose0=np.zeros((3, 3)))
    with pytest.raises(slam.SlamError, match="out of range"):
        slam.loc_replay_host(r2, AMIN, AMAX, wall, stream_of_traj=[0, 2])
    with pytest.raises(slam.SlamError, match="out of range"):
        slam.loc_replay_host(r2, AMIN, AMAX, wall, map_of_traj=[0, 1])


# ---- 6. stopping ------------------------------------------------------------------------------------

def test_stopped_trajectory(slam, syn, wall):
    n = 120
    streams = [make_stream(syn, seed, n, steps=5) for seed in (2, 4, 7)]
    r = np.stack([s[0] for s in streams])
    p0 = np.stack([s[1] for s in streams])
    r[1, 2] = np.inf
    h = host_class_run(slam, r[1], wall, p0[1])
    assert h["raised_at"] == 2                                        # the host class raises LinAlgError at step 2
    o = slam.loc_replay_host(r, AMIN, AMAX, wall, pose0=p0)
    assert o["status"].tolist() == [0, slam.loc_replay.LOC_NONFINITE, 0]
    assert np.max(np.abs(o["xest"][1, :2] - np.array(h["xest"]))) < 1e-9
    assert np.max(np.abs(o["xodom"][1, :2] - np.array(h["xodom"]))) < 1e-9
    assert np.max(np.abs(o["P"][1] - h["P"][2])) < 1e-9               # the state before step 2
    for k in ("xest", "xodom", "T_obs", "T_odom"):
        assert np.all(np.isnan(o[k][1, 2:])) and np.all(np.isfinite(o[k][1, :2])), k
    assert o["iters_obs"][1, 2:].tolist() == [-1, -1, -1] and np.all(o["iters_obs"][1, :2] >= 1)
    for l in (0, 2):
        solo = slam.loc_replay_host(r[l], AMIN, AMAX, wall, pose0=p0[l])
        assert same_bits(solo, pick(o, slice(l, l + 1))), l


# ---- 7. device path -----------------------------------------------------------------------------------

def test_device_form_back_to_back_and_guard_bytes(slam, syn, wall):
    import torch
    n = 120
    ra, pa = make_stream(syn, 2, n, steps=5)
    rb, pb = make_stream(syn, 7, n, steps=4)
    rng = np.random.default_rng(5)
    pa = pa + rng.uniform(-0.1, 0.1, size=(5, 3))
    sota = np.zeros(5, dtype=np.int32)
    ctx = slam.Context(0, torch.cuda.current_stream().cuda_stream)
    a = slam.DeviceLocalizationReplay(ra, AMIN, AMAX, wall, pose0=pa, stream_of_traj=sota, context=ctx)
    b = slam.DeviceLocalizationReplay.from_localization(types.SimpleNamespace(obstacle=wall[:, ::2]), rb, AMIN, AMAX, pose0=pb,
                                                        context=ctx)
    a.run()
    b.run()                                                            # no host synchronise in between
    oa, ob = a.results(), b.results()
    assert same_bits(oa, slam.loc_replay_host(ra, AMIN, AMAX, wall, pose0=pa, stream_of_traj=sota))
    assert same_bits(ob, slam.loc_replay_host(rb, AMIN, AMAX, wall[:, ::2], pose0=pb))
    # the host form writes exactly its outputs: a guard line behind each stays as it was
    abi = slam._abi
    L, S, n_scan = 5, 1, 5
    sizes = {"xest": (L * n_scan * 3, np.float64), "xodom": (L * n_scan * 3, np.float64), "P": (L * 9, np.float64),
             "status": (L, np.int32), "T_obs": (L * n_scan * 9, np.float64), "iters_obs": (L * n_scan, np.int32),
             "T_odom": (L * n_scan * 9, np.float64), "tar_pts": (L * n_scan * 2 * n, np.float64)}
    bufs = {k: np.full(cnt * np.dtype(dt).itemsize + 64, GUARD, dtype=np.uint8) for k, (cnt, dt) in sizes.items()}
    ct, st = abi.trig_tables(AMIN, AMAX, n)
    r32 = np.ascontiguousarray(ra[None], dtype=np.float32)
    ox, oy = np.ascontiguousarray(wall[0]), np.ascontiguousarray(wall[1])
    off = np.array([0, wall.shape[1]], dtype=np.int64)
    p0 = np.ascontiguousarray(pa)
    abi.check(abi.lib().slam_loc_replay(
        abi.default_context().handle, abi.ptr(r32), S, n_scan, n, abi.ptr(sota), abi.ptr(ox), abi.ptr(oy), abi.ptr(off), 1, None,
        abi.ptr(p0), L, abi.ptr(ct), abi.ptr(st), AMIN, (AMAX - AMIN) / (n - 1), 30, 0.001,
        *[abi.ptr(bufs[k]) for k in ("xest", "xodom", "P", "status", "T_obs", "iters_obs", "T_odom", "tar_pts")]))
    for k, (cnt, dt) in sizes.items():
        nb = cnt * np.dtype(dt).itemsize
        assert np.all(bufs[k][nb:] == GUARD), k
        if k != "tar_pts":
            assert bufs[k][:nb].tobytes() == oa[k].tobytes(), k
