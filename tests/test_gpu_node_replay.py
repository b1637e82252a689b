"""The landmark EKF-SLAM node on the device - slam_landmarks, slam_ekf_lm, slam_node_replay - against the
reference's own vectors (tests/golden/g7_w12_node.npz) and against the host classes Extraction, EKF and
SLAM_EKF(landmarks=True), which test_host_w12_node.py and test_gpu_w12_node.py pin to the same file.
Counts, ids, kept indices, iteration counts, statuses and maps are exact, landmark means bit-equal,
observation rows within 1e-12, states and covariances within 1e-9."""
import numpy as np
import pytest

from conftest import load_golden, pkg

pytestmark = pytest.mark.gpu
AMIN, AMAX = -3.14159, 3.14159
POLES = ((1.5, 1.0), (-1.8, -0.9), (0.5, -2.0), (-2.5, 1.5))


@pytest.fixture(scope="module")
def slam():
    p = pkg()
    p._abi.default_context()
    return p


@pytest.fixture(scope="module")
def g7():
    return load_golden("g7_w12_node.npz")


def host_node(slam, scans):
    """SLAM_EKF(landmarks=True) fed `scans` one message each (the decimation counter is set so that every
    message is the fifth): kept scan numbers, xEst[:3] and landmark count after every kept step, final state, map."""
    node = slam.SLAM_EKF(landmarks=True)
    kept, xest, nlm, raised = [], [], [], False
    for k, r in enumerate(scans):
        node.laser_count = 4
        before, x0, P0 = node._prev_ranges, node.xEst.copy(), node.PEst.copy()
        try:
            node.laserCallback(slam.LaserScan(ranges=tuple(float(v) for v in r), angle_min=AMIN, angle_max=AMAX))
        except ValueError:                        # ekf_lm.py:37-38 with its stale n1: the node dies here, before its map moves
            node.xEst, node.PEst, raised = x0, P0, True
            kept.append(k)
            break
        if node._prev_ranges is not before:
            kept.append(k)
            if k:
                xest.append(node.xEst[:3, 0].copy())
                nlm.append((len(node.xEst) - 3) // 2)
    return {"kept": kept, "xest": np.array(xest).reshape(-1, 3), "nlm": nlm, "x": node.xEst[:, 0].copy(),
            "P": node.PEst.copy(), "pmap": node.mapping.pmap.astype(np.int8), "raised": raised}


def assert_matches_host(out, l, ref, pmap=None):
    c, done = len(ref["kept"]), len(ref["nlm"])
    assert out["kept"][l, :c].tolist() == ref["kept"]
    if ref["raised"] or ref.get("stop"):          # the device stops where the reference raises, with the state before; "stop":
        assert out["status"][l] == (ref.get("stop") or 1) and out["kept_count"][l] >= c      # on a cap, `ref` being the scans before
    else:
        assert out["status"][l] == 0 and out["kept_count"][l] == c and np.all(out["kept"][l, c:] == -1)
    assert out["nlm"][l, :done].tolist() == ref["nlm"] and np.all(out["nlm"][l, done:] == -1)
    if done:
        assert np.max(np.abs(out["xest"][l, :done] - ref["xest"])) < 1e-9
    assert np.all(np.isnan(out["xest"][l, done:]))
    n = len(ref["x"])
    assert np.max(np.abs(out["x"][l, :n] - ref["x"])) < 1e-9 and np.all(out["x"][l, n:] == 0)
    assert np.max(np.abs(out["P"][l, :n, :n] - ref["P"])) < 1e-9
    assert np.all(out["P"][l, n:, :] == 0) and np.all(out["P"][l, :, n:] == 0)
    if pmap is not None:
        assert np.array_equal(pmap, ref["pmap"])


# ---- golden, through the new path ----------------------------------------------------------

def test_landmarks_golden(slam, g7):
    offs = g7["ext_offsets"]
    ranges = np.concatenate([g7["ext_ranges"], g7["ext_empty_ranges"]])
    out = slam.landmarks_host(ranges, AMIN, AMAX, lm_cap=8)
    k = len(offs) - 1
    assert out["count"].tolist() == np.diff(offs).tolist() + [0] * len(g7["ext_empty_ranges"])
    assert not out["overflow"].any() and 3 <= out["count"][:k].min() and out["count"][:k].max() <= 4
    for s in range(k):
        a, b = offs[s], offs[s + 1]
        assert out["ids"][s, :b - a].tolist() == g7["ext_id"][a:b].tolist() and np.all(out["ids"][s, b - a:] == -1)
        assert np.array_equal(out["means"][s, :b - a, 0], g7["ext_x"][a:b])          # same sums in the same order
        assert np.array_equal(out["means"][s, :b - a, 1], g7["ext_y"][a:b])
        assert np.max(np.abs(out["z"][s, :b - a] - g7["ext_z"][a:b, :2])) < 1e-12


def test_ekf_golden_after_every_step(slam, g7):
    """Trajectory t runs the first t + 1 of the 14 golden steps, so every intermediate state is an output."""
    zo, n_steps = g7["ekf_z_offsets"], len(g7["ekf_sizes"])
    u = g7["ekf_u"].reshape(n_steps, 3)
    z = [g7["ekf_z"][zo[t]:zo[t + 1]] for t in range(n_steps)]
    out = slam.ekf_lm_host([u[:t + 1] for t in range(n_steps)], [z[:t + 1] for t in range(n_steps)], max_lm=8)
    assert not out["status"].any()
    for t in range(n_steps):
        n = int(g7["ekf_sizes"][t])
        assert 3 + 2 * out["nlm"][t, t] == n and np.all(out["nlm"][t, t + 1:] == -1), t
        assert (3 + 2 * out["nlm"][n_steps - 1, t]) == n
        assert np.max(np.abs(out["x"][t, :n] - g7["ekf_x"][t][:n])) < 1e-9, t
        assert np.max(np.abs(out["P"][t, :n, :n] - g7["ekf_P"][t][:n, :n])) < 1e-9, t
        assert np.all(out["x"][t, n:] == 0) and np.all(out["P"][t, n:] == 0) and np.all(out["P"][t, :, n:] == 0)


def test_node_golden(slam, g7):
    scans = g7["node_ranges"][4::5]
    assert scans.shape[0] == 13
    grid = slam.DeviceGrid(1, 200, 200, 10.0, 10.0, 10.0)
    out = slam.node_replay_host(scans, AMIN, AMAX, grid=grid, max_lm=8)
    assert out["kept_count"][0] == 13 and out["kept"][0].tolist() == list(range(13)) and out["status"][0] == 0
    assert out["nlm"][0].tolist() == g7["node_nlm"].tolist() and out["nlm"][0, -1] == 5
    assert np.max(np.abs(out["xest"][0] - g7["node_xest"])) < 1e-9
    n = len(g7["node_final_x"])
    assert np.max(np.abs(out["x"][0, :n] - g7["node_final_x"])) < 1e-9
    assert np.max(np.abs(out["P"][0, :n, :n] - g7["node_final_P"])) < 1e-9
    assert np.array_equal(grid.read(0)["pmap"], g7["node_pmap"])


def test_device_form_equals_host_form(slam, g7):
    scans = g7["node_ranges"][4::5]
    rep = slam.DeviceNodeReplay(scans, AMIN, AMAX, max_lm=8)
    grid = rep.make_grid(1, 200, 200, 0.1)
    rep.run()
    rep.run()                                     # the second pass starts its map from zero again
    dev = rep.results()
    host = slam.node_replay_host(scans, AMIN, AMAX, max_lm=8)
    for k in ("kept", "kept_count", "nlm", "status", "iters", "xest", "x", "P", "T"):
        assert np.array_equal(dev[k], host[k], equal_nan=True), k
    assert np.array_equal(grid.read(0)["pmap"], g7["node_pmap"])


# ---- skipped scans ---------------------------------------------------------------------------

def with_empties(g7, places):
    scans = list(g7["node_ranges"][4::5])
    for i, p in enumerate(places):
        scans.insert(p, g7["ext_empty_ranges"][i % 2])
    return np.array(scans, dtype=np.float32)


def test_skipped_scans(slam, g7):
    scans = with_empties(g7, (3, 7, 15))
    assert scans.shape[0] == 16
    ref = host_node(slam, scans)
    assert ref["kept"] == [0, 1, 2, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14]
    grid = slam.DeviceGrid(1, 200, 200, 10.0, 10.0, 10.0)
    out = slam.node_replay_host(scans, AMIN, AMAX, grid=grid, max_lm=8)
    assert_matches_host(out, 0, ref, grid.read(0)["pmap"])


def test_skipped_scans_differ_by_trajectory(slam, g7):
    places = ((3, 7, 15), (1, 2, 10), (5, 14, 15))
    scans = np.stack([with_empties(g7, p) for p in places])
    grid = slam.DeviceGrid(3, 200, 200, 10.0, 10.0, 10.0)
    out = slam.node_replay_host(scans, AMIN, AMAX, grid=grid, grid_of_traj=[0, 1, 2], max_lm=8)
    for l in range(3):
        assert_matches_host(out, l, host_node(slam, scans[l]), grid.read(l)["pmap"])


# ---- batches ---------------------------------------------------------------------------------

def test_copies_of_one_trajectory_are_bit_equal(slam, g7):
    """300 trajectories: more workgroups than compute units.  The node replay fixes the scan matcher's launch shape, so a
    trajectory's results are the same bits alone and in any batch."""
    scans = with_empties(g7, (3, 7, 15))
    one = slam.node_replay_host(scans, AMIN, AMAX, max_lm=8)
    many = slam.node_replay_host(np.repeat(scans[None], 300, axis=0), AMIN, AMAX, max_lm=8)
    c = int(one["kept_count"][0])
    assert c == 13
    for k in ("kept", "kept_count", "nlm", "status", "xest", "x", "P"):
        assert np.array_equal(many[k], np.repeat(one[k], 300, axis=0), equal_nan=True), k
    for k in ("T", "iters"):                      # (entries behind a trajectory's steps are void)
        assert np.array_equal(many[k][:, :c - 1], np.repeat(one[k][:, :c - 1], 300, axis=0)), k


def test_synthetic_trajectories_against_host_node(slam, syn):
    world = syn.World(5.0, 4.0, POLES, 0.08)
    scans = []
    for seed in (5, 6, 7, 8):
        poses = syn.trajectory(world, 48 * 5, seed)[::5]
        scans.append(syn.scans_from_poses(world, poses, 360, seed))
    scans = np.stack(scans).astype(np.float32)
    assert scans.shape == (4, 48, 360)
    grid = slam.DeviceGrid(4, 200, 200, 10.0, 10.0, 10.0)
    out = slam.node_replay_host(scans, AMIN, AMAX, grid=grid, grid_of_traj=[0, 1, 2, 3], max_lm=16)
    lm = slam.landmarks_host(scans[0], AMIN, AMAX)
    assert lm["count"].min() >= 2 and lm["count"].max() <= 4
    for l in range(4):
        assert_matches_host(out, l, host_node(slam, scans[l]), grid.read(l)["pmap"])
