"""The landmark node where its loops wrap and its caps bite: the filter with a state that
fills the wave more than once, extraction past a workgroup of clusters and past 64 KiB of LDS, both kernels past
2^20 workgroups, the kept-scan rule past 64 scans, SLAM_NODE_OBS_CAP, step counts outside [0, steps] and the bytes
behind every output.  The references are the host classes Extraction, EKF and SLAM_EKF(landmarks=True) through the
helpers of test_gpu_landmark_bounds.py and test_gpu_node_replay.py, the bars those files state; the inputs and the
conditions on them come from landmark_cases.py."""
import math

import numpy as np
import pytest

import landmark_cases as lc
from conftest import load_golden, pkg
from test_gpu_landmark_bounds import check_filter, check_scans, circle_drive, host_filter
from test_gpu_node_replay import AMAX, AMIN, POLES, assert_matches_host, host_node

pytestmark = pytest.mark.gpu
GUARD = 0x5A
BIG = (1 << 20)                                    # kLandmarkMaxGroups of slam_internal.h


@pytest.fixture(scope="module")
def slam():
    p = pkg()
    p._abi.default_context()
    return p


@pytest.fixture(scope="module")
def g7():
    return load_golden("g7_w12_node.npz")


def same(a, b, keys):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


# ---- the raw entry points, with room behind every output -------------------------------------

def padded(shape, dtype, pad):
    buf = np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize + pad, GUARD, dtype=np.uint8)
    return buf, buf[:buf.size - pad].view(dtype).reshape(shape)


def untouched(bufs, pad):
    return all(np.all(b[b.size - pad:] == GUARD) for b in bufs.values())


def raw_ekf_lm(slam, u, counts, off, z, max_lm, x0=None, pad=0):
    """slam_ekf_lm as the caller of the C header sees it: u [B, steps, 3], any step_counts, ascending z_off."""
    abi = slam._abi
    u = np.ascontiguousarray(u, dtype=np.float64)
    B, steps, N = u.shape[0], u.shape[1], 3 + 2 * max_lm
    counts, off = np.ascontiguousarray(counts, dtype=np.int32), np.ascontiguousarray(off, dtype=np.int64)
    z = np.ascontiguousarray(z, dtype=np.float64).reshape(-1, 2)
    x0 = None if x0 is None else np.ascontiguousarray(x0, dtype=np.float64)
    bufs, out = {}, {}
    for k, shape, dt in (("x", (B, N), np.float64), ("P", (B, N, N), np.float64), ("nlm", (B, steps), np.int32),
                         ("status", (B,), np.int32)):
        bufs[k], out[k] = padded(shape, dt, pad)
    abi.check(abi.lib().slam_ekf_lm(abi.default_context().handle, abi.ptr(x0), abi.ptr(u), abi.ptr(counts), abi.ptr(off),
                                    abi.ptr(z) if len(z) else None, len(z), B, steps, max_lm,
                                    *[abi.ptr(bufs[k]) for k in ("x", "P", "nlm", "status")]))
    return out, bufs


def pack(cases, steps):
    """u, z_off and z of `cases` (each with exactly `steps` steps) as slam_ekf_lm takes them."""
    u = np.array([c["u"] for c in cases], dtype=np.float64).reshape(len(cases), steps, 3)
    rows = [np.asarray(zs, dtype=np.float64).reshape(-1, 2) for c in cases for zs in c["z"]]
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    return u, off, np.concatenate(rows)


# ---- 1. the filter with a state that fills the wave more than once ------------------------------

@pytest.fixture(scope="module")
def grown(slam):
    """The drive to 32 landmarks, the host class's state after every step, and the condition on the inputs."""
    drive = lc.grid_drive(1)
    states, worst = lc.nudge_stability(slam.EKF(), drive)
    assert worst < 1e-10, worst                    # the reference alone holds 1e-9 with an order to spare
    assert states[-1][3] == 0 and states[-1][2][-1] == lc.MAX_LM and len(states) == lc.GRID_STEPS + 1
    assert max(len(zs) for zs in drive["z"]) >= 20

    def host(slam_, u, z, x0=None):
        if len(u) and u[0] is drive["u"][0]:       # a prefix of the drive: the state the one host run passed through
            return states[len(u)]
        return host_filter(slam_, u, z, x0)
    return drive, states, host


def prefix(drive, t):
    return {"u": drive["u"][:t], "z": drive["z"][:t]}


def test_filter_every_state_size_up_to_32_landmarks(slam, grown):
    """Trajectory t runs the first t + 1 steps of the drive, so every state size from 5 to 67 is an output: the
    2 Nc loop makes its second trip from 15 landmarks on, the Nc loop at 31 and 32.  Measured on the MI355X at 32
    landmarks (13 trajectories, 67 x 67, cond(P) = 2.4e2): worst |x - host| = 5.3e-15, worst |P - host| = 1.2e-15."""
    drive, states, host = grown
    wrap = [lc.first_step_with(states, c) for c in (15, 16, 31, 32)]
    assert wrap == sorted(wrap) and wrap[-1] <= lc.GRID_STEPS
    short, empty = circle_drive(6, 5), {"u": [], "z": []}
    cases = [prefix(drive, t + 1) for t in range(lc.GRID_STEPS)] + [short, empty]
    out, refs = check_filter(slam, cases, max_lm=lc.MAX_LM, host=host)
    assert not out["status"].any()
    for t in range(lc.GRID_STEPS):
        assert out["nlm"][t, t] == states[t + 1][2][-1] and np.all(out["nlm"][t, t + 1:] == -1), t
    full = [t for t in range(lc.GRID_STEPS) if states[t + 1][2][-1] == lc.MAX_LM]
    dx = max(float(np.max(np.abs(out["x"][t] - refs[t][0]))) for t in full)
    dP = max(float(np.max(np.abs(out["P"][t] - refs[t][1]))) for t in full)
    print("32 landmarks, %d trajectories: worst |x - host| = %.3e, worst |P - host| = %.3e, cond(P) = %.1e"
          % (len(full), dx, dP, np.linalg.cond(refs[-3][1])))
    yaw = np.cumsum([u[2] for u in drive["u"]])
    assert yaw[-1] > 2 * math.pi                                           # the drive crossed +-pi on the way
    # alone and in the batch: the same bits
    last = lc.GRID_STEPS - 1
    for b, c in ((last, cases[last]), (lc.GRID_STEPS, short), (lc.GRID_STEPS + 1, empty)):
        alone, _ = check_filter(slam, [c], max_lm=lc.MAX_LM, host=host)
        assert np.array_equal(alone["x"][0], out["x"][b]) and np.array_equal(alone["P"][0], out["P"][b]), b
        assert alone["nlm"][0].tolist() == out["nlm"][b, :alone["nlm"].shape[1]].tolist(), b
    assert np.array_equal(out["P"][-1, :3, :3], np.eye(3)) and np.all(out["nlm"][-1] == -1)


def test_filter_stops_at_31_landmarks(slam, grown):
    """max_lm = 31: the step that would append the 32nd landmark does not happen, and the landmarks it matched before
    that row are undone - the state is that of the 31-landmark trajectory which ends a step earlier."""
    drive, states, host = grown
    stop = lc.first_step_with(states, 32) - 1                              # steps that happen
    assert states[stop][2][-1] == 31
    new_row = len(drive["z"][stop]) // 2
    assert new_row >= 5                                                    # rows matched before the one that stops it
    out, _ = check_filter(slam, [dict(drive, cap_at=stop), prefix(drive, stop)], max_lm=31, host=host)
    assert out["status"].tolist() == [slam._abi.NODE_LM_CAP, 0]
    assert np.array_equal(out["x"][0], out["x"][1]) and np.array_equal(out["P"][0], out["P"][1])
    assert out["nlm"][0, stop - 1] == 31 and np.all(out["nlm"][0, stop:] == -1)


def test_step_counts_outside_their_range_and_guard_bytes(slam):
    """step_counts of -3 and 0 run nothing, steps and steps + 5 run exactly `steps` steps; 64 bytes behind every
    output of the host form stay as they were."""
    steps = 6
    cases = [circle_drive(steps, 11 + b) for b in range(5)]
    u, off, z = pack(cases, steps)
    counts = [-3, 0, steps, steps + 5, 4]
    out, bufs = raw_ekf_lm(slam, u, counts, off, z, max_lm=4, pad=64)
    assert untouched(bufs, 64)
    want, _ = check_filter(slam, cases[2:4] + [prefix(cases[4], 4)], max_lm=4)
    assert out["status"].tolist() == [0] * 5
    for b in (0, 1):
        assert np.all(out["nlm"][b] == -1) and not out["x"][b].any()
        assert np.array_equal(out["P"][b, :3, :3], np.eye(3)) and not out["P"][b, 3:].any() and not out["P"][b, :, 3:].any()
    for b in (2, 3, 4):
        assert np.array_equal(out["x"][b], want["x"][b - 2]) and np.array_equal(out["P"][b], want["P"][b - 2]), b
        assert out["nlm"][b, :want["nlm"].shape[1]].tolist() == want["nlm"][b - 2].tolist(), b
    assert np.all(out["nlm"][2:4] >= 1) and out["nlm"][4].tolist()[4:] == [-1, -1]


# ---- 2. extraction past a workgroup of clusters, past 64 KiB of LDS, at the caps ----------------

@pytest.mark.parametrize("k", [255, 256, 257, 512])
def test_landmarks_past_a_workgroup_and_lm_cap(slam, k):
    """k landmarks, 2 k closed clusters in one scan: the ranks and the means loop make a second (k = 512: a fourth)
    trip; lm_cap = 256 and 300 keep the prefix of the uncapped run."""
    row = lc.pole_row(k, tail=(9.0, 9.01))
    assert row.size == 4 * k + 2
    full = check_scans(slam, row, 0.0, 0.0, lm_cap=1024)
    assert full["count"][0] == k and full["overflow"][0] == 0 and full["ids"][0, :k].tolist() == list(range(0, 2 * k, 2))
    for cap in (256, 300):
        got = check_scans(slam, row, 0.0, 0.0, lm_cap=cap)
        keep = min(k, cap)
        assert got["count"][0] == keep and got["overflow"][0] == (k > cap)
        for key in ("ids", "means", "z"):
            assert np.array_equal(got[key][0, :keep], full[key][0, :keep]), key
        assert np.all(got["ids"][0, keep:] == -1) and not got["means"][0, keep:].any() and not got["z"][0, keep:].any()
        assert np.array_equal(got["labels"], full["labels"])


@pytest.mark.parametrize("tail,nb", [((), 255), ((9.0, 9.01), 256), ((9.0, 5.0, 5.01), 257)])
def test_closed_clusters_at_a_workgroup(slam, tail, nb):
    """255, 256 and 257 closed clusters: block_prefix over the cluster flags ends its first trip exactly, or not."""
    out = check_scans(slam, lc.pole_row(128, tail=tail), 0.0, 0.0, lm_cap=1024)
    assert out["count"][0] == 128 and out["labels"][0].max() == nb - (1 if not tail else 0)


@pytest.mark.parametrize("n,lds", [(2047, 65520), (2048, 65552), (4096, 131088)])
def test_beams_around_64_kib_of_lds(slam, n, lds):
    """n = 2047 is the last scan within 64 KiB, 2048 the first for which the launch raises the dynamic-LDS limit,
    4096 the documented maximum; pole-sized clusters sit at both ends of the scan."""
    assert lc.landmark_lds_bytes(n) == lds and (lds <= 65536) == (n == 2047)
    out = check_scans(slam, lc.row_of_length(n), 0.0, 0.0, lm_cap=16)
    assert out["count"][0] == 5 and out["ids"][0, 0] == 0 and out["ids"][0, 4] == out["labels"][0].max()


def test_4096_beams_among_poles(slam, syn):
    world = syn.World(5.0, 4.0, POLES, 0.08)
    ranges = syn.scans_from_poses(world, syn.trajectory(world, 15, 3)[::5], 4096, 3)
    assert ranges.shape == (3, 4096)
    out = check_scans(slam, ranges, AMIN, AMAX)
    assert out["count"].min() >= 1


# ---- 3. grid-stride trips past 2^20 workgroups ---------------------------------------------------

def test_landmarks_second_trip_of_the_grid(slam):
    """2^20 + 5 scans of 8 beams: the last five are a workgroup's second scan, with the LDS of its first."""
    S = BIG + 5
    x0 = (1.0 + 1e-3 * (np.arange(S) % 1000)).astype(np.float32)
    rows = np.stack([x0, x0 + np.float32(0.05), x0 + np.float32(0.1), x0 + np.float32(4.0)] + [np.full(S, 9.0, np.float32)] * 4, axis=1)
    out = slam.landmarks_host(rows, 0.0, 0.0, lm_cap=2)
    r = rows.astype(np.float64)
    mean = (((0.0 + r[:, 0]) + r[:, 1]) + r[:, 2]) / 3
    assert np.all(out["count"] == 1) and not out["overflow"].any() and np.all(out["ids"] == np.array([0, -1]))
    assert np.array_equal(out["means"][:, 0, 0], mean) and not out["means"][:, 0, 1].any() and not out["means"][:, 1].any()
    assert np.array_equal(out["z"][:, 0, 0], mean) and not out["z"][:, 0, 1].any() and not out["z"][:, 1].any()
    check_scans(slam, rows[[0, BIG - 1, BIG, S - 1]], 0.0, 0.0, lm_cap=2)


def test_filter_second_trip_of_the_grid(slam):
    """2^20 + 3 trajectories of one step, max_lm = 1 (N = 5).  The inputs depend on b % 1000 only, so every
    trajectory must have the bits of its representative among the first 1000, which are compared with the host class;
    2^20 % 1000 = 576, so a workgroup's second trajectory differs from its first.  Every 7th kind gets two rows the
    filter cannot match (the early return, yaw left unwrapped), every 11th a second row equal to its first (the
    reference raises): workgroup 0 runs an early return and workgroup 1 a stopped trajectory before their second,
    ordinary ones."""
    B, period = BIG + 3, 1000
    c = np.arange(period)
    early = c % 7 == 0
    raises = (c % 11 == 1) & ~early
    x0 = np.stack([1e-3 * c, -2e-3 * c, 0.1 * (c % 63) - 3.1], axis=1)
    x0[early, 2] = 3.0
    u = np.stack([0.1 + 1e-4 * c, np.full(period, 0.01), np.full(period, 0.05)], axis=1)
    u[early, 2] = 0.5
    first = np.stack([2.0 + 3e-3 * c, -1.0 + 2e-3 * c], axis=1)
    cases = []
    for i in range(period):
        rows = [first[i]] + ([(3.0 + 3e-3 * i, 1.0)] if early[i] else [first[i]] if raises[i] else [])
        cases.append({"x0": x0[i], "u": [u[i]], "z": [np.array(rows)]})
    small, refs = check_filter(slam, cases, max_lm=1)
    assert np.all(small["status"][raises] == slam._abi.NODE_REF_RAISES) and not small["status"][~raises].any()
    assert np.all(small["x"][early, 2] > math.pi) and np.all(np.abs(small["x"][~early, 2]) <= math.pi)
    assert np.all(small["nlm"][raises, 0] == -1) and np.all(small["nlm"][~raises, 0] == 1)
    # the whole batch, packed without a Python loop over it
    rep = np.arange(B) % period
    n_rows = np.where(early | raises, 2, 1)[rep]
    off = np.concatenate([[0], np.cumsum(n_rows)])
    z = np.concatenate([cs["z"][0] for cs in cases])                       # one period of rows, tiled
    per = len(z)
    z = np.concatenate([np.tile(z, (B // period, 1)), z[:off[-1] - (B // period) * per]])
    assert len(z) == off[-1]
    out, _ = raw_ekf_lm(slam, u[rep][:, None, :], np.ones(B, dtype=np.int32), off, z, max_lm=1, x0=x0[rep])
    for k in ("x", "P", "nlm", "status"):
        assert np.array_equal(out[k][:period], small[k]), k
        assert np.array_equal(out[k], out[k][:period][rep]), k
    assert rep[BIG] == 576 and early[0] and raises[1]                      # what workgroups 0 and 1 ran first


# ---- 4. node replay: more than 64 scans, the observation cap, guard bytes ----------------------------

@pytest.fixture(scope="module")
def long_scans(slam, syn):
    """Three trajectories of 130 scans whose landmark-free scans straddle the 64-scan chunks of k_node_keep."""
    world = syn.World(5.0, 4.0, POLES, 0.08)
    empty = np.full(360, np.inf, dtype=np.float32)
    scans = []
    for l, places in enumerate(lc.EMPTY_AT):
        real = lc.N_SCAN - len(places)
        poses = syn.trajectory(world, real * 5, 5 + l)[::5]
        scans.append(lc.with_empties_at(syn.scans_from_poses(world, poses, 360, 5 + l), places, empty))
    scans = np.stack(scans)
    assert scans.shape == (3, lc.N_SCAN, 360)
    return scans


def test_kept_scans_across_the_64_scan_chunks(slam, long_scans):
    scans = long_scans
    grid = slam.DeviceGrid(3, 200, 200, 10.0, 10.0, 10.0)
    out = slam.node_replay_host(scans, AMIN, AMAX, grid=grid, grid_of_traj=[0, 1, 2], max_lm=16)
    for l, places in enumerate(lc.EMPTY_AT):
        counts = slam.landmarks_host(scans[l], AMIN, AMAX)["count"]
        assert not counts[list(places)].any() and counts.sum() > 0
        kept = lc.kept_rule(counts)
        assert kept == [k for k in range(lc.N_SCAN) if k not in places or k == 0], l
        assert out["kept_count"][l] == len(kept) and out["kept"][l, :len(kept)].tolist() == kept, l
        assert np.all(out["kept"][l, len(kept):] == -1), l
    assert_matches_host(out, 0, host_node(slam, scans[0]), grid.read(0)["pmap"])
    alone = slam.node_replay_host(scans[1], AMIN, AMAX, max_lm=16)
    c = int(alone["kept_count"][0])
    assert c == lc.N_SCAN - 63
    assert same({k: v[0] for k, v in alone.items()}, {k: v[1] for k, v in out.items()},
                ("kept", "kept_count", "nlm", "status", "xest", "x", "P"))
    for k in ("T", "iters"):                      # (entries behind a trajectory's steps are void)
        assert np.array_equal(alone[k][0, :c - 1], out[k][1, :c - 1]), k


NODE_COUNTS = [4, 4, 4, 4, 3, 4, 3, 4, 3, 4, 5, 4, 4]                     # landmarks of the g7 node scans


@pytest.mark.parametrize("cap", [3, 4])
def test_observation_cap_stops_the_trajectory(slam, g7, cap):
    """The g7 node scans show 3, 4 or 5 landmarks.  With lm_cap = 3 the trajectory stops with SLAM_NODE_OBS_CAP at
    scan 1, before its first step (scan 0 shows 4 as well, and is no reason); with lm_cap = 4 at scan 10, after nine
    steps.  Everything before the stop is as the lm_cap = 8 run has it, the state and the map are those of the scans
    before it, and an ordinary neighbour in the batch is not touched."""
    scans = np.array(g7["node_ranges"][4::5], dtype=np.float32)
    counts = slam.landmarks_host(scans, AMIN, AMAX)["count"]
    assert counts.tolist() == NODE_COUNTS
    stop = next(k for k in range(1, len(scans)) if counts[k] > cap)        # the scan that is one landmark too many
    done = stop - 1                                                        # steps that happen
    assert (cap, stop) in ((3, 1), (4, 10))
    other = scans.copy()
    other[1:][counts[1:] > cap] = np.inf                                   # dropped before the filter sees them
    grid = slam.DeviceGrid(2, 200, 200, 10.0, 10.0, 10.0)
    out = slam.node_replay_host(np.stack([scans, other]), AMIN, AMAX, grid=grid, grid_of_traj=[0, 1], max_lm=8, lm_cap=cap)
    wide = slam.node_replay_host(scans, AMIN, AMAX, max_lm=8, lm_cap=8)
    assert out["status"].tolist() == [slam._abi.NODE_OBS_CAP, 0] and wide["status"][0] == 0
    assert out["kept"][0].tolist() == list(range(len(scans))) and out["kept_count"][0] == len(scans)
    for k in ("xest", "nlm", "T", "iters"):
        assert np.array_equal(out[k][0, :done], wide[k][0, :done]), k
    assert np.all(np.isnan(out["xest"][0, done:])) and np.all(out["nlm"][0, done:] == -1)
    ref = host_node(slam, scans[:stop])                                    # the state and the map of the scans before
    assert ref["kept"] == list(range(stop)) and np.array_equal(grid.read(0)["pmap"], ref["pmap"])
    n = len(ref["x"])
    assert np.max(np.abs(out["x"][0, :n] - ref["x"])) < 1e-9 and np.max(np.abs(out["P"][0, :n, :n] - ref["P"])) < 1e-9
    assert not out["x"][0, n:].any() and not out["P"][0, n:].any() and not out["P"][0, :, n:].any()
    if done:
        assert np.max(np.abs(out["xest"][0, :done] - ref["xest"])) < 1e-9 and out["nlm"][0, :done].tolist() == ref["nlm"]
        before = slam.node_replay_host(scans[:stop], AMIN, AMAX, max_lm=8, lm_cap=8)
        assert np.array_equal(out["x"][0], before["x"][0]) and np.array_equal(out["P"][0], before["P"][0])
    else:
        assert n == 3 and not out["x"][0].any() and np.array_equal(out["P"][0, :3, :3], np.eye(3))
    # the neighbour: alone and beside the stopped trajectory
    alone_grid = slam.DeviceGrid(1, 200, 200, 10.0, 10.0, 10.0)
    alone = slam.node_replay_host(other, AMIN, AMAX, grid=alone_grid, max_lm=8, lm_cap=cap)
    c = int(alone["kept_count"][0])
    assert c == len(scans) - int((counts[1:] > cap).sum()) and c >= 4
    assert same({k: v[0] for k, v in alone.items()}, {k: v[1] for k, v in out.items()},
                ("kept", "kept_count", "nlm", "status", "xest", "x", "P"))
    assert np.array_equal(alone["T"][0, :c - 1], out["T"][1, :c - 1]) and np.array_equal(alone["iters"][0, :c - 1], out["iters"][1, :c - 1])
    assert np.array_equal(alone_grid.read(0)["pmap"], grid.read(1)["pmap"])
    assert_matches_host(out, 1, host_node(slam, other), grid.read(1)["pmap"])


def test_overflow_in_scan_0_only_is_no_stop(slam, g7):
    """Scan 0 is a target only and never observed: more than lm_cap landmarks in it leave the status at 0."""
    scans = np.array(g7["node_ranges"][4::5], dtype=np.float32)
    scans = np.concatenate([lc.crowded_scan(scans[0])[None], scans])
    lm = slam.landmarks_host(scans, AMIN, AMAX, lm_cap=5)
    assert lm["overflow"].tolist() == [1] + [0] * (len(scans) - 1) and lm["count"][1:].tolist() == NODE_COUNTS
    grid = slam.DeviceGrid(1, 200, 200, 10.0, 10.0, 10.0)
    out = slam.node_replay_host(scans, AMIN, AMAX, grid=grid, max_lm=8, lm_cap=5)
    assert out["status"][0] == 0 and out["kept_count"][0] == len(scans)
    assert_matches_host(out, 0, host_node(slam, scans), grid.read(0)["pmap"])


def test_guard_bytes_behind_landmarks_and_node_outputs(slam, g7):
    """The host forms of slam_landmarks and slam_node_replay write exactly their outputs (slam_ekf_lm: see
    test_step_counts_outside_their_range_and_guard_bytes)."""
    abi, pad = slam._abi, 64
    ctx = abi.default_context().handle
    r = np.ascontiguousarray(np.concatenate([g7["ext_ranges"][:2], g7["ext_empty_ranges"][:1]]), dtype=np.float32)
    S, n, cap = r.shape[0], r.shape[1], 5
    ct, st = abi.trig_tables(AMIN, AMAX, n)
    bufs, out = {}, {}
    for k, shape, dt in (("count", (S,), np.int32), ("overflow", (S,), np.int32), ("ids", (S, cap), np.int32),
                         ("means", (S, cap, 2), np.float64), ("z", (S, cap, 2), np.float64), ("labels", (S, n - 1), np.int32)):
        bufs[k], out[k] = padded(shape, dt, pad)
    abi.check(abi.lib().slam_landmarks(ctx, abi.ptr(r), abi.ptr(ct), abi.ptr(st), S, n, 1.0, 0.3, cap,
                                       *[abi.ptr(bufs[k]) for k in ("count", "overflow", "ids", "means", "z", "labels")]))
    assert untouched(bufs, pad) and same(out, slam.landmarks_host(r, AMIN, AMAX, lm_cap=cap, range_threshold=1.0, radius_max_th=0.3,
                                                                  labels=True), out.keys())
    scans = np.ascontiguousarray(g7["node_ranges"][4::5][:5], dtype=np.float32)
    L, n_scan, max_lm = 1, scans.shape[0], 8
    N, K = 3 + 2 * max_lm, n_scan - 1
    bufs, out = {}, {}
    for k, shape, dt in (("kept", (L, n_scan), np.int32), ("kept_count", (L,), np.int32), ("xest", (L, K, 3), np.float64),
                         ("nlm", (L, K), np.int32), ("x", (L, N), np.float64), ("P", (L, N, N), np.float64),
                         ("T", (L, K, 3, 3), np.float64), ("iters", (L, K), np.int32), ("status", (L,), np.int32)):
        bufs[k], out[k] = padded(shape, dt, pad)
    p0 = np.zeros((L, 3))
    abi.check(abi.lib().slam_node_replay(
        ctx, abi.ptr(scans), abi.ptr(ct), abi.ptr(st), L, n_scan, n, abi.DTYPES["f64"], 30, 0.001, 1.0, 0.3, 8, max_lm, abi.ptr(p0),
        None, None, *[abi.ptr(bufs[k]) for k in ("kept", "kept_count", "xest", "nlm", "x", "P", "T", "iters", "status")]))
    want = slam.node_replay_host(scans, AMIN, AMAX, max_lm=max_lm, lm_cap=8, max_iter=30, tolerance=0.001,
                                 range_threshold=1.0, radius_max_th=0.3)
    assert untouched(bufs, pad) and same(out, want, out.keys())
