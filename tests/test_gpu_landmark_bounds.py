"""slam_landmarks and slam_ekf_lm at their sizes and edges, each case against the host classes Extraction
(labels / process) and EKF (estimate) on the same numbers.  Labels, ids, counts and statuses are exact, landmark
means bit-equal, observation rows within 1e-12, states and covariances within 1e-9.
NaN ranges are not tested: they follow the host class (a NaN gap or distance compares false) and are documented
in include/slam_hip.h."""
import copy
import math

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu
AMIN, AMAX = -3.14159, 3.14159


@pytest.fixture(scope="module")
def slam():
    p = pkg()
    p._abi.default_context()
    return p


# ---- extraction ------------------------------------------------------------------------------

def check_scans(slam, ranges, amin, amax, lm_cap=8, rt=1.0, rm=0.3):
    """One slam_landmarks call over the rows of `ranges` against Extraction on the same points."""
    ranges = np.atleast_2d(np.asarray(ranges, dtype=np.float32))
    S, n = ranges.shape
    out = slam.landmarks_host(ranges, amin, amax, lm_cap=lm_cap, range_threshold=rt, radius_max_th=rm, labels=True)
    ct, st = slam._abi.trig_tables(amin, amax, n)
    ex = slam.Extraction()
    ex.range_threshold, ex.radius_max_th = rt, rm
    pi_2_pi = slam.EKF().pi_2_pi
    for s in range(S):
        r = ranges[s].astype(np.float64)
        r[np.isinf(r)] = 30.0
        pc = np.vstack([ct * r, st * r])
        labels, found = ex.labels(pc)
        lm = ex.process(pc)
        assert out["labels"][s].tolist() == labels.tolist(), s
        keep = min(len(found), lm_cap)
        assert out["count"][s] == keep and out["overflow"][s] == (len(found) > lm_cap), s
        assert out["ids"][s, :keep].tolist() == found[:keep] and np.all(out["ids"][s, keep:] == -1), s
        if keep:
            assert np.array_equal(out["means"][s, :keep, 0], np.array(lm.position_x[:keep])), s
            assert np.array_equal(out["means"][s, :keep, 1], np.array(lm.position_y[:keep])), s
            z = np.array([[math.hypot(x, y), pi_2_pi(math.atan2(y, x))] for x, y in zip(lm.position_x[:keep], lm.position_y[:keep])])
            assert np.max(np.abs(out["z"][s, :keep] - z)) < 1e-12, s
    return out


def line(*xs):
    """Ranges of a scan whose beams all point along +x (angle_min = angle_max = 0): point i is (xs[i], 0)."""
    return np.array(xs, dtype=np.float32)


def cluster(x0, k, step=0.0005):
    return [x0 + step * i for i in range(k)]


LINE_CASES = {
    "n1": line(1.0),
    "n2": line(1.0, 1.05),
    "n2_gap": line(1.0, 5.0),
    "n3": line(1.0, 1.05, 1.1),
    "n3_gap_last": line(1.0, 1.05, 5.0),
    "label_rules": line(0.0, 0.05, 0.10, 5.0, 9.0, 9.05, 20.0, 20.05, 20.10, 20.15),
    "wide_cluster": line(0.0, 0.05, 0.4, 5.0, 9.0, 9.05, 20.0, 20.05, 20.10, 20.15),
    "closed_by_last_gap": line(5.0, 9.0, 1.0, 1.05, 1.1, 3.0),      # the gap between the last two points closes it
    "left_open": line(5.0, 9.0, 1.0, 1.05, 1.1, 1.15),
    "lone_point": line(1.0, 1.05, 1.1, 5.0, 9.0, 9.05, 9.1, 12.0),
    "two_then_gap": line(1.0, 1.05, 5.0, 5.05, 9.0, 9.05, 9.1, 12.0),
}


@pytest.mark.parametrize("name", sorted(LINE_CASES))
def test_label_rules_on_hand_made_rows(slam, name):
    out = check_scans(slam, LINE_CASES[name], 0.0, 0.0)
    if name in ("label_rules", "closed_by_last_gap"):
        assert out["count"][0] == 1
    if name in ("n1", "n2", "n3", "left_open", "wide_cluster"):
        assert out["count"][0] == 0


@pytest.mark.parametrize("k", [63, 64, 65, 255, 256, 257])
def test_clusters_across_wave_and_workgroup_boundaries(slam, k):
    """Small in extent, so every pair is tested: k beams, a lane stride of 64 and a workgroup of 256."""
    row = line(*([9.0, 7.0] + cluster(1.0, k) + [4.0] + cluster(5.0, k) + [8.0, 8.01]))
    out = check_scans(slam, row, 0.0, 0.0)
    assert out["count"][0] == 2 and out["ids"][0, :2].tolist() == [2, 4]


def test_wall_whose_only_far_pair_is_first_and_last(slam):
    d = 0.00202                                   # 149 d > 0.3 > 148 d
    wall = [1.0 + d * i for i in range(150)]
    out = check_scans(slam, np.stack([line(*([9.0] + wall + [4.0, 4.01])), line(*([9.0] + wall[:-1] + [1.29, 4.0, 4.01]))]), 0.0, 0.0)
    assert out["count"].tolist() == [0, 1]


def test_extent_and_gap_exactly_at_their_thresholds(slam):
    row = line(9.0, 1.0, 1.125, 1.25, 2.25, 2.375, 2.5, 7.0, 7.01)   # extents 0.25, gap 1.0: exact in float32
    up = float(np.nextafter(0.25, 1.0))
    assert check_scans(slam, row, 0.0, 0.0, rt=1.0, rm=0.25)["count"][0] == 0       # extent == radius_max_th: not below
    assert check_scans(slam, row, 0.0, 0.0, rt=1.0, rm=up)["count"][0] == 2         # one ulp below it
    # a gap of exactly range_threshold separates; one ulp more joins the two into one cluster of extent 1.5
    assert check_scans(slam, row, 0.0, 0.0, rt=float(np.nextafter(1.0, 2.0)), rm=up)["count"][0] == 0
    assert check_scans(slam, row, 0.0, 0.0, rt=float(np.nextafter(1.0, 2.0)), rm=2.0)["count"][0] == 1


def test_all_inf_scan_is_one_open_cluster(slam):
    out = check_scans(slam, np.full(360, np.inf, dtype=np.float32), AMIN, AMAX)
    assert out["count"][0] == 0 and not out["labels"][0].any()


def test_1080_beams(slam, syn):
    world = syn.World(5.0, 4.0, ((1.5, 1.0), (-1.8, -0.9), (0.5, -2.0), (-2.5, 1.5)), 0.08)
    ranges = syn.scans_from_poses(world, syn.trajectory(world, 15, 3)[::5], 1080, 3)
    out = check_scans(slam, ranges, AMIN, AMAX)
    assert out["count"].min() >= 1


def test_lm_cap_and_one_more(slam):
    row = []
    for j in range(4):
        row += cluster(1.0 + 2.0 * j, 3, 0.01)
    row = line(*(row + [20.0, 20.01]))
    full = check_scans(slam, row, 0.0, 0.0, lm_cap=4)
    over = check_scans(slam, row, 0.0, 0.0, lm_cap=3)
    assert full["count"][0] == 4 and full["overflow"][0] == 0
    assert over["count"][0] == 3 and over["overflow"][0] == 1 and np.array_equal(over["means"][0], full["means"][0, :3])


def test_70000_scans_in_one_launch(slam):
    S = 70000
    x0 = (1.0 + 1e-3 * (np.arange(S) % 1000)).astype(np.float32)
    rows = np.stack([x0, x0 + np.float32(0.05), x0 + np.float32(0.1), x0 + np.float32(4.0)] + [np.full(S, 9.0, np.float32)] * 4, axis=1)
    out = slam.landmarks_host(rows, 0.0, 0.0, lm_cap=2)
    r = rows.astype(np.float64)
    mean = (((0.0 + r[:, 0]) + r[:, 1]) + r[:, 2]) / 3
    assert np.all(out["count"] == 1) and not out["overflow"].any() and np.all(out["ids"] == np.array([0, -1]))
    assert np.array_equal(out["means"][:, 0, 0], mean) and not out["means"][:, 0, 1].any() and not out["means"][:, 1].any()
    check_scans(slam, rows[[0, 999, S - 1]], 0.0, 0.0, lm_cap=2)


# ---- filter ----------------------------------------------------------------------------------

def host_filter(slam, u, z, x0=None):
    """EKF.estimate step by step: state after the last step that happened, landmark counts, status."""
    ekf = slam.EKF()
    x = np.zeros((3, 1)) if x0 is None else np.array(x0, dtype=float).reshape(3, 1)
    P, nlm, status = np.eye(3), [], 0
    for us, zs in zip(u, z):
        xb, Pb = copy.deepcopy(x), copy.deepcopy(P)               # the prediction writes into its arguments
        rows = np.zeros((0, 3)) if len(zs) == 0 else np.hstack([np.asarray(zs, dtype=float), np.zeros((len(zs), 1))])
        try:
            x, P = ekf.estimate(x, P, rows, np.array(us, dtype=float).reshape(3, 1))
        except ValueError:
            x, P, status = xb, Pb, 1
            break
        nlm.append((len(x) - 3) // 2)
    return x[:, 0], P, nlm, status


def check_filter(slam, cases, max_lm, host=host_filter):
    """One slam_ekf_lm call over `cases` against `host` (host_filter, or a function that returns what it would)."""
    out = slam.ekf_lm_host([c["u"] for c in cases], [c["z"] for c in cases], x0=[c.get("x0", (0, 0, 0)) for c in cases],
                           max_lm=max_lm)
    refs = []
    for b, c in enumerate(cases):
        # a trajectory that would pass max_lm stops before that step: the host class runs the steps before it
        x, P, nlm, status = host(slam, c["u"], c["z"], c.get("x0"))
        if c.get("cap_at") is not None:
            x, P, nlm, status = host(slam, c["u"][:c["cap_at"]], c["z"][:c["cap_at"]], c.get("x0"))
            status = 2
        n = len(x)
        assert out["status"][b] == status, b
        assert out["nlm"][b, :len(nlm)].tolist() == nlm and np.all(out["nlm"][b, len(nlm):] == -1), b
        assert np.max(np.abs(out["x"][b, :n] - x)) < 1e-9 and np.all(out["x"][b, n:] == 0), b
        assert np.max(np.abs(out["P"][b, :n, :n] - P)) < 1e-9, b
        assert np.all(out["P"][b, n:] == 0) and np.all(out["P"][b, :, n:] == 0), b
        refs.append((x, P, nlm, status))
    return out, refs


def circle_drive(steps, seed, skip=(), poles=((4.0, 3.0), (-5.0, -2.5), (1.5, -6.0), (-6.5, 4.5))):
    """Odometry and exact range / bearing rows of a robot turning 0.2 rad a step (the yaw passes +-pi more than
    once in 40 steps) among poles several metres apart; the steps in `skip` see nothing."""
    rng = np.random.default_rng(seed)
    pose = np.zeros(3)
    u, z = [], []
    for s in range(steps):
        us = np.array([0.25, 0.01, 0.2]) + rng.normal(0, [0.01, 0.005, 0.01])
        c, sn = math.cos(pose[2]), math.sin(pose[2])
        pose = pose + np.array([c * us[0] - sn * us[1], sn * us[0] + c * us[1], us[2]])
        rows = []
        for k, (px, py) in enumerate(poles):
            if s in skip or (s + k) % 3 == 0:                     # every pole is out of view now and then
                continue
            dx, dy = px - pose[0], py - pose[1]
            rows.append([math.hypot(dx, dy) + rng.normal(0, 0.01), math.atan2(dy, dx) - pose[2] + rng.normal(0, 0.002)])
        u.append(us)
        z.append(np.array(rows).reshape(-1, 2))
    return {"u": u, "z": z}


def test_filter_quirks_beside_ordinary_trajectories(slam):
    early = {"x0": (0.0, 0.0, 3.0), "u": [(0.1, 0.0, 0.5), (0.0, 0.0, 0.0)],
             "z": [[(2.0, 0.1), (3.0, -1.0)], [(2.0, 0.1)]]}
    early_only = {"x0": (0.0, 0.0, 3.0), "u": early["u"][:1], "z": early["z"][:1]}
    raises = {"u": [(0.1, 0.0, 0.02), (0.1, 0.0, 0.02), (0.1, 0.0, 0.02)],
              "z": [[(2.0, 0.1)], [(3.0, -1.0), (3.0, -1.0)], [(2.0, 0.1)]]}
    cases = [circle_drive(40, 1), early, raises, circle_drive(40, 2, skip=(0, 5, 6, 39)), early_only, {"u": [], "z": []},
             circle_drive(1, 3), circle_drive(40, 1)]
    out, refs = check_filter(slam, cases, max_lm=8)
    assert out["status"].tolist() == [0, 0, 1, 0, 0, 0, 0, 0]
    assert refs[4][0][2] > math.pi and out["x"][4, 2] > math.pi           # the early return leaves the yaw unwrapped
    assert -math.pi <= out["x"][1, 2] < math.pi and out["nlm"][1].tolist()[:2] == [1, 1]
    assert out["nlm"][2].tolist()[:3] == [1, -1, -1]                       # stops exactly where the host class raises
    assert out["nlm"][5].tolist() == [-1] * 40 and np.array_equal(out["P"][5, :3, :3], np.eye(3))
    assert out["nlm"][0, -1] == 4
    for k in ("x", "P", "nlm"):                                            # the neighbours in the batch are unaffected
        assert np.array_equal(out[k][0], out[k][7]), k
    alone, _ = check_filter(slam, cases[:1], max_lm=8)
    assert np.array_equal(alone["x"][0], out["x"][0]) and np.array_equal(alone["P"][0], out["P"][0])
    yaw = [r for r in np.cumsum([u[2] for u in cases[0]["u"]])]
    assert max(yaw) > 2 * math.pi                                          # the drive crossed +-pi on the way


def test_filter_at_max_lm(slam):
    drive = circle_drive(12, 4)
    first_four = next(s for s in range(12) if host_filter(slam, drive["u"][:s + 1], drive["z"][:s + 1])[2][-1] == 4)
    three = {"u": drive["u"][:first_four], "z": drive["z"][:first_four]}
    over = dict(drive, cap_at=first_four)
    out, refs = check_filter(slam, [three, over], max_lm=3)
    assert refs[0][2][-1] == 3 and out["status"].tolist() == [0, 2]
    out4, _ = check_filter(slam, [drive], max_lm=4)                        # reaches max_lm exactly: passes
    assert out4["status"][0] == 0 and out4["nlm"][0, -1] == 4
    out32, _ = check_filter(slam, [drive], max_lm=32)                      # the largest supported state, 67 x 67
    assert np.array_equal(out32["x"][0, :11], out4["x"][0]) and np.array_equal(out32["P"][0, :11, :11], out4["P"][0])
