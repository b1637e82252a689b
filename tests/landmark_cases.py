"""Inputs of test_gpu_landmark_sizes.py and the conditions they must meet before a launch, all on the CPU:
the drive that grows the landmark filter to 32 landmarks and its stability under a nudge of its rows, the LDS
bytes of the extraction at the beam counts around 64 KiB, and the empty scans that straddle the 64-scan chunks of
the kept-scan rule.  test_landmark_cases.py checks them without a GPU."""
import copy
import math

import numpy as np

MAX_LM = 32
GRID_STEPS = 44


def grid_poles(seed, places=36, pitch=3.0, jitter=0.3):
    """Poles on a 6 x 6 grid of `pitch` metres around the origin, nearest place first, each moved by +-jitter."""
    rng = np.random.default_rng(1000 + seed)
    side = int(round(math.sqrt(places)))
    grid = [((i - (side - 1) / 2) * pitch, (j - (side - 1) / 2) * pitch) for i in range(side) for j in range(side)]
    grid.sort(key=lambda p: (round(math.hypot(*p), 9), p))
    return [(x + rng.uniform(-jitter, jitter), y + rng.uniform(-jitter, jitter)) for x, y in grid]


def grid_drive(seed, steps=GRID_STEPS, n_poles=MAX_LM):
    """circle_drive's odometry (0.25 m and 0.2 rad a step) among the first `n_poles` of grid_poles: step s shows
    pole s for the first time, in the middle of its rows, and every earlier pole but those with (s + k) % 3 == 0."""
    rng = np.random.default_rng(seed)
    poles = grid_poles(seed)[:n_poles]
    pose = np.zeros(3)
    u, z = [], []

    def row(k):
        dx, dy = poles[k][0] - pose[0], poles[k][1] - pose[1]
        return [math.hypot(dx, dy) + rng.normal(0, 0.01), math.atan2(dy, dx) - pose[2] + rng.normal(0, 0.002)]

    for s in range(steps):
        us = np.array([0.25, 0.01, 0.2]) + rng.normal(0, [0.01, 0.005, 0.01])
        c, sn = math.cos(pose[2]), math.sin(pose[2])
        pose = pose + np.array([c * us[0] - sn * us[1], sn * us[0] + c * us[1], us[2]])
        rows = [row(k) for k in range(min(s, n_poles)) if (s + k) % 3 != 0]
        if s < n_poles:
            rows.insert(len(rows) // 2, row(s))
        u.append(us)
        z.append(np.array(rows).reshape(-1, 2))
    return {"u": u, "z": z}


def filter_states(ekf, u, z, x0=None):
    """EKF.estimate step by step, as host_filter of test_gpu_landmark_bounds.py, keeping every state on the way:
    entry t is (x, P, landmark counts, status) after the first t steps."""
    x = np.zeros((3, 1)) if x0 is None else np.array(x0, dtype=float).reshape(3, 1)
    P, nlm = np.eye(3), []
    states = [(x[:, 0].copy(), P.copy(), [], 0)]
    for us, zs in zip(u, z):
        xb, Pb = copy.deepcopy(x), copy.deepcopy(P)
        rows = np.zeros((0, 3)) if len(zs) == 0 else np.hstack([np.asarray(zs, dtype=float), np.zeros((len(zs), 1))])
        try:
            x, P = ekf.estimate(x, P, rows, np.array(us, dtype=float).reshape(3, 1))
        except ValueError:
            states.append((xb[:, 0].copy(), Pb.copy(), list(nlm), 1))
            break
        nlm.append((len(x) - 3) // 2)
        states.append((x[:, 0].copy(), P.copy(), list(nlm), 0))
    return states


def nudge_stability(ekf, drive, eps=1e-12, runs=4, seed=99):
    """(states of the drive, worst move of x and P over `runs` re-runs with every observation row moved by a uniform
    +-eps; inf if a landmark count or the status changes); the drive may carry its start pose as "x0".  The pattern is
    loc_ref.stable: association and the append rule are discontinuous, and a drive is usable when nothing jumps."""
    ref = filter_states(ekf, drive["u"], drive["z"], drive.get("x0"))
    rng = np.random.default_rng(seed)
    worst = 0.0
    for _ in range(runs):
        z = [zs + rng.uniform(-eps, eps, size=zs.shape) for zs in drive["z"]]
        got = filter_states(ekf, drive["u"], z, drive.get("x0"))
        if len(got) != len(ref):
            return ref, float("inf")
        for (x, P, nlm, st), (xr, Pr, nr, sr) in zip(got, ref):
            if nlm != nr or st != sr:
                return ref, float("inf")
            worst = max(worst, float(np.max(np.abs(x - xr))), float(np.max(np.abs(P - Pr))))
    return ref, worst


def first_step_with(states, count):
    """Number of steps after which the landmark count is `count` for the first time."""
    return next(t for t, s in enumerate(states) if s[2] and s[2][-1] == count)


# ---- extraction ------------------------------------------------------------------------------

def landmark_lds_bytes(n):
    """landmark_lds_bytes of landmark_kernels.hip: two doubles per beam, four index arrays (two of n, two of n + 1
    words) and 8 bytes of alignment."""
    return n * 16 + (4 * n + 2) * 4 + 8


def pole_row(k, tail=()):
    """Ranges along +x (angle_min = angle_max = 0): k times a 3-beam cluster and one far beam - one landmark per
    4 beams, the far beam closing the cluster before it - then `tail`."""
    row = []
    for j in range(k):
        x0 = 1.0 + 0.01 * (j % 97)
        row += [x0, x0 + 0.0005, x0 + 0.001, 20.0 + 0.25 * (j % 13)]
    return np.array(row + list(tail), dtype=np.float32)


def row_of_length(n):
    """n beams: pole-sized clusters at both ends of the scan, a wall (too wide for a landmark) and far beams between."""
    head, tail = pole_row(3), pole_row(2, tail=(9.0,))
    mid = n - len(head) - len(tail)
    wall = [3.0 + 0.002 * i for i in range(min(400, mid // 2))]
    fill = [25.0 if i % 2 else 12.0 for i in range(mid - len(wall))]
    row = np.concatenate([head, np.array(wall + fill, dtype=np.float32), tail])
    assert row.shape == (n,)
    return row


# ---- kept scans ------------------------------------------------------------------------------

N_SCAN = 130
EMPTY_AT = ((62, 63, 64, 65, 127, 128), tuple(range(1, 64)), (129,))


def with_empties_at(scans, places, empty):
    """`empty` inserted into `scans` so that it stands at every index of `places` of the result."""
    out = list(scans)
    for p in sorted(places):
        out.insert(p, empty)
    return np.array(out, dtype=np.float32)


def crowded_scan(scan, r=0.5):
    """`scan` with 3-beam poles at range `r` set into every stretch whose beams are all at least 1.2 m behind them:
    each is one more landmark (its neighbours on both sides are a gap away)."""
    out = np.array(scan, dtype=np.float32)
    for p in range(8, len(out) - 8, 24):
        if np.all(out[p - 3:p + 6] > r + 1.2):
            out[p:p + 3] = r
    return out


def host_counts(extraction, scans, amin, amax):
    """Landmarks per scan by Extraction.labels on the points SLAM_EKF.laserToNumpy forms (inf -> 30 m)."""
    ang = np.linspace(amin, amax, scans.shape[1])
    ct, st = np.cos(ang), np.sin(ang)
    counts = []
    for row in scans:
        r = row.astype(np.float64)
        r[np.isinf(r)] = 30.0
        counts.append(len(extraction.labels(np.vstack([ct * r, st * r]))[1]))
    return counts


def kept_rule(counts):
    """slam_ekf.py:74-82 on the landmark counts of one trajectory's scans."""
    return [k for k, c in enumerate(counts) if k == 0 or c >= 1]
