"""Seeded cases for the landmark filter and the node around it (test infrastructure only): slam_ekf_lm / slam_ekf_lm_dev
and slam_node_replay where the association is ambiguous.  The third sweep, in the shape of tests/map_cases.py and
tests/plan_cases.py, whose helpers it uses.

    case_of(kind, seed) -> dict     a pure function of (kind, seed): numpy.random.default_rng([KIND_ID[kind], seed]) is the
                                    only source of randomness (the gate rows are found with the package's host class EKF,
                                    which is deterministic)
    answer(case)                    per trajectory what the host class says of it, with the marks `margin` and `moved`

An `ekf` case is one slam_ekf_lm call: B trajectories of different lengths, each of one style (STYLES below).  What the
styles are for: the reference appends at most ONE landmark a step - its n1 is never refreshed - so a second never-seen pole
in a step ends the step early (before the yaw wrap) or, when it falls under the gate of the landmark just appended, raises;
two poles closer than the gate resolves put several distances under 0.6, and the first minimum decides.
A `node` case is one slam_node_replay call on synthetic worlds with such poles.

To reproduce a failure:  python -c "import filter_cases as F; print(F.case_of('ekf', 17))"  from tests/."""
import copy
import math

import numpy as np

import landmark_cases as lc
from map_cases import SMALL, pick, seeds, size  # noqa: F401  (seeds is re-exported for the two test files)

KINDS = ("ekf", "node")
KIND_ID = {k: i + 201 for i, k in enumerate(KINDS)}     # map_cases.py has 1 .. 8, plan_cases.py 101 .. 105

GATE = 0.6                                # M_DIST_TH of ekf_lm.py
SURE_MARGIN, SURE_MOVED, NUDGE = 1e-6, 1e-10, 1e-12
OK, RAISES, LM_CAP, OBS_CAP = 0, 1, 2, 3  # SLAM_NODE_* of include/slam_hip.h


def rng_of(kind, seed):
    return np.random.default_rng([KIND_ID[kind], int(seed)])


# ---------------------------------------------------------------- the host class, with its decisions written down
_recording = None


def recording_ekf():
    """The package's EKF with a log: per estimate call the state size it started from (`n1`) and, per observation row it
    looked at, the list of distances (threshold entry last) and the chosen index; `wraps` counts the innovations whose
    bearing left [-pi, pi) before the outer pi_2_pi.  Every number comes from the class's own methods."""
    global _recording
    if _recording is None:
        from conftest import pkg
        mod = pkg("ekf_lm")

        class Recording(mod.EKF):
            def __init__(self):
                self.n1, self.rows, self.wraps, self._angles = 3, [], 0, []

            def pi_2_pi(self, angle):
                self._angles.append(float(np.asarray(angle).reshape(-1)[0]))
                return super().pi_2_pi(angle)

            def laser_correction(self, lm, xEst, PEst, z, LMid):
                k = len(self._angles)
                out = super().laser_correction(lm, xEst, PEst, z, LMid)
                if abs(self._angles[k + 1]) > math.pi:           # the argument of the outer pi_2_pi (ekf_lm.py:118)
                    self.wraps += 1
                del self._angles[:]
                return out

            def search_correspond_landmark_id(self, xAug, PAug, zi):
                dists = []
                for i in range((len(xAug) - 3) // 2):
                    y, S, _ = self.laser_correction(self.get_landmark_position_from_state(xAug, i), xAug, PAug, zi, i)
                    dists.append(float(np.dot(np.dot(y.T, np.linalg.inv(S)), y)[0, 0]))
                dists.append(mod.M_DIST_TH)
                best = super().search_correspond_landmark_id(xAug, PAug, zi)
                self.rows.append((dists, int(best), len(xAug)))
                return best

            def estimate(self, xEst, PEst, z, u):
                self.n1 = len(xEst)
                del self.rows[:]
                return super().estimate(xEst, PEst, z, u)

        _recording = Recording
    return _recording()


def branches(n1, rows):
    """[(dists, chosen, branch)] of one estimate call from the recording's rows: ekf_lm.py:36-42 with its stale n1."""
    num_lm = (n1 - 3) // 2
    out = []
    for dists, best, size_now in rows:
        nlm = (size_now - 3) // 2
        if best == num_lm:
            branch = "appended" if nlm == num_lm else "raises"
        else:
            branch = "early" if best == nlm else "matched"
        out.append((dists, best, branch))
    return out


def gap(dists):
    """Winner to runner-up of one decision (inf when the threshold entry stands alone)."""
    a = sorted(dists)
    return a[1] - a[0] if len(a) > 1 else math.inf


def host_run(u, z, x0, max_lm):
    """EKF.estimate step by step as slam_ekf_lm defines the stops: from the step at which the reference raises (status 1) or
    the state would pass max_lm (status 2) the trajectory keeps the state it had before that step.  Returns a dict: x, P
    (final), nlm (after every step that happened), status, steps [(x, P, [(dists, chosen, branch)])] for every step that
    was started - a stopped step with the state before it - and wraps."""
    ekf = recording_ekf()
    x, P = np.array(x0, dtype=float).reshape(3, 1), np.eye(3)
    nlm, status, steps = [], OK, []
    with np.errstate(all="ignore"):
        for us, zs in zip(u, z):
            xb, Pb = copy.deepcopy(x), copy.deepcopy(P)           # the prediction writes into its arguments
            zs = np.asarray(zs, dtype=float).reshape(-1, 2)
            rows = np.hstack([zs, np.zeros((len(zs), 1))])
            try:
                x, P = ekf.estimate(x, P, rows, np.array(us, dtype=float).reshape(3, 1))
            except ValueError:
                status = RAISES
            log = branches(ekf.n1, ekf.rows)
            if (ekf.n1 - 3) // 2 == max_lm and any(b == "appended" for _, _, b in log):
                status = LM_CAP                                    # the kernel stops at the append, whatever follows it
                log = log[:[b for _, _, b in log].index("appended") + 1]
            if status != OK:
                x, P = xb, Pb
                steps.append((x[:, 0].copy(), P.copy(), log))
                break
            nlm.append((len(x) - 3) // 2)
            steps.append((x[:, 0].copy(), P.copy(), log))
    return dict(x=x[:, 0].copy(), P=P.copy(), nlm=nlm, status=status, steps=steps, wraps=ekf.wraps)


# ---------------------------------------------------------------- drives
STYLES = ("pairs", "near", "far", "ring", "gate", "wrap", "burst", "cap", "quiet")
MAX_LMS = (1, 2, 3, 8, 16, 32)
MAX_LMS_P = (0.07, 0.08, 0.10, 0.30, 0.25, 0.20)
PAIR_GAPS = (0.05, 0.3, 0.8)
RANGE_NOISE, BEARING_NOISE = (0.0, 0.01, 0.2), (0.0, 0.002, 0.05)
DROP = 0.35
GATE_FACTORS = (0.5, 0.9, 1.1, 2.0)
STEPS = (1, 2, 5, 9, 14)
ODOMETRY = np.array([0.25, 0.01, 0.2])     # circle_drive's, tests/test_gpu_landmark_bounds.py
NONFINITE = ("nan", "inf", "zero")
CAP_ROWS = 3.0                             # the 50-digit restatement of a 67 x 67 update takes about 30 ms


def advance(pose, us):
    c, s = math.cos(pose[2]), math.sin(pose[2])
    return pose + np.array([c * us[0] - s * us[1], s * us[0] + c * us[1], us[2]])


def odometry(rng, steps, turn=None):
    u = ODOMETRY + rng.normal(0, [0.01, 0.005, 0.01], (steps, 3))
    if turn is not None:
        u[:, 2] = turn * np.where(rng.random(steps) < 0.8, 1.0, -1.0) + rng.normal(0, 0.01, steps)
    return u


def path_of(x0, u):
    """The true poses after every step: the odometry is exact, the noise sits on the rows."""
    poses, pose = [], np.array(x0, dtype=float)
    for us in u:
        pose = advance(pose, us)
        poses.append(pose)
    return np.array(poses).reshape(-1, 3)


def row_of(rng, pose, pole, noise, wrapped):
    dx, dy = pole[0] - pose[0], pole[1] - pose[1]
    b = math.atan2(dy, dx) - pose[2] + rng.normal(0, 1) * noise[1]      # the true yaw is never wrapped: |b| passes pi
    if wrapped:
        b = (b + math.pi) % (2 * math.pi) - math.pi
    return [math.hypot(dx, dy) + rng.normal(0, 1) * noise[0], b]


def observe(rng, poses, poles, noise, wrapped, view=math.inf, show=None, drop=DROP, quiet=()):
    """Rows per step: every pole within `view` that `show(step, pole)` lets through and that does not drop out, shuffled."""
    z = []
    for s, pose in enumerate(poses):
        rows = []
        for k, p in enumerate(poles):
            seen = s not in quiet and math.hypot(p[0] - pose[0], p[1] - pose[1]) <= view and (show is None or show(s, k))
            if seen and rng.random() >= drop:
                rows.append(row_of(rng, pose, p, noise, wrapped))
        rows = [rows[i] for i in rng.permutation(len(rows))]
        z.append(np.array(rows, dtype=np.float64).reshape(-1, 2))
    return z


def around(rng, centre, k, lo, hi):
    a, r = rng.uniform(-math.pi, math.pi, k), rng.uniform(lo, hi, k)
    return [(centre[0] + r[i] * math.cos(a[i]), centre[1] + r[i] * math.sin(a[i])) for i in range(k)]


def spaced(rng, centre, k, lo, hi, apart):
    """k poles around `centre`, each at least `apart` from the others (fewer when they do not fit in 200 draws)."""
    out = []
    for _ in range(200):
        if len(out) == k:
            break
        p = around(rng, centre, 1, lo, hi)[0]
        if all(math.hypot(p[0] - q[0], p[1] - q[1]) >= apart for q in out):
            out.append(p)
    return out


def traj_of(rng, seed, style, max_lm):
    """One trajectory: dict with style, x0, u [T, 3], z (T arrays [m, 2]) and what the style adds."""
    x0 = np.array([rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(-math.pi, math.pi)])
    noise = (float(RANGE_NOISE[int(rng.integers(3))]), float(BEARING_NOISE[int(rng.integers(3))]))
    wrapped = bool(rng.random() < 0.5)
    T = int(pick(rng, seed, STEPS))
    few = max(1, min(max_lm, 6)) if rng.random() < 0.85 else 6          # mostly no more poles than the state holds
    t = dict(style=style, x0=x0, noise=noise, wrapped=wrapped)
    if style == "pairs":
        u = odometry(rng, T)
        poles = []
        for c in spaced(rng, x0, max(1, few // 2), 2.0, 6.0, 2.0):
            g, a = float(PAIR_GAPS[int(rng.integers(3))]), rng.uniform(-math.pi, math.pi)
            poles += [c, (c[0] + g * math.cos(a), c[1] + g * math.sin(a))]
        first = rng.integers(0, 2, len(poles) // 2)                     # one pole of a pair shows a step before the other
        z = observe(rng, path_of(x0, u), poles, noise, wrapped, show=lambda s, k: s > (k // 2) + (k % 2 != first[k // 2]) - 1)
        t.update(poles=poles)
    elif style == "near":
        u = odometry(rng, T)
        poses = path_of(x0, u)
        poles = [around(rng, poses[int(rng.integers(T))], 1, 0.15, 1.0)[0] for _ in range(few)]
        z = observe(rng, poses, poles, noise, wrapped, show=lambda s, k: s >= k)
        t.update(poles=poles)
    elif style == "far":
        u = odometry(rng, T)
        poles = spaced(rng, x0, few, 5.0, 25.0, 3.0)
        z = observe(rng, path_of(x0, u), poles, noise, wrapped, show=lambda s, k: s >= k)
        t.update(poles=poles)
    elif style == "ring":
        u = odometry(rng, T)
        r, a0 = rng.uniform(2.0, 6.0), rng.uniform(-math.pi, math.pi)
        poles = [(x0[0] + r * math.cos(a0 + 2 * math.pi * i / few), x0[1] + r * math.sin(a0 + 2 * math.pi * i / few)) for i in range(few)]
        z = observe(rng, path_of(x0, u), poles, noise, wrapped, show=lambda s, k: s >= k)
        t.update(poles=poles)
    elif style == "wrap":
        u = odometry(rng, max(T, 5), turn=1.5)
        poses = path_of(x0, u)
        # behind the robot at every other step: the bearing sits next to +-pi, and the noise puts it on either side
        poles = [(poses[s][0] - d * math.cos(poses[s][2]), poses[s][1] - d * math.sin(poses[s][2]))
                 for s, d in zip(range(0, len(poses), 2), rng.uniform(2.0, 5.0, len(poses)))][:few]
        # two new poles a step: one is appended, the other returns early, before the wrap of a yaw that turned by 1.5
        z = observe(rng, poses, poles, (noise[0], max(noise[1], 0.002)), wrapped, show=lambda s, k: s >= (k + 1) // 2, drop=0.2)
        t.update(poles=poles)
    elif style == "quiet":
        u = odometry(rng, max(T, 9) + int(rng.integers(0, 12)))
        quiet, s = set(), int(rng.integers(0, 3))
        while s < len(u):
            run = int(rng.integers(3, 9))
            quiet.update(range(s, s + run))
            s += run + int(rng.integers(1, 4))
        poles = spaced(rng, x0, few, 2.0, 7.0, 1.5)
        z = observe(rng, path_of(x0, u), poles, noise, wrapped, show=lambda s, k: True, quiet=quiet)
        first = next((s for s in range(len(u)) if s not in quiet), None)
        if first is not None and len(z[first]) > 1:                     # one landmark to start from, not an early return
            z[first] = z[first][:1]
        t.update(poles=poles, quiet=sorted(q for q in quiet if q < len(u)))
    elif style == "burst":
        u = odometry(rng, max(T, 5))
        poses = path_of(x0, u)
        at0 = bool(rng.random() < 0.4)                                  # the first burst in step 0, where num_lm == 0
        b1 = 0 if at0 else int(rng.integers(1, 3))
        b2 = b1 + int(rng.integers(1, 3))
        known = spaced(rng, x0, 0 if at0 else min(few, b1), 2.0, 6.0, 2.0)
        fresh = []
        for n_new in (2, 3):
            close = bool(rng.random() < 0.5)                            # under the gate of the one just appended: raises
            c = spaced(rng, x0, 1, 2.0, 6.0, 0.0)[0]
            grp = [c] + ([(c[0] + d * math.cos(a), c[1] + d * math.sin(a)) for d, a in
                          zip(rng.uniform(0.02, 0.15, n_new - 1), rng.uniform(-math.pi, math.pi, n_new - 1))] if close else
                         spaced(rng, c, n_new - 1, 2.5, 5.0, 2.5))
            fresh.append(grp)
        poles = known + fresh[0] + fresh[1]
        k0, k1 = len(known), len(known) + 2

        def show(s, k):
            if k < k0:
                return s >= k
            return s >= (b1 if k < k1 else b2)
        z = observe(rng, poses, poles, noise, wrapped, show=show, drop=0.0)
        t.update(poles=poles, bursts=(b1, b2))
    elif style == "cap":
        over = bool(rng.random() < 0.5)                                  # reaches max_lm exactly, or would pass it
        n_poles = max_lm + (1 if over else 0)
        u = odometry(rng, n_poles + int(rng.integers(1, 4)))
        poles = spaced(rng, x0, n_poles, 2.0, 4.0 + 0.4 * n_poles, 1.6)
        while len(poles) < n_poles:                                      # (a crowded draw: further out)
            poles += spaced(rng, x0, n_poles - len(poles), 5.0 + 0.4 * n_poles, 30.0, 1.6)
        new_row = rng.random(len(u))

        # pole s shows for the first time in step s and never drops out there; the older ones come and go
        z = []
        for s, pose in enumerate(path_of(x0, u)):
            stay = min(1.0 - DROP, CAP_ROWS / max(s, 1))                  # about CAP_ROWS old poles a step in a long one
            rows = [row_of(rng, pose, poles[k], noise, wrapped) for k in range(min(s, n_poles)) if rng.random() < stay]
            if s < n_poles:
                rows.insert(int(new_row[s] * (len(rows) + 1)), row_of(rng, pose, poles[s], noise, wrapped))
            z.append(np.array(rows, dtype=np.float64).reshape(-1, 2))
        t.update(poles=poles, over=over)
    elif style == "gate":
        u = odometry(rng, int(rng.integers(3, 6)) + 1)
        poles = spaced(rng, x0, min(few, 3), 2.0, 6.0, 2.5)
        z = observe(rng, path_of(x0, u), poles, noise, wrapped, show=lambda s, k: s >= k)
        z[-1] = np.zeros((0, 2))
        t.update(poles=poles, factor=None)
    else:
        raise KeyError(style)
    t.update(u=np.ascontiguousarray(u, dtype=np.float64), z=z)
    if style == "gate":
        gate_row(rng, t, max_lm)
    return t


def mahalanobis(ekf, x, P, i, row):
    y, S, _ = ekf.laser_correction(ekf.get_landmark_position_from_state(x, i), x, P, np.asarray(row, dtype=float), i)
    return float(np.dot(np.dot(y.T, np.linalg.inv(S)), y)[0, 0])


def gate_row(rng, t, max_lm):
    """The last step of a gate trajectory gets one row on the ray to a chosen landmark of the host class's state, moved
    along the range axis (by bisection on the class's own distance) until that distance is `factor` times the threshold.
    Kept only when the row's margin to 0.6 is at least 1e-6 and every other landmark is further away than the gate."""
    from conftest import pkg
    ekf = pkg("ekf_lm").EKF()
    T = len(t["u"])
    ref = host_run(t["u"][:T - 1], t["z"][:T - 1], t["x0"], max_lm)
    if ref["status"] != OK or not ref["nlm"] or ref["nlm"][-1] == 0:
        return
    n = 3 + 2 * ref["nlm"][-1]
    x, P = ref["x"][:n].reshape(-1, 1).copy(), ref["P"][:n, :n].copy()
    x, P = ekf.estimate(x, P, np.zeros((0, 3)), t["u"][T - 1].reshape(3, 1))     # the state the step's first row meets
    i = int(rng.integers(ref["nlm"][-1]))
    factor = float(GATE_FACTORS[int(rng.integers(len(GATE_FACTORS)))])
    dx, dy = x[3 + 2 * i, 0] - x[0, 0], x[4 + 2 * i, 0] - x[1, 0]
    r0, b = math.hypot(dx, dy), math.atan2(dy, dx) - x[2, 0]
    lo, hi = 0.0, 20.0                                                   # the distance grows with the range offset
    if mahalanobis(ekf, x, P, i, (r0 + hi, b)) < factor * GATE:
        return
    for _ in range(100):
        mid = 0.5 * (lo + hi)
        if mahalanobis(ekf, x, P, i, (r0 + mid, b)) < factor * GATE:
            lo = mid
        else:
            hi = mid
    row = (r0 + hi, b)
    d = [mahalanobis(ekf, x, P, j, row) for j in range(ref["nlm"][-1])]
    if abs(d[i] - GATE) < SURE_MARGIN or any(dj <= GATE for j, dj in enumerate(d) if j != i):
        return
    t["z"][T - 1] = np.array([row], dtype=np.float64)
    t.update(factor=factor, gate_lm=i)


def spoil(rng, t, what):
    """One non-finite or degenerate row in front of a step: a NaN range, an inf range, or a range of exactly 0 (a landmark
    at the robot's own position when it is appended: q == 0 at once).  Returns the step."""
    T = len(t["u"])
    s = int(rng.integers(0, T))
    if what == "zero":
        s = 0                                                            # nothing to match yet: it is appended
    row = np.array([[{"nan": np.nan, "inf": np.inf, "zero": 0.0}[what], rng.uniform(-3.0, 3.0)]])
    t["z"][s] = np.vstack([row, t["z"][s]])
    t.update(spoiled=(s, what))
    return s


def case_ekf(rng, seed):
    B = int(rng.integers(1, 6))
    max_lm = int(MAX_LMS[int(rng.choice(len(MAX_LMS), p=MAX_LMS_P))])
    if seed % 6 == 1:
        max_lm = (1, 32)[(seed // 6) % 2]                               # both ends of the list, at seeds that are known
    styles = [STYLES[int(rng.integers(len(STYLES)))] for _ in range(B)]
    styles[0] = STYLES[seed % len(STYLES)]                              # every style takes its turn
    trajs = [traj_of(rng, seed, s, max_lm) for s in styles]
    if B > 1 and rng.random() < 0.5:                                    # one empty trajectory
        k = int(rng.integers(1, B))
        trajs[k].update(u=np.zeros((0, 3)), z=[], style="empty")
    run = []
    for t in trajs:                                                      # some step counts below the rows given
        T = len(t["u"])
        run.append(int(rng.integers(1, T + 1)) if T > 1 and t["style"] not in ("gate", "cap") and rng.random() < 0.25 else T)
    # the yaw an early return leaves outside [-pi, pi) is an output only when that step is the trajectory's last (a later
    # step wraps it, and everything else is periodic in it): some trajectories end there, by the host class's account
    for b, t in enumerate(trajs):
        if t["style"] in ("wrap", "burst", "pairs", "ring", "near", "far") and rng.random() < 0.6:
            r = host_run(t["u"][:run[b]], t["z"][:run[b]], t["x0"], max_lm)
            ends = [k for k, (x, _, log) in enumerate(r["steps"][:len(r["nlm"])]) if log and log[-1][2] == "early" and abs(x[2]) > math.pi]
            if ends:
                run[b] = ends[0] + 1
                t.update(ends_early=True)
    spoiled = None
    if seed % 10 == 7:
        live = [b for b, t in enumerate(trajs) if len(t["u"])]
        spoiled = live[int(rng.integers(len(live)))]
        s = spoil(rng, trajs[spoiled], NONFINITE[(seed // 10) % 3])
        run[spoiled] = max(run[spoiled], min(s + 2, len(trajs[spoiled]["u"])))
    return dict(B=B, max_lm=max_lm, trajs=trajs, run=run, spoiled=spoiled)


def packed(c, order=None):
    """The arrays of the slam_ekf_lm call: x0 [B][3], u [B][steps][3], step_counts [B], z_off [B * steps + 1], z [nz][2].
    Every trajectory's rows are given in full; step_counts says how many of its steps run.  ``order``: the trajectories
    of the call, by their index in the case (default: all, in the case's order)."""
    order = list(range(c["B"])) if order is None else list(order)
    trajs, B = [c["trajs"][b] for b in order], len(order)
    steps = max(1, max(len(t["u"]) for t in trajs))
    x0 = np.array([t["x0"] for t in trajs], dtype=np.float64).reshape(B, 3)
    u = np.zeros((B, steps, 3))
    off = np.zeros(B * steps + 1, dtype=np.int64)
    rows, total = [], 0
    for b, t in enumerate(trajs):
        u[b, :len(t["u"])] = t["u"]
        for s in range(steps):
            if s < len(t["u"]):
                rows.append(t["z"][s])
                total += len(t["z"][s])
            off[b * steps + s + 1] = total
    z = np.ascontiguousarray(np.concatenate(rows)) if total else np.zeros((0, 2))
    return dict(x0=x0, u=u, counts=np.array([c["run"][b] for b in order], dtype=np.int32), z_off=off, z=z, steps=steps, B=B)


def answer_ekf(c):
    """Per trajectory host_run of the steps that run, with `finite` (no NaN or inf anywhere in its rows or states),
    `margin` (the smallest winner-to-runner-up gap over its decisions, gate entry included), `moved` (nudge_stability of
    tests/landmark_cases.py at 1e-12 over the steps that happened) and `sure`."""
    from conftest import pkg
    out = []
    for t, run in zip(c["trajs"], c["run"]):
        u, z = t["u"][:run], t["z"][:run]
        r = host_run(u, z, t["x0"], c["max_lm"])
        r["finite"] = bool(all(np.all(np.isfinite(zs)) for zs in z) and np.all(np.isfinite(r["x"])) and np.all(np.isfinite(r["P"])))
        r["margin"] = min([gap(d) for _, _, log in r["steps"] for d, _, _ in log] + [math.inf])
        if not r["finite"]:
            r["margin"] = min([gap(d) for _, _, log in r["steps"] for d, _, _ in log if np.all(np.isfinite(d))] + [math.inf])
            r["moved"] = math.inf
        else:
            done = len(r["nlm"])
            with np.errstate(all="ignore"):
                r["moved"] = lc.nudge_stability(pkg("ekf_lm").EKF(), dict(u=list(u[:done]), z=list(z[:done]), x0=t["x0"]), eps=NUDGE)[1]
        r["sure"] = bool(r["finite"] and r["margin"] >= SURE_MARGIN and r["moved"] < SURE_MOVED)
        out.append(r)
    return out


# ---------------------------------------------------------------- the node
NODE_BEAMS = (120, 360, 361)
NODE_MAPS = (96, 200)
POLE_R = 0.08
AMIN, AMAX = -3.14159, 3.14159


def case_node(rng, seed):
    """1 .. 3 trajectories of 6 .. 14 scans in a room whose poles include one pair closer than the association gate
    resolves and one pole behind a range limit that the robot passes late (far_from: its beams read inf before)."""
    from conftest import pkg
    syn = pkg("synthetic")
    L = int(rng.integers(1, 4))
    n_scan = int(rng.integers(6, 15 if seed >= SMALL else 10))
    n = int(NODE_BEAMS[int(rng.integers(len(NODE_BEAMS)))])
    side = int(NODE_MAPS[int(rng.integers(len(NODE_MAPS)))])
    max_lm = int((2, 3, 8, 16)[int(rng.choice(4, p=(0.15, 0.15, 0.4, 0.3)))])
    lm_cap = int((2, 3, 8)[int(rng.choice(3, p=(0.15, 0.15, 0.7)))])
    scans, worlds = [], []
    for l in range(L):
        base = [(1.5, 1.0), (-1.8, -0.9), (0.5, -2.0), (-2.5, 1.5)]
        keep = [base[i] for i in rng.permutation(4)[:int(rng.integers(1, 4))]]
        a, g = rng.uniform(-math.pi, math.pi), rng.uniform(0.45, 0.8)
        c = keep[0]
        pair = (c[0] + g * math.cos(a), c[1] + g * math.sin(a))        # its partner stands `g` metres beside it
        late = (float(rng.uniform(-0.5, 0.5)), float(rng.uniform(2.6, 3.2)))
        world = syn.World(5.0, 4.0, tuple(keep + [pair, late]), POLE_R)
        s = int(rng.integers(1 << 20))
        poses = syn.trajectory(world, n_scan * 5, s)[::5]
        r = syn.scans_from_poses(world, poses, n, s)
        # the late pole: its beams read the wall behind it until the scan at which it enters the view
        enter = int(rng.integers(2, n_scan))
        hidden = syn.scans_from_poses(syn.World(5.0, 4.0, tuple(keep + [pair]), POLE_R), poses, n, s)
        r[:enter] = hidden[:enter]
        scans.append(r)
        worlds.append(dict(poles=keep + [pair, late], pair_gap=float(g), enter=enter, seed=s))
    return dict(L=L, n_scan=n_scan, n=n, side=side, reso=0.1, max_lm=max_lm, lm_cap=lm_cap, ranges=np.stack(scans).astype(np.float32),
                worlds=worlds)


def node_counts(c):
    """Landmarks per scan by the host class Extraction, per trajectory."""
    from conftest import pkg
    ex = pkg("extraction").Extraction()
    return [lc.host_counts(ex, c["ranges"][l], AMIN, AMAX) for l in range(c["L"])]


def obs_stop(c, counts):
    """The first kept scan after scan 0 that shows more than lm_cap landmarks (None: no such scan): slam_node_replay
    stops there with SLAM_NODE_OBS_CAP."""
    return next((k for k in lc.kept_rule(counts) if k > 0 and counts[k] > c["lm_cap"]), None)


def answer_node(c, host_node):
    """Per trajectory the result of ``host_node`` (tests/test_gpu_node_replay.py; it drives SLAM_EKF(landmarks=True), whose
    scan matcher and map are library calls, so this needs the device) on the scans before the trajectory's stop, with
    "stop": 0, SLAM_NODE_LM_CAP or SLAM_NODE_OBS_CAP (the reference's raise is host_node's own "raised")."""
    out = []
    for l, counts in enumerate(node_counts(c)):
        scans = c["ranges"][l]
        k = obs_stop(c, counts)
        ref = host_node(scans if k is None else scans[:k])
        stop = OK if k is None else OBS_CAP
        over = next((i for i, v in enumerate(ref["nlm"]) if v > c["max_lm"]), None)
        if over is not None:                                             # the kept step i + 1 is the one that would pass max_lm
            ref = host_node(scans[:ref["kept"][over + 1]])
            stop = LM_CAP
        if ref["raised"]:                                                # a raise follows an append in its own step: at max_lm
            stop = LM_CAP if (ref["nlm"][-1] if ref["nlm"] else 0) == c["max_lm"] else OK      # landmarks the append stops first
        ref["stop"] = stop
        out.append(ref)
    return out


# ---------------------------------------------------------------- the answers
def answer(case, host_node=None):
    if case["kind"] == "ekf":
        return answer_ekf(case)
    if case["kind"] == "node":
        return answer_node(case, host_node)
    raise KeyError(case["kind"])


MAKERS = dict(ekf=case_ekf, node=case_node)


def case_of(kind, seed):
    """The case of (kind, seed): a dict of plain Python values and NumPy arrays, with "kind" and "seed" in it."""
    c = MAKERS[kind](rng_of(kind, seed), int(seed))
    c.update(kind=kind, seed=int(seed))
    return c
