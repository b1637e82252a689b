"""NumPy restatement of the particle-filter operators (include/slam_hip.h, "Monte Carlo localisation on the distance
field"), written from their stated semantics on ``raycast_ref.to_cell`` and ``match_ref.field``:

    cost_scalar(...)     one particle's cost, beam by beam in Python floats: the matcher's expression
    weigh(...)           slam_mcl_weigh: motion, cost, dead particles, accumulation; the same float64 operations as
                         cost_scalar, beam by beam, over arrays of particles (IEEE: identical bits)
    resample(...)        slam_mcl_resample: weights, estimate, ESS, gate and systematic resampling, the ancestors
                         decided with Python integers (resample_ints) - or, from 4 096 particles up, by the same
                         comparison in uint64 (cum * P < 2^61), which test_mcl_ref.py pins to the Python one
    weight_table(...)    the table of mcl_weight_table

Plus the inputs the CPU and the GPU tests share (the room recovery case)."""
import numpy as np

import match_ref as M
import raycast_ref as R

DEAD = 2 ** 31 - 1
ACC_MAX = 1 << 30
W_MAX = 1 << 20


def weight_table(sigma_cells, shift=0, T=4096, floor=0):
    k = np.arange(int(T), dtype=np.int64) << int(shift)
    t = np.rint(float(W_MAX) * np.exp(-k.astype(np.float64) / (2.0 * float(sigma_cells) ** 2)))
    return np.maximum(t, float(floor)).astype(np.uint32)


def used_beams(ranges, cos_t, sin_t, max_range):
    """[(lx, ly)] of the used beams, in beam order."""
    ranges = np.asarray(ranges, dtype=np.float32)
    mr = np.float32(max_range)
    out = []
    for t in range(len(ranges)):
        rr = float(ranges[t])
        if np.isfinite(rr) and ranges[t] < mr:
            out.append((float(cos_t[t]) * rr, float(sin_t[t]) * rr))
    return out


def cost_scalar(fld, scale, off_x, off_y, beams, px, py, c, s, cap):
    xw, yw = fld.shape
    cost = 0
    for lx, ly in beams:
        x = c * lx + (-s) * ly + px * 1.0
        y = s * lx + c * ly + py * 1.0
        ex, ey = R.to_cell(x, scale, off_x), R.to_cell(y, scale, off_y)
        cost += int(fld[ex][ey]) if ex is not None and ey is not None and 0 <= ex < xw and 0 <= ey < yw else cap
    return cost


def _cells(v, scale, off):
    """to_cell over an array: (index int64, ok)."""
    with np.errstate(all="ignore"):
        c = scale * (v + off)
        ok = ~np.isnan(c) & (np.abs(c) < R.MAX_CELL)
        return np.where(ok, np.trunc(np.where(ok, c, 0.0)), 0.0).astype(np.int64), ok


def _costs(fld, scale, off_x, off_y, beams, px, py, c, s, cap):
    """cost_scalar for arrays of particles: the same operations in the same order, one beam at a time."""
    xw, yw = fld.shape
    cost = np.zeros(px.shape, dtype=np.int64)
    f64 = fld.astype(np.int64)
    with np.errstate(all="ignore"):
        for lx, ly in beams:
            x = c * lx + (-s) * ly + px * 1.0
            y = s * lx + c * ly + py * 1.0
            ex, okx = _cells(x, scale, off_x)
            ey, oky = _cells(y, scale, off_y)
            inb = okx & oky & (ex >= 0) & (ex < xw) & (ey >= 0) & (ey < yw)
            cost += np.where(inb, f64[np.where(inb, ex, 0), np.where(inb, ey, 0)], cap)
    return cost


def move(poses, motion=None, noise=None):
    """The pose step's composition (icp.py:185-190) with d = motion[f] + noise[f][p]; a copy when motion is None."""
    poses = np.array(poses, dtype=np.float64)
    F, P, _ = poses.shape
    if motion is None:
        return poses
    d = np.asarray(motion, dtype=np.float64).reshape(F, 1, 3)
    d = d + np.asarray(noise, dtype=np.float64).reshape(F, P, 3) if noise is not None else np.broadcast_to(d, (F, P, 3))
    with np.errstate(all="ignore"):
        c0, s0 = np.cos(poses[..., 2]), np.sin(poses[..., 2])
        x = (poses[..., 0] + c0 * d[..., 0]) - s0 * d[..., 1]
        y = (poses[..., 1] + s0 * d[..., 0]) + c0 * d[..., 1]
        return np.stack([x, y, poses[..., 2] + d[..., 2]], axis=-1)


def weigh(fields, scale, off_x, off_y, poses, ranges, cos_t, sin_t, max_range, cap, motion=None, noise=None, maps=None,
          acc=None, moved=None, ulp=False):
    """slam_mcl_weigh.  fields [G, xw, yw]; poses [F, P, 3]; ranges [F, n].  Returns a dict: poses (after the motion),
    cost [F, P], acc [F, P] (None without acc), used [F] and, with ``ulp``, unsure [F, P]: the live particles whose
    cost changes when the cosine or the sine of the heading is moved one ulp either way.  ``moved``: poses to take the
    cost from instead of the restated motion's (the device's own, which may differ from it in the last place)."""
    poses = move(poses, motion, noise)
    F, P, _ = poses.shape
    ranges = np.asarray(ranges, dtype=np.float32).reshape(F, -1)
    src = poses if moved is None else np.asarray(moved, dtype=np.float64).reshape(F, P, 3)
    cost = np.full((F, P), -1, dtype=np.int32)
    used = np.zeros(F, dtype=np.int32)
    unsure = np.zeros((F, P), dtype=bool)
    new_acc = None if acc is None else np.array(acc, dtype=np.int32).reshape(F, P)
    for f in range(F):
        beams = used_beams(ranges[f], cos_t, sin_t, max_range)
        used[f] = len(beams)
        gi = 0 if maps is None else int(maps[f])
        px, py, th = src[f, :, 0], src[f, :, 1], src[f, :, 2]
        live = np.isfinite(px) & np.isfinite(py) & np.isfinite(th) & _cells(px, scale, off_x)[1] & _cells(py, scale, off_y)[1]
        if not 0 <= gi < len(fields):
            live[:] = False
        if new_acc is not None:
            live &= new_acc[f] != DEAD
        idx = np.flatnonzero(live)
        if len(idx):
            c, s = np.cos(th[idx]), np.sin(th[idx])
            k = _costs(fields[gi], scale, off_x, off_y, beams, px[idx], py[idx], c, s, cap)
            cost[f, idx] = k
            if ulp:
                bad = np.zeros(len(idx), dtype=bool)
                for cc in (np.nextafter(c, -np.inf), c, np.nextafter(c, np.inf)):
                    for ss in (np.nextafter(s, -np.inf), s, np.nextafter(s, np.inf)):
                        if cc is not c or ss is not s:
                            bad |= _costs(fields[gi], scale, off_x, off_y, beams, px[idx], py[idx], cc, ss, cap) != k
                unsure[f, idx] = bad
        if new_acc is not None:
            tot = np.minimum(new_acc[f].astype(np.int64) + cost[f], ACC_MAX)
            new_acc[f] = np.where(live, tot, DEAD).astype(np.int32)
    return dict(poses=poses, cost=cost, acc=new_acc, used=used, unsure=unsure)


def is_unsure(fld, scale, off_x, off_y, beams, pose, cap):
    """Does one ulp either way in the cosine or the sine of the heading change this particle's cost?"""
    px, py, th = (float(v) for v in pose)
    c, s = float(np.cos(th)), float(np.sin(th))
    k = cost_scalar(fld, scale, off_x, off_y, beams, px, py, c, s, cap)
    return any(cost_scalar(fld, scale, off_x, off_y, beams, px, py, cc, ss, cap) != k
               for cc in (float(np.nextafter(c, -np.inf)), c, float(np.nextafter(c, np.inf)))
               for ss in (float(np.nextafter(s, -np.inf)), s, float(np.nextafter(s, np.inf))))


def weights(acc, table, shift):
    """(w int64 [P], amin, best, live) of one filter."""
    acc = np.asarray(acc, dtype=np.int64)
    table = np.minimum(np.asarray(table, dtype=np.int64), W_MAX)
    live = acc != DEAD
    if not live.any():
        return np.zeros(len(acc), dtype=np.int64), 0, -1, 0
    amin = int(acc[live].min())
    best = int(np.flatnonzero(live & (acc == amin))[0])
    idx = np.minimum((np.where(live, acc, amin) - amin) >> int(shift), len(table) - 1)
    return np.where(live, table[idx], 0), amin, best, int(live.sum())


def offset(u0, S):
    return min(int(float(u0) * float(S)), S - 1)


def resample_ints(w, u0):
    """Ancestors of systematic resampling with Python integers: a_j = the smallest i with cum[i] * P > o + j * S."""
    w = [int(v) for v in w]
    P, S = len(w), sum(w)
    o = offset(u0, S)
    anc, i, cum = [], 0, w[0]
    for j in range(P):
        t = o + j * S
        while not cum * P > t:
            i += 1
            cum += w[i]
        anc.append(i)
    return np.array(anc, dtype=np.int32)


def resample_u64(w, u0):
    """The same comparison in uint64: w <= 2^20 and P <= 2^20 keep both sides below 2^61."""
    w = np.asarray(w, dtype=np.uint64)
    P, S = len(w), int(w.sum())
    t = np.uint64(offset(u0, S)) + np.arange(P, dtype=np.uint64) * np.uint64(S)
    return np.searchsorted(np.cumsum(w) * np.uint64(P), t, side="right").astype(np.int32)


def resample(poses, acc, table, shift, u0, ess_frac):
    """slam_mcl_resample.  Returns a dict: poses [F, P, 3], acc, ancestors int32 [F, P], est [F, 4], info int32 [F, 4]."""
    poses = np.asarray(poses, dtype=np.float64)
    F, P, _ = poses.shape
    acc = np.array(acc, dtype=np.int32).reshape(F, P)
    out = poses.copy()
    anc = np.tile(np.arange(P, dtype=np.int32), (F, 1))
    est = np.full((F, 4), np.nan)
    info = np.zeros((F, 4), dtype=np.int32)
    for f in range(F):
        w, amin, best, live = weights(acc[f], table, shift)
        S, Q = int(w.sum()), int((w * w).sum())
        ess = float(S) * float(S) / float(Q) if S else 0.0
        if S:
            nz = w > 0
            wd = w[nz].astype(np.float64)
            est[f, :3] = (np.sum(wd * poses[f, nz, 0]) / float(S), np.sum(wd * poses[f, nz, 1]) / float(S),
                          np.arctan2(np.sum(wd * np.sin(poses[f, nz, 2])), np.sum(wd * np.cos(poses[f, nz, 2]))))
        est[f, 3] = ess
        go = S > 0 and ess < float(ess_frac) * float(P)
        info[f] = (best, live, int(go), amin)
        if go:
            anc[f] = resample_ints(w, u0[f]) if P < 4096 else resample_u64(w, u0[f])
            out[f] = poses[f, anc[f]]
            acc[f] = 0
    return dict(poses=out, acc=acc, ancestors=anc, est=est, info=info)


# ---------------------------------------------------------------- the room recovery case (issue text)
# The map is the room map (the six scans of raycast_ref.room); the filter then follows the ten scans with which the same
# seeded trajectory goes on, moved by that trajectory's own odometry (the true pose step in the robot frame) plus seeded
# noise.  P = 4096 particles drawn within +-0.3 m / +-0.1 rad of the true pose of the room's last scan.
REC = dict(P=4096, steps=10, spread=(0.3, 0.3, 0.1), sigma_cells=2.0, shift=0, T=4096, cap=64, max_range=30.0, ess_frac=0.5,
           noise=(0.01, 0.01, 0.005))
REC_BOUND = (0.05, 0.02)                # metres (one cell), radians

_rec = {}


def odometry(p0, p1):
    """The step d with which the pose step's formula takes p0 to p1."""
    c, s = np.cos(p0[2]), np.sin(p0[2])
    dx, dy = p1[0] - p0[0], p1[1] - p0[1]
    return np.array([c * dx + s * dy, -s * dx + c * dy, p1[2] - p0[2]])


def recovery_case(syn):
    """Inputs of the recovery case, made once per process: pmap, field, beam tables, table, particles [1, P, 3], scans
    [steps, n], motion [steps, 3], noise [steps, P, 3], u0 [steps], true poses [steps, 3]."""
    if not _rec:
        room = M.room_case(syn)
        steps, P = REC["steps"], REC["P"]
        rep = syn.make_replay(6 + steps, 120, seed=4)
        ranges, poses = np.asarray(rep.ranges, dtype=np.float32), np.asarray(rep.poses_true, dtype=np.float64)
        assert np.array_equal(ranges[:6], room["ranges"]) and np.array_equal(poses[:6], room["poses"])
        rng = np.random.default_rng(0)
        parts = poses[5] + rng.uniform(-1.0, 1.0, (P, 3)) * np.array(REC["spread"])
        _rec.update(pmap=room["pmap"], field=room["field"], cos_t=room["cos_t"], sin_t=room["sin_t"],
                    table=weight_table(REC["sigma_cells"], REC["shift"], REC["T"]), particles=parts[None],
                    scans=ranges[6:], true=poses[6:], motion=np.stack([odometry(poses[5 + k], poses[6 + k]) for k in range(steps)]),
                    noise=rng.normal(0.0, 1.0, (steps, P, 3)) * np.array(REC["noise"]), u0=rng.uniform(0.0, 1.0, steps))
    return _rec


def recovery_run(case):
    """The ten steps in the restatement: est [steps, 4], info [steps, 4], the final particles."""
    poses = case["particles"]
    acc = np.zeros((1, REC["P"]), dtype=np.int32)
    est, info = [], []
    for k in range(REC["steps"]):
        w = weigh(case["field"][None], 20.0, 10.0, 10.0, poses, case["scans"][k][None], case["cos_t"], case["sin_t"], REC["max_range"],
                  REC["cap"], motion=case["motion"][k][None], noise=case["noise"][k][None], acc=acc)
        r = resample(w["poses"], w["acc"], case["table"], REC["shift"], case["u0"][k:k + 1], REC["ess_frac"])
        poses, acc = r["poses"], r["acc"]
        est.append(r["est"][0])
        info.append(r["info"][0])
    return np.array(est), np.array(info), poses


def pose_error(est, true):
    d = est[2] - true[2]
    return float(np.hypot(est[0] - true[0], est[1] - true[1])), float(abs(np.arctan2(np.sin(d), np.cos(d))))


# ---------------------------------------------------------------- weigh cases on the ring map (shared with the GPU tests)
RING = dict(scale=1.0, off_x=0.0, off_y=0.0)
# (F, P, n, seed): lane, wave and workgroup edges of P; beam counts around a wave; the scan past one block (65 537)
# and the scan of block sums past one block (2^20) with 8 beams; many small filters
RING_SHAPES = [(1, 1, 24, 1), (1, 63, 24, 2), (2, 64, 24, 3), (1, 65, 24, 4), (1, 255, 24, 5), (2, 257, 24, 6), (1, 1025, 24, 7),
               (2, 40, 1, 8), (1, 40, 63, 9), (1, 40, 65, 10), (1, 40, 120, 11), (1, 65537, 8, 12), (1, 1 << 20, 8, 13), (4096, 16, 8, 14)]


def ring_case(F, P, n, seed, spread=3.0):
    """Seeded particles around the middle of the 64 x 64 ring map (raycast_ref.ring_pmap), beams that end around its
    rings, a motion and noise: a dict of poses [F, P, 3], ranges [F, n], cos_t, sin_t, motion [F, 3], noise [F, P, 3]."""
    rng = np.random.default_rng(seed)
    ang = np.linspace(-3.0, 3.0, n) if n > 1 else np.array([0.3])
    poses = np.concatenate([32.5 + rng.uniform(-spread, spread, (F, P, 2)), rng.uniform(-3.0, 3.0, (F, P, 1))], axis=-1)
    return dict(poses=poses, ranges=rng.uniform(5.0, 20.0, (F, n)).astype(np.float32), cos_t=np.cos(ang), sin_t=np.sin(ang),
                motion=rng.uniform(-0.5, 0.5, (F, 3)), noise=rng.normal(0.0, 0.1, (F, P, 3)))
