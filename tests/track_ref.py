"""slam_track (include/slam_track.h) restated in NumPy from its contract (test infrastructure only), on the restatements
of its parts: ``match_ref.match`` (through ``match_fast``, the same rule over arrays, pinned to it in
tests/test_track_cases.py), ``refine_ref.refine``, ``gridslam_ref.update_particles`` / ``pmap_of`` / ``fast_field``.

    predict(prev, motion)     the pose step of step 1 with math.cos / math.sin
    rot_table(c0, s0, cs)     the rotation table of step 3 from the written-out c0, s0
    first_ok(pose, geom)      step 2's test of a first scan's pose
    keep(...) / gate(...)     steps 4 and 5 on doubles
    track(...)                S scans of L trajectories, in place on the counters; returns state, poses, info, trace
    run_case(...)             the two "tracks better than odometry" cases of the issue, on the restatement
"""
import math

import numpy as np

import gridslam_ref as G
import match_ref as M
import mcl_ref as X
import raycast_ref as R
import refine_ref as RF

MATCHED, REFINED, INTEGRATED, LOST = 1, 2, 4, 8
DEFAULTS = dict(n_rot=11, rot_step=0.01, nx=4, ny=4, iters=10, damping=0.01, step_cells=0.5, step_rad=0.02, max_range=30.0, cap=64,
                min_used=1, gate_dist=0.2, gate_turn=0.1)


def rotations(n_rot, rot_step):
    off = (np.arange(int(n_rot)) - int(n_rot) // 2) * float(rot_step)
    return off, np.stack([np.cos(off), np.sin(off)], axis=-1)


def predict(prev, motion):
    x, y, th = (float(v) for v in prev)
    if motion is not None:
        dx, dy, dth = (float(v) for v in motion)
        c, s = (math.cos(th), math.sin(th)) if math.isfinite(th) else (math.nan, math.nan)
        x, y, th = (x + c * dx) - s * dy, (y + s * dx) + c * dy, th + dth
    return np.array([x, y, th])


def rot_table(c0, s0, rot_off_cs):
    cs = np.asarray(rot_off_cs, dtype=np.float64).reshape(-1, 2)
    return np.stack([c0 * cs[:, 0] - s0 * cs[:, 1], s0 * cs[:, 0] + c0 * cs[:, 1]], axis=-1)


def first_ok(pose, geom):
    scale, off_x, off_y = geom
    return bool(np.isfinite(pose).all()) and R.to_cell(float(pose[0]), scale, off_x) is not None \
        and R.to_cell(float(pose[1]), scale, off_y) is not None


def match_fast(fld, scale, off_x, off_y, ranges, centre, cos_t, sin_t, rot_cs, nx, ny, step, max_range, cap):
    """(best, best cost, used) of ``match_ref.match``: the same expressions over arrays [K, wx, wy, used beams]."""
    cx, cy = float(centre[0]), float(centre[1])
    if (fld is None or not (np.isfinite(cx) and np.isfinite(cy)) or R.to_cell(cx, scale, off_x) is None
            or R.to_cell(cy, scale, off_y) is None):
        return -1, -1, 0
    r = np.asarray(ranges, dtype=np.float32)
    keep = np.isfinite(r) & (r < np.float32(max_range))
    rr = r[keep].astype(np.float64)
    lx, ly = np.asarray(cos_t, dtype=np.float64)[keep] * rr, np.asarray(sin_t, dtype=np.float64)[keep] * rr
    rot = np.asarray(rot_cs, dtype=np.float64).reshape(-1, 2)
    c, s = rot[:, 0][:, None], rot[:, 1][:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        qx, qy = c * lx + (-s) * ly, s * lx + c * ly                         # [K, m]
        px = cx + (np.arange(2 * nx + 1) - nx).astype(np.float64) * step
        py = cy + (np.arange(2 * ny + 1) - ny).astype(np.float64) * step
        x = qx[:, None, :] + px[None, :, None] * 1.0                         # [K, wx, m]
        y = qy[:, None, :] + py[None, :, None] * 1.0                         # [K, wy, m]
        u, v = scale * (x + off_x), scale * (y + off_y)
        okx, oky = np.abs(u) < R.MAX_CELL, np.abs(v) < R.MAX_CELL            # (false for NaN)
        ex, ey = np.trunc(np.where(okx, u, -1.0)).astype(np.int64), np.trunc(np.where(oky, v, -1.0)).astype(np.int64)
    xw, yw = fld.shape
    okx &= (ex >= 0) & (ex < xw)
    oky &= (ey >= 0) & (ey < yw)
    f = np.asarray(fld).astype(np.int64)
    K = rot.shape[0]
    costs = np.empty((K, 2 * nx + 1, 2 * ny + 1), dtype=np.int64)
    for k in range(K):
        inside = okx[k][:, None, :] & oky[k][None, :, :]                     # [wx, wy, m]
        vals = f[np.clip(ex[k], 0, xw - 1)[:, None, :], np.clip(ey[k], 0, yw - 1)[None, :, :]]
        costs[k] = np.where(inside, vals, int(cap)).sum(axis=2)
    best = int(np.argmin(costs.reshape(-1)))
    return best, int(costs.reshape(-1)[best]), int(keep.sum())


def matched_pose(pred, rot_off, best, nx, ny, step):
    wy, W = 2 * ny + 1, (2 * nx + 1) * (2 * ny + 1)
    k, rem = best // W, best % W
    i, j = rem // wy, rem % wy
    return np.array([pred[0] + float(i - nx) * step, pred[1] + float(j - ny) * step, pred[2] + float(rot_off[k])])


def keep(status, cost):
    """Step 4: is the refined pose kept?"""
    return bool(status == RF.OK and cost[1] <= cost[0])


def gate(pose, key, gate_dist, gate_turn):
    """Step 5 on doubles; both comparisons are false for NaN."""
    dx, dy, dth = (float(pose[k]) - float(key[k]) for k in range(3))
    return bool(dx * dx + dy * dy >= gate_dist * gate_dist or abs(dth) >= gate_turn)


def track(pass_, hit, geom, ranges, state, cos_t, sin_t, motion, rot_off, rot_off_cs, nx, ny, step, iters, damping, step_cells,
          step_rad, max_range, cap, min_used, gate_dist, gate_turn, map0=0, make=G.new_mapping, field_of=G.fast_field):
    """In place on the counters [G, xw, yw].  geom = (scale, off_x, off_y).  Returns (state [L, 8], poses [L, S, 3],
    info int32 [L, S, 4], trace [L, S, 13])."""
    ranges = np.asarray(ranges, dtype=np.float32)
    L, S, n = ranges.shape
    state = np.array(state, dtype=np.float64).reshape(L, 8)
    poses, info, trace = np.zeros((L, S, 3)), np.zeros((L, S, 4), dtype=np.int32), np.zeros((L, S, 13))
    for s in range(S):
        cast_pose, acc = np.zeros((L, 1, 3)), np.full((L, 1), G.DEAD, dtype=np.int64)
        for l in range(L):
            st = state[l]
            pred = predict(st[0:3], None if motion is None else motion[l][s])
            with np.errstate(invalid="ignore"):
                c0, s0 = (math.cos(pred[2]), math.sin(pred[2])) if math.isfinite(pred[2]) else (math.nan, math.nan)
            trace[l, s, 0:5] = (*pred, c0, s0)
            pose, flags, integrate = pred, 0, False
            best, bcost, used = -1, -1, 0
            if st[6] == 0.0:
                if first_ok(pred, geom):
                    integrate = True
                else:
                    flags |= LOST
            else:
                gi = map0 + l
                fld = field_of(G.pmap_of(pass_[gi], hit[gi]), cap)
                best, bcost, used = match_fast(fld, *geom, ranges[l, s], pred[:2], cos_t, sin_t, rot_table(c0, s0, rot_off_cs), nx, ny,
                                               step, max_range, cap)
                if best < 0:
                    flags |= LOST
                elif used >= min_used:
                    flags |= MATCHED
                    pose = matched_pose(pred, rot_off, best, nx, ny, step)
                    trace[l, s, 5:8] = pose
                    r = RF.refine(fld, *geom, ranges[l, s], pose, cos_t, sin_t, iters, damping, step_cells, step_rad, max_range, cap)
                    trace[l, s, 8:11], trace[l, s, 11:13] = r["pose"], r["cost"]
                    if keep(r["status"], r["cost"]):
                        flags |= REFINED
                        pose = r["pose"]
                    integrate = gate(pose, st[3:6], gate_dist, gate_turn)
            if integrate:
                flags |= INTEGRATED
                acc[l, 0] = 0
                st[3:6], st[6] = pose, 1.0
            st[0:3] = pose
            cast_pose[l, 0] = pose
            poses[l, s], info[l, s] = pose, (best, bcost, used, flags)
        G.update_particles(pass_, hit, geom, ranges[:, s], cos_t, sin_t, cast_pose, acc=acc, map0=map0, make=make)
    return state, poses, info, trace


# ---------------------------------------------------------------- "it tracks better than odometry" (issue text)
# 400 x 400 cells of 0.05 m; odometry = the true steps plus a fixed bias per step; the tracker at its defaults.
CASES = {"dense": dict(scans=40, beams=360, seed=1, dead_end=0.59), "sparse": dict(scans=40, beams=120, seed=4, dead_end=0.63)}
MAP = dict(xw=400, yw=400, scale=20.0, off=10.0)
BIAS = (0.015, 0.0, 0.01)
BOUND = (0.10, 0.03)                    # two cells, radians: the largest error over the run

_cases = {}


def case_inputs(syn, name):
    """Scans [S, n], true poses, biased motion [S, 3] (row 0: zero, the first scan is taken at the start), beam tables and
    dead reckoning's poses - made once per process."""
    if name not in _cases:
        k = CASES[name]
        rep = syn.make_replay(k["scans"], k["beams"], seed=k["seed"])
        scans, true = np.asarray(rep.ranges, dtype=np.float32), np.asarray(rep.poses_true, dtype=np.float64)
        ang = np.linspace(rep.angle_min, rep.angle_max, k["beams"])
        motion = np.zeros((k["scans"], 3))
        motion[1:] = np.stack([X.odometry(true[i], true[i + 1]) for i in range(k["scans"] - 1)]) + np.array(BIAS)
        dead = [true[0]]
        for m in motion[1:]:
            dead.append(predict(dead[-1], m))
        _cases[name] = dict(scans=scans, true=true, motion=motion, cos_t=np.cos(ang), sin_t=np.sin(ang), dead=np.array(dead),
                            angle_min=rep.angle_min, angle_max=rep.angle_max)
    return _cases[name]


def errors(poses, true):
    """(position error [S], heading error [S]) of a trajectory."""
    d = np.asarray(poses) - np.asarray(true)
    return np.hypot(d[:, 0], d[:, 1]), np.abs((d[:, 2] + np.pi) % (2 * np.pi) - np.pi)


_runs = {}


def run_case(syn, name, gate=None):
    """The case on the restatement with the C oracle's mapping; (poses [S, 3], info [S, 4]), once per process and gate."""
    key = (name, gate)
    if key not in _runs:
        c, p = case_inputs(syn, name), dict(DEFAULTS)
        if gate is not None:
            p["gate_dist"], p["gate_turn"] = gate
        off, cs = rotations(p.pop("n_rot"), p.pop("rot_step"))
        geom = (MAP["scale"], MAP["off"], MAP["off"])
        pass_ = np.zeros((1, MAP["xw"], MAP["yw"]), dtype=np.int64)
        hit = np.zeros_like(pass_)
        state = np.zeros((1, 8))
        state[0, :3] = c["true"][0]
        _, poses, info, _ = track(pass_, hit, geom, c["scans"][None], state, c["cos_t"], c["sin_t"], c["motion"][None], off, cs,
                                  step=1.0 / MAP["scale"], make=G.c_mapping, **p)
        _runs[key] = (poses[0], info[0])
    return _runs[key]
