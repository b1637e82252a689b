"""Cases of slam_track and the teacher-forced walk that checks a run of it against the public calls
(tests/test_gpu_track.py, tests/test_gpu_track_properties.py; tests/test_track_cases.py looks at the cases on the host).

    replay_case(syn, n, ...)    L synthetic trajectories through the room with biased odometry: the shape of test (A)
    case_of(seed)               a seeded case on refine_cases' small maps and index rules
    make_grids(slam, case)      (the tracker's grid, the shadow grid), both holding the case's prebuilt maps
    run(slam, grid, case, ...)  slam_track (host form) or slam_track_dev (device form) on a case -> dict of arrays
    walk(slam, case, out, shadow)   the walk: every scan of ``out`` beside the shadow grid
    counters(grid)              (pass, hit) of every map
    edges_of(case, out)         the names of the edges a case reaches, from its inputs and the flags of a run
    seeds()                     range(SLAM_HYP_EXAMPLES), default 30

A case is a dict: shape (xw, yw), geom (scale, off_x, off_y), G, map0, ranges float32 [L, S, n], motion [L, S, 3] or None,
state [L, 8], ct / st [n], rot_off [K], rot_off_cs [K, 2], par (the call's scalar parameters by name) and pre: None or
(ranges [L, n], poses [L, 3]) integrated into maps map0 .. map0 + L - 1 before the run (a prebuilt map).

The walk is teacher-forced: every stage is checked on the values the call recorded for the stage before it (its trace), so
one differing bit shows where it arose and cannot move the rest of the run.  Its tolerances are the issue's: the
prediction within the project's 1e-9 of mcl_ref.move (bit-equal without motion), c0 and s0 within 1e-12 of NumPy's, and
everything after that - the matcher's answer on the table formed from the recorded c0, s0, the refinement from the
recorded matched pose, the keep rule, the gate, the pose, the flags, the state and the counters - equal bit for bit."""
import os

import numpy as np

import mcl_ref as X
import refine_cases as RC
import track_ref as T

PAR = ("nx", "ny", "step", "iters", "damping", "step_cells", "step_rad", "max_range", "cap", "min_used", "gate_dist", "gate_turn")
BIAS = np.array(T.BIAS)
EDGES = ("motion == NULL", "a first scan (keyed = 0)", "a prebuilt map (keyed = 1)", "a scan that is not integrated", "a scan behind the gate that is integrated",
         "gates of +inf", "gates of 0", "a refined pose kept", "a matched pose that stands", "used < min_used", "a lost scan",
         "more than one trajectory", "map0 > 0", "iters = 0")


def seeds():
    return range(int(os.environ.get("SLAM_HYP_EXAMPLES", "30")))


def replay_case(syn, n, L=3, S=8, K=5, nx=2, ny=2, iters=3, gate=(0.15, 0.05), stride=3, G=None, map0=0, with_motion=True):
    """L trajectories of S scans of n beams through the synthetic room on a 200 x 200 map at 0.1 m; odometry = the true
    steps plus the bias (row 0: no step, the first scan is taken at the start pose)."""
    reps = [syn.make_replay(S, n, seed=11 + l, stride=stride) for l in range(L)]
    ang = np.linspace(reps[0].angle_min, reps[0].angle_max, n)
    true = np.stack([np.asarray(r.poses_true, dtype=np.float64) for r in reps])
    motion = np.zeros((L, S, 3))
    for l in range(L):
        motion[l, 1:] = np.stack([X.odometry(true[l, i], true[l, i + 1]) for i in range(S - 1)]) + BIAS
    state = np.zeros((L, 8))
    state[:, :3] = true[:, 0]
    off, cs = T.rotations(K, 0.02)
    par = dict(nx=nx, ny=ny, step=0.1, iters=iters, damping=0.01, step_cells=0.5, step_rad=0.02, max_range=30.0, cap=64, min_used=1,
               gate_dist=float(gate[0]), gate_turn=float(gate[1]))
    return dict(shape=(200, 200), geom=(10.0, 10.0, 10.0), G=L + map0 if G is None else G, map0=map0,
                ranges=np.ascontiguousarray(np.stack([np.asarray(r.ranges, dtype=np.float32) for r in reps])),
                motion=motion if with_motion else None, state=state, ct=np.cos(ang), st=np.sin(ang), rot_off=off, rot_off_cs=cs, par=par,
                pre=None, true=true)


def case_of(seed):
    rng = np.random.default_rng(7000 + seed)
    shape = RC.SHAPES[(seed // 3) % len(RC.SHAPES)]
    scale, off_x, off_y = RC.RULES[(seed // 2) % len(RC.RULES)]
    n = RC.BEAMS[seed % len(RC.BEAMS)]
    L, S = 1 + seed % 3, int(rng.integers(2, 7))
    map0 = int(rng.integers(0, 3)) if seed % 4 == 1 else 0
    G = map0 + L + int(rng.integers(0, 2))
    th = -np.pi + np.arange(n) * (2.0 * np.pi / n) + rng.uniform(0, 0.1)
    reach = float(rng.choice((4.0, 12.0, 40.0)))                       # cells
    max_range = float(np.float32(reach / scale))
    ranges = rng.uniform(0.5 / scale, 1.1 * max_range, size=(L, S, n)).astype(np.float32)
    # a NaN range raises the sticky status when its scan is integrated, as it does in slam_grid_update_particles (Python's
    # int(nan)): NaN only where nothing is ever integrated (a prebuilt map behind gates of +inf), +inf (30 m) elsewhere
    never = (seed // 2) % 3 == 2 and seed % 3 == 2
    hole = rng.choice((np.nan, np.inf))
    ranges[rng.random(ranges.shape) < 0.05] = hole if never else np.inf
    if rng.random() < 0.4:                                             # a scan with no used beam, mid-stream
        ranges[rng.integers(0, L), rng.integers(1, S)] = np.inf
    cells = np.stack([rng.integers(1, shape[0] - 1, size=L), rng.integers(1, shape[1] - 1, size=L)], axis=1)
    frac = rng.uniform(0.05, 0.95, size=(L, 2))
    start = np.stack([(cells[:, 0] + frac[:, 0]) / scale - off_x, (cells[:, 1] + frac[:, 1]) / scale - off_y, rng.uniform(-3.2, 3.2, size=L)], axis=1)
    state = np.zeros((L, 8))
    state[:, :3] = start
    pre = None
    if seed % 3 == 2:                                                  # a prebuilt map: tracking from keyed = 1
        pre = (rng.uniform(0.5 / scale, max_range, size=(L, n)).astype(np.float32), start + rng.normal(0, 0.3 / scale, size=(L, 3)))
        state[:, 3:6], state[:, 6] = pre[1], 1.0
    if rng.random() < 0.15:                                            # a start the map cannot take
        state[rng.integers(0, L), rng.integers(0, 2)] = rng.choice((np.nan, np.inf, 3.0e6))
    motion = None
    if seed % 2 == 0:
        motion = rng.normal(0.0, 1.0, size=(L, S, 3)) * np.array([1.2 / scale, 0.6 / scale, 0.04])
    small = float(rng.choice((0.5, 1.5))) / scale
    gate = ((0.0, 0.0), (small, 0.03), (np.inf, np.inf))[(seed // 2) % 3]
    K, nx, ny = int(rng.choice((1, 3, 5))), int(rng.integers(0, 3)), int(rng.integers(0, 3))
    off, cs = T.rotations(K, float(rng.choice((0.01, 0.05))))
    par = dict(nx=nx, ny=ny, step=1.0 / scale, iters=int(RC.ITERS[(seed // 5) % len(RC.ITERS)]), damping=float(rng.choice((1e-3, 1e-2, 0.1))),
               step_cells=float(rng.choice((0.5, 1.0))), step_rad=float(rng.choice((0.02, 0.05))), max_range=max_range,
               cap=int(rng.choice((64, 64, 9))), min_used=int(rng.choice((1, 1, n // 2 + 1))), gate_dist=float(gate[0]), gate_turn=float(gate[1]))
    return dict(shape=shape, geom=(scale, off_x, off_y), G=G, map0=map0, ranges=np.ascontiguousarray(ranges), motion=motion, state=state,
                ct=np.cos(th), st=np.sin(th), rot_off=off, rot_off_cs=cs, par=par, pre=pre)


# ---------------------------------------------------------------- running a case
def maps_of(case):
    return (case["map0"] + np.arange(case["ranges"].shape[0])).astype(np.int32)


def make_grid(slam, case, context=None):
    g = slam.DeviceGrid(case["G"], case["shape"][0], case["shape"][1], *case["geom"], context=context)
    if case["pre"] is not None:
        slam.grid_update_particles_host(g, case["pre"][0], case["ct"], case["st"], case["pre"][1][:, None, :], map0=case["map0"])
    return g


def make_grids(slam, case):
    return make_grid(slam, case), make_grid(slam, case)


def counters(grid):
    got = [grid.read(g, want=("pass", "hit")) for g in range(grid.G)]
    return np.stack([o["pass"] for o in got]), np.stack([o["hit"] for o in got])


def run(slam, grid, case, device=False, scans=None, state=None, rows=None):
    """The case (or its scans ``scans``, a slice, from ``state``; or its trajectories ``rows``, a list) through the host
    form or the device form.  Returns a dict: state, poses, info, trace."""
    sl = slice(None) if scans is None else scans
    rows = list(range(case["ranges"].shape[0])) if rows is None else rows
    ranges = np.ascontiguousarray(case["ranges"][rows][:, sl])
    motion = None if case["motion"] is None else np.ascontiguousarray(case["motion"][rows][:, sl])
    st = np.ascontiguousarray(case["state"][rows] if state is None else state)
    if not device:
        out = slam.track_host(grid, ranges, st, case["ct"], case["st"], motion=motion, map0=case["map0"], rot_off=case["rot_off"],
                              rot_off_cs=case["rot_off_cs"], return_trace=True, **case["par"])
        return dict(zip(("state", "poses", "info", "trace"), out))
    import torch
    dev = torch.device("cuda", grid._ctx.device)
    tr = slam.DeviceTracker(grid, len(rows), case["ct"], case["st"], map0=case["map0"], rot_off=case["rot_off"],
                            rot_off_cs=case["rot_off_cs"], **case["par"])
    tr.state.copy_(torch.from_numpy(st))
    tr.run(torch.from_numpy(ranges).to(dev), None if motion is None else torch.from_numpy(motion).to(dev))
    out = tr.results()
    grid._ctx.check_status()
    return out


def ref_run(case, make=None):
    """The case on the restatement (tests/track_ref.py).  Returns (dict as ``run``, pass, hit)."""
    import gridslam_ref as G
    pass_ = np.zeros((case["G"],) + tuple(case["shape"]), dtype=np.int64)
    hit = np.zeros_like(pass_)
    make = G.c_mapping if make is None else make
    if case["pre"] is not None:
        G.update_particles(pass_, hit, case["geom"], case["pre"][0], case["ct"], case["st"], case["pre"][1][:, None, :], map0=case["map0"], make=make)
    out = T.track(pass_, hit, case["geom"], case["ranges"], case["state"], case["ct"], case["st"], case["motion"], case["rot_off"],
                  case["rot_off_cs"], map0=case["map0"], make=make, **case["par"])
    return dict(zip(("state", "poses", "info", "trace"), out)), pass_, hit


# ---------------------------------------------------------------- the walk
def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def walk(slam, case, out, shadow, scans=None, state=None):
    """Every scan of ``out`` checked beside ``shadow`` (a grid that holds what the tracker's grid held before the call; the
    walk integrates into it).  Returns the state the walk ends in, which the caller compares with the call's."""
    sl = slice(None) if scans is None else scans
    ranges = case["ranges"][:, sl]
    motion = None if case["motion"] is None else case["motion"][:, sl]
    L, S, n = ranges.shape
    p, geom, maps = case["par"], case["geom"], maps_of(case)
    st = np.array(case["state"] if state is None else state, dtype=np.float64)
    poses, info, trace = out["poses"], out["info"], out["trace"]
    W, wy = (2 * p["nx"] + 1) * (2 * p["ny"] + 1), 2 * p["ny"] + 1
    for s in range(S):
        where = "scan %d" % s
        prev, keyed = st[:, 0:3], st[:, 6] != 0.0
        pred, c0, s0 = trace[:, s, 0:3], trace[:, s, 3], trace[:, s, 4]
        if motion is None:
            assert same(pred, prev), where
        else:
            want = X.move(prev[:, None, :], motion[:, s])[:, 0]
            fin = np.isfinite(want)
            assert np.array_equal(fin, np.isfinite(pred)), where
            assert np.all(np.abs(pred[fin] - want[fin]) <= 1e-9), (where, pred, want)
        with np.errstate(invalid="ignore"):
            fin = np.isfinite(pred[:, 2])
            assert np.all(np.abs(c0[fin] - np.cos(pred[fin, 2])) <= 1e-12) and np.all(np.abs(s0[fin] - np.sin(pred[fin, 2])) <= 1e-12), where
        rot = np.stack([T.rot_table(c0[l], s0[l], case["rot_off_cs"]) for l in range(L)])
        gob = np.where(keyed, maps, -1).astype(np.int32)
        best, cost, used = slam.grid_match_host(shadow, ranges[:, s], pred[:, 0:2], case["ct"], case["st"], rot, p["nx"], p["ny"], p["step"],
                                                max_range=p["max_range"], cap=p["cap"], grid_of_batch=gob)
        assert same(info[:, s, 0], best) and same(info[:, s, 1], cost) and same(info[:, s, 2], used), (where, info[:, s], best, cost, used)
        matched = keyed & (best >= 0) & (used >= p["min_used"])
        start = np.zeros((L, 3))
        for l in np.flatnonzero(matched):
            start[l] = T.matched_pose(pred[l], case["rot_off"], int(best[l]), p["nx"], p["ny"], p["step"])
            assert 0 <= best[l] < len(case["rot_off"]) * W and wy > 0
        assert same(trace[:, s, 5:8], start), (where, trace[:, s, 5:8], start)
        rp, rc, _ru, rs = slam.grid_refine_host(shadow, ranges[:, s], trace[:, s, 5:8], case["ct"], case["st"], iters=p["iters"],
                                                damping=p["damping"], step_cells=p["step_cells"], step_rad=p["step_rad"],
                                                max_range=p["max_range"], cap=p["cap"], grid_of_batch=np.where(matched, maps, -1).astype(np.int32))
        rp[~matched], rc[~matched] = 0.0, 0.0
        assert same(trace[:, s, 8:11], rp) and same(trace[:, s, 11:13], rc), (where, trace[:, s, 8:13], rp, rc)
        flags, pose = np.zeros(L, dtype=np.int32), pred.copy()
        for l in range(L):
            integrate = False
            if not keyed[l]:
                if T.first_ok(pred[l], geom):
                    integrate = True
                else:
                    flags[l] |= T.LOST
            elif best[l] < 0:
                flags[l] |= T.LOST
            elif matched[l]:
                flags[l] |= T.MATCHED
                pose[l] = trace[l, s, 5:8]
                if T.keep(rs[l], trace[l, s, 11:13]):
                    flags[l] |= T.REFINED
                    pose[l] = trace[l, s, 8:11]
                integrate = T.gate(pose[l], st[l, 3:6], p["gate_dist"], p["gate_turn"])
            if integrate:
                flags[l] |= T.INTEGRATED
                st[l, 3:6], st[l, 6] = pose[l], 1.0
            st[l, 0:3] = pose[l]
        assert same(info[:, s, 3], flags), (where, info[:, s, 3], flags)
        assert same(poses[:, s], pose), (where, poses[:, s], pose)
        acc = np.where(flags & T.INTEGRATED, 0, slam.MCL_DEAD).astype(np.int32)
        slam.grid_update_particles_host(shadow, ranges[:, s], case["ct"], case["st"], poses[:, s][:, None, :], acc=acc[:, None], map0=case["map0"])
    return st


def edges_of(case, out):
    e, p, f = set(), case["par"], out["info"][..., 3]
    L, S, _ = case["ranges"].shape
    if case["motion"] is None:
        e.add(EDGES[0])
    if (case["state"][:, 6] == 0).any():
        e.add(EDGES[1])
    if case["pre"] is not None:
        e.add(EDGES[2])
    later = f[:, 1:] if case["pre"] is None else f
    if ((later & T.INTEGRATED) == 0).any():
        e.add(EDGES[3])
    if ((later & T.INTEGRATED) != 0).any() and ((later & T.MATCHED) != 0).any() and ((later & (T.MATCHED | T.INTEGRATED)) == (T.MATCHED | T.INTEGRATED)).any():
        e.add(EDGES[4])
    if np.isinf(p["gate_dist"]):
        e.add(EDGES[5])
    if p["gate_dist"] == 0:
        e.add(EDGES[6])
    if (f & T.REFINED).any():
        e.add(EDGES[7])
    if ((f & T.MATCHED) != 0).any() and (((f & T.MATCHED) != 0) & ((f & T.REFINED) == 0)).any():
        e.add(EDGES[8])
    keyed_before = np.concatenate([case["state"][:, 6:7] != 0, np.cumsum((f & T.INTEGRATED) != 0, axis=1)[:, :-1] > 0], axis=1) | (case["state"][:, 6:7] != 0)
    if (keyed_before & ((f & (T.MATCHED | T.LOST)) == 0)).any():
        e.add(EDGES[9])
    if (f & T.LOST).any():
        e.add(EDGES[10])
    if L > 1:
        e.add(EDGES[11])
    if case["map0"] > 0:
        e.add(EDGES[12])
    if p["iters"] == 0:
        e.add(EDGES[13])
    return e
