"""NumPy restatement of the grid FastSLAM operators (include/slam_hip.h, "grid FastSLAM: a map per particle that follows
resampling"), written from their stated semantics on ``mcl_ref`` and the oracle's ``Mapping.update``:

    settle(anc)            slam_mcl_settle for one filter, with Python integers
    settle_batch(...)      the same for [F, P], with poses, map sources and moved counts
    copy_maps(...)         slam_grid_copy_maps on counter arrays [G, xw, yw]
    update_particles(...)  slam_grid_update_particles: a loop over the oracle's generalised Mapping.update
    weigh_maps(...)        slam_mcl_weigh_maps: mcl_ref's weigh with a map per particle
    fast_field(pmap, cap)  match_ref.field by two separable passes (pinned to it in test_gridslam_ref.py)
    step(...)              one SLAM step on arrays; slam_run(...) the "maps better than odometry" case
"""
import numpy as np

import match_ref as M
import mcl_ref as X
import raycast_ref as R
from oracle import oracle_np as O

DEAD = X.DEAD


# ---------------------------------------------------------------- settle
def settle(anc):
    """settled[j] for one filter: a slot that is somebody's ancestor keeps itself; the free slots, ascending, take the
    surplus list (every i repeated cnt[i] - 1 times), ascending."""
    anc = [int(a) for a in anc]
    P = len(anc)
    cnt = [0] * P
    for a in anc:
        assert 0 <= a < P
        cnt[a] += 1
    free = [i for i in range(P) if cnt[i] == 0]
    surplus = [i for i in range(P) for _ in range(cnt[i] - 1)]
    assert len(free) == len(surplus)
    out = list(range(P))
    for j, i in zip(free, surplus):
        out[j] = i
    return out


def settle_batch(anc, poses_src=None, map0=0, clamp=False):
    anc = np.asarray(anc, dtype=np.int64)
    F, P = anc.shape
    if clamp:
        anc = np.clip(anc, 0, P - 1)
    settled = np.array([settle(a) for a in anc], dtype=np.int32).reshape(F, P)
    poses = None if poses_src is None else np.stack([np.asarray(poses_src, dtype=np.float64)[f][settled[f]] for f in range(F)])
    map_src = (int(map0) + np.arange(F, dtype=np.int64)[:, None] * P + settled).astype(np.int32)
    moved = (settled != np.arange(P)[None]).sum(axis=1).astype(np.int32)
    return dict(settled=settled, poses=poses, map_src=map_src, moved=moved)


# ---------------------------------------------------------------- copy
def copy_kinds(src, first, G):
    """copied_out of the device form: 1 copied, 0 kept, -1 a source that is itself a destination."""
    src = [int(s) for s in src]
    out = []
    for k, s in enumerate(src):
        d = first + k
        if s == d or not 0 <= s < G:
            out.append(0)
        elif first <= s < first + len(src) and src[s - first] != s:
            out.append(-1)
        else:
            out.append(1)
    return np.array(out, dtype=np.int32)


def copy_maps(arrays, src, first=0):
    """In place on every array [G, ...] of ``arrays``; returns copied_out."""
    G = len(arrays[0])
    kinds = copy_kinds(src, first, G)
    before = [a.copy() for a in arrays]
    for k, kind in enumerate(kinds):
        if kind == 1:
            for a, b in zip(arrays, before):
                a[first + k] = b[int(src[k])]
    return kinds


# ---------------------------------------------------------------- update
def new_mapping(xw, yw, scale, off_x, off_y):
    return O.Mapping(xw, yw, 1.0 / scale, scale=scale, offset_x=off_x, offset_y=off_y)


def update_particles(pass_, hit, geom, ranges, cos_t, sin_t, poses, acc=None, map0=0, make=new_mapping):
    """In place on the counters [G, xw, yw] (any integer dtype).  geom = (scale, off_x, off_y).  ``make``: the mapping
    of one map (``new_mapping``: the oracle's Python one; the SLAM run passes the C oracle's for speed)."""
    poses = np.asarray(poses, dtype=np.float64)
    F, P, _ = poses.shape
    xw, yw = pass_.shape[1:]
    for f in range(F):
        pc = R.table_points(ranges[f], cos_t, sin_t)
        for p in range(P):
            if acc is not None and int(acc[f][p]) == DEAD:
                continue
            gi = map0 + f * P + p
            m = make(xw, yw, *geom)
            obs = O.world_points(poses[f, p], pc)
            m.update(obs[0], obs[1], poses[f, p, 0], poses[f, p, 1])
            pass_[gi] += np.asarray(m.pass_cnt).astype(pass_.dtype)
            hit[gi] += np.asarray(m.hit_cnt).astype(hit.dtype)


def pmap_of(pass_, hit):
    """The finalize rule of the default increments: untouched 50, a hit or 1001 passes 100, else 0."""
    touched = (pass_.astype(np.int64) + hit) > 0
    return np.where(touched, np.where((hit >= 1) | (pass_ >= 1001), 100, 0), 50).astype(np.int8)


# ---------------------------------------------------------------- field and weigh
def fast_field(pmap, cap):
    """match_ref.field(pmap, cap) for cap <= 4096: the nearest occupied cell of a row within r = ceil(sqrt(cap)) columns,
    then the rows within r: min over dx of dx^2 + g[x + dx][y] (g: that squared distance), all in integers."""
    occ = np.asarray(pmap) == 100
    xw, yw = occ.shape
    r = int(np.ceil(np.sqrt(cap)))
    big = 1 << 20
    g = np.full((xw, yw), big, dtype=np.int64)
    for d in range(0, r + 1):
        for sgn in ((1,) if d == 0 else (1, -1)):
            dy = d * sgn
            if d >= yw:
                continue
            sh = np.zeros_like(occ)
            if dy >= 0:
                sh[:, :yw - dy] = occ[:, dy:]
            else:
                sh[:, -dy:] = occ[:, :yw + dy]
            np.minimum(g, np.where(sh, d * d, big), out=g)
    out = np.full((xw, yw), int(cap), dtype=np.int64)
    for dx in range(-min(r, xw - 1), min(r, xw - 1) + 1):
        sh = np.full((xw, yw), big, dtype=np.int64)
        if dx >= 0:
            sh[:xw - dx] = g[dx:]
        else:
            sh[-dx:] = g[:xw + dx]
        np.minimum(out, sh + dx * dx, out=out)
    return out.astype(np.int16)


def weigh_maps(fields, scale, off_x, off_y, poses, ranges, cos_t, sin_t, max_range, cap, motion=None, noise=None, pmaps=None,
               acc=None, moved=None):
    """slam_mcl_weigh_maps: ``mcl_ref.weigh`` of every particle as a filter of its own on map pmaps[f][p] (None: f * P + p).
    fields [G, xw, yw].  Returns the dict of ``mcl_ref.weigh`` with [F, P] shapes."""
    poses = np.asarray(poses, dtype=np.float64)
    F, P, _ = poses.shape
    maps = np.arange(F * P) if pmaps is None else np.asarray(pmaps).reshape(F * P)
    rep = lambda a, k: None if a is None else np.repeat(np.asarray(a).reshape(F, -1), P, axis=0).reshape(F * P, k)
    w = X.weigh(fields, scale, off_x, off_y, poses.reshape(F * P, 1, 3), rep(ranges, len(cos_t)), cos_t, sin_t, max_range, cap,
                motion=rep(motion, 3), noise=None if noise is None else np.asarray(noise).reshape(F * P, 1, 3), maps=maps,
                acc=None if acc is None else np.asarray(acc).reshape(F * P, 1),
                moved=None if moved is None else np.asarray(moved).reshape(F * P, 1, 3))
    return dict(poses=w["poses"].reshape(F, P, 3), cost=w["cost"].reshape(F, P), acc=None if acc is None else w["acc"].reshape(F, P),
                used=w["used"].reshape(F, P)[:, 0].copy())


# ---------------------------------------------------------------- one step and the SLAM case
def step_after_costs(pass_, hit, geom, poses_moved, acc_after_weigh, table, shift, u0, ess_frac, ranges, cos_t, sin_t, make=new_mapping):
    """Everything of a step after the weigh: resample, settle, copy, update - in place on the counters.  Returns a dict of
    poses, acc, ancestors, settled, map_src, moved, copied, est, info."""
    r = X.resample(poses_moved, acc_after_weigh, table, shift, u0, ess_frac)
    s = settle_batch(r["ancestors"], poses_moved)
    copied = copy_maps([pass_, hit], s["map_src"].reshape(-1))
    update_particles(pass_, hit, geom, ranges, cos_t, sin_t, s["poses"], acc=r["acc"], make=make)
    return dict(poses=s["poses"], acc=r["acc"], ancestors=r["ancestors"], settled=s["settled"], map_src=s["map_src"], moved=s["moved"],
                copied=copied, est=r["est"], info=r["info"])


# "It maps better than odometry" (issue text): make_replay(16, 120, seed=4), one filter of 64 particles that start at the
# true first pose, 400 x 400 cells of 0.05 m.  The motion input is the trajectory's own steps with a fixed bias; the noise
# covers the bias; MCL's recovery parameters otherwise.
SLAM = dict(P=64, scans=16, beams=120, seed=4, xw=400, yw=400, scale=20.0, off=10.0, sigma_cells=2.0, shift=0, T=4096, cap=64,
            max_range=30.0, ess_frac=0.5, bias=(0.015, 0.0, 0.01), noise=(0.02, 0.01, 0.01), rng_seed=0)
SLAM_BOUND = (0.05, 0.02)               # one cell, radians

_slam = {}


def slam_case(syn):
    """Inputs made once per process: scans [S, n], true poses [S, 3], motion [S - 1, 3] (biased), noise [S - 1, P, 3], u0 [S],
    beam tables, the table, and dead reckoning's poses [S, 3]."""
    if not _slam:
        k = SLAM
        rep = syn.make_replay(k["scans"], k["beams"], seed=k["seed"])
        scans, true = np.asarray(rep.ranges, dtype=np.float32), np.asarray(rep.poses_true, dtype=np.float64)
        ang = np.linspace(rep.angle_min, rep.angle_max, k["beams"])
        motion = np.stack([X.odometry(true[i], true[i + 1]) for i in range(k["scans"] - 1)])
        motion += np.array(k["bias"])
        rng = np.random.default_rng(k["rng_seed"])
        dead = [true[0]]
        for m in motion:
            dead.append(X.move(dead[-1][None, None], m[None])[0, 0])
        _slam.update(scans=scans, true=true, motion=motion, cos_t=np.cos(ang), sin_t=np.sin(ang),
                     noise=rng.normal(0.0, 1.0, (k["scans"] - 1, k["P"], 3)) * np.array(k["noise"]),
                     u0=rng.uniform(0.0, 1.0, k["scans"]), table=X.weight_table(k["sigma_cells"], k["shift"], k["T"]),
                     dead=np.array(dead))
    return _slam


def c_mapping(xw, yw, scale, off_x, off_y):
    from oracle import c_oracle as co
    return co.Grid(xw, yw, scale, off_x, off_y)


def slam_run(case, make=c_mapping):
    """The case on the restatement.  Returns (best pose after the last step, est [S, 4], info [S, 4], moved [S])."""
    k = SLAM
    P, geom = k["P"], (k["scale"], k["off"], k["off"])
    pass_ = np.zeros((P, k["xw"], k["yw"]), dtype=np.int64)
    hit = np.zeros_like(pass_)
    poses = np.tile(case["true"][0], (1, P, 1))
    acc = np.zeros((1, P), dtype=np.int32)
    est, info, moved = [], [], []
    cache = {}
    for s in range(k["scans"]):
        pm = pmap_of(pass_, hit)
        fields = np.empty(pm.shape, dtype=np.int16)
        for g in range(P):                                                # copies of one map share their field
            key = pm[g].tobytes()
            if key not in cache:
                cache[key] = fast_field(pm[g], k["cap"])
            fields[g] = cache[key]
        cache = {pm[g].tobytes(): fields[g] for g in range(P)}
        w = weigh_maps(fields, *geom, poses, case["scans"][s][None], case["cos_t"], case["sin_t"], k["max_range"], k["cap"],
                       motion=None if s == 0 else case["motion"][s - 1][None], noise=None if s == 0 else case["noise"][s - 1][None], acc=acc)
        out = step_after_costs(pass_, hit, geom, w["poses"], w["acc"], case["table"], k["shift"], case["u0"][s:s + 1], k["ess_frac"],
                               case["scans"][s][None], case["cos_t"], case["sin_t"], make=make)
        poses, acc = out["poses"], out["acc"]
        est.append(out["est"][0])
        info.append(out["info"][0])
        moved.append(int(out["moved"][0]))
    best = int(info[-1][0])
    return poses[0, best].copy(), np.array(est), np.array(info), np.array(moved)
