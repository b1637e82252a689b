"""How many scans, trajectories, hypotheses or pairs ONE call may carry: every batched entry point at the 65 535 that a
16-bit launch slot holds and one past it, against the C oracle.  Beams and maps are kept tiny so that only the batch
count is large.

Part A: the group bound of the two casts for maps much larger than a window - the direction wedges (grid_mode 1 on a
large map, and 4) and the recorded-walk tiles (grid_mode 2).  Their workgroup grids carry one row per group of scans
(k_tile_cast: gridDim.y; k_wedge_order / k_wedge_cast: a unit number of 20 bits, group x 16 classes), so a call with more
than 65 535 groups is cast in successive launches of at most 65 535 groups - over whole trajectories, or over scan
ranges of one trajectory - and must give the counters of one launch bit for bit.

Part B: the batch axis on gridDim.y (k_nn, the ICP launch, k_grid_update_win, k_grid_update_own and the single-scan
owner kernels, k_wedge_sort, k_ray_bits, k_virtual_scan) with 65 537 rows.

Counters (pass, hit, pmap) bit-exact, visits equal to the oracle's, iteration counts and NN indices exact, poses and
transforms to 1e-9."""
import numpy as np
import pytest

from conftest import load_golden, pkg
from oracle import c_oracle as co
from oracle import checks
from oracle import oracle_np as on

pytestmark = pytest.mark.gpu
FTOL = 1e-9
AMIN, AMAX = -3.14159, 3.14159
BOUND = 65535                     # rows of a 16-bit launch slot


@pytest.fixture(scope="module")
def slam():
    p = pkg()
    p._abi.default_context()
    return p


@pytest.fixture(scope="module")
def g5():
    return load_golden("g5_map_observation.npz")


def _ctx(slam, mode, group):
    ctx = slam.Context(0)
    ctx.set_option("grid_mode", mode)
    ctx.set_option("grid_group", group)
    return ctx


def _assert_grid(grid, gi, og, visits=None):
    r = grid.read(gi, want=("pmap", "pass", "hit"))
    assert np.array_equal(r["pass"], og.pass_cnt), int(np.sum(r["pass"] != og.pass_cnt))
    assert np.array_equal(r["hit"], og.hit_cnt), int(np.sum(r["hit"] != og.hit_cnt))
    assert np.array_equal(r["pmap"], og.pmap), int(np.sum(r["pmap"] != og.pmap))
    if visits is not None:
        assert grid.visits() == visits, (grid.visits(), visits)
    return r


# ------------------------------------------------------------------ A: group bound of the wedge and tile casts
@pytest.mark.parametrize("B", [BOUND, BOUND + 1])
def test_explicit_scans_past_the_group_bound(slam, B):
    """A1: B scans of 4 random beams (slam_grid_update) into one 560 x 560 map (more than 8 windows: the large-map
    casts apply), one scan per group (grid_group 1): B groups.  Automatic choice (1: wedges), tiles (2), wedges (4)."""
    rng = np.random.default_rng(B)
    n = 4
    cx, cy = rng.uniform(-11, 11, B), rng.uniform(-11, 11, B)
    ang, d = rng.uniform(-np.pi, np.pi, (B, n)), rng.uniform(0.05, 4.0, (B, n))
    ox, oy = cx[:, None] + np.cos(ang) * d, cy[:, None] + np.sin(ang) * d
    og = co.Grid(560, 560, 20.0, 14.0, 14.0)
    for b in range(B):
        og.update(ox[b], oy[b], cx[b], cy[b])
    assert int(og.hit_cnt.sum()) > 0.99 * B * n                           # (a ray inside its origin's cell takes no hit)
    for mode in (1, 2, 4):
        ctx = _ctx(slam, mode, 1)
        g = slam.DeviceGrid(1, 560, 560, 20.0, 14.0, 14.0, context=ctx)
        try:
            g.update_host(ox, oy, cx, cy)
            _assert_grid(g, 0, og, og.visits)
        finally:
            g.close()
            ctx.close()


@pytest.mark.parametrize("n_scan", [BOUND + 1, BOUND + 2])
def test_one_long_replay_past_the_group_bound(slam, syn, n_scan):
    """A2: one trajectory of n_scan - 1 scan pairs x 16 beams into one shared 560 x 560 @ 0.05 m map, grid_group 1:
    65 535 / 65 536 groups in one trajectory (a split over scan ranges).  Modes 1, 2 and 4."""
    rep = syn.make_replay(n_scan, 16, seed=21, stride=5)
    og = checks.metric_grid(560, 560, 0.05)
    oposes, oT, oit, ov = co.replay(rep.ranges, AMIN, AMAX, og, threads=16, mt_grid=True)
    assert int(og.hit_cnt.sum()) > (n_scan - 1) * 8                       # most rays end inside the map
    for mode in (1, 2, 4):
        ctx = _ctx(slam, mode, 1)
        grid = slam.DeviceGrid.metric(1, 560, 560, 0.05, context=ctx)
        try:
            poses, T, it = slam.replay_host(rep.ranges, AMIN, AMAX, grid=grid, context=ctx)
            assert np.array_equal(it, oit), mode
            assert np.max(np.abs(poses - oposes)) < FTOL and np.max(np.abs(T - oT)) < FTOL, mode
            _assert_grid(grid, 0, og, ov)
        finally:
            grid.close()
            ctx.close()


@pytest.mark.parametrize("n_scan", [BOUND // 2 + 1, BOUND // 2 + 2])
def test_map_per_trajectory_past_the_group_bound(slam, syn, n_scan):
    """A3 (a), the regression of round 5's review: a map per trajectory (grid_of_traj) on large maps goes to the
    wedges, which refused more than 65 535 groups with nothing to fall back to.  L = 2 trajectories x (n_scan - 1)
    scans, grid_group 1: 65 534 / 65 536 groups, 560 x 560 @ 0.05 m maps in reverse order.  Modes 1 and 4."""
    L = 2
    reps = [syn.make_replay(n_scan, 16, seed=22 + l, stride=5) for l in range(L)]
    ranges = np.stack([r.ranges for r in reps])
    p0 = np.array([[0.0, 0.0, 0.0], [0.4, -0.3, 0.5]])
    got = [1, 0]
    ref = []
    for l in range(L):
        og = checks.metric_grid(560, 560, 0.05)
        ref.append((og,) + tuple(checks.replay_reference(ranges[l], AMIN, AMAX, og, pose0=tuple(p0[l]), threads=16)))
    for mode in (1, 4):
        ctx = _ctx(slam, mode, 1)
        grid = slam.DeviceGrid.metric(L, 560, 560, 0.05, context=ctx)
        try:
            poses, T, it = slam.replay_host(ranges, AMIN, AMAX, grid=grid, pose0=p0, grid_of_traj=got, context=ctx)
            for l in range(L):
                og, op, oT, oit, _ = ref[l]
                assert np.array_equal(it[l], oit), (mode, l)
                assert np.max(np.abs(poses[l] - op)) < FTOL and np.max(np.abs(T[l] - oT)) < FTOL, (mode, l)
                _assert_grid(grid, got[l], og)
            assert grid.visits() == sum(r[4] for r in ref), mode
        finally:
            grid.close()
            ctx.close()


def test_batch_of_trajectories_into_their_own_maps_past_the_group_bound(slam, syn):
    """A3 (b): L = 1 041 trajectories x 1 009 scans x 16 beams, each into its own 544 x 544 @ 0.05 m map, the
    library's group choice (16 scans: 63 groups a trajectory, 65 583 in all).  Eight distinct trajectories tiled, every
    trajectory with a start pose of its own, so that every map differs.  Checked against the oracle: trajectories 0, 1,
    the last, both sides of the 65 535-group boundary (1 040 trajectories of 63 groups) and 40 random others; every map
    received its hits."""
    L, n_scan, n = 1041, 1009, 16
    base = [syn.make_replay(n_scan, n, seed=30 + k, stride=5).ranges for k in range(8)]
    ranges = np.stack([base[l % 8] for l in range(L)])
    p0 = np.random.default_rng(31).normal(0, [0.6, 0.6, 0.8], size=(L, 3))
    ctx = slam.Context(0)
    grid = slam.DeviceGrid.metric(L, 544, 544, 0.05, context=ctx)
    try:
        poses, T, it = slam.replay_host(ranges, AMIN, AMAX, grid=grid, pose0=p0, grid_of_traj=np.arange(L), context=ctx)
        per = BOUND // ((n_scan - 1 + 15) // 16)
        sample = {0, 1, L - 1} | {per - 1, per} | set(np.random.default_rng(32).choice(L, 40, replace=False).tolist())
        for l in sorted(sample):
            og = checks.metric_grid(544, 544, 0.05)
            op, oT, oit, _ = checks.replay_reference(ranges[l], AMIN, AMAX, og, pose0=tuple(p0[l]), threads=16)
            assert np.array_equal(it[l], oit), l
            assert np.max(np.abs(poses[l] - op)) < FTOL and np.max(np.abs(T[l] - oT)) < FTOL, l
            _assert_grid(grid, l, og)
        _, h = grid.counters_torch()
        hits = h.sum(dim=(1, 2)).cpu().numpy()
        assert hits.shape == (L,) and int(hits.min()) > 0, np.nonzero(hits <= 0)[0][:10]
        assert not np.array_equal(grid.read(0, want=("pass",))["pass"], grid.read(8, want=("pass",))["pass"])
    finally:
        grid.close()
        ctx.close()


# ------------------------------------------------------------------ B: the batch axis on gridDim.y
def test_nn_pairs_past_the_row_bound(slam):
    """B1: slam_nn with B = 65 537 pairs of 24 x 24 points (k_nn: a row of the grid per pair): every index and
    distance against the oracle."""
    B, n = BOUND + 2, 24
    rng = np.random.default_rng(41)
    src = rng.uniform(-5, 5, (B, 2, n))
    tar = src[:, :, rng.permutation(n)] + rng.normal(0, 0.3, (B, 2, n))
    dist, idx = np.empty((B, n)), np.empty((B, n), dtype=np.int32)
    ctx = slam.Context(0)
    try:
        A = slam._abi
        A.check(A.lib().slam_nn(ctx.handle, A.ptr(src), A.ptr(tar), B, n, n, A.F64, A.ptr(dist), A.ptr(idx)))
    finally:
        ctx.close()
    for b in range(B):
        od, oi = co.find_nearest(src[b].T, tar[b].T)
        assert np.array_equal(idx[b], oi) and np.max(np.abs(dist[b] - od)) < 1e-12, b


def _pair_trajectories(syn, L, n, seeds):
    """L two-scan trajectories cut from a few longer replays (consecutive scans), a start pose each."""
    base = [syn.make_replay(L // len(seeds) + 2, n, seed=s, stride=5).ranges for s in seeds]
    per = L // len(seeds) + 1
    ranges = np.stack([base[l // per][l % per: l % per + 2] for l in range(L)])
    p0 = np.random.default_rng(seeds[0]).normal(0, [1.5, 1.5, 1.0], size=(L, 3))
    return ranges, p0


def _oracle_pairs(ranges, p0, og):
    L = ranges.shape[0]
    poses, T, it, visits = np.empty((L, 1, 3)), np.empty((L, 1, 3, 3)), np.empty((L, 1), dtype=np.int32), 0
    for l in range(L):
        poses[l], T[l], it[l], v = co.replay(ranges[l], AMIN, AMAX, og, pose0=tuple(p0[l]), threads=1, mt_grid=True)
        visits += v
    return poses, T, it, visits


def test_replay_trajectories_past_the_row_bound(slam, syn):
    """B2: replay_host with L = 65 537 trajectories of 2 scans x 32 beams into one shared map - the scan matcher, the
    pose step and the ray casts with a row per trajectory.  200 x 200 with direct atomics (0), the automatic choice (1:
    the window) and the window (3); 560 x 560 with the tiles (2) and wedges (4), whose group count (one a trajectory)
    also crosses the bound of part A.  Every pose, transform and iteration count, counters and visits."""
    L, n = BOUND + 2, 32
    ranges, p0 = _pair_trajectories(syn, L, n, (51, 52, 53, 54))
    for xw, reso, modes in ((200, 0.1, (0, 1, 3)), (560, 0.05, (2, 4))):
        og = checks.metric_grid(xw, xw, reso)
        oposes, oT, oit, ov = _oracle_pairs(ranges, p0, og)
        assert len(set(oit[:, 0].tolist())) > 1
        for mode in modes:
            ctx = _ctx(slam, mode, 0)
            grid = slam.DeviceGrid.metric(1, xw, xw, reso, context=ctx)
            try:
                poses, T, it = slam.replay_host(ranges, AMIN, AMAX, grid=grid, pose0=p0, context=ctx)
                assert np.array_equal(it, oit), (mode, np.nonzero(it != oit)[0][:10])
                assert np.max(np.abs(poses - oposes)) < FTOL and np.max(np.abs(T - oT)) < FTOL, mode
                _assert_grid(grid, 0, og, ov)
            finally:
                grid.close()
                ctx.close()


def test_particle_hypotheses_past_the_row_bound(slam, syn):
    """B3: slam_particles with P = 65 537 hypotheses of one 90-beam scan pair, a 64 x 64 @ 0.25 m map each (the matcher
    and the per-map casts with a row per hypothesis).  T, pose, iterations and map cells of hypotheses 0, 1, 65 534 ..
    65 536 and 60 random others against the oracle; every map received its hits."""
    P, n = BOUND + 2, 90
    rep = syn.make_replay(2, n, seed=61, stride=5)
    mats = slam.prior_matrices(syn.particle_priors(P, seed=62))
    pose_prev = np.random.default_rng(63).normal(0, 1.5, size=(P, 3))
    ctx = slam.Context(0)
    grid = slam.DeviceGrid.metric(P, 64, 64, 0.25, context=ctx)
    try:
        poses, T, it = slam.particles_host(rep.ranges[0], rep.ranges[1], AMIN, AMAX, mats, pose_prev, grid=grid, context=ctx)
        sample = sorted({0, 1, P - 3, P - 2, P - 1} | set(np.random.default_rng(64).choice(P, 60, replace=False).tolist()))
        par = checks.compare_particles(poses, T, it, lambda p: grid.read(p, want=("pmap", "pass", "hit")), sample,
                                       rep.ranges[0], rep.ranges[1], AMIN, AMAX, mats, pose_prev, 64, 64, 0.25)
        assert par["iters_equal"] and par["pose_max_abs_err"] < FTOL and par["T_max_abs_err"] < FTOL, par
        assert par["counter_cell_mismatches"] == 0 and par["pmap_cell_mismatches"] == 0, par
        _, h = grid.counters_torch()
        hits = h.sum(dim=(1, 2)).cpu().numpy()
        assert hits.shape == (P,) and int(hits.min()) > 0, np.nonzero(hits <= 0)[0][:10]
        assert len(set(it.tolist())) > 1
    finally:
        grid.close()
        ctx.close()


def test_map_observation_past_the_row_bound(slam, syn, g5):
    """B4: Localization.map_observation_batch with 65 537 pose hypotheses of one 90-beam scan (k_virtual_scan: a row
    per pose, then the matcher): hypotheses 0, 1, 65 534 .. 65 536 and 60 random others against the oracle."""
    B, n = BOUND + 2, 90
    rng = np.random.default_rng(71)
    loc = slam.Localization()
    loc.obstacle = g5["obs_wall"]
    true_pose = np.array([0.7, -0.4, 0.3])
    r = syn.scans_from_poses(syn.World(5.0, 4.0, (), 0.0), true_pose[None], n, 5)[0]
    msg = slam.LaserScan(ranges=tuple(float(v) for v in r), angle_min=AMIN, angle_max=AMAX, angle_increment=(AMAX - AMIN) / (n - 1))
    loc.src_pc = loc.laserToNumpy(msg)
    poses = true_pose + rng.normal(0, [0.1, 0.1, 0.03], size=(B, 3))
    T, it = loc.map_observation_batch(msg, poses)
    assert T.shape == (B, 3, 3) and it.shape == (B,)
    src = on.laser_to_numpy(np.asarray(msg.ranges), AMIN, AMAX)
    for k in sorted({0, 1, B - 3, B - 2, B - 1} | set(rng.choice(B, 60, replace=False).tolist())):
        want = on.map_observation(g5["obs_wall"], poses[k], src, AMIN, AMAX, msg.angle_increment)
        assert np.max(np.abs(T[k] - want)) < FTOL, k
    assert it.min() >= 1
