"""The scan matcher's workgroup shapes (k_icp<T, QPT, UNROLL>, one workgroup per pair: 1, 2, 3, 4 or 8 queries per lane)
at the edges of their launch decision, against the C oracle: iteration counts equal, transforms and poses within 1e-9;
two device runs against each other within 1e-12 or bit for bit.  Every case sets icp_one_wave = 0.

Every size at which the launch changes - another instance, more than 64 KiB of LDS, a shorter or no first-iteration list,
no unpadded copy of the target - comes from tests/icp_shapes.py, which asks the library's own planner (slam_plan_icp); tests/test_icp_launch_shapes_cpu.py
asserts the sizes."""
import math

import numpy as np
import pytest

import icp_shapes as sh
from conftest import pkg
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu

AMIN, AMAX = -3.14159, 3.14159
SHAPE_TOL, ORACLE_TOL = 1e-12, 1e-9
NPDT = {"f64": np.float64, "f32": np.float32, "f16": np.float16}
SCANS, CLOUDS = sh.edges(True), sh.edges(False)
# first size of each shape past the one-query shape: 1 025, 2 049, 3 073, 4 097
QPT2, QPT3, QPT4, QPT8 = (CLOUDS[k] for k in ("qpt2", "qpt3", "qpt4", "qpt8"))
assert all(SCANS[k] == CLOUDS[k] for k in ("qpt2", "qpt3", "qpt4", "qpt8"))


@pytest.fixture(scope="module")
def slam():
    return pkg()


def run(slam, fn, **options):
    """fn(ctx) in a context of its own that never takes the one-wave shape."""
    ctx = slam.Context(0)
    try:
        ctx.set_option("icp_one_wave", 0)
        for k, v in options.items():
            ctx.set_option(k, v)
        return fn(ctx)
    finally:
        ctx.close()


def batch(slam, tar, src, max_iter=30, tol=0.001, **options):
    kw = {k: options.pop(k) for k in ("dtype", "prior") if k in options}
    T, it, _ = run(slam, lambda ctx: slam.icp_batch_host(tar, src, max_iter, tol, context=ctx, **kw), **options)
    return T, it


def replay(slam, ranges, max_iter=30, tol=0.001, **options):
    return run(slam, lambda ctx: slam.replay_host(ranges, AMIN, AMAX, max_iter=max_iter, tolerance=tol, context=ctx), **options)


def against_oracle(what, T, it, oT, oit, poses=None, oposes=None):
    d = float(np.max(np.abs(T - np.asarray(oT).reshape(T.shape))))
    dp = 0.0 if poses is None else float(np.max(np.abs(poses - oposes)))
    print("%s against the oracle: max |dT| = %.3e, max |dpose| = %.3e, iterations %s" % (what, d, dp, np.asarray(it).tolist()[:8]))
    assert np.array_equal(it, oit), (it, oit)
    assert d < ORACLE_TOL and dp < ORACLE_TOL


def clouds(rng, B, m, n):
    """B pairs of point clouds: n source points near a rigidly moved copy of m target points on a curve."""
    s = np.sort(rng.uniform(0, 1, size=(B, max(m, n))), axis=1)
    curve = np.stack([6 * s + np.sin(9 * s), 3 * np.cos(5 * s) + 2 * s * s], axis=1)
    tar = curve[:, :, np.linspace(0, max(m, n) - 1, m).astype(int)]
    th = rng.uniform(-0.05, 0.05, size=B)
    R = np.stack([np.stack([np.cos(th), -np.sin(th)], -1), np.stack([np.sin(th), np.cos(th)], -1)], 1)
    src = np.einsum("bij,bjk->bik", R, curve[:, :, np.linspace(0, max(m, n) - 1, n).astype(int)]) + rng.normal(0, 0.1, size=(B, 2, 1))
    return np.ascontiguousarray(tar), np.ascontiguousarray(src + rng.normal(0, 0.01, size=src.shape))


def room(slam, scans, n, seed):
    return slam.synthetic.make_replay(scans, n, seed=seed, stride=5).ranges.copy()


# ---- a. the first and last size of every shape, point clouds ---------------------------------------------------------

@pytest.mark.parametrize("n_src", [QPT2 - 1, QPT2, QPT3 - 1, QPT3, QPT4 - 1, QPT4, QPT8 - 1, QPT8, sh.N_MAX - 1, sh.N_MAX])
def test_point_clouds_either_side_of_every_shape(slam, n_src):
    """1 024 | 1 025, 2 048 | 2 049, 3 072 | 3 073, 4 096 | 4 097 and 8 191, 8 192 source points against 700 targets: the last
    full block of one instance and the first size of the next, where all but one lane of the last wave lack their later
    queries."""
    want = {QPT2 - 1: 1, QPT2: 2, QPT3 - 1: 2, QPT3: 3, QPT4 - 1: 3, QPT4: 4, QPT8 - 1: 4, QPT8: 8, sh.N_MAX - 1: 8, sh.N_MAX: 8}
    assert sh.launch(3, n_src, 700, False).qpt == want[n_src]
    tar, src = clouds(np.random.default_rng(n_src), 3, 700, n_src)
    T, it = batch(slam, tar, src)
    oT, oit, _ = co.icp_batch(tar, src, 30, 0.001)
    against_oracle("%d points" % n_src, T, it, oT, oit)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("n_src", [QPT2, QPT3, QPT4, QPT8])
def test_point_clouds_in_reduced_storage_past_every_shape_boundary(slam, n_src, dtype):
    """f32 / f16 are storage types, arithmetic stays float64: the oracle is fed the rounded points.  In f16 thousands of
    points on a curve a few units long round onto each other: exact ties throughout."""
    tar, src = clouds(np.random.default_rng(n_src + 1), 3, 700, n_src)
    tar, src = tar.astype(NPDT[dtype]), src.astype(NPDT[dtype])
    T, it = batch(slam, tar, src, dtype=dtype)
    oT, oit, _ = co.icp_batch(tar.astype(np.float64), src.astype(np.float64), 30, 0.001)
    against_oracle("%d points, %s" % (n_src, dtype), T, it, oT, oit)


# ---- b. the second pass in the wide shapes ---------------------------------------------------------------------------

def tie_clouds(rng, n_src, n_tar):
    """One pair -> (tar [2][n_tar], src [2][n_src]) with distance ties built in, in thirds:
      staircase  the first third of the targets is a polar scan with ranges in steps of 0.25; a staircase query sits on a
                 beam whose two neighbours hold the query's range, mirror images about the query's beam: tied in real
                 arithmetic, their squares round apart, and where they share a square root the reference's rule (lowest
                 index) differs from the order of the squares (there are more queries than such beams: beams repeat);
      lattice    targets on multiples of 1/4 (sites taken twice: exact ties), queries on multiples of 1/8;
      free       uniform in the square.
    No NaN anywhere: the reference's transform would be NaN."""
    kt, ks = n_tar // 3, n_src // 3
    ang = np.linspace(-math.pi, math.pi, kt, endpoint=False)
    rt = np.clip(3.0 + 0.25 * np.cumsum(rng.integers(-1, 2, size=kt)), 0.5, 6.0)
    beams = 1 + 3 * rng.choice((kt - 2) // 3, size=ks, replace=True)
    rq = rt[beams]
    rt[beams - 1] = rt[beams + 1] = rq
    rt[beams] = rq + 0.25
    tar = [np.column_stack((np.cos(ang) * rt, np.sin(ang) * rt)),
           rng.integers(-24, 25, size=(kt, 2)) * 0.25, rng.uniform(-6.0, 6.0, size=(n_tar - 2 * kt, 2))]
    src = [np.column_stack((np.cos(ang[beams]) * rq, np.sin(ang[beams]) * rq)),
           rng.integers(-48, 49, size=(ks, 2)) * 0.125, rng.uniform(-6.0, 6.0, size=(n_src - 2 * ks, 2))]
    return np.ascontiguousarray(np.vstack(tar).T), np.ascontiguousarray(np.vstack(src).T)


def tie_pairs(n_src, n_tar, B=3):
    """B pairs of tie_clouds and the oracle's solve of them, drawn again from the case's seed until the oracle counts
    at least one query that ordering by the square would answer differently: the second pass is needed."""
    rng = np.random.default_rng(5000 + n_src)
    for _ in range(16):
        pairs = [tie_clouds(rng, n_src, n_tar) for _ in range(B)]
        tar, src = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        co.nn_rule_splits()
        oT, oit, _ = co.icp_batch(tar, src, 30, 0.001)
        splits = co.nn_rule_splits()
        if splits > 0:
            return tar, src, oT, oit, splits
    raise AssertionError("no draw exercises the tie rule")


@pytest.mark.parametrize("n_src", [QPT3, QPT4, QPT8])
def test_second_pass_with_three_four_and_eight_queries_per_lane(slam, n_src):
    """Clouds with built-in ties at the first size of the three wide shapes, 900 targets: the first pass flags the pair
    (the flag crosses the waves through LDS) and the whole workgroup re-does it with the reference's own rule."""
    tar, src, oT, oit, splits = tie_pairs(n_src, 900)
    print("%d points: the oracle counts %d queries that the order of the squares would answer differently" % (n_src, splits))
    T, it = batch(slam, tar, src)
    against_oracle("%d points with ties" % n_src, T, it, oT, oit)


def lone_tie_pair(rng, n_src, n_tar, at):
    """One pair of unrelated uniform clouds whose ONLY built-in tie is source point `at`: it sits on a beam of a staircase
    scan (the first third of the targets) between two mirror-image neighbours, on a beam chosen so that the oracle counts
    it - the two squares differ and share a square root."""
    for _ in range(64):
        tar, src = tie_clouds(rng, 3 * ((n_tar // 3 - 2) // 3), n_tar)          # a staircase query on every third beam
        stair = src[:, :(n_tar // 3 - 2) // 3]
        for k in range(stair.shape[1]):
            co.nn_rule_splits()
            co.find_nearest(np.ascontiguousarray(stair[:, k:k + 1].T), np.ascontiguousarray(tar.T))
            if co.nn_rule_splits() == 1:
                out = rng.uniform(-6.0, 6.0, size=(2, n_src))
                out[:, at] = stair[:, k]
                return tar, out
    raise AssertionError("no beam exercises the tie rule")


@pytest.mark.parametrize("n_src", [QPT3, QPT4, QPT8])
def test_second_pass_asked_for_by_one_lane_of_the_last_wave(slam, n_src):
    """The only query that needs the reference's rule belongs to the LAST wave of the workgroup (its first query): the flag
    has to cross the waves for the pair to be re-done.  One iteration, so that the one match is in the transform: the
    oracle with the order of the squares instead answers differently by far more than the bound."""
    s = sh.launch(3, n_src, 900, False)
    at = (s.waves - 1) * 64 + 5
    assert s.waves >= 9 and at < n_src
    rng = np.random.default_rng(6000 + n_src)
    pairs = [lone_tie_pair(rng, n_src, 900, at) for _ in range(3)]
    tar, src = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    co.nn_rule_splits()
    oT, oit, _ = co.icp_batch(tar, src, 1, 0.001)
    assert co.nn_rule_splits() == 3                                   # the planted query of each pair and no other
    co.set_nn_rule(1)
    try:
        oT1, _, _ = co.icp_batch(tar, src, 1, 0.001)
    finally:
        co.set_nn_rule(0)
    assert np.min(np.max(np.abs(oT - oT1).reshape(3, -1), axis=1)) > 1000 * ORACLE_TOL
    T, it = batch(slam, tar, src, 1, 0.001)
    against_oracle("%d points, one tie in wave %d" % (n_src, s.waves - 1), T, it, oT, oit)


# ---- c. collapsed sets across 13 and 9 waves --------------------------------------------------------------------------

@pytest.mark.parametrize("n_src", [QPT4, QPT8])
def test_collapsed_sets_in_the_wide_shapes(slam, n_src):
    """Every source point matched to ONE of three far-apart targets, and a source set of one repeated point: every wave's
    verdict must reach the others (13 waves at 3 073 points, 9 at 4 097, the last with one live lane).  R = I to 1e-12."""
    rng = np.random.default_rng(n_src)
    cloud = np.array([[0.3, 103.1, 211.7], [0.7, 97.3, -54.9]])
    srcs = np.stack([cloud[:, k:k + 1] + rng.normal(0, 0.2, size=(2, n_src)) for k in (0, 1, 2, 0)])
    tars = np.broadcast_to(cloud, (4, 2, 3)).copy()
    T, it = batch(slam, tars, srcs)
    oT, oit, _ = co.icp_batch(tars, srcs, 30, 0.001)
    against_oracle("%d points about one target" % n_src, T, it, oT, oit)
    assert np.max(np.abs(T[:, 0, 0] - 1.0)) < 1e-12 and np.max(np.abs(T[:, 1, 0])) < 1e-12
    assert np.max(np.abs(oT[:, 0, 0] - 1.0)) < 1e-12 and np.max(np.abs(oT[:, 1, 0])) < 1e-12
    src = np.broadcast_to(np.tile(np.array([[0.1], [0.7]]), (1, n_src)), (3, 2, n_src)).copy()
    tar = rng.normal(0, 2, size=(3, 2, 230))
    T, it = batch(slam, tar, src)
    oT, oit, _ = co.icp_batch(tar, src, 30, 0.001)
    against_oracle("%d times one point" % n_src, T, it, oT, oit)
    assert np.max(np.abs(T[:, :2, :2] - np.eye(2))) < 1e-12
    # ... and ONE source point that differs, far enough to match another target: neither set is collapsed, and only one
    # lane of one wave knows - the very last point, or the second lane of the last wave
    waves = sh.launch(3, n_src, 230, False).waves
    for at in (n_src - 1, (waves - 1) * 64 + 1):
        other = src.copy()
        other[:, :, at] += 1.5
        T, it = batch(slam, tar, other)
        oT, oit, _ = co.icp_batch(tar, other, 30, 0.001)
        against_oracle("%d times one point and another at %d" % (n_src, at), T, it, oT, oit)
        assert np.min(np.abs(oT[:, 1, 0])) > 1e-6                     # (a rotation: the oracle did not see a collapsed set)


# ---- d. iteration limits through the hand-over ----------------------------------------------------------------------

@pytest.mark.parametrize("max_iter", [0, 1, 2, 30])
@pytest.mark.parametrize("n", [QPT3, QPT8])
def test_iteration_limits_with_tolerance_zero(slam, n, max_iter):
    """tol = 0 never converges, so max_iter decides: 0 - no iteration; 1 - the first form alone; 2 - exactly one iteration
    of the later form, in which the pair's first wave finishes the iteration and hands the result to the others; 30.
    Point clouds against 700 targets, and a replay of three scans of n beams."""
    tar, src = clouds(np.random.default_rng(n + max_iter), 3, 700, n)
    T, it = batch(slam, tar, src, max_iter, 0.0)
    oT, oit, _ = co.icp_batch(tar, src, max_iter, 0.0)
    against_oracle("%d points, max_iter %d" % (n, max_iter), T, it, oT, oit)
    assert np.all(it == max_iter)
    if max_iter == 0:
        assert np.array_equal(T, np.broadcast_to(np.eye(3), T.shape))
    r = room(slam, 3, n, seed=n)
    poses, T, it = replay(slam, r, max_iter, 0.0)
    oposes, oT, oit, _ = co.replay(r, AMIN, AMAX, None, max_iter=max_iter, tolerance=0.0, threads=8)
    against_oracle("%d beams, max_iter %d" % (n, max_iter), T, it, oT, oit, poses, oposes)
    assert np.all(it == max_iter)


# ---- e. shared sets and priors --------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [QPT2, QPT3])
def test_shared_sets_with_priors(slam, n):
    """One target and one source for five pairs (tar_shared, src_shared), a prior [5][6] applied to the source first: the
    oracle solves the five transformed sources."""
    pair = slam.synthetic.scan_pair(n, seed=n)
    tar = np.array(co.laser_to_points(pair.ranges[0], AMIN, AMAX))
    src = np.array(co.laser_to_points(pair.ranges[1], AMIN, AMAX))
    mats = slam.prior_matrices(slam.synthetic.particle_priors(5, seed=n))
    T, it = batch(slam, tar, src, prior=mats)
    srcs = np.stack([np.stack([m[0, 0] * src[0] + m[0, 1] * src[1] + m[0, 2], m[1, 0] * src[0] + m[1, 1] * src[1] + m[1, 2]]) for m in mats])
    oT, oit, _ = co.icp_batch(np.repeat(tar[None], 5, 0), srcs, 30, 0.001)
    against_oracle("%d shared points, five priors" % n, T, it, oT, oit)
    assert np.max(np.abs(T - T[0])) > 1e-6                            # the priors do make five different solves


# ---- f. the batch-size preference ------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,icp_qpt,applies", [(128, 0, False), (129, 0, True), (192, 3, False), (193, 3, True)])
def test_preference_rule_at_its_edges(slam, n, icp_qpt, applies):
    """B > 64 && qpt < pref && n_src > 64 * pref.  The first 64 pairs run as B = 64 and inside B = 65: where the rule
    applies the 65 take two (icp_qpt 3: three) queries per lane, the same iteration counts and transforms to 1e-12 - and
    NOT the same bits in every pair, the sums are added in another order; one point fewer and the two runs are the same
    launch shape, bit for bit.  Point clouds, and a replay of 66 scans (65 pairs) against its first 65 scans."""
    opts = {"icp_qpt": icp_qpt} if icp_qpt else {}
    for scans in (False, True):
        s64, s65 = sh.launch(64, n, n, scans, icp_qpt=icp_qpt), sh.launch(65, n, n, scans, icp_qpt=icp_qpt)
        assert s64.qpt == 1 and s65.qpt == ((icp_qpt or 2) if applies else 1)
    tar, src = clouds(np.random.default_rng(n), 65, n, n)
    T64, it64 = batch(slam, tar[:64], src[:64], **opts)
    T65, it65 = batch(slam, tar, src, **opts)
    r = room(slam, 66, n, seed=n)
    p64, R64, rit64 = replay(slam, r[:65], **opts)
    p65, R65, rit65 = replay(slam, r, **opts)
    for what, a, ia, b, ib in (("clouds", T64, it64, T65[:64], it65[:64]), ("scans", R64, rit64, R65[:64], rit65[:64])):
        print("%s, n = %d: 64 pairs alone against the same among 65: max |dT| = %.3e, %d of 64 transforms differ in their bits"
              % (what, n, float(np.max(np.abs(a - b))), int(np.sum(np.any(a.reshape(64, -1) != b.reshape(64, -1), axis=1)))))
        assert np.array_equal(ia, ib)
        if applies:
            assert np.max(np.abs(a - b)) <= SHAPE_TOL and not np.array_equal(a, b)
        else:
            assert np.array_equal(a, b)
    oT, oit, _ = co.icp_batch(tar, src, 30, 0.001)
    against_oracle("65 pairs of %d points" % n, T65, it65, oT, oit)
    against_oracle("64 pairs of %d points" % n, T64, it64, oT[:64], oit[:64])
    oposes, oT, oit, _ = co.replay(r, AMIN, AMAX, None, threads=8)
    against_oracle("66 scans of %d beams" % n, R65, rit65, oT, oit, p65, oposes)
    against_oracle("65 scans of %d beams" % n, R64, rit64, oT[:64], oit[:64], p64, oposes[:64])


# ---- g. scans at the LDS decisions ----------------------------------------------------------------------------------

SCAN_SIZES = [("last under 64 KiB", SCANS["raised"] - 1), ("first over 64 KiB", SCANS["raised"]),
              ("first with three per lane", SCANS["qpt3"]), ("first with four per lane", SCANS["qpt4"]),
              ("last full list", SCANS["cut"] - 1), ("first cut list", SCANS["cut"]),
              ("first with eight per lane", SCANS["qpt8"]),
              ("last list", SCANS["zero"] - 1), ("first without a list", SCANS["zero"]),
              ("last with the unpadded copy", SCANS["dropped"] - 1), ("first without the copy", SCANS["dropped"])]


@pytest.mark.parametrize("what,n", SCAN_SIZES, ids=[w.replace(" ", "_") for w, _ in SCAN_SIZES])
def test_scans_either_side_of_every_lds_decision(slam, what, n):
    """A replay of three scans of n beams at the sizes where the launch first raises the dynamic-LDS limit, cuts the
    first-iteration list to the room the LDS has, has no room for a list, and drops the unpadded copy of the target."""
    s, before = sh.launch(2, n, n, True), sh.launch(2, n - 1, n - 1, True)
    print("%s: n = %d, %s" % (what, n, s))
    if what.startswith("first"):                                      # the size is the first on its side of a decision
        assert (s.lds > sh.LDS_DEFAULT, s.qpt, s.team_cap < s.cap_wanted, s.team_cap == 0, s.polar_copy) != \
               (before.lds > sh.LDS_DEFAULT, before.qpt, before.team_cap < before.cap_wanted, before.team_cap == 0, before.polar_copy)
    r = room(slam, 3, n, seed=21)
    poses, T, it = replay(slam, r)
    oposes, oT, oit, _ = co.replay(r, AMIN, AMAX, None, threads=8)
    against_oracle("%d beams" % n, T, it, oT, oit, poses, oposes)


JUMP_SIZES = [SCANS["cut"], SCANS["qpt8"], SCANS["zero"] - 1, SCANS["zero"]]


@pytest.mark.parametrize("n", JUMP_SIZES)
def test_jumpy_scans_where_the_list_is_cut_or_absent(slam, n):
    """Every other beam of the odd scans at an unrelated range: half of the first-iteration queries have no usable window
    and ask for a list slot.  With the list (icp_team 0; what it cannot take goes to the box search of the query's own
    lane) and without (icp_team 1): bit-identical, and equal to the oracle.
    That the list overflows is inferred, it cannot be read back from the device: on such scans about half of the queries
    are listed (a fifth even on smooth ones), against room for 1 760 of 3 526, 800 of 4 097, 32 of 4 544 and none of 4 545."""
    s = sh.launch(2, n, n, True)
    assert s.polar_copy and s.team_cap < s.cap_wanted and (s.team_cap == 0) == (n == SCANS["zero"])
    assert sh.launch(2, n, n, True, icp_team=1).team_cap == 0
    print("n = %d: %d list slots, %d wanted" % (n, s.team_cap, s.cap_wanted))
    rng = np.random.default_rng(n)
    r = room(slam, 3, n, seed=22)
    r[1::2, ::2] = rng.uniform(0.5, 20.0, size=r[1::2, ::2].shape).astype(np.float32)
    p0, T0, it0 = replay(slam, r, icp_team=0)
    p1, T1, it1 = replay(slam, r, icp_team=1)
    assert np.array_equal(it0, it1) and np.array_equal(T0, T1) and np.array_equal(p0, p1)
    oposes, oT, oit, _ = co.replay(r, AMIN, AMAX, None, threads=8)
    against_oracle("%d jumpy beams" % n, T0, it0, oT, oit, p0, oposes)
