"""The scan matcher's one-wave-per-pair shape (context option "icp_one_wave", k_icp<T>) against the oracle AND against
the other shapes (option 0) on the same inputs: iteration counts equal, transforms within 1e-12 of the other shape (sums
are added in another order, nothing else differs) and within 1e-9 of the oracle.

That the shape under test really ran is read off the transforms: two shapes add a pair's sums in different orders, so
on ordinary scans some transform differs in its last bits, while a fall-back to the other shapes is bit-identical."""
import numpy as np
import pytest

from conftest import load_golden, pkg
from oracle import c_oracle as co
from oracle import checks

pytestmark = pytest.mark.gpu

AMIN, AMAX = -3.14159, 3.14159
SHAPE_TOL, ORACLE_TOL = 1e-12, 1e-9


@pytest.fixture(scope="module")
def slam():
    return pkg()


def with_option(slam, one_wave, fn, **options):
    ctx = slam.Context(0)
    try:
        ctx.set_option("icp_one_wave", one_wave)
        for k, v in options.items():
            ctx.set_option(k, v)
        return fn(ctx)
    finally:
        ctx.close()


def both(slam, fn, **options):
    """fn(ctx) -> (T, iters) with the one-wave shape wherever a pair fits, and never; checked against each other."""
    T1, it1 = with_option(slam, 1, fn, **options)
    T0, it0 = with_option(slam, 0, fn, **options)
    print("one wave vs other shapes: max |dT| = %.3e, iters equal: %s" % (float(np.max(np.abs(T1 - T0))), np.array_equal(it1, it0)))
    assert np.array_equal(it1, it0), (it1, it0)
    assert np.max(np.abs(T1 - T0)) <= SHAPE_TOL
    return T1, it1, T0


def against_oracle(T, it, oT, oit):
    print("against the oracle: max |dT| = %.3e" % float(np.max(np.abs(T - np.asarray(oT).reshape(T.shape)))))
    assert np.array_equal(it, oit), (it, oit)
    assert np.max(np.abs(T - np.asarray(oT).reshape(T.shape))) < ORACLE_TOL


def room(slam, scans, n, seed=3, stride=5):
    return slam.synthetic.make_replay(scans, n, seed=seed, stride=stride).ranges.copy()


def replay_fn(slam, ranges, **kw):
    def fn(ctx):
        _, T, it = slam.replay_host(ranges, AMIN, AMAX, context=ctx, **kw)
        return T, it
    return fn


def batch_fn(slam, tar, src, **kw):
    def fn(ctx):
        T, it, _ = slam.icp_batch_host(tar, src, context=ctx, **kw)
        return T, it
    return fn


def clouds(rng, B, m, n):
    """B pairs of point clouds: n source points near a rigidly moved copy of m target points on a curve."""
    s = np.sort(rng.uniform(0, 1, size=(B, max(m, n))), axis=1)
    curve = np.stack([6 * s + np.sin(9 * s), 3 * np.cos(5 * s) + 2 * s * s], axis=1)
    tar = curve[:, :, np.linspace(0, max(m, n) - 1, m).astype(int)]
    th = rng.uniform(-0.05, 0.05, size=B)
    R = np.stack([np.stack([np.cos(th), -np.sin(th)], -1), np.stack([np.sin(th), np.cos(th)], -1)], 1)
    src = np.einsum("bij,bjk->bik", R, curve[:, :, np.linspace(0, max(m, n) - 1, n).astype(int)]) + rng.normal(0, 0.1, size=(B, 2, 1))
    return np.ascontiguousarray(tar), np.ascontiguousarray(src + rng.normal(0, 0.01, size=src.shape))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 359, 360, 383, 384, 385])
def test_sizes_scans_and_point_clouds(slam, n):
    """Every size at which the lanes' six queries fill up differently; 385 source points do not fit and fall back."""
    rng = np.random.default_rng(n)
    tar, src = clouds(rng, 7, n, n)                                   # point clouds: the box search alone
    T1, it1, T0 = both(slam, batch_fn(slam, tar, src))
    oT, oit, _ = co.icp_batch(tar, src, 30, 0.001)
    against_oracle(T1, it1, oT, oit)
    if n == 385:
        assert np.array_equal(T1, T0)
    if n >= 2:                                                        # raw scans: beam windows, the list, the box search behind them
        r = room(slam, 6, n, seed=n)
        T1, it1, T0 = both(slam, replay_fn(slam, r))
        _, oT, oit, _ = co.replay(r, AMIN, AMAX, None, threads=8)
        against_oracle(T1, it1, oT, oit)
        if n == 385:
            assert np.array_equal(T1, T0)
        if n == 360:
            assert not np.array_equal(T1, T0)                         # (another order of additions: the shape did run)


@pytest.mark.parametrize("m,n", [(300, 360), (384, 100), (1000, 384), (17, 383)])
def test_target_and_source_of_different_sizes(slam, m, n):
    rng = np.random.default_rng(m + n)
    tar, src = clouds(rng, 9, m, n)
    T1, it1, _ = both(slam, batch_fn(slam, tar, src))
    oT, oit, _ = co.icp_batch(tar, src, 30, 0.001)
    against_oracle(T1, it1, oT, oit)


@pytest.mark.parametrize("points", ["f64", "f32", "f16"])
def test_storage_types(slam, points):
    r = room(slam, 9, 360, seed=11)
    T1, it1, _ = both(slam, replay_fn(slam, r, dtype=points))
    _, oT, oit, _ = checks.replay_reference(r, AMIN, AMAX, None, points, 30, 1e-3, threads=8)
    against_oracle(T1, it1, oT, oit)
    rng = np.random.default_rng(12)
    tar, src = clouds(rng, 5, 360, 360)
    npdt = {"f64": np.float64, "f32": np.float32, "f16": np.float16}[points]
    tar, src = tar.astype(npdt), src.astype(npdt)
    T1, it1, _ = both(slam, batch_fn(slam, tar, src, dtype=points))
    oT, oit, _ = co.icp_batch(tar.astype(np.float64), src.astype(np.float64), 30, 0.001)
    against_oracle(T1, it1, oT, oit)


def test_priors_point_clouds_and_particles(slam):
    """The particle form: a prior applied to the source before the solve - the originals of the final transform are
    formed a second time from source and prior."""
    rng = np.random.default_rng(21)
    pri = slam.prior_matrices(slam.synthetic.particle_priors(40, seed=4))
    tar, src = clouds(rng, 1, 360, 360)
    T1, it1, _ = both(slam, batch_fn(slam, tar[0], src[0], prior=pri))
    moved = np.stack([np.stack([m[0, 0] * src[0, 0] + m[0, 1] * src[0, 1] + m[0, 2], m[1, 0] * src[0, 0] + m[1, 1] * src[0, 1] + m[1, 2]]) for m in pri])
    oT, oit, _ = co.icp_batch(np.broadcast_to(tar[0], (40, 2, 360)).copy(), moved, 30, 0.001)
    against_oracle(T1, it1, oT, oit)
    r = room(slam, 2, 360, seed=8)

    def fn(ctx):
        _, T, it = slam.particles_host(r[0], r[1], AMIN, AMAX, pri, np.zeros((40, 3)), context=ctx)
        return T, it
    T1, it1, T0 = both(slam, fn)
    tp, sp = np.array(co.laser_to_points(r[0], AMIN, AMAX)), np.array(co.laser_to_points(r[1], AMIN, AMAX))
    moved = np.stack([np.stack([m[0, 0] * sp[0] + m[0, 1] * sp[1] + m[0, 2], m[1, 0] * sp[0] + m[1, 1] * sp[1] + m[1, 2]]) for m in pri])
    oT, oit, _ = co.icp_batch(np.broadcast_to(tp, (40, 2, 360)).copy(), moved, 30, 0.001)
    against_oracle(T1, it1, oT, oit)
    assert not np.array_equal(T1, T0)


@pytest.mark.parametrize("team", [0, 1])
def test_pairs_flagged_for_the_exact_pass(slam, team):
    """Quantised ranges: the reference's tie rule decides dozens of queries (counted by the oracle; ordering by squares
    would change iteration counts), so flagged pairs are re-done by the second pass of the one-wave shape - and G10's
    replays, whose iteration counts depend on it."""
    rng = np.random.default_rng(6)
    scans, n, span = 120, 360, 6.28318
    r = np.round(rng.uniform(0.5, 8.0, size=(scans, 1)) + np.cumsum(rng.integers(-1, 2, size=(scans, n)), axis=1) * 0.25, 2).clip(0.25, 30).astype(np.float32)
    co.nn_rule_splits()
    _, oT, oit, _ = checks.replay_reference(r, -span / 2, span / 2, None, "f64", 30, 1e-3, threads=8)
    assert co.nn_rule_splits() >= 30                                 # some pairs ARE flagged: the rule is exercised ...
    co.set_nn_rule(1)
    try:
        _, oT1, oit1, _ = checks.replay_reference(r, -span / 2, span / 2, None, "f64", 30, 1e-3, threads=8)
    finally:
        co.set_nn_rule(0)
    assert not np.array_equal(oit, oit1)                             # ... and a solve without the second pass would be found out

    def fn(ctx):
        _, T, it = slam.replay_host(r, -span / 2, span / 2, context=ctx)
        return T, it
    T1, it1, _ = both(slam, fn, icp_team=team)
    against_oracle(T1, it1, oT, oit)
    g10 = load_golden("g10_sqrt_ties.npz")
    for c, (seed, n, span) in enumerate(g10["cases"]):
        rr = g10["c%d_ranges" % c]

        def fn(ctx):
            _, T, it = slam.replay_host(rr, -span / 2, span / 2, context=ctx)
            return T, it
        T1, it1, _ = both(slam, fn, icp_team=team)
        against_oracle(T1, it1, g10["c%d_T" % c], g10["c%d_iters" % c])


def test_collapsed_source_and_target_sets(slam):
    rng = np.random.default_rng(1)
    cloud = np.array([[0.3, 103.1, 211.7], [0.7, 97.3, -54.9]])
    srcs = np.stack([cloud[:, :1] + rng.normal(0, 0.2, size=(2, 300)) for _ in range(20)])       # every match is target 0
    tars = np.broadcast_to(cloud, (20, 2, 3)).copy()
    T1, it1, _ = both(slam, batch_fn(slam, tars, srcs))
    oT, oit, _ = co.icp_batch(tars, srcs, 30, 0.001)
    against_oracle(T1, it1, oT, oit)
    assert np.max(np.abs(T1[:, 0, 0] - 1.0)) < 1e-12 and np.max(np.abs(T1[:, 1, 0])) < 1e-12
    same = np.tile(cloud[:, :1], (1, 5))                                                         # coinciding targets, other indices
    tars = np.broadcast_to(np.hstack([same, same]), (20, 2, 10)).copy()
    T1, it1, _ = both(slam, batch_fn(slam, tars, srcs))
    oT, oit, _ = co.icp_batch(tars, srcs, 30, 0.001)
    against_oracle(T1, it1, oT, oit)
    assert np.max(np.abs(T1[:, 0, 0] - 1.0)) < 1e-12 and np.max(np.abs(T1[:, 1, 0])) < 1e-12
    src = np.tile(np.array([[0.1], [0.7]]), (1, 200))                                           # collapsed source
    tar = rng.normal(0, 2, size=(6, 2, 230))
    T1, it1, _ = both(slam, batch_fn(slam, tar, np.broadcast_to(src, (6, 2, 200)).copy()))
    oT, oit, _ = co.icp_batch(tar, np.broadcast_to(src, (6, 2, 200)).copy(), 30, 0.001)
    against_oracle(T1, it1, oT, oit)
    assert np.array_equal(T1[:, :2, :2], np.broadcast_to(np.eye(2), (6, 2, 2)))


@pytest.mark.parametrize("team", [0, 1])
def test_first_iteration_that_overfills_the_list(slam, team):
    """Range jumps in 70 % of the beams: some 250 of 360 first-iteration queries have no usable window, the list holds 96."""
    rng = np.random.default_rng(31)
    r = room(slam, 8, 360, seed=5)
    m = rng.random(r.shape) < 0.7
    r[m] = rng.uniform(0.3, 25.0, size=int(m.sum())).astype(np.float32)
    T1, it1, _ = both(slam, replay_fn(slam, r), icp_team=team)
    _, oT, oit, _ = co.replay(r, AMIN, AMAX, None, threads=8)
    against_oracle(T1, it1, oT, oit)


@pytest.mark.parametrize("max_iter", [0, 1, 30])
def test_iteration_limits(slam, max_iter):
    r = room(slam, 8, 360, seed=17, stride=12)
    T1, it1, _ = both(slam, replay_fn(slam, r, max_iter=max_iter))
    _, oT, oit, _ = co.replay(r, AMIN, AMAX, None, max_iter=max_iter, threads=8)
    against_oracle(T1, it1, oT, oit)
    assert int(it1.max()) <= max_iter
    tar, src = clouds(np.random.default_rng(max_iter), 4, 200, 250)
    T1, it1, _ = both(slam, batch_fn(slam, tar, src, max_iter=max_iter))
    oT, oit, _ = co.icp_batch(tar, src, max_iter, 0.001)
    against_oracle(T1, it1, oT, oit)


def test_automatic_rule_takes_the_shape_for_a_batch_that_fills_the_chip(slam):
    """17 x 999 = 16 983 pairs of 360 beams - four rounds of the pairs resident in this shape - with the option left at
    -1: the same iteration counts as with 0, transforms to rounding - and not bit for bit, as they would be from the same
    shape.  Smaller launches keep their shape, bit-identical: 3 x 999 pairs, and a lone 999-pair launch."""
    r = np.stack([room(slam, 1000, 360, seed=40 + k) for k in range(17)])
    Ta, ita = with_option(slam, -1, replay_fn(slam, r))
    T0, it0 = with_option(slam, 0, replay_fn(slam, r))
    print("automatic vs never: max |dT| = %.3e" % float(np.max(np.abs(Ta - T0))))
    assert np.array_equal(ita, it0) and np.max(np.abs(Ta - T0)) <= SHAPE_TOL
    assert not np.array_equal(Ta, T0)
    T1, it1 = with_option(slam, 1, replay_fn(slam, r))
    assert np.array_equal(T1, Ta) and np.array_equal(it1, ita)        # ... and it is the shape option 1 takes
    for part, opts in ((r[:3], {}), (r[0], {"icp_qpt": 3})):
        Ta, ita = with_option(slam, -1, replay_fn(slam, part), **opts)
        T0, it0 = with_option(slam, 0, replay_fn(slam, part), **opts)
        assert np.array_equal(ita, it0) and np.array_equal(Ta, T0)


def test_particle_batches_keep_their_shape_under_the_automatic_rule(slam):
    """2 500 and 10 000 hypotheses of one scan pair (the batch sizes from which the particle path asks for three queries a
    lane): below four rounds of one-wave pairs, so -1 leaves them the shape they had - bit-identical to 0 - while 1 takes
    the one-wave shape: same iteration counts, transforms to rounding."""
    r = room(slam, 2, 360, seed=9)
    for P in (2500, 10000):
        pri = slam.prior_matrices(slam.synthetic.particle_priors(P, seed=6))

        def fn(ctx):
            _, T, it = slam.particles_host(r[0], r[1], AMIN, AMAX, pri, np.zeros((P, 3)), context=ctx)
            return T, it
        Ta, ita = with_option(slam, -1, fn)
        T0, it0 = with_option(slam, 0, fn)
        assert np.array_equal(ita, it0) and np.array_equal(Ta, T0), P
        T1, it1 = with_option(slam, 1, fn)
        print("%d particles, one wave vs other shapes: max |dT| = %.3e" % (P, float(np.max(np.abs(T1 - T0)))))
        assert np.array_equal(it1, it0) and np.max(np.abs(T1 - T0)) <= SHAPE_TOL, P
        assert not np.array_equal(T1, T0)
