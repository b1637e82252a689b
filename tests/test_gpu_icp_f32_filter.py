"""The float32 pre-filter of the one-wave scan matcher's beam windows (context option "icp_f32_filter", F32Image in
csrc/icp_kernels.hip): the later iterations' trips run on a float32 image of the target, a wave all of whose lanes proved
their nearest target takes it, every other wave runs the float64 scan as before.  The option may change NO result, so
every case runs with the option 0 and 1 - the one-wave shape forced by "icp_one_wave" = 1, a handful of pairs a launch -
and asks for byte-identical transforms, poses and iteration counts; the filtered run is then held against the oracle as
tests/test_gpu_icp_one_wave.py holds the shape: iteration counts exact, transforms to 1e-9.

Correctness rests on the fall-back: a case passes whether its waves were settled in float32 or not.  How often they are
is a performance figure (profiles/icp_f32_filter.txt)."""
import numpy as np
import pytest

import test_gpu_icp_one_wave as ow
from conftest import load_golden, pkg
from oracle import c_oracle as co
from oracle import checks

pytestmark = pytest.mark.gpu

AMIN, AMAX = ow.AMIN, ow.AMAX


@pytest.fixture(scope="module")
def slam():
    return pkg()


def filtered_and_not(slam, fn, **options):
    """fn(ctx) -> tuple of arrays, under "icp_f32_filter" 1 and 0 in the one-wave shape: byte-identical, NaN included."""
    on = ow.with_option(slam, 1, fn, icp_f32_filter=1, **options)
    off = ow.with_option(slam, 1, fn, icp_f32_filter=0, **options)
    for a, b in zip(on, off):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    return on


def replay_fn(slam, ranges, amin=AMIN, amax=AMAX, **kw):
    def fn(ctx):
        poses, T, it = slam.replay_host(ranges, amin, amax, context=ctx, **kw)
        return T, it, poses
    return fn


def against_oracle(T, it, oT, oit):
    """ow.against_oracle, for results that may hold NaN (a scan with invalid beams as the source): the same places, and
    the bound on the finite ones."""
    oT = np.asarray(oT).reshape(T.shape)
    assert np.array_equal(it, np.asarray(oit).reshape(it.shape)), (it, oit)
    assert np.array_equal(np.isnan(T), np.isnan(oT))
    fin = ~np.isnan(oT)
    print("against the oracle: max |dT| = %.3e over %d finite of %d" % (float(np.max(np.abs(T[fin] - oT[fin]))) if fin.any() else 0.0, fin.sum(), fin.size))
    assert not fin.any() or np.max(np.abs(T[fin] - oT[fin])) < ow.ORACLE_TOL


def check_replay(slam, r, amin=AMIN, amax=AMAX, points="f64", max_iter=30, tol=1e-3, **options):
    T, it, _ = filtered_and_not(slam, replay_fn(slam, r, amin, amax, dtype=points, max_iter=max_iter, tolerance=tol), **options)
    for k, traj in enumerate(r if r.ndim == 3 else [r]):              # (the oracle replays one trajectory at a time)
        _, oT, oit, _ = checks.replay_reference(traj, amin, amax, None, points, max_iter, tol, threads=8)
        against_oracle(T[k] if r.ndim == 3 else T, it[k] if r.ndim == 3 else it, oT, oit)
    return T, it


# ---- sizes

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 360, 384])
def test_beam_counts(slam, n):
    """One slot only, a last slot with one lane, the shape's most; 9 scans: 8 pairs a launch."""
    check_replay(slam, ow.room(slam, 9, n, seed=100 + n))


@pytest.mark.parametrize("m,n", [(300, 360), (384, 100), (17, 383)])
def test_target_and_source_of_different_sizes(slam, m, n):
    """Point clouds (a scan pair has one beam count): no beam windows, so the option must be inert."""
    tar, src = ow.clouds(np.random.default_rng(m + n), 9, m, n)

    def fn(ctx):
        return slam.icp_batch_host(tar, src, context=ctx)
    T, it, _ = filtered_and_not(slam, fn)
    oT, oit, _ = co.icp_batch(tar, src, 30, 0.001)
    against_oracle(T, it, oT, oit)


# ---- the main path

@pytest.mark.parametrize("max_iter,tol", [(30, 1e-3), (10, 0.0)])
def test_benchmark_like_pairs(slam, max_iter, tol):
    """The benchmark's replay (seed 1, 360 beams, every fifth scan), 32 pairs; (10, 0): ten iterations for every pair."""
    r = slam.synthetic.make_replay(33, 360, seed=1, stride=5).ranges.copy()
    T, it = check_replay(slam, r, max_iter=max_iter, tol=tol)
    if tol == 0.0:
        assert np.all(it == max_iter)


@pytest.mark.parametrize("team", [0, 1])
def test_two_trajectories_with_and_without_the_list(slam, team):
    """"icp_team" = 1: no list in the first iteration, the image lies behind the boxes alone."""
    r = np.stack([ow.room(slam, 9, 360, seed=s) for s in (41, 42)])
    check_replay(slam, r, icp_team=team)


# ---- ties: the fall-back carries the tie rule

def test_golden_tie_replays(slam):
    """G10: iteration counts that depend on the reference's tie rule, as the golden file has them; G9's staircase scans."""
    g10 = load_golden("g10_sqrt_ties.npz")
    for c, (seed, n, span) in enumerate(g10["cases"]):
        rr = g10["c%d_ranges" % c]
        T, it, _ = filtered_and_not(slam, replay_fn(slam, rr, -span / 2, span / 2))
        against_oracle(T, it, g10["c%d_T" % c], g10["c%d_iters" % c])
    check_replay(slam, load_golden("g9_near_ties.npz")["stair_ranges"], -1.5, 1.5)


def test_quantised_ranges_and_circles(slam):
    """Ranges on a 0.01 m raster over staircase walls (tests/test_gpu_icp_one_wave.py: dozens of queries decided by the
    tie rule); circles about the sensor, every beam equally far, of equal and of different radius."""
    rng = np.random.default_rng(6)
    scans, n, span = 41, 360, 6.28318
    r = np.round(rng.uniform(0.5, 8.0, size=(scans, 1)) + np.cumsum(rng.integers(-1, 2, size=(scans, n)), axis=1) * 0.25, 2).clip(0.25, 30).astype(np.float32)
    check_replay(slam, r, -span / 2, span / 2)
    circles = np.repeat(np.array([4.0, 4.0, 4.1, 3.9, 4.1, 12.5, 12.5, 0.25, 0.26], dtype=np.float32)[:, None], 360, axis=1)
    check_replay(slam, circles)
    check_replay(slam, circles, -span / 2, span / 2)                  # (a full turn: first and last beam nearly coincide)


# ---- invalid beams

def invalid_beams(r, rng):
    r = r.copy()
    r[:, 0] = np.nan                                                  # the first and the last beam,
    r[:, -1] = np.inf
    r[:, 50:60] = np.nan                                              # runs,
    r[:, 200:207] = np.inf
    r[:, 100:104] = 0.0
    m = rng.random(r.shape)                                           # and scattered
    r[m < 0.03] = np.nan
    r[(m >= 0.03) & (m < 0.05)] = np.inf
    r[(m >= 0.05) & (m < 0.06)] = 0.0
    return r


def test_invalid_beams_in_a_replay(slam):
    """NaN, +inf (taken as 30 m) and 0 ranges; every scan is a target and a source, so NaN reaches the transforms - the
    same in both runs and in the oracle.  Negative ranges: no usable scan geometry, the box search alone."""
    rng = np.random.default_rng(8)
    r = ow.room(slam, 9, 360, seed=5)
    bad = invalid_beams(r, rng)
    bad[:, 0] = 0.0                                                   # (the first beam finite here: inf and 0 alone leave the results finite)
    bad[np.isnan(bad)] = np.inf
    check_replay(slam, bad)
    check_replay(slam, invalid_beams(r, rng))
    neg = r.copy()
    neg[:, 7] = -1.0
    neg[:, 200:203] = -0.5
    check_replay(slam, neg)


def test_invalid_beams_in_the_target_alone(slam):
    """The particle form: one scan pair under 16 priors.  NaN beams in the target only - the solves stay finite and the
    windows run over NaN targets - and a target with three valid beams: trips without a finite candidate."""
    rng = np.random.default_rng(9)
    r = ow.room(slam, 2, 360, seed=8)
    pri = slam.prior_matrices(slam.synthetic.particle_priors(16, seed=4))
    few = np.full(360, np.nan, dtype=np.float32)
    few[[10, 180, 300]] = r[0, [10, 180, 300]]
    for tar in (invalid_beams(r[:1], rng)[0], few):
        def fn(ctx):
            poses, T, it = slam.particles_host(tar, r[1], AMIN, AMAX, pri, np.zeros((16, 3)), context=ctx)
            return T, it, poses
        T, it, _ = filtered_and_not(slam, fn)
        tp, sp = np.array(co.laser_to_points(tar, AMIN, AMAX)), np.array(co.laser_to_points(r[1], AMIN, AMAX))
        moved = np.stack([np.stack([m[0, 0] * sp[0] + m[0, 1] * sp[1] + m[0, 2], m[1, 0] * sp[0] + m[1, 1] * sp[1] + m[1, 2]]) for m in pri])
        oT, oit, _ = co.icp_batch(np.broadcast_to(tp, (16, 2, 360)).copy(), moved, 30, 0.001)
        assert not np.isnan(np.asarray(oT)).any()
        against_oracle(T, it, oT, oit)


# ---- where float32 separates nothing

def test_ranges_times_100(slam):
    """Walls at 50 to 1 000 m, neighbouring beams metres apart: the error bound grows with the coordinates."""
    r = ow.room(slam, 9, 360, seed=13) * np.float32(100.0)
    check_replay(slam, r)


@pytest.mark.parametrize("max_iter", [2, 30])
def test_clouds_offset_by_a_million_times_their_spread(slam, max_iter):
    """The clouds of test_icp_final_transform_offset_million_times_spread (tests/test_gpu_parity.py), with its bounds: the
    rotation to 1e-9, the translation to 1e-9 of the offset."""
    reps = [slam.synthetic.make_replay(7, 120, seed=60 + s, stride=5) for s in range(3)]
    off = np.array([1.0e6, -4.0e6])
    rng = np.random.default_rng(61)
    tars, srcs = [], []
    for rep in reps:
        pts = np.stack([np.array(co.laser_to_points(r, AMIN, AMAX)) for r in rep.ranges]) * 0.25
        tars.append(pts[:-1] + off[None, :, None])
        th, tr = rng.normal(0, 0.02, len(pts) - 1), rng.normal(0, 0.03, (len(pts) - 1, 2))
        src = pts[1:]
        c, sn = np.cos(th)[:, None], np.sin(th)[:, None]
        srcs.append(np.stack([c * src[:, 0] - sn * src[:, 1] + tr[:, 0:1], sn * src[:, 0] + c * src[:, 1] + tr[:, 1:2]], axis=1) + off[None, :, None])
    tars, srcs = np.concatenate(tars), np.concatenate(srcs)

    def fn(ctx):
        return slam.icp_batch_host(tars, srcs, max_iter, 0.001, context=ctx)
    T, it, _ = filtered_and_not(slam, fn)
    oT, oit, _ = co.icp_batch(tars, srcs, max_iter, 0.001)
    oT = np.asarray(oT).reshape(T.shape)
    assert np.array_equal(it, oit), (it, oit)
    assert np.max(np.abs(T[:, :2, :2] - oT[:, :2, :2])) < ow.ORACLE_TOL
    assert np.max(np.abs(T[:, :2, 2] - oT[:, :2, 2])) < ow.ORACLE_TOL * np.abs(off).max()


# ---- storage types, collapsed sets

@pytest.mark.parametrize("points", ["f32", "f16"])
def test_storage_types(slam, points):
    """The stored target already is its float32 value: the image equals it."""
    check_replay(slam, ow.room(slam, 9, 360, seed=11), points=points)


def test_collapsed_sets(slam):
    """G8: every target point one point; the canonical answer, unchanged by the option."""
    g8 = load_golden("g8_collapsed.npz")
    src, tar = g8["src"], g8["tar_rows"]

    def fn(ctx):
        return slam.icp_batch_host(tar, src, 30, 0.001, context=ctx)
    T, it, _ = filtered_and_not(slam, fn)
    oT, oit, _ = co.icp_batch(tar, src, 30, 0.001)
    against_oracle(T, it, oT, oit)
    assert np.max(np.abs(T[:, :2, :2] - np.eye(2))) < 1e-12
