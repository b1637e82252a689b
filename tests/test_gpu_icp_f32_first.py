"""The float32 pre-filter in the FIRST iteration of the one-wave scan matcher (context option "icp_f32_filter", F32Image and
nn_listed_wave in csrc/icp_kernels.hip): the float32 image of the target is built before the first iteration, in the
list's place, and the list is kept in registers, dealt to the lanes by a lane exchange; the lanes' own windows, the probe of the listed queries and their windows
run in float32 first, a wave with an unsettled lane runs the float64 scan, the row search and the box search stay float64.

As in tests/test_gpu_icp_f32_filter.py the option may change NO result: every case runs with the option 0 and 1 in the
one-wave shape ("icp_one_wave" = 1) and asks for byte-identical transforms, poses and iteration counts, then holds the
filtered run against the oracle at that file's tolerance (iteration counts exact, transforms to 1e-9)."""
import numpy as np
import pytest

import test_gpu_icp_f32_filter as f32
import test_gpu_icp_one_wave as ow
from conftest import load_golden, pkg
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu

AMIN, AMAX = ow.AMIN, ow.AMAX


@pytest.fixture(scope="module")
def slam():
    return pkg()


@pytest.fixture(scope="module")
def six_scans(slam):
    """The benchmark's room, 360 beams, every fifth scan: 5 pairs."""
    r = ow.room(slam, 6, 360, seed=1)
    r.setflags(write=False)
    return r


# ---- the first iteration alone, two, and a whole solve

@pytest.mark.parametrize("max_iter", [1, 2, 30])
@pytest.mark.parametrize("points", ["f64", "f32", "f16"])
def test_replay_by_storage_type_and_iteration_limit(slam, six_scans, points, max_iter):
    T, it = f32.check_replay(slam, six_scans, points=points, max_iter=max_iter)
    assert int(it.max()) <= max_iter and (max_iter > 1 or np.all(it == 1))


@pytest.mark.parametrize("n", [65, 384])
def test_a_lone_and_a_full_last_query_slot(slam, n):
    """65 beams: the second slot holds lane 0's query alone; 384: all six slots full."""
    f32.check_replay(slam, ow.room(slam, 6, n, seed=200 + n))


# ---- the list

def test_more_listed_queries_than_the_list_holds(slam):
    """Range jumps in 70 % of the beams (tests/test_gpu_icp_one_wave.py): some 250 of 360 first-iteration queries have no
    usable window, the list holds 96, the box search takes the rest."""
    rng = np.random.default_rng(31)
    r = ow.room(slam, 6, 360, seed=5)
    m = rng.random(r.shape) < 0.7
    r[m] = rng.uniform(0.3, 25.0, size=int(m.sum())).astype(np.float32)
    for max_iter in (1, 30):
        f32.check_replay(slam, r, max_iter=max_iter)


def test_no_listed_query(slam, six_scans):
    """Every scan the first one stretched by a thousandth a step: query and guess lie on one ray a few millimetres apart,
    every first-iteration window is a beam or two wide and nothing is listed."""
    r = np.stack([six_scans[0] * np.float32(1.0 + 1e-3 * k) for k in range(6)])
    for max_iter in (1, 30):
        f32.check_replay(slam, r, max_iter=max_iter)


def test_without_the_list(slam, six_scans):
    """"icp_team" = 1: no list; the lanes search windows of up to 96 beams themselves."""
    f32.check_replay(slam, six_scans, max_iter=1, icp_team=1)
    f32.check_replay(slam, six_scans, icp_team=1)


# ---- the ends of the scan

def test_windows_past_both_ends_of_a_full_turn(slam):
    """A full turn (first and last beam nearly coincide) of a smooth closed wall, turned by four beams a scan: the windows
    of the first and the last queries reach past beam 0 and past beam n - 1 in the first iteration already."""
    n, span = 360, 6.28318
    th = np.linspace(-span / 2, span / 2, n)
    rng = np.random.default_rng(44)
    r = np.stack([5.0 + 1.5 * np.sin(th + 0.07 * k) + 0.6 * np.cos(3 * (th + 0.07 * k)) for k in range(6)])
    r = (r + rng.normal(0, 0.003, size=r.shape)).astype(np.float32)
    for max_iter in (1, 30):
        f32.check_replay(slam, r, -span / 2, span / 2, max_iter=max_iter)


# ---- invalid beams, collapsed targets

def test_nan_and_zero_beams(slam, six_scans):
    """NaN, +inf and 0 ranges in every scan of a replay (NaN reaches the transforms, the same in both runs and in the
    oracle), and in the target alone, under 16 priors: the first iteration's trips run over +inf image points."""
    rng = np.random.default_rng(8)
    bad = f32.invalid_beams(six_scans, rng)
    for max_iter in (1, 30):
        f32.check_replay(slam, bad, max_iter=max_iter)
    pri = slam.prior_matrices(slam.synthetic.particle_priors(16, seed=4))
    tar, src = f32.invalid_beams(six_scans[:1], rng)[0], six_scans[1]

    def fn(ctx):
        poses, T, it = slam.particles_host(tar, src, AMIN, AMAX, pri, np.zeros((16, 3)), context=ctx)
        return T, it, poses
    T, it, _ = f32.filtered_and_not(slam, fn)
    tp, sp = np.array(co.laser_to_points(tar, AMIN, AMAX)), np.array(co.laser_to_points(src, AMIN, AMAX))
    moved = np.stack([np.stack([m[0, 0] * sp[0] + m[0, 1] * sp[1] + m[0, 2], m[1, 0] * sp[0] + m[1, 1] * sp[1] + m[1, 2]]) for m in pri])
    oT, oit, _ = co.icp_batch(np.broadcast_to(tp, (16, 2, 360)).copy(), moved, 30, 0.001)
    f32.against_oracle(T, it, oT, oit)


def test_collapsed_target(slam, six_scans):
    """A scan of range 0 throughout - every point the origin - as the target of one pair and the source of the next; and
    G8's collapsed point clouds, where the option is inert."""
    r = six_scans.copy()
    r[2] = 0.0
    for max_iter in (1, 30):
        f32.check_replay(slam, r, max_iter=max_iter)
    g8 = load_golden("g8_collapsed.npz")

    def fn(ctx):
        return slam.icp_batch_host(g8["tar_rows"], g8["src"], 30, 0.001, context=ctx)
    T, it, _ = f32.filtered_and_not(slam, fn)
    oT, oit, _ = co.icp_batch(g8["tar_rows"], g8["src"], 30, 0.001)
    f32.against_oracle(T, it, oT, oit)


# ---- ties

def test_golden_tie_replays_take_the_second_pass_where_they_did(slam):
    """G10: iteration counts that depend on the reference's tie rule, as the golden file has them - with and without the
    filter, so the second pass is taken for the same pairs; G9's staircase scans."""
    g10 = load_golden("g10_sqrt_ties.npz")
    for c, (seed, n, span) in enumerate(g10["cases"]):
        rr = g10["c%d_ranges" % c]
        T, it, _ = f32.filtered_and_not(slam, f32.replay_fn(slam, rr, -span / 2, span / 2))
        f32.against_oracle(T, it, g10["c%d_T" % c], g10["c%d_iters" % c])
    f32.check_replay(slam, load_golden("g9_near_ties.npz")["stair_ranges"], -1.5, 1.5)
