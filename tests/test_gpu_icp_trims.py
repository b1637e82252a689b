"""The one-wave-per-pair shape of the scan matcher (context option "icp_one_wave" = 1, k_icp<T>) after its trims: the
square root without range scaling (sqrt_unscaled / match_distance_wave in csrc/icp_kernels.hip), and with it the paths
the shape keeps - small replays in every storage type and at its edge sizes, collapsed sets, coinciding targets, pairs
flagged for the exact second pass.  Bounds between the shapes and against the oracle are those of
tests/test_gpu_icp_one_wave.py.

The square root is reached through point-cloud pairs whose match distances are chosen: target j at (S j, 0), source i at
(S i, d_i) with d_i < S / 2, so that source i's nearest target is target i at the square fl(d_i^2) - asserted on the CPU
first.  The routine accepts 2^-766 <= square < 2^400; everything else takes sqrt() behind a wave-uniform branch."""
import numpy as np
import pytest

import test_gpu_icp_one_wave as ow
from conftest import load_golden, pkg
from oracle import c_oracle as co
from oracle import checks

pytestmark = pytest.mark.gpu

AMIN, AMAX = ow.AMIN, ow.AMAX
SQRT_LO, SQRT_HI = 2.0 ** -766, 2.0 ** 400           # the accepted range of sqrt_unscaled: [SQRT_LO, SQRT_HI)


@pytest.fixture(scope="module")
def slam():
    return pkg()


# ---- small replays

@pytest.mark.parametrize("points", ["f64", "f32", "f16"])
@pytest.mark.parametrize("max_iter", [0, 1, 30])
def test_small_replays_storage_types_and_iteration_limits(slam, points, max_iter):
    r = ow.room(slam, 6, 360, seed=23)
    T1, it1, _ = ow.both(slam, ow.replay_fn(slam, r, dtype=points, max_iter=max_iter))
    _, oT, oit, _ = checks.replay_reference(r, AMIN, AMAX, None, points, max_iter, 1e-3, threads=8)
    ow.against_oracle(T1, it1, oT, oit)
    assert int(it1.max()) <= max_iter


@pytest.mark.parametrize("n", [65, 384])
def test_small_replays_at_the_edges_of_the_shape(slam, n):
    """65 beams: the second query of a lane exists in one lane only; 384: the most the shape holds."""
    r = ow.room(slam, 6, n, seed=n + 1)
    T1, it1, T0 = ow.both(slam, ow.replay_fn(slam, r))
    _, oT, oit, _ = co.replay(r, AMIN, AMAX, None, threads=8)
    ow.against_oracle(T1, it1, oT, oit)
    assert not np.array_equal(T1, T0)                                 # (another order of additions: the shape did run)


# ---- the square root

N_SQ = 70                                             # two queries a lane: the second in six lanes only


def chosen_distances(d, S):
    """One pair: target j at (S j, 0), source i at (S i, d[i])."""
    j = np.arange(N_SQ, dtype=np.float64)
    tar = np.stack([S * j, np.zeros(N_SQ)])
    src = np.stack([S * j, np.asarray(d, dtype=np.float64) * np.ones(N_SQ)])
    return tar, src


def squares_of(tar, src):
    """What the kernels form for source i against target i, fma(dy, dy, dx dx) with dx = 0: fl(dy^2)."""
    assert np.array_equal(tar[0], src[0])
    dy = src[1] - tar[1]
    return dy * dy


def sqrt_cases():
    """(name, tar, src, check of the squares) for the seven pairs of the batch."""
    below = np.full(N_SQ, 2.0 ** -383)
    below[[3, 40, 66]] = 2.0 ** -383 * (1 - 2.0 ** -53)               # three lanes a last place or two under the range: the wave takes sqrt()
    above = np.full(N_SQ, 2.0 ** 200 * (1 - 2.0 ** -53))
    above[[0, 17, 69]] = 2.0 ** 200                                    # three lanes at the upper bound itself (excluded)
    tiny = np.finfo(np.float64).tiny
    return [
        ("exact zero", *chosen_distances(0.0, 10.0), lambda q: np.all(q == 0.0)),
        ("subnormal squares", *chosen_distances(2.0 ** -530, 10.0), lambda q: np.all((q > 0.0) & (q < tiny))),
        ("lower end, inside", *chosen_distances(2.0 ** -383, 10.0), lambda q: np.all(q == SQRT_LO)),
        ("lower end, some lanes outside", *chosen_distances(below, 10.0),
         lambda q: np.sum(q < SQRT_LO) == 3 and np.all(q[q < SQRT_LO] >= SQRT_LO * (1 - 2.0 ** -51)) and np.sum(q == SQRT_LO) == N_SQ - 3),
        ("upper end, inside", *chosen_distances(2.0 ** 200 * (1 - 2.0 ** -53), 2.0 ** 202),
         lambda q: np.all(q < SQRT_HI) and np.all(q >= SQRT_HI * (1 - 2.0 ** -51))),
        ("upper end, some lanes outside", *chosen_distances(above, 2.0 ** 202), lambda q: np.sum(q == SQRT_HI) == 3 and np.sum(q < SQRT_HI) == N_SQ - 3),
        ("scan-sized squares", *chosen_distances(np.linspace(0.01, 3.0, N_SQ), 10.0), lambda q: np.all((q >= 1e-4) & (q <= 9.0))),
    ]


SQRT_CASE_NAMES = ["exact zero", "subnormal squares", "lower end, inside", "lower end, some lanes outside", "upper end, inside",
                   "upper end, some lanes outside", "scan-sized squares"]


@pytest.fixture(scope="module")
def sqrt_runs(slam):
    """The seven-pair batch, solved once per iteration limit by the oracle and by both settings of the option."""
    cases = sqrt_cases()
    assert [c[0] for c in cases] == SQRT_CASE_NAMES
    tar = np.stack([c[1] for c in cases])
    src = np.stack([c[2] for c in cases])
    runs = {}
    for max_iter in (1, 3):
        oT, oit, oerr = co.icp_batch(tar, src, max_iter, 0.001)
        got = {}
        for one_wave in (1, 0):
            def fn(ctx):
                return slam.icp_batch_host(tar, src, max_iter, 0.001, context=ctx)
            got[one_wave] = ow.with_option(slam, one_wave, fn)
        runs[max_iter] = (np.asarray(oT).reshape(-1, 3, 3), oit, oerr, got)
    return cases, tar, src, runs


@pytest.mark.parametrize("max_iter", [1, 3])
@pytest.mark.parametrize("k", range(7), ids=[n.replace(",", "").replace(" ", "_") for n in SQRT_CASE_NAMES])
def test_square_root_at_chosen_match_distances(sqrt_runs, k, max_iter):
    """After one iteration err_out is the mean of the roots of the chosen squares.  Bounds: the roots are correctly
    rounded on both sides and 70 of them are added in two orders - 1e-12 of the largest distance is a hundred times
    that; the transform within the oracle bound of the one-wave tests, which is meant for scans of some 10 m, scaled to
    the pair's largest coordinate.  Squares of 1e300: test_square_root_of_1e300."""
    cases, tar, src, runs = sqrt_runs
    name, tk, sk, ok = cases[k]
    assert ok(squares_of(tk, sk)), name
    oT, oit, oerr, got = runs[max_iter]
    if max_iter == 1:                                                 # the oracle agrees that these ARE the distances
        want = np.mean(np.sqrt(squares_of(tk, sk)))
        assert abs(oerr[k] - want) <= 1e-12 * want, (oerr[k], want)
    scale = max(1.0, float(np.max(np.abs(np.concatenate([tk, sk], axis=1)))) / 10.0)
    dmax = float(np.max(np.abs(sk[1])))
    for one_wave in (1, 0):
        T, it, err = got[one_wave]
        print("%-32s one_wave %d: iters %d (oracle %d), err %.17g (oracle %.17g), max |dT| / scale %.3e"
              % (name, one_wave, it[k], oit[k], err[k], oerr[k], float(np.max(np.abs(T[k] - oT[k]))) / scale))
        assert it[k] == oit[k], (one_wave, it[k], oit[k])
        assert abs(err[k] - oerr[k]) <= 1e-12 * dmax, (one_wave, err[k], oerr[k])
        assert np.max(np.abs(T[k] - oT[k])) <= ow.ORACLE_TOL * scale, one_wave


def far_pairs():
    """Seven pairs of TWO points, the source 1e150 above the target: squares of 1e300 (1e300 + S^2 rounds to it: both targets
    tie for both sources under either ordering, the first wins, and the pair is flagged for the exact pass).  Two points
    because this is about the root and nothing else may leave the float64 range on the way: the solve forms its rotation as
    (A, B) / sqrt(A A + B B) from products of centred coordinates, in every launch shape, and a sum of three or more
    values of 1e150 rounds - the centred rows are then noise of 1e134 whose products square past 1e308 (seen with 70 points:
    rotation 0 / inf where the oracle, which takes hypot, has the identity).  a + a is exact, so the centred rows are zero."""
    S = 10.0 * np.arange(1, 8)
    tar = np.stack([np.array([[0.0, s], [0.0, 0.0]]) for s in S])
    src = np.stack([np.array([[0.0, s], [1e150, 1e150]]) for s in S])
    return tar, src


@pytest.mark.parametrize("max_iter", [1, 3])
def test_square_root_of_1e300(slam, max_iter):
    """Far outside the accepted range: every wave takes sqrt().  Bounds as in test_square_root_at_chosen_match_distances."""
    tar, src = far_pairs()
    q = (src[:, 1] - tar[:, 1]) ** 2
    assert np.all(np.abs(q - 1e300) <= 1e300 * 2.0 ** -51) and np.all(q + (tar[:, 0, 1:] ** 2) == q)
    oT, oit, oerr = co.icp_batch(tar, src, max_iter, 0.001)
    oT = np.asarray(oT).reshape(-1, 3, 3)
    if max_iter == 1:
        assert np.all(np.abs(oerr - 1e150) <= 1e-12 * 1e150), oerr
    for one_wave in (1, 0):
        def fn(ctx):
            return slam.icp_batch_host(tar, src, max_iter, 0.001, context=ctx)
        T, it, err = ow.with_option(slam, one_wave, fn)
        print("one_wave %d: iters %s (oracle %s), err %s (oracle %s), max |dT| / 1e149 %.3e" % (one_wave, it, oit, err, oerr, float(np.max(np.abs(T - oT))) / 1e149))
        assert np.array_equal(it, oit), (one_wave, it, oit)
        assert np.all(np.abs(err - oerr) <= 1e-12 * oerr), (one_wave, err, oerr)
        assert np.max(np.abs(T - oT)) <= ow.ORACLE_TOL * 1e149, one_wave


def test_never_won_queries(slam):
    """All-NaN target rows: no candidate ever wins, the query's square stays infinite and its distance is 0 (icp.py:97) -
    in a wave of its own and next to ordinary pairs."""
    rng = np.random.default_rng(77)
    tar, src = ow.clouds(rng, 7, N_SQ, N_SQ)
    tar[2] = np.nan
    tar[5] = np.nan
    oT, oit, oerr = co.icp_batch(tar, src, 30, 0.001)
    oT = np.asarray(oT).reshape(-1, 3, 3)
    assert np.all(np.isnan(oT[[2, 5], :2])) and oerr[2] == 0.0 and oerr[5] == 0.0     # what "never won" means for the oracle
    for one_wave in (1, 0):
        def fn(ctx):
            return slam.icp_batch_host(tar, src, 30, 0.001, context=ctx)
        T, it, err = ow.with_option(slam, one_wave, fn)
        print("one_wave %d: iters %s (oracle %s), err %s" % (one_wave, it, oit, err))
        assert np.array_equal(it, oit)
        assert np.array_equal(np.isnan(T), np.isnan(oT))
        fin = ~np.isnan(oT)
        assert np.max(np.abs(T[fin] - oT[fin])) < ow.ORACLE_TOL
        assert np.all(np.abs(err - oerr) <= 1e-12)


# ---- collapsed sets and ties

def test_collapsed_sets_and_coinciding_targets(slam):
    rng = np.random.default_rng(2)
    cloud = np.array([[0.3, 103.1, 211.7], [0.7, 97.3, -54.9]])
    srcs = np.stack([cloud[:, :1] + rng.normal(0, 0.2, size=(2, 330)) for _ in range(7)])        # every match is target 0
    for tars in (np.broadcast_to(cloud, (7, 2, 3)).copy(),
                 np.broadcast_to(np.hstack([np.tile(cloud[:, :1], (1, 5))] * 2), (7, 2, 10)).copy()):   # coinciding targets, other indices
        T1, it1, _ = ow.both(slam, ow.batch_fn(slam, tars, srcs))
        oT, oit, _ = co.icp_batch(tars, srcs, 30, 0.001)
        ow.against_oracle(T1, it1, oT, oit)
        assert np.max(np.abs(T1[:, 0, 0] - 1.0)) < 1e-12 and np.max(np.abs(T1[:, 1, 0])) < 1e-12
    src = np.broadcast_to(np.tile(np.array([[0.1], [0.7]]), (1, 200)), (7, 2, 200)).copy()       # collapsed source
    tar = rng.normal(0, 2, size=(7, 2, 230))
    T1, it1, _ = ow.both(slam, ow.batch_fn(slam, tar, src))
    oT, oit, _ = co.icp_batch(tar, src, 30, 0.001)
    ow.against_oracle(T1, it1, oT, oit)
    assert np.array_equal(T1[:, :2, :2], np.broadcast_to(np.eye(2), (7, 2, 2)))


def test_scan_with_several_beams_of_range_zero(slam):
    """Targets that coincide on different beams: the matches of a wave can differ in index and be one point."""
    r = ow.room(slam, 6, 360, seed=29)
    r[:, 100:140] = 0.0
    T1, it1, _ = ow.both(slam, ow.replay_fn(slam, r))
    _, oT, oit, _ = co.replay(r, AMIN, AMAX, None, threads=8)
    ow.against_oracle(T1, it1, oT, oit)


def test_near_tie_replay_takes_the_exact_pass(slam):
    """One G10 replay, twice in a batch: its iteration counts are those of the reference's ordering by distance - the
    oracle under the ordering by squares counts differently - so equal counts say the flagged pairs were re-done."""
    g10 = load_golden("g10_sqrt_ties.npz")
    for c, (seed, n, span) in enumerate(g10["cases"]):                # the first replay whose counts depend on the ordering
        rr = g10["c%d_ranges" % c]
        co.set_nn_rule(1)
        try:
            _, _, oit1, _ = checks.replay_reference(rr, -span / 2, span / 2, None, "f64", 30, 1e-3, threads=8)
        finally:
            co.set_nn_rule(0)
        if not np.array_equal(oit1, g10["c%d_iters" % c]):
            break
    else:
        raise AssertionError("no G10 replay tells the orderings apart")
    twice = np.stack([rr, rr])

    def fn(ctx):
        _, T, it = slam.replay_host(twice, -span / 2, span / 2, context=ctx)
        return T, it
    T1, it1, _ = ow.both(slam, fn)
    for k in range(2):
        ow.against_oracle(T1[k], it1[k], g10["c%d_T" % c], g10["c%d_iters" % c])
    assert np.array_equal(T1[0], T1[1])
