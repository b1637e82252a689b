"""The NumPy restatement of the particle-filter operators (tests/mcl_ref.py), pinned without a GPU: a particle's cost is
the window matcher's for one candidate, the integer resampler agrees with the textbook float one away from its
boundaries, the recovery case recovers the pose, and the header and the binding carry the four entry points."""
import numpy as np
import pytest

import match_ref as M
import mcl_ref as X
import raycast_ref as R
from conftest import pkg


def test_cost_is_the_matchers_for_one_candidate(syn):
    case = M.room_case(syn)
    rng = np.random.default_rng(21)
    poses = case["true"] + rng.uniform(-1.0, 1.0, (200, 3)) * np.array([0.5, 0.5, 0.3])
    poses[:5, 0] += np.array([9.0, -9.5, 0.0, 0.0, 11.0])          # beams that leave the map, and a pose outside it
    beams = X.used_beams(case["scan"], case["cos_t"], case["sin_t"], 30.0)
    w = X.weigh(case["field"][None], 20.0, 10.0, 10.0, poses[None], case["scan"][None], case["cos_t"], case["sin_t"], 30.0, 64)
    assert w["used"][0] == len(beams) > 100 and np.array_equal(w["poses"][0], poses)
    for p, got in zip(poses, w["cost"][0]):
        c, s = float(np.cos(p[2])), float(np.sin(p[2]))
        _, cost, used, _ = M.match(case["field"], 20.0, 10.0, 10.0, case["scan"], p[:2], case["cos_t"], case["sin_t"], [[c, s]], 0, 0, 0.05,
                                   30.0, 64)
        assert used == len(beams)
        assert cost == got == X.cost_scalar(case["field"], 20.0, 10.0, 10.0, beams, float(p[0]), float(p[1]), c, s, 64)
    assert len(set(w["cost"][0].tolist())) > 50 and w["cost"][0, 4] == 64 * len(beams)


def test_weigh_motion_dead_and_accumulation():
    pm = R.ring_pmap()
    fld = M.field(pm, 64)[None]
    k = X.ring_case(2, 9, 24, 40)
    poses = k["poses"].copy()
    poses[0, 2] = [np.nan, 32.0, 0.0]
    poses[0, 3] = [32.0, np.inf, 0.0]
    poses[0, 4] = [32.0, 32.0, np.inf]
    poses[0, 5] = [float(1 << 21), 32.0, 0.0]
    acc = np.zeros((2, 9), dtype=np.int32)
    acc[1, 0], acc[1, 1], acc[1, 2] = X.DEAD, X.ACC_MAX - 3, 7
    w = X.weigh(fld, 1.0, 0.0, 0.0, poses, k["ranges"], k["cos_t"], k["sin_t"], 19.0, 64, acc=acc)
    assert np.array_equal(w["cost"][0, 2:6], [-1] * 4) and np.all(w["acc"][0, 2:6] == X.DEAD) and np.all(w["cost"][0, :2] >= 0)
    assert w["cost"][1, 0] == -1 and w["acc"][1, 0] == X.DEAD and w["acc"][1, 1] == X.ACC_MAX and w["acc"][1, 2] == 7 + w["cost"][1, 2]
    assert np.array_equal(acc[1, :3], [X.DEAD, X.ACC_MAX - 3, 7])          # the caller's array is not changed
    # the motion is the pose step's composition, the cost is taken from the moved pose
    m = X.weigh(fld, 1.0, 0.0, 0.0, k["poses"], k["ranges"], k["cos_t"], k["sin_t"], 19.0, 64, motion=k["motion"], noise=k["noise"])
    p, d = k["poses"][1, 4], k["motion"][1] + k["noise"][1, 4]
    want = [(p[0] + np.cos(p[2]) * d[0]) - np.sin(p[2]) * d[1], (p[1] + np.sin(p[2]) * d[0]) + np.cos(p[2]) * d[1], p[2] + d[2]]
    assert np.array_equal(m["poses"][1, 4], want)
    again = X.weigh(fld, 1.0, 0.0, 0.0, m["poses"], k["ranges"], k["cos_t"], k["sin_t"], 19.0, 64)
    assert np.array_equal(again["cost"], m["cost"])
    # a filter that names no map: every particle dead; no used beam: cost 0
    n = X.weigh(fld, 1.0, 0.0, 0.0, k["poses"], k["ranges"], k["cos_t"], k["sin_t"], 19.0, 64, maps=[0, 1])
    assert np.all(n["cost"][1] == -1) and np.array_equal(n["cost"][0], m["cost"][0] * 0 + n["cost"][0]) and n["used"][1] > 0
    z = X.weigh(fld, 1.0, 0.0, 0.0, k["poses"], np.full((2, 24), np.inf, np.float32), k["cos_t"], k["sin_t"], 19.0, 64)
    assert np.all(z["cost"] == 0) and np.all(z["used"] == 0)


def test_ring_cases_are_sure_of_their_costs():
    """The inputs of the GPU tests: at most 2 % of a case's particles may have a cost that one ulp in the cosine or the
    sine of the heading changes (those the GPU tests leave out)."""
    fld = M.field(R.ring_pmap(), 64)[None]
    for F, P, n, seed in X.RING_SHAPES:
        if F * P > 70000:
            continue                                                   # (the two largest are checked where they are run)
        k = X.ring_case(F, P, n, seed)
        w = X.weigh(fld, 1.0, 0.0, 0.0, k["poses"], k["ranges"], k["cos_t"], k["sin_t"], 19.0, 64, motion=k["motion"], noise=k["noise"],
                    ulp=True)
        assert w["unsure"].mean() <= 0.02, (F, P, n, seed, w["unsure"].sum())
        assert len(np.unique(w["cost"])) > min(P, 8) // 2


@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 1000])
def test_integer_resampler_against_floats(P):
    slots, left_out = 0, []
    for seed in range(8):
        rng = np.random.default_rng(100 * P + seed)
        w = rng.integers(0, X.W_MAX + 1, P)
        if seed % 3 == 1:
            w[rng.uniform(size=P) < 0.5] = 0
        if w.sum() == 0:
            w[P // 2] = 5
        u0 = rng.uniform()
        anc = X.resample_ints(w, u0)
        assert np.array_equal(anc, X.resample_u64(w, u0))
        S = float(w.sum())
        cum, q = np.cumsum(w) / S, (u0 + np.arange(P)) / P
        want = np.searchsorted(cum, q, side="right")
        near = np.array([np.min(np.abs(cum - v)) < 1e-12 for v in q])
        slots += P
        left_out += [(seed, int(j)) for j in np.flatnonzero(near)]
        assert np.array_equal(anc[~near], want[~near]), (P, seed)
        assert np.all(np.diff(anc) >= 0) and np.all(w[anc] > 0)
    # slots left out because the float quotient lies within 1e-12 of a boundary: (seed, slot)
    print("P = %d: left out %r" % (P, left_out))
    assert len(left_out) < 0.01 * slots or P <= 2 and len(left_out) == 0, left_out


def test_equal_weights_and_one_weight():
    for P in (1, 2, 63, 64, 65, 1000, 5000):
        for u0 in (0.0, 0.25, 0.5, 0.999, float(np.nextafter(1.0, 0.0))):
            for wv in (1, 7, X.W_MAX):
                f = X.resample_ints if P < 4096 else X.resample_u64
                assert np.array_equal(f(np.full(P, wv), u0), np.arange(P)), (P, u0, wv)
            one = np.zeros(P, dtype=np.int64)
            one[P // 3] = 12345
            assert np.all(X.resample_ints(one, u0) == P // 3) and np.all(X.resample_u64(one, u0) == P // 3)


def test_resample_gate_estimate_and_info():
    rng = np.random.default_rng(3)
    poses = rng.uniform(-1.0, 1.0, (3, 50, 3))
    acc = rng.integers(0, 40, (3, 50)).astype(np.int32)
    acc[1] = X.DEAD                                                    # nobody alive
    acc[2, 10:] = X.DEAD
    table = X.weight_table(2.0, 0, 64)
    r = X.resample(poses, acc, table, 0, np.array([0.3, 0.3, 0.3]), np.inf)
    assert r["info"][:, 2].tolist() == [1, 0, 1] and r["info"][1].tolist() == [-1, 0, 0, 0] and r["info"][2, 1] == 10
    assert np.all(np.isnan(r["est"][1, :3])) and r["est"][1, 3] == 0.0
    assert np.array_equal(r["ancestors"][1], np.arange(50)) and np.all(r["acc"][1] == X.DEAD) and np.all(r["acc"][[0, 2]] == 0)
    assert r["ancestors"][2].max() < 10 and r["info"][0, 0] == np.argmin(acc[0]) and r["info"][0, 3] == acc[0].min()
    ess = r["est"][0, 3]
    assert 1.0 < ess < 50.0
    for frac, go in ((0.0, 0), (ess / 50 * 0.99, 0), (ess / 50 * 1.01, 1)):
        assert X.resample(poses, acc, table, 0, np.array([0.3] * 3), frac)["info"][0, 2] == go
    w = X.weights(acc[0], table, 0)[0].astype(np.float64)
    assert np.allclose(r["est"][0, :2], (w[:, None] * poses[0, :, :2]).sum(0) / w.sum(), atol=1e-12)
    # a table that ends in 0: live particles, S = 0, no resampling
    z = X.resample(poses[:1], np.arange(50, dtype=np.int32)[None] + 5, np.array([0], np.uint32), 0, np.array([0.5]), np.inf)
    assert z["info"][0].tolist() == [0, 50, 0, 5] and np.all(np.isnan(z["est"][0, :3]))
    assert np.array_equal(X.weight_table(1.5, 3, 16, floor=2),
                          np.maximum(np.rint(2.0 ** 20 * np.exp(-(np.arange(16) * 8) / 4.5)), 2).astype(np.uint32))


def test_recovery_in_the_room(syn):
    """P = 4096 particles within +-0.3 m / +-0.1 rad of the true pose, sigma = 2 cells (table of 4096 entries, shift 0),
    cap 64, noise (0.01 m, 0.01 m, 0.005 rad), ess_frac 0.5, ten scans: the estimate of the tenth lies 0.0136 m and
    0.0004 rad from the true pose (bound: one cell, 0.05 m, and 0.02 rad); no step is further than 0.02 m / 0.004 rad."""
    case = X.recovery_case(syn)
    est, info, poses = X.recovery_run(case)
    errs = [X.pose_error(est[k], case["true"][k]) for k in range(X.REC["steps"])]
    print("recovery errors (m, rad):", errs)
    assert errs[-1][0] < X.REC_BOUND[0] and errs[-1][1] < X.REC_BOUND[1], errs[-1]
    assert all(e[0] < X.REC_BOUND[0] and e[1] < X.REC_BOUND[1] for e in errs)
    assert np.all(info[:, 1] == X.REC["P"]) and info[:, 2].sum() >= 5 and est[0, 3] < 100 < est[-1, 3]
    spread0 = case["particles"][0].std(axis=0)
    assert np.all(poses[0].std(axis=0) < 0.5 * spread0)


def test_header_and_binding_carry_the_entry_points():
    abi = pkg("_abi")
    names = abi.header_symbols()
    for s in ("slam_mcl_weigh", "slam_mcl_weigh_dev", "slam_mcl_resample", "slam_mcl_resample_dev"):
        assert s in names and s in abi._SIGS, s
        assert hasattr(abi.lib(), s)
    assert len(abi._SIGS["slam_mcl_weigh"][0]) == 18 and len(abi._SIGS["slam_mcl_resample"][0]) == 14
    assert abi.MCL_DEAD == X.DEAD == 2 ** 31 - 1
    slam = pkg()
    assert np.array_equal(slam.mcl_weight_table(2.0, 0, 4096), X.weight_table(2.0, 0, 4096))
    assert np.array_equal(slam.mcl_weight_table(1.5, 3, 16, floor=2), X.weight_table(1.5, 3, 16, floor=2))
