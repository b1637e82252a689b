"""The conditions test_gpu_loc_replay_bounds.py puts on its inputs, checked without a GPU: every run it compares with
``loc_ref.chain`` is stable under a nudge of ``xEst`` (no obstacle near a bin edge, no nearest neighbour near a tie), the
route tables have the properties the routing test names, the padding of the refused routes would change a result, the
CPU chain raises at exactly the step each bad beam sits in, the lane cases straddle the rule of ``launch_loc_step``, the
start poses reach the iteration caps, and the batches lie past the thresholds of the scan matcher's shape rule."""
import numpy as np
import pytest

import loc_cases as lc
import loc_ref
from conftest import load_golden
from oracle import oracle_np as on

AMIN, AMAX = lc.AMIN, lc.AMAX


@pytest.fixture(scope="module")
def wall():
    return np.ascontiguousarray(load_golden("g5_map_observation.npz")["obs_wall"])


def assert_stable(r, obstacle, pose0, eps=1e-11, **kw):
    ref, worst = loc_ref.stable(r, obstacle, AMIN, AMAX, pose0, eps=eps, **kw)
    assert worst < 1e-10, worst
    return ref


def test_loc_ref_extensions(syn, wall):
    r, p0 = lc.make_stream(syn, 2, 120, steps=3)
    inc = (AMAX - AMIN) / 119
    a, b = loc_ref.chain(r, wall, AMIN, AMAX, p0), loc_ref.chain(r, wall, AMIN, AMAX, p0, angle_increment=inc)
    assert all(np.array_equal(a[k], b[k]) for k in a)                     # the default is the present formula
    ref, worst = loc_ref.stable(r, wall, AMIN, AMAX, p0)
    assert worst < 1e-10 and all(np.array_equal(a[k], ref[k]) for k in a)
    capped, _ = loc_ref.stable(r, wall, AMIN, AMAX, p0, max_iter=1, tol=0.5)
    assert capped["iters_obs"].tolist() == [1, 1, 1] and not np.array_equal(capped["xest"], a["xest"])
    assert loc_ref.stable_bound(1e-12, 64) == pytest.approx(2.56e-10)


def test_routing_tables(syn, wall):
    c = lc.routing_case(syn, wall)
    props = lc.routing_properties(c)
    assert all(props.values()), props
    assert c["sot"].shape == c["mot"].shape == (11,) and c["ranges"].shape == (3, 4, 64) and c["maps"][2].shape == (2, 0)
    assert len(set(c["sot"][list(lc.ROUTE_CHAIN)].tolist())) == 3 and len(set(c["mot"][list(lc.ROUTE_CHAIN)].tolist())) == 3
    for l in lc.ROUTE_CHAIN:
        assert c["maps"][c["mot"][l]].shape[1] > 0
        assert_stable(c["ranges"][c["sot"][l]], c["maps"][c["mot"][l]], c["pose0"][l])
    # the streams differ and the maps differ, so a wrong route is a wrong number
    o = [loc_ref.chain(c["ranges"][s], c["maps"][m], AMIN, AMAX, c["pose0"][0])["xest"] for s, m in ((1, 1), (0, 1), (1, 3))]
    assert np.max(np.abs(o[0] - o[1])) > 1e-3 and np.max(np.abs(o[0] - o[2])) > 1e-6


def test_refused_routes_and_their_padding(syn, wall):
    c = lc.bad_route_case(syn, wall)
    S, M, K = c["S"], c["M"], c["K"]
    ok = (c["sot"] >= 0) & (c["sot"] < S) & (c["mot"] >= 0) & (c["mot"] < M)
    assert np.nonzero(ok)[0].tolist() == list(c["good"]) and np.nonzero(~ok)[0].tolist() == list(c["bad"])
    assert c["sot"].tolist() == [0, -1, S, 1, 0, 1] and c["mot"].tolist() == [0, 0, 0, -1, M, 1]
    for name in ("ranges_padded", "ox_padded", "oy_padded", "off_padded", "off_wild_padded", "pose0"):
        assert np.all(np.isfinite(c[name])), name
    assert c["ranges_padded"].shape[0] == S + 2 and np.array_equal(c["ranges_padded"][1:-1], c["ranges"].astype(np.float32))
    assert c["ox_padded"].shape == (K + 2 * lc.PAD_OBS,) and c["off_padded"][2:5].tolist() == c["off"].tolist() == [0, c["k1"], K]
    # whatever pair of entries a route in [-1, M] reads from the padded tables stays inside the padded obstacle arrays
    for table in (c["off_padded"], c["off_wild_padded"]):
        assert table.min() >= -lc.PAD_OBS and table.max() <= K + lc.PAD_OBS
    wild = c["off_wild_padded"][2:5]
    assert wild[0] < 0 and wild[-1] > K and np.clip(wild, 0, K).tolist() == c["off"].tolist()
    # an unclamped table reads ring points that are nearer than the walls: the virtual scan changes for both maps
    cat = np.vstack([c["ox_padded"], c["oy_padded"]])
    inc = (AMAX - AMIN) / (c["n"] - 1)
    for l in c["good"]:
        m = c["mot"][l]
        lo, hi = lc.PAD_OBS + wild[m], lc.PAD_OBS + wild[m + 1]
        clean = on.laser_estimation(c["maps"][m], c["pose0"][l], AMIN, inc, c["n"])
        assert not np.array_equal(clean, on.laser_estimation(cat[:, lo:hi], c["pose0"][l], AMIN, inc, c["n"])), l
        assert_stable(c["ranges"][c["sot"][l]], c["maps"][m], c["pose0"][l])
    # a stream of the padding is not the stream beside it
    assert np.max(np.abs(c["ranges_padded"][0] - c["ranges_padded"][1])) > 0.1


@pytest.mark.filterwarnings("ignore::RuntimeWarning")                   # NumPy's own, on the way to the LinAlgError
@pytest.mark.parametrize("value_a,value_b", lc.STOP_VALUES)
def test_chain_raises_at_the_step_of_the_bad_beam(syn, wall, value_a, value_b):
    c = lc.stop_case(syn, value_a, value_b)
    r = c["ranges"]
    bad = ~np.isfinite(r)
    assert bad.sum() == 2 and bad[0, 0, lc.STOP_BEAMS[0]] and bad[1, 3, lc.STOP_BEAMS[1]] and r.shape == (3, 4, 64)
    for group, step in (("A", 0), ("B", 3), ("C", None)):
        assert len(c[group]) == 2
        for l in c[group]:
            assert lc.raise_step(r[c["sot"][l]], wall, c["pose0"][l]) == step, (group, l)
    assert not np.array_equal(c["pose0"][0], c["pose0"][3])
    for l in c["B"]:
        assert_stable(r[1, :3], wall, c["pose0"][l])
    for l in c["C"]:
        assert_stable(r[2], wall, c["pose0"][l])


def test_stop_values_cover_every_kind_at_both_places():
    for col in (0, 1):
        kinds = sorted("nan" if np.isnan(v[col]) else "+inf" if v[col] > 0 else "-inf" for v in lc.STOP_VALUES)
        assert kinds == ["+inf", "-inf", "nan"]
    assert lc.STOP_VALUES[0][0] == np.inf and np.isnan(lc.STOP_VALUES[0][1])


@pytest.mark.parametrize("n,K,seed,eps", lc.LANE_CASES)
def test_lane_cases_are_stable(syn, wall, n, K, seed, eps):
    c = lc.lane_case(syn, wall, n, K, seed)
    assert c["ranges"].shape == (3, n) and c["obstacle"].shape == (2, K)
    ref, worst = loc_ref.stable(c["ranges"], c["obstacle"], AMIN, AMAX, c["pose0"], eps=eps)
    assert worst < 1e-10, worst
    assert (eps == 1e-11) == (K > 0)


def test_lane_cases_straddle_the_launch_rule():
    threads = {(n, K): lc.loc_step_threads(n, K) for n, K, _, _ in lc.LANE_CASES}
    assert threads == {(63, 64): 64, (64, 64): 64, (65, 64): 256, (63, 65): 256, (64, 65): 256, (65, 65): 256,
                       (8, 1): 64, (64, 0): 64}


ITER_COUNTS = {((0.3, 0.3, 0.1), 5): [5, 3, 2], ((0.3, 0.3, 0.1), 30): [8, 2, 2], ((1.5, -1.0, 0.6), 5): [5, 5, 5],
               ((1.5, -1.0, 0.6), 30): [30, 3, 3], ((0.0, 0.0, 2.0), 5): [5, 3, 2], ((0.0, 0.0, 2.0), 30): [9, 2, 20]}


@pytest.mark.parametrize("offset", lc.ITER_OFFSETS)
def test_iteration_cases(syn, wall, offset):
    """Every (offset, max_iter) is stable, so the GPU test compares them all; (1.5, -1.0, 0.6) ends on both caps."""
    c = lc.iter_case(syn, offset)
    for mi in lc.ITER_LIMITS:
        ref = assert_stable(c["ranges"], wall, c["pose0"], max_iter=mi)
        want = {0: [0, 0, 0], 1: [1, 1, 1]}.get(mi) or ITER_COUNTS[(tuple(offset), mi)]
        assert ref["iters_obs"].tolist() == want, (offset, mi)
        assert np.all(np.isfinite(ref["xest"]))
    ref = assert_stable(c["ranges"], wall, c["pose0"], tol=10.0)
    assert ref["iters_obs"].tolist() == [1, 1, 1]


def test_iteration_cases_reach_both_caps():
    assert ITER_COUNTS[((1.5, -1.0, 0.6), 30)][0] == 30 and ITER_COUNTS[((1.5, -1.0, 0.6), 5)] == [5, 5, 5]


def test_increment_case(syn, wall):
    c = lc.increment_case(syn)
    assert c["angle_increment"] != (AMAX - AMIN) / (c["n"] - 1) and c["n"] == 360
    ref = assert_stable(c["ranges"], wall, c["pose0"], angle_increment=c["angle_increment"])
    other = loc_ref.chain(c["ranges"], wall, AMIN, AMAX, c["pose0"])
    assert np.max(np.abs(ref["xest"] - other["xest"])) > 1e-4              # the increment is seen in the result


@pytest.mark.parametrize("n", [120, 361])
def test_option_streams_are_stable(syn, wall, n):
    r, p0 = lc.make_stream(syn, lc.OPTION_SEED, n, steps=3)
    assert_stable(r, wall, p0)


def test_batches_lie_past_the_shape_thresholds(syn, wall):
    """launch_icp turns to three queries per lane from 7 500 waves at two (for more than 192 points) and to one wave per
    pair from 4 x 4 096 pairs; the existing 257 hypotheses of 120 beams are below both."""
    assert lc.icp_waves_at_two(257, 120) < 7500
    r, p0, sot = lc.hypotheses_case(syn, **lc.SHAPE_A)
    assert r.shape == (2, 361) and p0.shape == (2600, 3) and lc.icp_waves_at_two(2600, 361) == 7800 >= 7500
    r, p0, sot = lc.hypotheses_case(syn, **lc.SHAPE_C)
    assert r.shape == (1, 200) and len(p0) == 16500 >= 4 * 4096 and lc.icp_waves_at_two(16500, 200) >= 7500 and 200 > 192
    assert len({tuple(q) for q in p0}) == 16500 and not sot.any()
    c = lc.many_streams_case(syn)
    S, n_scan, n = c["ranges"].shape
    assert (S, n_scan, n) == (2600, 2, 200) and lc.icp_waves_at_two(S * (2 * n_scan - 1), n) >= 7500 and n > 192
    assert sorted((c["sot"] % 4).tolist()) == [0, 1, 2, 3]                  # four different streams are routed to
    for l, s in enumerate(c["sot"]):
        assert np.array_equal(c["ranges"][s], c["alone"][l])
        assert all(not np.array_equal(c["alone"][l], c["alone"][k]) for k in range(l))


def test_bounds_cases(syn, wall):
    c = lc.max_hypotheses_case(syn, wall)
    assert c["pose0"].shape == (65535, 3) and c["ranges"].shape == (2, 8) and c["obstacle"].shape == (2, 16)
    assert len({tuple(q) for q in c["five"]}) == 5 and np.array_equal(c["pose0"][5:10], c["five"])
    c = lc.stream_index_case(syn)
    S, n_scan, n = c["ranges"].shape
    assert (S, n_scan, n) == (65537, 2, 16) and S * (2 * n_scan - 1) == 196611 > 1 << 16
    assert c["sot"].tolist() == [0, 32768, 65536]
    for l, s in enumerate(c["sot"]):
        assert np.array_equal(c["ranges"][s], c["alone"][l]) and not np.array_equal(c["alone"][l], c["filler"])
        # a pair number cut to 16 bits lands in another stream, whose scans differ
        assert s == 0 or not np.array_equal(c["ranges"][((int(s) * 3) & 0xFFFF) // 3], c["alone"][l])
    assert np.array_equal(c["ranges"][1], c["filler"]) and np.array_equal(c["ranges"][65535], c["filler"])


def test_workspace_case(syn):
    c = lc.workspace_case(syn)
    (rs, ps, zs), (rl, pl, zl) = c["small"], c["large"]
    assert rs.shape == (3, 64) and ps.shape == (2, 3) and rl.shape == (2, 361) and pl.shape == (600, 3)
    assert lc.loc_workspace_bytes(1, 2, 361, 600) >= 8 * (lc.loc_workspace_bytes(1, 3, 64, 2) + 8192)


def test_long_run_is_stable(syn, wall):
    r, p0 = lc.make_stream(syn, lc.LONG_SEED, 120, steps=lc.LONG_STEPS)
    ref, worst = loc_ref.stable(r, wall, AMIN, AMAX, p0, eps=lc.LONG_EPS)
    print("64 steps, eps %.0e: worst %.3e" % (lc.LONG_EPS, worst))
    assert worst < loc_ref.stable_bound(lc.LONG_EPS, lc.LONG_STEPS) and ref["xest"].shape == (64, 3)
