"""The batched W9 node (``slam_loc_replay(_dev)``, ``k_loc_step``, ``k_loc_stream_pairs``) at its routes, stops, launch
shapes and bounds.  test_gpu_loc_replay.py has the node's parity; this file runs the paths that file leaves out, on the
inputs tests/loc_cases.py builds and tests/test_loc_cases.py has checked on the CPU.

Bars (DESIGN.md sections 2 and 12): iteration counts and statuses exact; ``xest``, ``xodom``, ``P``, ``T_obs``, ``T_odom``
within 1e-9 of ``loc_ref.chain`` (NumPy float64); every step's target points bit-equal to ``slam_virtual_scan`` +
``slam_scan_to_points_f64`` at the ``xEst`` the step started from; the same trajectory in another call bit-equal on every
key of ``KEYS``.  The worst deviation of every group is printed (``pytest -s``)."""
import numpy as np
import pytest

import loc_cases as lc
import loc_ref
import test_gpu_loc_replay as base
from conftest import load_golden, pkg
from loc_cases import AMAX, AMIN, GUARD, KEYS, make_stream, pick, same_bits

pytestmark = pytest.mark.gpu
OUTS = KEYS + ("tar_pts",)


@pytest.fixture(scope="module")
def slam():
    p = pkg()
    p._abi.default_context()
    return p


@pytest.fixture(scope="module")
def g5():
    return load_golden("g5_map_observation.npz")


@pytest.fixture(scope="module")
def wall(g5):
    return np.ascontiguousarray(g5["obs_wall"])


def against_chain(group, o, l, ref, steps=None):
    """Trajectory l of a result against the CPU chain over its first ``steps`` scans, at the bars; prints the worst."""
    steps = len(ref["iters_obs"]) if steps is None else steps
    assert o["iters_obs"][l, :steps].tolist() == ref["iters_obs"].tolist(), group
    worst = float(np.max(np.abs(o["P"][l] - ref["P"])))
    for k in ("xest", "xodom", "T_obs", "T_odom"):
        worst = max(worst, float(np.max(np.abs(o[k][l, :steps] - ref[k]))))
    print("%s: worst deviation from the chain %.3e" % (group, worst))
    assert worst < 1e-9, group
    return worst


def out_sizes(L, n_scan, n):
    f, i = np.float64, np.int32
    return {"xest": (L * n_scan * 3, f), "xodom": (L * n_scan * 3, f), "P": (L * 9, f), "status": (L, i),
            "T_obs": (L * n_scan * 9, f), "iters_obs": (L * n_scan, i), "T_odom": (L * n_scan * 9, f),
            "tar_pts": (L * n_scan * 2 * n, f)}


def raw_call(slam, ctx, form, a, want=OUTS):
    """``slam_loc_replay`` (form "host") or ``slam_loc_replay_dev`` ("dev", torch tensors for pointers) with the outputs in
    ``want`` and NULL for the others -> (return code, outputs, "the guard line behind every output is intact").  ``a``:
    ranges, S, n_scan, n, sot, ox, oy, off, M, K, mot, pose0, L, and optionally angle_min, inc, max_iter, tol; for "dev" an
    entry may already be a tensor (a view into a larger allocation)."""
    import torch
    A = slam._abi
    dev = form == "dev"
    L, n_scan, n = a["L"], a["n_scan"], a["n"]
    ct, st = A.trig_tables(AMIN, AMAX, max(n, 1))
    ins = dict(a, cos_t=ct, sin_t=st)
    for k in ("ranges", "sot", "ox", "oy", "off", "mot", "pose0", "cos_t", "sin_t"):
        v = ins.get(k)
        if v is not None and not hasattr(v, "data_ptr"):
            v = np.ascontiguousarray(v)
            v = torch.from_numpy(v).cuda() if dev else v
        ins[k] = v
    # a rejected call may name sizes no buffer could have: its outputs are cut to 1 MiB (nothing may be written anyway)
    sizes = {k: (min(max(c, 0) * np.dtype(t).itemsize, 1 << 20), t) for k, (c, t) in out_sizes(L, n_scan, n).items()}
    bufs = {}
    for k in want:
        nb = sizes[k][0] + 64
        bufs[k] = torch.full((nb,), GUARD, dtype=torch.uint8, device="cuda") if dev else np.full(nb, GUARD, dtype=np.uint8)
    p = lambda k: A.ptr(ins.get(k))
    args = [ctx.handle, p("ranges"), a["S"], n_scan, n, p("sot"), p("ox"), p("oy"), p("off"), a["M"]]
    if dev:
        args.append(a["K"])
    args += [p("mot"), p("pose0"), L, p("cos_t"), p("sin_t"), a.get("angle_min", AMIN),
             a.get("inc", (AMAX - AMIN) / (n - 1) if n > 1 else 1.0), a.get("max_iter", 30), a.get("tol", 0.001)]
    args += [A.ptr(bufs.get(k)) for k in OUTS]
    rc = (A.lib().slam_loc_replay_dev if dev else A.lib().slam_loc_replay)(*args)
    if dev:
        ctx.synchronize()
    raw = {k: (b.cpu().numpy() if dev else b) for k, b in bufs.items()}
    out = {k: raw[k][:sizes[k][0]].view(sizes[k][1]) for k in want}
    intact = all(np.all(raw[k][-64:] == GUARD) for k in want)
    if rc == A.SLAM_OK:
        out["xest"], out["xodom"] = out["xest"].reshape(L, n_scan, 3), out["xodom"].reshape(L, n_scan, 3)
        out["P"] = out["P"].reshape(L, 3, 3)
        for k in ("T_obs", "T_odom"):
            if k in out:
                out[k] = out[k].reshape(L, n_scan, 3, 3)
        if "iters_obs" in out:
            out["iters_obs"] = out["iters_obs"].reshape(L, n_scan)
        if "tar_pts" in out:
            out["tar_pts"] = out["tar_pts"].reshape(L, n_scan, 2, n)
    return rc, out, intact


def flat_maps(maps):
    cat = np.concatenate(maps, axis=1)
    off = np.zeros(len(maps) + 1, dtype=np.int64)
    off[1:] = np.cumsum([m.shape[1] for m in maps])
    return np.ascontiguousarray(cat[0]), np.ascontiguousarray(cat[1]), off


def rows_same_bits(a):
    b = np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)
    return bool(np.all(b == b[0]))


# ---- 1. random routing ----------------------------------------------------------------------------------------------

def test_random_routes(slam, syn, wall):
    c = lc.routing_case(syn, wall)
    n, L = c["n"], len(c["sot"])
    o = slam.loc_replay_host(c["ranges"], AMIN, AMAX, c["maps"], pose0=c["pose0"], stream_of_traj=c["sot"], map_of_traj=c["mot"],
                             target_points=True)
    assert o["status"].tolist() == [0] * L and np.all(np.isfinite(o["xest"]))
    for l in range(L):
        solo = slam.loc_replay_host(c["ranges"][c["sot"][l]], AMIN, AMAX, c["maps"][c["mot"][l]], pose0=c["pose0"][l:l + 1],
                                    target_points=True)
        assert same_bits(solo, pick(o, slice(l, l + 1))), l
        assert np.array_equal(solo["tar_pts"][0], o["tar_pts"][l]), l
    for l in lc.ROUTE_CHAIN:
        ref = loc_ref.chain(c["ranges"][c["sot"][l]], c["maps"][c["mot"][l]], AMIN, AMAX, c["pose0"][l])
        against_chain("routing, trajectory %d" % l, o, l, ref)
    base.check_targets(slam, o, c["maps"], c["mot"], c["pose0"], n)


# ---- 2. routes the kernel refuses -------------------------------------------------------------------------------------

def test_device_form_refuses_bad_routes_and_clamps_obs_off(slam, syn, wall):
    import torch
    c = lc.bad_route_case(syn, wall)
    S, M, K, n, P = c["S"], c["M"], c["K"], c["n"], lc.PAD_OBS
    ctx = slam.Context(0, torch.cuda.current_stream().cuda_stream)
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    rp, oxp, oyp = up(c["ranges_padded"]), up(c["ox_padded"]), up(c["oy_padded"])
    offp, wildp = up(c["off_padded"]), up(c["off_wild_padded"])
    a = {"ranges": rp[1:S + 1], "S": S, "n_scan": 3, "n": n, "sot": c["sot"], "ox": oxp[P:P + K], "oy": oyp[P:P + K],
         "off": offp[2:M + 3], "M": M, "K": K, "mot": c["mot"], "pose0": c["pose0"], "L": 6}
    rc, o, intact = raw_call(slam, ctx, "dev", a)
    assert rc == slam._abi.SLAM_OK and intact
    LOC = slam.loc_replay
    assert o["status"].tolist() == [LOC.LOC_OK] + [LOC.LOC_BAD_ROUTE] * 4 + [LOC.LOC_OK]
    for l in c["bad"]:
        for k in ("xest", "xodom", "T_obs", "T_odom"):
            assert np.all(np.isnan(o[k][l])), (l, k)
        assert o["iters_obs"][l].tolist() == [-1, -1, -1], l
        assert np.array_equal(o["P"][l], np.eye(3)), l
    for l in c["good"]:
        solo = slam.loc_replay_host(c["ranges"][c["sot"][l]], AMIN, AMAX, c["maps"][c["mot"][l]], pose0=c["pose0"][l:l + 1],
                                    target_points=True)
        assert same_bits(solo, pick(o, slice(l, l + 1))), l
        assert np.array_equal(solo["tar_pts"][0], o["tar_pts"][l]), l
    ctx.check_status()                                                # a refused route is a per-trajectory status, not an error
    # an obs_off whose first entry is negative and whose last lies past K: the bits of the clamped table
    good = dict(a, sot=np.array([0, 1, 0, 1, 0, 1], dtype=np.int32), mot=np.array([0, 1, 1, 0, 0, 1], dtype=np.int32))
    rc1, clamped, i1 = raw_call(slam, ctx, "dev", good)
    rc2, wild, i2 = raw_call(slam, ctx, "dev", dict(good, off=wildp[2:M + 3]))
    assert rc1 == rc2 == slam._abi.SLAM_OK and i1 and i2
    assert clamped["status"].tolist() == [0] * 6 and np.all(np.isfinite(clamped["xest"]))
    assert same_bits(wild, clamped, OUTS)
    assert same_bits(pick(clamped, slice(5, 6)), pick(o, slice(5, 6)))
    ctx.check_status()
    ctx.close()


# ---- 3. nullable outputs ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["dev", "host"])
def test_nullable_outputs(slam, syn, wall, form):
    import torch
    n = 64
    streams = [make_stream(syn, s, n, steps=3) for s in (2, 4)]
    ox, oy, off = flat_maps([wall, np.ascontiguousarray(wall[:, ::2])])
    a = {"ranges": np.stack([s[0] for s in streams]).astype(np.float32), "S": 2, "n_scan": 3, "n": n,
         "sot": np.array([1, 0, 1], dtype=np.int32), "ox": ox, "oy": oy, "off": off, "M": 2, "K": int(off[-1]),
         "mot": np.array([0, 1, 1], dtype=np.int32), "pose0": np.stack([streams[s][1] for s in (1, 0, 1)]), "L": 3}
    ctx = slam.Context(0, torch.cuda.current_stream().cuda_stream)
    rc, full, intact = raw_call(slam, ctx, form, a)
    assert rc == slam._abi.SLAM_OK and intact and full["status"].tolist() == [0, 0, 0]
    must = ("xest", "xodom", "P", "status")
    rc, lean, intact = raw_call(slam, ctx, form, a, want=must)
    assert rc == slam._abi.SLAM_OK and intact and sorted(lean) == sorted(must)
    assert same_bits(lean, full, must)
    for one in ("T_obs", "iters_obs", "T_odom", "tar_pts"):           # each nullable output alone
        rc, o, intact = raw_call(slam, ctx, form, a, want=must + (one,))
        assert rc == slam._abi.SLAM_OK and intact and same_bits(o, full, must + (one,)), one
    ctx.check_status()
    ctx.close()


# ---- 4. stops ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("value_a,value_b", lc.STOP_VALUES)
def test_stops_at_the_first_and_the_last_step(slam, syn, wall, value_a, value_b):
    c = lc.stop_case(syn, value_a, value_b)
    r, sot, p0 = c["ranges"], c["sot"], c["pose0"]
    LOC = slam.loc_replay
    o = slam.loc_replay_host(r, AMIN, AMAX, wall, pose0=p0, stream_of_traj=sot)
    want = {l: (LOC.LOC_NONFINITE if l in c["A"] + c["B"] else LOC.LOC_OK) for l in range(6)}
    assert o["status"].tolist() == [want[l] for l in range(6)]
    for l in c["A"]:                                                  # stopped at step 0: nothing was ever finite
        for k in ("xest", "xodom", "T_obs", "T_odom"):
            assert np.all(np.isnan(o[k][l])), (l, k)
        assert o["iters_obs"][l].tolist() == [-1] * 4 and np.array_equal(o["P"][l], np.eye(3)), l
    for l in c["B"]:                                                  # stopped at the last step
        ref = loc_ref.chain(r[1, :3], wall, AMIN, AMAX, p0[l])
        against_chain("stop at the last step, trajectory %d" % l, o, l, ref, steps=3)
        for k in ("xest", "xodom", "T_obs", "T_odom"):
            assert np.all(np.isnan(o[k][l, 3])) and np.all(np.isfinite(o[k][l, :3])), (l, k)
        assert o["iters_obs"][l, 3] == -1
    for l in c["C"]:
        solo = slam.loc_replay_host(r[2], AMIN, AMAX, wall, pose0=p0[l:l + 1])
        assert solo["status"].tolist() == [0] and same_bits(solo, pick(o, slice(l, l + 1))), l


# ---- 5. lane count of k_loc_step ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,K,seed,eps", lc.LANE_CASES)
def test_both_sides_of_the_64_lane_launch(slam, syn, wall, n, K, seed, eps):
    c = lc.lane_case(syn, wall, n, K, seed)
    o = slam.loc_replay_host(c["ranges"], AMIN, AMAX, c["obstacle"], pose0=c["pose0"], target_points=True)
    assert o["status"].tolist() == [0]
    against_chain("lanes n %d K %d (%d lanes)" % (n, K, lc.loc_step_threads(n, K)), o, 0,
                  loc_ref.chain(c["ranges"], c["obstacle"], AMIN, AMAX, c["pose0"]))
    base.check_targets(slam, o, [c["obstacle"]], [0], c["pose0"][None], n)


# ---- 6. iteration limits --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("offset", lc.ITER_OFFSETS)
def test_iteration_limits(slam, syn, wall, offset):
    """Every (offset, max_iter) below is stable on the CPU (test_loc_cases.py), so all are compared; offset
    (1.5, -1.0, 0.6) ends on the cap at 30 (counts [30, 3, 3]) and at 5 ([5, 5, 5])."""
    c = lc.iter_case(syn, offset)
    r, p0 = c["ranges"], c["pose0"]
    capped = set()
    for mi in lc.ITER_LIMITS:
        o = slam.loc_replay_host(r, AMIN, AMAX, wall, pose0=p0, max_iter=mi)
        ref = loc_ref.chain(r, wall, AMIN, AMAX, p0, max_iter=mi)
        assert o["status"].tolist() == [0]
        against_chain("max_iter %d from %s, counts %s" % (mi, offset, ref["iters_obs"].tolist()), o, 0, ref)
        assert o["iters_obs"].max() <= mi
        if mi and o["iters_obs"].max() == mi:
            capped.add(mi)
        if mi == 0:
            assert o["iters_obs"][0].tolist() == [0, 0, 0]
    assert {1} <= capped and (tuple(offset) != (1.5, -1.0, 0.6) or capped == {1, 5, 30})
    o = slam.loc_replay_host(r, AMIN, AMAX, wall, pose0=p0, tolerance=10.0)
    assert o["iters_obs"][0].tolist() == [1, 1, 1]
    against_chain("tolerance 10 from %s" % (offset,), o, 0, loc_ref.chain(r, wall, AMIN, AMAX, p0, tol=10.0))


# ---- 7. the caller's increment ----------------------------------------------------------------------------------------------

def test_callers_angle_increment(slam, syn, wall):
    c = lc.increment_case(syn)
    inc = c["angle_increment"]
    o = slam.loc_replay_host(c["ranges"], AMIN, AMAX, wall, pose0=c["pose0"], angle_increment=inc, target_points=True)
    assert o["status"].tolist() == [0]
    against_chain("increment 2 pi / 360", o, 0, loc_ref.chain(c["ranges"], wall, AMIN, AMAX, c["pose0"], angle_increment=inc))
    base.check_targets(slam, o, [wall], [0], c["pose0"][None], c["n"], angle_increment=inc)
    plain = slam.loc_replay_host(c["ranges"], AMIN, AMAX, wall, pose0=c["pose0"])
    assert np.max(np.abs(plain["xest"] - o["xest"])) > 1e-4          # the increment reached the kernel


# ---- 8. batch invariance past the second threshold of the shape rule ------------------------------------------------------

@pytest.mark.parametrize("shape,samples", [(lc.SHAPE_A, (0, 1300, 2599)), (lc.SHAPE_C, (0, 8191, 16499))],
                         ids=["2600x361", "16500x200"])
def test_many_hypotheses_in_the_per_step_launch(slam, syn, wall, shape, samples):
    """2 600 hypotheses of 361 beams are 7 800 waves at two queries per lane, over the 7 500 at which the automatic rule
    turns to three; 16 500 of 200 beams are past 4 x kWaveRound, where it would turn to one wave per pair."""
    r, p0, sot = lc.hypotheses_case(syn, **shape)
    assert lc.icp_waves_at_two(len(p0), r.shape[1]) >= 7500 and r.shape[1] > 192
    o = slam.loc_replay_host(r, AMIN, AMAX, wall, pose0=p0, stream_of_traj=sot)
    assert np.all(o["status"] == 0) and np.all(np.isfinite(o["xest"]))
    for l in samples:
        solo = slam.loc_replay_host(r, AMIN, AMAX, wall, pose0=p0[l:l + 1])
        assert same_bits(solo, pick(o, slice(l, l + 1))), l


def test_2600_streams_in_the_stream_only_launch(slam, syn, wall):
    c = lc.many_streams_case(syn)
    S, _, n = c["ranges"].shape
    assert lc.icp_waves_at_two(S * 3, n) >= 7500 and n > 192
    o = slam.loc_replay_host(c["ranges"], AMIN, AMAX, wall, pose0=c["pose0"], stream_of_traj=c["sot"])
    assert o["status"].tolist() == [0] * 4
    for l in range(4):
        solo = slam.loc_replay_host(c["alone"][l], AMIN, AMAX, wall, pose0=c["pose0"][l:l + 1])
        assert same_bits(solo, pick(o, slice(l, l + 1))), l


@pytest.fixture(scope="module")
def option_streams(syn, wall):
    out = {}
    for n in (120, 361):
        r, p0 = make_stream(syn, lc.OPTION_SEED, n, steps=3)
        out[n] = (r, p0, loc_ref.chain(r, wall, AMIN, AMAX, p0))
    return out


@pytest.mark.parametrize("n", [120, 361])
@pytest.mark.parametrize("option,value", lc.OPTION_CASES)
def test_explicit_shape_options_hold_for_every_batch(slam, wall, option_streams, option, value, n):
    ctx = slam.Context(0)
    ctx.set_option(option, value)
    r, p, ref = option_streams[n]
    o = slam.loc_replay_host(r, AMIN, AMAX, wall, pose0=p, context=ctx)
    assert o["status"].tolist() == [0]
    against_chain("%s = %d, n %d" % (option, value, n), o, 0, ref)
    L = 300
    p0 = lc.hypotheses(p, L, 23)
    sot = np.zeros(L, dtype=np.int32)
    many = slam.loc_replay_host(r, AMIN, AMAX, wall, pose0=p0, stream_of_traj=sot, context=ctx)
    assert np.all(many["status"] == 0)
    assert same_bits(o, pick(many, slice(0, 1)))                      # hypothesis 0 is the stream's own start pose
    for l in (150, 299):
        solo = slam.loc_replay_host(r, AMIN, AMAX, wall, pose0=p0[l:l + 1], context=ctx)
        assert same_bits(solo, pick(many, slice(l, l + 1))), l
    ctx.close()


# ---- 9. bounds ------------------------------------------------------------------------------------------------------------

def test_65535_hypotheses(slam, syn, wall):
    c = lc.max_hypotheses_case(syn, wall)
    r, obs, five = c["ranges"], c["obstacle"], c["five"]
    o = slam.loc_replay_host(r, AMIN, AMAX, obs, pose0=c["pose0"], stream_of_traj=c["sot"])
    assert o["status"].shape == (65535,)
    assert np.all(o["status"] == 0) and np.all(np.isfinite(o["xest"])) and np.all(o["iters_obs"] >= 1)
    for j in range(5):
        solo = slam.loc_replay_host(r, AMIN, AMAX, obs, pose0=five[j:j + 1])
        assert same_bits(solo, pick(o, slice(j, j + 1))), j
        for k in KEYS:
            assert rows_same_bits(o[k][j::5]), (j, k)
    assert not same_bits(pick(o, slice(0, 1)), pick(o, slice(1, 2)))


def test_65537_streams(slam, syn, wall):
    """The pair index of k_loc_stream_pairs past 16 bits: 196 611 pairs, the last stream's among them."""
    c = lc.stream_index_case(syn)
    o = slam.loc_replay_host(c["ranges"], AMIN, AMAX, wall, pose0=c["pose0"], stream_of_traj=c["sot"])
    assert o["status"].tolist() == [0, 0, 0]
    for l in range(3):
        solo = slam.loc_replay_host(c["alone"][l], AMIN, AMAX, wall, pose0=c["pose0"][l:l + 1])
        assert same_bits(solo, pick(o, slice(l, l + 1))), l
        other = slam.loc_replay_host(c["filler"], AMIN, AMAX, wall, pose0=c["pose0"][l:l + 1])
        assert not same_bits(other, pick(o, slice(l, l + 1))), l


def test_documented_bounds_are_rejected(slam, g5, wall):
    """Every rejection listed under "Bounds" in DESIGN.md section 12: SLAM_ERR_INVALID, a message that names the bound, no
    launch (the scan matcher's launch counter stays 0, the outputs keep their fill), and the context still works."""
    A = slam._abi
    ctx = slam.Context(0)
    ctx.timing_enable(True)
    ctx.timing_read()
    n = 16
    ox, oy, off = flat_maps([wall])
    good = {"ranges": np.ones((1, 2, n), dtype=np.float32), "S": 1, "n_scan": 2, "n": n, "sot": np.zeros(4, dtype=np.int32),
            "ox": ox, "oy": oy, "off": off, "M": 1, "K": int(off[-1]), "mot": np.zeros(4, dtype=np.int32),
            "pose0": np.zeros((4, 3)), "L": 4}
    cases = [({"L": 0}, "0 < L <= 65535"), ({"L": 65536}, "0 < L <= 65535"), ({"n": 0}, "1 <= n <= 4096"),
             ({"n_scan": 0}, "n_scan >= 1"), ({"S": 0}, "at least one stream"),
             ({"L": 32768, "n_scan": 65536}, "too many scans"),                       # L n_scan = 2^31
             ({"L": 1, "S": 32768, "n_scan": 32769}, "too many scans"),               # S (2 n_scan - 1) >= 2^31
             ({"max_iter": -1}, "max_iter"), ({"inc": 0.0}, "angles"), ({"inc": float("nan")}, "angles"),
             ({"inc": float("inf")}, "angles"), ({"angle_min": float("nan")}, "angles"), ({"ox": None}, "ox and oy")]
    per_form = {"dev": [({"M": 0}, "at least one stream and one map")],
                "host": [({"M": 0}, "M >= 1"), ({"M": 2, "off": np.array([0, 200, 100], dtype=np.int64)}, "ascend"),
                         ({"M": 2, "off": np.array([-3, 100, 364], dtype=np.int64)}, "ascend")]}
    for form in ("dev", "host"):
        for change, words in cases + per_form[form]:
            rc, out, intact = raw_call(slam, ctx, form, dict(good, **change))
            msg = (A.lib().slam_last_error() or b"").decode()
            assert rc == A.ERR_INVALID and words in msg, (form, change, rc, msg)
            assert intact and all(np.all(v.view(np.uint8) == GUARD) for v in out.values()), (form, change)
    assert all(count == 0 for _, count in ctx.timing_read().values())             # nothing was launched
    ctx.check_status()
    rc, o, intact = raw_call(slam, ctx, "dev", good)                               # the unchanged arguments do run,
    assert rc == A.SLAM_OK and intact
    assert sum(count for _, count in ctx.timing_read().values()) == 3              # and the counter sees their 3 launches
    ctx.timing_enable(False)
    r = g5["node9_ranges"][g5["node9_steps"]]
    o = slam.loc_replay_host(r, AMIN, AMAX, wall, context=ctx)
    assert o["status"].tolist() == [0] and np.max(np.abs(o["xest"][0] - g5["node9_xest"])) < 1e-9
    assert np.max(np.abs(o["P"][0] - g5["node9_P"])) < 1e-9
    ctx.close()


# ---- 10. workspace and state ------------------------------------------------------------------------------------------------

def test_workspace_grows_between_device_calls_and_run_twice(slam, syn, wall):
    import torch
    ctx = slam.Context(0, torch.cuda.current_stream().cuda_stream)
    c = lc.workspace_case(syn)
    (rs, ps, z2), (rl, pl, z600) = c["small"], c["large"]
    assert lc.loc_workspace_bytes(1, 2, 361, 600) >= 8 * (lc.loc_workspace_bytes(1, 3, 64, 2) + 8192)
    new = lambda r, p, z: slam.DeviceLocalizationReplay(r, AMIN, AMAX, wall, pose0=p, stream_of_traj=z, context=ctx)
    a, b, a2 = new(rs, ps, z2), new(rl, pl, z600), new(rs, ps, z2)
    a.run()
    b.run()                                                            # the arena grows here, with a's kernels enqueued
    a2.run()                                                           # no host synchronise between the three
    oa, ob, oa2 = a.results(), b.results(), a2.results()
    assert same_bits(oa, slam.loc_replay_host(rs, AMIN, AMAX, wall, pose0=ps, stream_of_traj=z2))
    assert same_bits(ob, slam.loc_replay_host(rl, AMIN, AMAX, wall, pose0=pl, stream_of_traj=z600))
    assert same_bits(oa, oa2) and np.all(oa["status"] == 0) and np.all(ob["status"] == 0)
    # run() again on one object: step 0 starts from pose0 and eye(3), not from the 16 doubles the last run left
    a.run()
    assert same_bits(a.results(), oa)
    b.run()
    b.run()
    assert same_bits(b.results(), ob)
    ctx.close()


# ---- 11. a long recurrence ----------------------------------------------------------------------------------------------------

def test_64_steps(slam, syn, wall):
    r, p = make_stream(syn, lc.LONG_SEED, 120, steps=lc.LONG_STEPS)
    ref = loc_ref.chain(r, wall, AMIN, AMAX, p)
    o = slam.loc_replay_host(r, AMIN, AMAX, wall, pose0=p)
    assert o["status"].tolist() == [0]
    against_chain("64 steps, L = 1", o, 0, ref)
    p0 = lc.hypotheses(p, 64, 27)
    p0[40] = p
    many = slam.loc_replay_host(r, AMIN, AMAX, wall, pose0=p0, stream_of_traj=np.zeros(64, dtype=np.int32))
    against_chain("64 steps, trajectory 40 of 64", many, 40, ref)
    assert same_bits(o, pick(many, slice(40, 41)))
