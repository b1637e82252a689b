"""slam_grid_refine on the GPU (include/slam_refine.h) against the 50-digit restatement (tests/refine_ref.py) on the seeded
cases of tests/refine_cases.py, and the batch rule: every hypothesis gets the same bits alone, in any batch, in any order,
under any chunking, from the host and the device form, with the field given or rebuilt.

The allowance is 16 E, E the NumPy restatement's own deviation from the 50-digit run (tests/refine_cases.py); a seed that
is not sure - some u or v within 1e-9 of an integer in the 50-digit run - is compared in its statuses only."""
import numpy as np
import pytest

import refine_cases as RC
import refine_ref as R
from conftest import pkg
from test_gpu_view import grid_of, up
from view_ref import counters_of

pytestmark = pytest.mark.gpu
KEYS = ("pose", "cost", "used", "status", "normal")


@pytest.fixture(scope="module")
def slam():
    p = pkg()
    p._abi.default_context()   # fails loudly when there is no gfx950 device
    return p


@pytest.fixture(scope="module")
def ctx(slam):
    c = slam.Context(0)
    yield c
    c.close()


_grids = {}


def setting(slam, ctx, seed):
    """(case, its DeviceGrid), made once per seed."""
    if seed not in _grids:
        case = RC.case_of("refine", seed)
        _grids[seed] = (case, grid_of(slam, ctx, case["pmaps"], case["scale"], case["off_x"], case["off_y"]))
    return _grids[seed]


def args_of(case, rows, over):
    a = dict({k: case[k] for k in RC.ARGS}, **over)
    r = case["ranges"] if case["ranges"].ndim == 1 else np.ascontiguousarray(case["ranges"][rows])
    return a, r, np.ascontiguousarray(case["poses"][rows]), np.ascontiguousarray(case["maps"][rows])


def host(slam, g, case, rows=slice(None), field=None, **over):
    a, r, p, m = args_of(case, rows, over)
    out = slam.grid_refine_host(g, r, p, case["ct"], case["st"], grid_of_batch=m, field=field, return_normal=True, **a)
    return dict(zip(KEYS, out))


def dev(g, ctx, case, rows=slice(None), field=None, **over):
    import torch
    a, r, p, m = args_of(case, rows, over)
    d = [up(r), up(p), up(case["ct"]), up(case["st"])]
    dm, df = up(m), None if field is None else up(field)
    torch.cuda.synchronize()
    out = g.refine(*d, grid_of_batch=dm, field=df, return_normal=True, **a)
    ctx.synchronize()
    return dict(zip(KEYS, (o.cpu().numpy() for o in out)))


def same_bits(a, b, what):
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k, a[k], b[k])


def pick(ans, rows):
    return {k: ans[k][rows] for k in KEYS}


def within(got, want, what):
    d = RC.deviation(got, want)
    print("%s: pose %.3g (allowed %.3g) cost %.3g (%.3g) normal %.3g (%.3g)" % (what, d[0], RC.ALLOW_POSE, d[1], RC.ALLOW_COST, d[2], RC.ALLOW_NORMAL))
    assert d[0] <= RC.ALLOW_POSE and d[1] <= RC.ALLOW_COST and d[2] <= RC.ALLOW_NORMAL, (what, d)


@pytest.mark.parametrize("seed", list(RC.seeds()))
def test_against_50_digits(slam, ctx, seed):
    """The host form on every seed, the device form on every third; statuses, used beams and the rows without an answer on
    all of them, the figures on the sure ones."""
    case, g = setting(slam, ctx, seed)
    want = RC.answer_mp(seed)
    got = [("host", host(slam, g, case))] + ([("device", dev(g, ctx, case))] if seed % 3 == 0 else [])
    for what, ans in got:
        assert ans["pose"].dtype == np.float64 and ans["status"].dtype == np.int32
        if RC.sure(want):
            within(ans, want, "seed %d %s" % (seed, what))
        else:
            assert np.array_equal(ans["status"], want["status"]) and np.array_equal(ans["used"], want["used"])
        bad = want["status"] != R.OK
        assert np.array_equal(ans["pose"][bad], case["poses"][bad], equal_nan=True) and np.all(ans["cost"][bad] == -1.0)
        assert not ans["normal"][bad].any() and not ans["used"][bad].any()
        flat = np.array([want["status"][b] == R.OK and not (case["pmaps"][case["maps"][b]] == 100).any() for b in range(len(bad))])
        assert ans["pose"][flat].tobytes() == case["poses"][flat].tobytes() and not ans["normal"][flat].any()    # g = 0: the pose must not move
    ctx.check_status()


@pytest.mark.parametrize("seed", list(RC.seeds()))
def test_batch_rule_bit_for_bit(slam, ctx, seed):
    case, g = setting(slam, ctx, seed)
    B = len(case["poses"])
    whole = host(slam, g, case)
    for b in range(B):
        same_bits(host(slam, g, case, rows=slice(b, b + 1)), pick(whole, slice(b, b + 1)), "alone %d" % b)
    rev = host(slam, g, case, rows=slice(None, None, -1))
    same_bits(pick(rev, slice(None, None, -1)), whole, "reversed")
    if B > 1:
        cut = (B + 1) // 2
        two = [host(slam, g, case, rows=slice(0, cut)), host(slam, g, case, rows=slice(cut, B))]
        same_bits({k: np.concatenate([t[k] for t in two]) for k in KEYS}, whole, "two chunks")
    same_bits(dev(g, ctx, case), whole, "device form")
    field = slam.grid_distance_field_host(g, case["cap"])
    assert np.array_equal(field, case["fields"])
    same_bits(host(slam, g, case, field=field), whole, "field given, host form")
    same_bits(dev(g, ctx, case, field=field), whole, "field given, device form")


@pytest.mark.parametrize("seed", [0, 4, 7, 13, 24])
def test_no_iterations(slam, ctx, seed):
    """iters = 0: one evaluation.  Both costs are the start's, the pose comes back bit for bit, and normal_out is what
    the first evaluation of any longer run starts from."""
    case, g = setting(slam, ctx, seed)
    got = host(slam, g, case, iters=0)
    ok = got["status"] == R.OK
    assert np.array_equal(got["cost"][:, 0], got["cost"][:, 1])
    assert got["pose"].tobytes() == case["poses"].tobytes()
    want = RC.answer(case, R.refine_mp, iters=0)
    if RC.sure(want):
        within(got, want, "seed %d, no iterations" % seed)
    longer = host(slam, g, case, iters=3)
    assert np.array_equal(longer["cost"][:, 0], got["cost"][:, 0]) and np.array_equal(longer["used"], got["used"])
    assert ok.any() or seed != 0


# ------------------------------------------------------------------ Mapping.refine_scan and match_scan(refine=)
AMIN, AMAX, NB = -3.14159, 3.14159, 90


def mapping_of(slam, ctx, pmap, scale, off_x, off_y):
    import torch
    m = slam.Mapping(pmap.shape[0], pmap.shape[1], 1.0 / scale, index_scale=scale, index_offset=off_x, index_offset_y=off_y, context=ctx)
    ctx.synchronize()
    p, h = m.grid.counters_torch()
    cnt = counters_of(pmap)
    p.copy_(up(cnt[0][None]))
    h.copy_(up(cnt[1][None]))
    torch.cuda.synchronize()
    assert np.array_equal(m.grid.read(0)["pmap"], pmap.astype(np.int8))
    return m


@pytest.fixture(scope="module")
def walls(slam, ctx):
    """A 64 x 64 room at 0.1 m with walls of occupied cells, a scan of 90 beams taken at its middle by exact ray-wall
    distances, and its Mapping."""
    pm = np.full((64, 64), 0, dtype=np.int8)
    pm[[4, 59], 4:60] = 100
    pm[4:60, [4, 52]] = 100
    scale, off = 10.0, 3.2
    true = np.array([0.13, -0.21, 0.3])
    ct, st = slam._abi.trig_tables(AMIN, AMAX, NB)
    ang = np.linspace(AMIN, AMAX, NB) + true[2]
    x0, x1, y0, y1 = 0.45 - off, 5.95 - off, 0.45 - off, 5.25 - off                 # the middles of the wall cells
    with np.errstate(divide="ignore"):
        tx = np.where(np.cos(ang) > 0, (x1 - true[0]) / np.cos(ang), (x0 - true[0]) / np.cos(ang))
        ty = np.where(np.sin(ang) > 0, (y1 - true[1]) / np.sin(ang), (y0 - true[1]) / np.sin(ang))
    scan = np.minimum(tx, ty).astype(np.float32)
    return dict(m=mapping_of(slam, ctx, pm, scale, off, off), field=R_field(pm), scale=scale, off=off, true=true, scan=scan, ct=ct, st=st)


def R_field(pm):
    import match_ref as MR
    return MR.field(pm, 64)


def test_refine_scan_keeps_the_start_when_the_end_costs_more(slam, ctx, walls):
    """The device rule has no decisions; Mapping.refine_scan adds the host's: the start when the end costs more.  On the
    clean room ten default steps never end above the start, so the rising case is made on purpose: three beams, no
    damping, one step of up to 30 cells and 1 rad (found by a search over random three-beam scans on the restatement, which
    says 79.8 -> 128.2 and is asked first)."""
    w, m = walls, walls["m"]
    far = np.array([0.36511274, -0.96985004, 2.53635412])
    scan3 = np.array([2.8475378, 1.2704368, 2.4189746], dtype=np.float32)
    ct3, st3 = slam._abi.trig_tables(AMIN, AMAX, 3)
    kw = dict(iters=1, damping=0.0, max_step=(30.0, 1.0))
    raw_kw = dict(iters=1, damping=0.0, step_cells=30.0, step_rad=1.0)
    ref = R.refine(w["field"], w["scale"], w["off"], w["off"], scan3, far, ct3, st3, 1, 0.0, 30.0, 1.0, 30.0, 64)
    print("the restatement's costs at the start and after one free step:", ref["cost"])
    assert ref["cost"][1] > 1.5 * ref["cost"][0]
    raw = slam.grid_refine_host(m.grid, scan3, far, ct3, st3, **raw_kw)
    assert raw[1][0, 1] > raw[1][0, 0] and raw[0][0].tobytes() != far.tobytes()          # the call itself does not choose
    pose, cost, used, H, g = m.refine_scan(scan3, AMIN, AMAX, far, return_normal=True, **kw)
    assert pose.tobytes() == far.tobytes() and cost == raw[1][0, 0] and used == raw[2][0] == 3
    zero = slam.grid_refine_host(m.grid, scan3, far, ct3, st3, iters=0, return_normal=True)
    H0, g0 = slam.refine_normal(zero[4][0])
    assert np.array_equal(H, H0) and np.array_equal(g, g0) and np.array_equal(H, H.T) and H.any()
    pose, cost, used = m.refine_scan(scan3, AMIN, AMAX, far, **kw)
    assert pose.tobytes() == far.tobytes() and cost == raw[1][0, 0] and used == 3
    near = w["true"] + np.array([0.08, -0.06, 0.008])
    pose, cost, used = m.refine_scan(w["scan"], AMIN, AMAX, near)
    end = slam.grid_refine_host(m.grid, w["scan"], near, w["ct"], w["st"])
    assert end[1][0, 1] <= end[1][0, 0] and pose.tobytes() == end[0][0].tobytes() and cost == end[1][0, 1]
    assert abs(pose[2] - w["true"][2]) < abs(near[2] - w["true"][2])


def test_match_scan_with_refine(slam, ctx, walls):
    w, m = walls, walls["m"]
    start = w["true"] + np.array([0.17, -0.12, 0.02])
    plain = m.match_scan(w["scan"], AMIN, AMAX, start, return_costs=True)
    zero = m.match_scan(w["scan"], AMIN, AMAX, start, return_costs=True, refine=0)
    assert len(plain) == len(zero) == 4
    for a, b in zip(plain, zero):
        assert type(a) is type(b) and np.array_equal(a, b)
    five = m.match_scan(w["scan"], AMIN, AMAX, start, refine=5)
    then = m.refine_scan(w["scan"], AMIN, AMAX, plain[0], iters=5)
    assert five[0].tobytes() == then[0].tobytes() and five[1] == then[1] and five[2] == then[2] == plain[2]
    assert five[0].tobytes() != plain[0].tobytes()
    vol = m.match_scan(w["scan"], AMIN, AMAX, start, refine=5, return_costs=True)
    assert np.array_equal(vol[3], plain[3]) and vol[0].tobytes() == five[0].tobytes()
