"""slam_grid_refine at the sizes where its launch changes: beam counts around one wave of lanes and at the bound, batches
around one workgroup of four waves, more than one wave of workgroups, and a batch past the launch cap, which the kernel
takes grid-stride; every invalid argument; and the two signatures of include/slam_refine.h."""
import ctypes as C

import numpy as np
import pytest

import match_ref as MR
import refine_cases as RC
import refine_ref as R
from conftest import pkg
from test_gpu_view import grid_of, up

KEYS = ("pose", "cost", "used", "status", "normal")
ARGS = dict(iters=3, damping=1e-3, step_cells=0.5, step_rad=0.02, max_range=30.0, cap=16)


def test_signatures_of_the_second_header():
    """Exactly the two names, bound beside the 95 of include/slam_hip.h, and the widths at damping, step_cells, step_rad
    (double) and max_range (float): a slip there shifts every later argument."""
    abi = pkg("_abi")
    assert sorted(abi._SIGS_REFINE) == ["slam_grid_refine", "slam_grid_refine_dev"]
    assert not set(abi._SIGS_REFINE) & set(abi._SIGS) and len(abi._SIGS) == 95
    vp = C.c_void_p
    want = [vp, vp, vp, C.c_int, vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_float, C.c_int,
            vp, vp, vp, vp, vp, vp]
    for name in abi._SIGS_REFINE:
        args, res = abi._SIGS_REFINE[name]
        assert args == want and res is C.c_int, name
    assert abi.header_symbols(abi.REFINE_HEADER_PATH) == sorted(abi._SIGS_REFINE)


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


def small_map():
    pm = np.full((8, 8), 0, dtype=np.int8)
    pm[1, 1:7] = pm[6, 2:6] = pm[2:5, 6] = 100
    return pm


@pytest.fixture(scope="module")
def small(slam, ctx):
    pm = small_map()
    return dict(g=grid_of(slam, ctx, [pm]), field=MR.field(pm, ARGS["cap"])[None], pm=pm)


def scan_of(n, seed):
    rng = np.random.default_rng(seed)
    th = -np.pi + np.arange(n) * (2.0 * np.pi / n)
    r = rng.uniform(0.5, 6.0, n).astype(np.float32)
    if n > 8:
        r[rng.integers(0, n, size=n // 8)] = np.inf
    return r, np.cos(th), np.sin(th)


def plan(slam, name, a=0):
    out = C.c_int64(0)
    slam._abi.check(slam._abi.lib().slam_plan_query(name.encode(), int(a), 0, 0, -1, C.byref(out)))
    return int(out.value)


def refine_host(slam, g, r, poses, ct, st, **over):
    out = slam.grid_refine_host(g, r, poses, ct, st, return_normal=True, **dict(ARGS, **over))
    return dict(zip(KEYS, out))


def mp_of(field, r, poses, ct, st, **over):
    """The 50-digit answer, with the NumPy restatement's own deviation from it on this very case under "E"."""
    a = dict(ARGS, **over)
    rest = (field, 1.0, 0.0, 0.0, r, poses, ct, st, a["iters"], a["damping"], a["step_cells"], a["step_rad"], a["max_range"], a["cap"])
    want = R.batch(R.refine_mp, *rest)
    want["E"] = RC.deviation(R.batch(R.refine, *rest), want)
    return want


def within(got, want, what):
    """The rule of tests/refine_cases.py for a case outside its sweep: 16 times the NumPy restatement's deviation from the
    50-digit run - on the default cases or on this case, whichever is larger, since a case of few beams can be worse
    conditioned than any of those (one beam: H has rank 1 and only the damping holds A up) - and 1e-9 at most for poses."""
    allow = (min(16 * max(RC.E_POSE, want["E"][0]), 1e-9), 16 * max(RC.E_COST, want["E"][1]), 16 * max(RC.E_NORMAL, want["E"][2]))
    d = RC.deviation(got, want)
    print("%s: pose %.3g (allowed %.3g) cost %.3g (%.3g) normal %.3g (%.3g)" % (what, d[0], allow[0], d[1], allow[1], d[2], allow[2]))
    assert d[0] <= allow[0] and d[1] <= allow[1] and d[2] <= allow[2], (what, d, allow)


POSES = np.array([[3.3, 3.6, 0.2], [4.7, 2.2, -1.1], [2.4, 4.4, 2.9], [5.2, 4.9, 0.7], [3.9, 3.1, -2.5]])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4096])
def test_beam_counts(slam, ctx, small, n):
    """One lane with a beam; one lane short of a wave; a full wave; one beam in a second round; the bound (64 rounds).  Two
    hypotheses against the 50-digit run (at n = 4096 with one iteration: the 50-digit run takes a second per 10 000 beam
    evaluations)."""
    r, ct, st = scan_of(n, 11 + n)
    over = dict(iters=1) if n == 4096 else {}
    want = mp_of(small["field"], r, POSES[:2], ct, st, **over)
    assert RC.sure(want) and want["used"][0] >= (n > 1)
    got = refine_host(slam, small["g"], r, POSES[:2], ct, st, **over)
    within(got, want, "n = %d" % n)
    ctx.check_status()


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3, 4, 5, 1025])
def test_batch_sizes(slam, ctx, small, B):
    """A partial workgroup, a full one, one hypothesis in a second, and more workgroups than one wave of them: five distinct
    hypotheses (checked against the 50-digit run) repeated to B rows, every copy bit-equal to its original; a scan each."""
    rs = [scan_of(65, 40 + k) for k in range(5)]
    ct, st = rs[0][1], rs[0][2]
    base_r = np.stack([x[0] for x in rs])
    five = refine_host(slam, small["g"], base_r, POSES, ct, st)
    within(five, mp_of(small["field"], base_r, POSES, ct, st), "the five")
    idx = np.arange(B) % 5
    got = refine_host(slam, small["g"], np.ascontiguousarray(base_r[idx]), np.ascontiguousarray(POSES[idx]), ct, st)
    for k in KEYS:
        assert got[k].tobytes() == np.ascontiguousarray(five[k][idx]).tobytes(), k
    assert plan(slam, "refine", B) == (B + 3) // 4 == plan(slam, "refine_blocks", B)
    ctx.check_status()


@pytest.mark.gpu
def test_batch_past_the_launch_cap(slam, ctx, small):
    """More hypotheses than one sweep of the largest launch takes: the rest go grid-stride.  n = 1, a shared scan."""
    cap = plan(slam, "refine_cap")
    assert cap == plan(slam, "kRefineMaxBlocks") * plan(slam, "kRefineWaves") and plan(slam, "kRefineThreads") == 64 * plan(slam, "kRefineWaves")
    B = cap + 5
    assert plan(slam, "refine", B) == plan(slam, "kRefineMaxBlocks") < plan(slam, "refine_blocks", B) and plan(slam, "refine_pass", B) == cap
    r, ct, st = np.array([2.5], dtype=np.float32), np.array([1.0]), np.array([0.0])
    five = refine_host(slam, small["g"], r, POSES, ct, st)
    within(five, mp_of(small["field"], r, POSES, ct, st), "the five, one beam")
    idx = np.arange(B) % 5
    got = refine_host(slam, small["g"], r, np.ascontiguousarray(POSES[idx]), ct, st)
    for k in KEYS:
        assert got[k].tobytes() == np.ascontiguousarray(five[k][idx]).tobytes(), k
    ctx.check_status()


BAD = [("n", 0), ("n", 4097), ("B", 0), ("B", -1), ("iters", -1), ("iters", 65), ("damping", -1e-3), ("damping", float("nan")),
       ("damping", float("inf")), ("step_cells", 0.0), ("step_cells", float("nan")), ("step_rad", 0.0), ("step_rad", -0.1),
       ("step_rad", float("nan")), ("cap", 0), ("cap", 32768), ("max_range", 0.0), ("max_range", float("nan")), ("ranges", None),
       ("poses", None), ("cos_t", None), ("sin_t", None), ("pose_out", None), ("cost_out", None), ("status_out", None), ("grid", None),
       ("B*n", None)]


@pytest.mark.gpu
@pytest.mark.parametrize("what,value", BAD, ids=["%s=%s" % (k, v) for k, v in BAD])
def test_invalid_arguments_enqueue_nothing(slam, ctx, small, what, value):
    """SLAM_ERR_INVALID from both forms, the outputs untouched after a synchronise, the sticky status clean, and the next
    valid call answers as before."""
    import torch
    abi = slam._abi
    r, ct, st = scan_of(65, 3)
    a = dict(ARGS, n=65, B=2, grid=small["g"]._h)
    h = dict(ranges=r, poses=np.ascontiguousarray(POSES[:2]), cos_t=ct, sin_t=st, pose_out=np.full((2, 3), 77.0), cost_out=np.full((2, 2), 77.0),
             used_out=np.full(2, 77, dtype=np.int32), normal_out=np.full((2, 9), 77.0), status_out=np.full(2, 77, dtype=np.int32))
    d = {k: up(v) for k, v in h.items()}
    torch.cuda.synchronize()
    if what == "B*n":
        a.update(B=(1 << 31) // 4096, n=4096)               # B * n = 2^31: rejected before anything is read
    elif what in h:
        h[what] = d[what] = None
    else:
        a[what] = value
    for fn, arr in ((abi.lib().slam_grid_refine, h), (abi.lib().slam_grid_refine_dev, d)):
        rc = fn(ctx.handle, a["grid"], abi.ptr(arr["ranges"]), 0, abi.ptr(arr["poses"]), a["B"], None, abi.ptr(arr["cos_t"]), abi.ptr(arr["sin_t"]),
                a["n"], a["iters"], a["damping"], a["step_cells"], a["step_rad"], a["max_range"], a["cap"], None, abi.ptr(arr["pose_out"]),
                abi.ptr(arr["cost_out"]), abi.ptr(arr["used_out"]), abi.ptr(arr["normal_out"]), abi.ptr(arr["status_out"]))
        assert rc == abi.ERR_INVALID, (fn, rc)
        assert b"slam_grid_refine" in abi.lib().slam_last_error()
    ctx.synchronize()
    ctx.check_status()
    for k in ("pose_out", "cost_out", "used_out", "normal_out", "status_out"):
        if h[k] is not None:
            assert np.all(h[k] == 77) and bool((d[k] == 77).all()), k
    got = refine_host(slam, small["g"], r[None].repeat(2, axis=0), POSES[:2], ct, st)
    assert np.array_equal(got["status"], [0, 0]) and np.all(got["cost"][:, 1] <= got["cost"][:, 0])


@pytest.mark.gpu
def test_infinite_limits_are_valid(slam, ctx, small):
    """max_range = +inf uses every finite range; step_cells = step_rad = +inf clamp nothing: the restatement's answer."""
    r, ct, st = scan_of(65, 5)
    over = dict(max_range=float("inf"), step_cells=float("inf"), step_rad=float("inf"), damping=0.1)
    want = mp_of(small["field"], r, POSES[:3], ct, st, **over)
    assert want["used"][0] == int(np.isfinite(r).sum()) and RC.sure(want)
    within(refine_host(slam, small["g"], r, POSES[:3], ct, st, **over), want, "no clamp")
