"""slam_mcl_weigh / slam_mcl_resample refuse every argument set outside their stated bounds with SLAM_ERR_INVALID and a
message, before anything is enqueued: each refusal is followed by a good call on the same context that still gives the
restatement's answer."""
import ctypes as C

import numpy as np
import pytest

import match_ref as M
import mcl_ref as X
import raycast_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    slam = pkg()
    ctx = slam.Context(0)
    g = slam.DeviceGrid(1, 64, 64, 1.0, 0.0, 0.0, context=ctx)
    for ox, oy, cx, cy in R.ring_updates():
        g.update_host(ox, oy, cx, cy)
    yield slam, ctx, g, M.field(g.read()["pmap"], 64)[None]
    ctx.close()


F, P, N = 2, 40, 24
K = X.ring_case(F, P, N, 61)


def weigh_args(ctx, g, **kw):
    """The 18 arguments of slam_mcl_weigh on host arrays (kept alive by the returned list), with overrides."""
    abi = pkg("_abi")
    a = dict(poses=K["poses"].copy(), motion=K["motion"].copy(), noise=K["noise"].copy(), ranges=K["ranges"].copy(), cos_t=K["cos_t"].copy(),
             sin_t=K["sin_t"].copy(), gof=np.zeros(F, np.int32), F=F, P=P, n=N, max_range=19.0, cap=64, field=None,
             acc=np.zeros((F, P), np.int32), cost=np.empty((F, P), np.int32), used=np.empty(F, np.int32), grid=g._h)
    a.update(kw)
    p = lambda k: abi.ptr(a[k]) if a[k] is not None else None
    return a, [ctx.handle, a["grid"], p("poses"), p("motion"), p("noise"), p("ranges"), p("cos_t"), p("sin_t"), p("gof"), a["F"], a["P"],
               a["n"], C.c_float(a["max_range"]), a["cap"], p("field"), p("acc"), p("cost"), p("used")]


def resample_args(ctx, **kw):
    abi = pkg("_abi")
    rng = np.random.default_rng(62)
    a = dict(poses=K["poses"].copy(), acc=rng.integers(0, 30, (F, P)).astype(np.int32), table=X.weight_table(2.0, 0, 64), T=64, shift=0,
             u0=np.array([0.25, 0.75]), ess_frac=float("inf"), F=F, P=P, out=np.empty((F, P, 3)), anc=np.empty((F, P), np.int32),
             est=np.empty((F, 4)), info=np.empty((F, 4), np.int32))
    a.update(kw)
    p = lambda k: abi.ptr(a[k]) if a[k] is not None else None
    return a, [ctx.handle, p("poses"), p("acc"), p("table"), a["T"], a["shift"], p("u0"), C.c_double(a["ess_frac"]), a["F"], a["P"],
               p("out"), p("anc"), p("est"), p("info")]


def good_weigh(slam, ctx, g, fld, fn):
    abi = pkg("_abi")
    a, args = weigh_args(ctx, g)
    assert getattr(abi.lib(), fn)(*args) == abi.SLAM_OK
    assert np.allclose(a["poses"], X.move(K["poses"], K["motion"], K["noise"]), rtol=0, atol=1e-9)
    ref = X.weigh(fld, 1.0, 0.0, 0.0, a["poses"], K["ranges"], K["cos_t"], K["sin_t"], 19.0, 64, acc=np.zeros((F, P), np.int32))
    assert np.mean(a["cost"] != ref["cost"]) <= 0.02 and np.array_equal(a["used"], ref["used"]) and np.array_equal(a["acc"], a["cost"])


def good_resample(slam, ctx):
    abi = pkg("_abi")
    a, args = resample_args(ctx)
    before = a["acc"].copy()
    assert abi.lib().slam_mcl_resample(*args) == abi.SLAM_OK
    ref = X.resample(a["poses"], before, a["table"], 0, a["u0"], np.inf)
    assert np.array_equal(a["anc"], ref["ancestors"]) and np.array_equal(a["info"], ref["info"]) and np.all(a["acc"] == 0)
    assert a["out"].tobytes() == ref["poses"].tobytes() and np.allclose(a["est"], ref["est"], rtol=0, atol=1e-9)


WEIGH_BAD = [
    (dict(F=0), "F < 1"), (dict(F=-1), "F < 1"), (dict(P=0), "P outside"), (dict(P=(1 << 20) + 1), "P outside"),
    (dict(F=2048, P=1 << 20), "F \\* P >= 2\\^31"), (dict(n=0), "n outside"), (dict(n=4097), "n outside"),
    (dict(F=1 << 20, P=1, n=2048), "F \\* n >= 2\\^31"), (dict(cap=0), "cap outside"), (dict(cap=32768), "cap outside"),
    (dict(max_range=0.0), "max_range"), (dict(max_range=-1.0), "max_range"), (dict(max_range=float("nan")), "max_range"),
    (dict(motion=None), "noise without motion"), (dict(poses=None), "null pointer"), (dict(ranges=None), "null pointer"),
    (dict(cos_t=None), "null pointer"), (dict(sin_t=None), "null pointer"), (dict(grid=None), "null pointer"),
]

RESAMPLE_BAD = [
    (dict(F=0), "F < 1"), (dict(P=0), "P outside"), (dict(P=(1 << 20) + 1), "P outside"), (dict(F=2048, P=1 << 20), "F \\* P >= 2\\^31"),
    (dict(T=0), "T outside"), (dict(T=65537), "T outside"), (dict(shift=-1), "shift outside"), (dict(shift=31), "shift outside"),
    (dict(ess_frac=-0.5), "ess_frac"), (dict(ess_frac=float("nan")), "ess_frac"), (dict(poses=None), "null pointer"),
    (dict(acc=None), "null pointer"), (dict(table=None), "null pointer"), (dict(u0=None), "null pointer"), (dict(out=None), "null pointer"),
    (dict(est=None), "null pointer"), (dict(info=None), "null pointer"),
]


@pytest.mark.parametrize("fn", ["slam_mcl_weigh", "slam_mcl_weigh_dev"])
def test_weigh_rejects(env, fn):
    import re
    slam, ctx, g, fld = env
    abi = pkg("_abi")
    L = abi.lib()
    for kw, msg in WEIGH_BAD:
        a, args = weigh_args(ctx, g, **kw)
        before = {k: a[k].copy() for k in ("poses", "acc") if a[k] is not None}
        assert getattr(L, fn)(*args) == abi.ERR_INVALID, kw           # (the _dev form is refused before it touches a pointer)
        err = L.slam_last_error().decode()
        assert err.startswith(fn + ":") and re.search(msg, err), (kw, err)
        for k, v in before.items():
            assert np.array_equal(a[k], v)
        good_weigh(slam, ctx, g, fld, "slam_mcl_weigh")
    assert L.slam_mcl_weigh(None, *weigh_args(ctx, g)[1][1:]) == abi.ERR_INVALID
    ctx.check_status()


@pytest.mark.parametrize("fn", ["slam_mcl_resample", "slam_mcl_resample_dev"])
def test_resample_rejects(env, fn):
    import re
    slam, ctx, g, fld = env
    abi = pkg("_abi")
    L = abi.lib()
    for kw, msg in RESAMPLE_BAD:
        a, args = resample_args(ctx, **kw)
        acc = None if a["acc"] is None else a["acc"].copy()
        assert getattr(L, fn)(*args) == abi.ERR_INVALID, kw
        err = L.slam_last_error().decode()
        assert err.startswith(fn + ":") and re.search(msg, err), (kw, err)
        assert acc is None or np.array_equal(a["acc"], acc)
        good_resample(slam, ctx)
    a, args = resample_args(ctx)
    args[10] = args[1]                                                 # poses_out == poses
    assert getattr(L, fn)(*args) == abi.ERR_INVALID and "poses_out must not be poses" in L.slam_last_error().decode()
    good_resample(slam, ctx)
    ctx.check_status()


def test_host_forms_reject_u0_and_table(env):
    slam, ctx, g, fld = env
    abi = pkg("_abi")
    L = abi.lib()
    for kw, msg in ((dict(u0=np.array([0.25, 1.0])), "u0 outside"), (dict(u0=np.array([-1e-9, 0.5])), "u0 outside"),
                    (dict(u0=np.array([0.25, np.nan])), "u0 outside"), (dict(table=np.full(64, (1 << 20) + 1, np.uint32)), "table entry above")):
        a, args = resample_args(ctx, **kw)
        assert L.slam_mcl_resample(*args) == abi.ERR_INVALID and msg in L.slam_last_error().decode(), kw
        good_resample(slam, ctx)
    a, args = resample_args(ctx, table=np.full(64, 1 << 20, np.uint32), u0=np.array([0.0, float(np.nextafter(1.0, 0.0))]))
    assert L.slam_mcl_resample(*args) == abi.SLAM_OK and np.array_equal(a["anc"], np.tile(np.arange(P, dtype=np.int32), (F, 1)))
