"""The landmark filter and the node around it - slam_ekf_lm, slam_ekf_lm_dev, slam_node_replay - over the seeded cases of
tests/filter_cases.py, against the package's host classes EKF and SLAM_EKF(landmarks=True) on the same numbers.

Statuses and the landmark count after every step are exact wherever the host class's decisions have a margin of 1e-6; x
and P lie within 1e-9 of the host class on the trajectories the sweep calls sure (tests/test_filter_cases.py holds the host
class within 1e-11 of the 50-digit answer on those, and caps the unsure ones at 2 %); a trajectory that was given a
non-finite row is compared by status, counts and NaN pattern.  Outside the live block x and P are exact zeros.  Every call
also runs with its batch reversed, with its first trajectory alone and at max_lm = 32 (another row stride of the state in
LDS): the same bits.  Every third seed runs the device form twice back to back without a synchronise in between.
tests/test_filter_cases.py asserts, without a device, which decisions these cases reach.  A failure names (kind, seed):
filter_cases.case_of(kind, seed) rebuilds the case."""
import time

import numpy as np
import pytest

import filter_cases as F
from conftest import pkg
from mcl_checks import same_bits
from test_gpu_map_properties import device_form, named, tag, up
from test_gpu_node_replay import assert_matches_host, host_node

pytestmark = pytest.mark.gpu
AMIN, AMAX = F.AMIN, F.AMAX
DEFAULT = 60                                # the seeds over which the node's stops are counted


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


@pytest.fixture(autouse=True)
def _clock(request):
    t = time.perf_counter()
    yield
    print("%s: %.1f s over %d seeds" % (request.node.name, time.perf_counter() - t, len(F.seeds())))


# ------------------------------------------------------------------ the filter
def ekf_host(slam, ctx, c, order=None, max_lm=None):
    """One slam_ekf_lm call over the case's trajectories ``order`` (default: all); dict of x, P, nlm, status."""
    abi = slam._abi
    p = F.packed(c, order)
    max_lm = c["max_lm"] if max_lm is None else max_lm
    B, N = p["B"], 3 + 2 * max_lm
    out = {"x": np.full((B, N), -9.0), "P": np.full((B, N, N), -9.0), "nlm": np.full((B, p["steps"]), -9, dtype=np.int32),
           "status": np.full(B, -9, dtype=np.int32)}
    abi.check(abi.lib().slam_ekf_lm(ctx.handle, abi.ptr(p["x0"]), abi.ptr(p["u"]), abi.ptr(p["counts"]), abi.ptr(p["z_off"]),
                                    abi.ptr(p["z"]) if len(p["z"]) else None, len(p["z"]), B, p["steps"], max_lm, abi.ptr(out["x"]),
                                    abi.ptr(out["P"]), abi.ptr(out["nlm"]), abi.ptr(out["status"])))
    return out


def ekf_dev(slam, ctx, c):
    """slam_ekf_lm_dev on torch tensors twice back to back; the outputs of both."""
    import torch
    abi = slam._abi
    p = F.packed(c)
    B, N = p["B"], 3 + 2 * c["max_lm"]
    dev = torch.device("cuda", ctx.device)
    x0, u, counts, off = (up(p[k], ctx) for k in ("x0", "u", "counts", "z_off"))
    z = up(p["z"], ctx) if len(p["z"]) else None
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    runs = [dict(x=torch.full((B, N), -9.0, **f64), P=torch.full((B, N, N), -9.0, **f64), nlm=torch.full((B, p["steps"]), -9, **i32),
                 status=torch.full((B,), -9, **i32)) for _ in range(2)]
    torch.cuda.synchronize()
    for o in runs:
        abi.check(abi.lib().slam_ekf_lm_dev(ctx.handle, abi.ptr(x0), abi.ptr(u), abi.ptr(counts), abi.ptr(off), abi.ptr(z), len(p["z"]), B,
                                            p["steps"], c["max_lm"], abi.ptr(o["x"]), abi.ptr(o["P"]), abi.ptr(o["nlm"]), abi.ptr(o["status"])))
    ctx.synchronize()
    return [{k: v.cpu().numpy() for k, v in o.items()} for o in runs]


def check_trajectory(c, b, out, r):
    """Row b of the call's outputs against the host class's answer ``r`` for that trajectory."""
    where = tag(c) + ("trajectory %d" % b, c["trajs"][b]["style"])
    x, P, n, done = out["x"][b], out["P"][b], len(r["x"]), len(r["nlm"])
    decided = r["margin"] >= F.SURE_MARGIN
    if decided:
        assert out["status"][b] == r["status"], where + ("status", int(out["status"][b]), r["status"])
        assert out["nlm"][b, :done].tolist() == r["nlm"] and np.all(out["nlm"][b, done:] == -1), where + ("counts", out["nlm"][b].tolist(), r["nlm"])
        assert np.all(x[n:] == 0) and np.all(P[n:] == 0) and np.all(P[:, n:] == 0), where + ("not zero outside the live block",)
    else:                                                                # what holds whatever was decided
        last = int(out["nlm"][b][out["nlm"][b] >= 0][-1]) if np.any(out["nlm"][b] >= 0) else 0
        m = 3 + 2 * last
        assert np.all(x[m:] == 0) and np.all(P[m:] == 0) and np.all(P[:, m:] == 0), where + ("not zero outside the live block",)
    if r["sure"]:
        dx, dP = np.max(np.abs(x[:n] - r["x"])), np.max(np.abs(P[:n, :n] - r["P"]))
        assert dx < 1e-9 and dP < 1e-9, where + ("x, P", float(dx), float(dP))
    elif decided and not r["finite"]:
        assert np.array_equal(np.isnan(x[:n]), np.isnan(r["x"])), where + ("NaN pattern of x",)
        assert np.array_equal(np.isnan(P[:n, :n]), np.isnan(r["P"])), where + ("NaN pattern of P",)


def test_ekf(slam, ctx):
    for seed in F.seeds():
        c = F.case_of("ekf", seed)
        with named(c):
            want = F.answer(c)
            got = ekf_host(slam, ctx, c)
            for b, r in enumerate(want):
                check_trajectory(c, b, got, r)
            # batch invariance: reversed (every trajectory in another workgroup), and the first trajectory alone
            B = c["B"]
            for name, order in (("reversed", list(range(B))[::-1]), ("alone", [0])):
                part = ekf_host(slam, ctx, c, order)
                steps = part["nlm"].shape[1]
                for k in ("x", "P", "status"):
                    assert same_bits(part[k], np.ascontiguousarray(got[k][order])), tag(c) + (name, k)
                assert np.array_equal(part["nlm"], got["nlm"][order][:, :steps]) and np.all(got["nlm"][order][:, steps:] == -1), tag(c) + (name, "nlm")
            # the same call at max_lm = 32: another row stride of the LDS state, the same live blocks
            if c["max_lm"] != 32:
                big = ekf_host(slam, ctx, c, max_lm=32)
                N = 3 + 2 * c["max_lm"]
                for b in range(B):
                    if got["status"][b] == F.LM_CAP:
                        continue                                         # it goes on where there is room
                    assert big["status"][b] == got["status"][b] and np.array_equal(big["nlm"][b], got["nlm"][b]), tag(c) + ("max_lm 32", b)
                    assert same_bits(np.ascontiguousarray(big["x"][b, :N]), got["x"][b]), tag(c) + ("max_lm 32", b, "x")
                    assert same_bits(np.ascontiguousarray(big["P"][b, :N, :N]), got["P"][b]), tag(c) + ("max_lm 32", b, "P")
                    assert np.all(big["x"][b, N:] == 0) and np.all(big["P"][b, N:] == 0) and np.all(big["P"][b, :, N:] == 0), tag(c) + ("max_lm 32", b)
            if device_form(c):
                for o in ekf_dev(slam, ctx, c):
                    for k in ("x", "P", "nlm", "status"):
                        assert same_bits(o[k], got[k]), tag(c) + ("device form", k)
    ctx.check_status()


GROUPS = 1 << 20                            # kLandmarkMaxGroups of slam_internal.h: more trajectories are taken grid-stride


def test_ekf_past_the_group_count(slam, ctx):
    """GROUPS + 5 trajectories of 3 steps at max_lm = 2, three different ones in turn (GROUPS % 3 == 1): the last five run
    second in their workgroup, each in the LDS another one left behind - one with two landmarks before one with none,
    one that raised before one that appends.  Every copy equals its own trajectory in a call of three, which the host
    class answers."""
    abi = slam._abi
    max_lm, steps, N = 2, 3, 7
    u = np.tile(np.array([0.25, 0.01, 0.2]), (3, steps, 1))
    x0 = np.array([[0.0, 0.0, 0.3], [1.0, -1.0, 2.9], [-1.0, 0.5, -1.0]])
    rows = [[[(3.0, 0.2)], [(3.1, 0.1), (4.0, 2.0)], [(3.0, -0.1), (4.1, 1.8)]],        # two landmarks, one a step
            [[], [], []],                                                              # none: P stays 3 x 3
            [[(2.0, 1.0)], [(5.0, -1.0), (5.01, -1.0)], [(2.0, 0.8)]]]                 # appends, then raises in step 1
    z = np.array([r for t in rows for s in t for r in s], dtype=np.float64)             # one period of the call's rows
    off = np.concatenate([[0], np.cumsum([len(s) for t in rows for s in t])]).astype(np.int64)

    def run(periods):
        B = 3 * periods
        zz = np.tile(z, (periods, 1))
        zo = np.concatenate([(off[:-1][None, :] + len(z) * np.arange(periods)[:, None]).reshape(-1), [len(zz)]]).astype(np.int64)
        out = {"x": np.empty((B, N)), "P": np.empty((B, N, N)), "nlm": np.empty((B, steps), dtype=np.int32), "status": np.empty(B, dtype=np.int32)}
        uu, xx, counts = np.tile(u, (periods, 1, 1)), np.tile(x0, (periods, 1)), np.full(B, steps, dtype=np.int32)
        abi.check(abi.lib().slam_ekf_lm(ctx.handle, abi.ptr(xx), abi.ptr(uu), abi.ptr(counts), abi.ptr(zo), abi.ptr(zz), len(zz), B, steps, max_lm,
                                        abi.ptr(out["x"]), abi.ptr(out["P"]), abi.ptr(out["nlm"]), abi.ptr(out["status"])))
        return out
    one = run(1)
    for b in range(3):
        r = F.host_run(u[b], [np.array(s, dtype=np.float64).reshape(-1, 2) for s in rows[b]], x0[b], max_lm)
        n, done = len(r["x"]), len(r["nlm"])
        assert one["status"][b] == r["status"] and one["nlm"][b].tolist() == r["nlm"] + [-1] * (steps - done), b
        assert np.max(np.abs(one["x"][b, :n] - r["x"])) < 1e-9 and np.max(np.abs(one["P"][b, :n, :n] - r["P"])) < 1e-9, b
    assert one["status"].tolist() == [0, 0, 1] and one["nlm"][:, -1].tolist() == [2, 0, -1]
    assert (GROUPS + 5) % 3 == 0 and GROUPS % 3 == 1
    many = run((GROUPS + 5) // 3)
    for k in ("x", "P", "nlm", "status"):
        assert np.array_equal(many[k].reshape((-1,) + one[k].shape), np.broadcast_to(one[k], (len(many[k]) // 3,) + one[k].shape)), k
    ctx.check_status()


# ------------------------------------------------------------------ the node
def node_map(c):
    """The host node's map geometry for the length of a block: `side` cells of 0.1 m, the reference's index rule."""
    import contextlib
    param = pkg("param")

    @contextlib.contextmanager
    def block():
        names = ("/slam/map_width", "/slam/map_height", "/slam/map_resolution")
        param.set_param(names[0], c["side"] * c["reso"])
        param.set_param(names[1], c["side"] * c["reso"])
        param.set_param(names[2], c["reso"])
        try:
            yield
        finally:
            for k in names:
                param._PARAMS.pop(k, None)
    return block()


def test_node(slam, ctx):
    stops = {F.OK: 0, F.RAISES: 0, F.LM_CAP: 0, F.OBS_CAP: 0}
    for seed in F.seeds():
        c = F.case_of("node", seed)
        with named(c):
            L, side = c["L"], c["side"]
            with node_map(c):
                refs = F.answer(c, lambda scans: host_node(slam, scans))
            grid = slam.DeviceGrid(L, side, side, 10.0, 10.0, 10.0)
            kw = dict(grid_of_traj=list(range(L)), max_lm=c["max_lm"], lm_cap=c["lm_cap"])
            out = slam.node_replay_host(c["ranges"], AMIN, AMAX, grid=grid, **kw)
            pmaps = [grid.read(l)["pmap"] for l in range(L)]
            for l, ref in enumerate(refs):
                assert_matches_host(out, l, ref, pmaps[l])
                if seed < DEFAULT:
                    stops[int(out["status"][l])] += 1
            grid.close()
            if device_form(c):
                rep = slam.DeviceNodeReplay(c["ranges"], AMIN, AMAX, **kw)
                rep.grid = slam.DeviceGrid(L, side, side, 10.0, 10.0, 10.0, context=rep.ctx)
                rep.run()
                rep.run()                                                # the second pass starts its maps from zero again
                dev = rep.results()
                for k in ("kept", "kept_count", "nlm", "status", "xest", "x", "P"):
                    assert np.array_equal(dev[k], out[k], equal_nan=True), tag(c) + ("device form", k)
                for l in range(L):
                    done = int(np.sum(out["nlm"][l] >= 0))               # (entries behind a trajectory's steps are void)
                    for k in ("T", "iters"):
                        assert np.array_equal(dev[k][l, :done], out[k][l, :done]), tag(c) + ("device form", k, l)
                    assert np.array_equal(rep.grid.read(l)["pmap"], pmaps[l]), tag(c) + ("device form", "map", l)
                rep.grid.close()
    print("node trajectories of the first %d seeds by status (ok, raises, max_lm, lm_cap): %s" % (DEFAULT, [stops[k] for k in sorted(stops)]))
    if len(F.seeds()) >= DEFAULT:                                        # the sweep reaches every stop
        assert stops[F.RAISES] >= 1 and stops[F.LM_CAP] >= 1 and stops[F.OBS_CAP] >= 1 and stops[F.OK] >= 1, stops
    ctx.check_status()
    slam._abi.default_context().check_status()
