"""The operators built on the map - distance field, window matcher, global localisation, frontiers, the two weighs,
resampling, settle and the in-place map copy - over the seeded cases of tests/map_cases.py, against the NumPy
restatements under tests/, through the C ABI's host forms; every third seed also through the device form on torch
tensors, two calls back to back without a synchronise in between.

Everything is integer and compares with array_equal, except the float outputs of the weigh and of the resample's
estimate, which follow tests/mcl_checks.py (poses and estimates at 1e-9, ESS exact, the 2 % unsure rule on the device's own
moved poses).  Maps go straight into the counters; the restatement reads the pmap read back from the device.  The
matcher, the localisation and the frontiers also run their batch reversed and its first entry alone: the same rows.
tests/test_map_cases.py asserts, without a device, which edges these cases reach.  A failure names (kind, seed):
map_cases.case_of(kind, seed) rebuilds the case."""
import contextlib

import numpy as np
import pytest

import frontier_cases as FC
import locate_cases as LC
import map_cases as C
from conftest import pkg
from mcl_checks import check_resample, check_weigh, same_bits

pytestmark = pytest.mark.gpu


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


def tag(c):
    return (c["kind"], c["seed"])


def device_form(c):
    return c["seed"] % 3 == 0


def up(a, ctx):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", ctx.device))


def counters(g):
    """(pass, hit) of every map as uint32 arrays; synchronises."""
    import torch
    g._ctx.synchronize()
    p, h = g.counters_torch()
    out = p.cpu().numpy().view(np.uint32).copy(), h.cpu().numpy().view(np.uint32).copy()
    torch.cuda.synchronize()
    return out


def untouched(g, before, c):
    after = counters(g)
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1]), tag(c)


def grid_of_cells(slam, ctx, c):
    """The case's maps on the device, occupied cells written into the hit counters; (grid, pmaps read back)."""
    g = slam.DeviceGrid(c["G"], c["xw"], c["yw"], c["scale"], c["off_x"], c["off_y"], context=ctx)
    pm = LC.occupy(g, c["cells"])
    assert np.array_equal(pm, C.pmaps_of_cells(c)), tag(c)
    return g, pm


@contextlib.contextmanager
def named(c):
    """Every assertion that fails inside carries (kind, seed) in front."""
    try:
        yield
    except AssertionError as e:
        first = e.args[0] if e.args else None
        if isinstance(first, tuple) and len(first) >= 2 and isinstance(first[0], str) and first[:2] == tag(c):
            raise
        raise AssertionError(tag(c), *e.args) from e


@contextlib.contextmanager
def option(ctx, name, value, default):
    """A context option for the length of a block; ``value`` None leaves the default."""
    if value is not None:
        ctx.set_option(name, value)
    try:
        yield
    finally:
        ctx.set_option(name, default)


# ------------------------------------------------------------------ the distance field
def test_field(slam, ctx):
    import torch
    for seed in C.seeds():
        c = C.case_of("field", seed)
        with named(c):
            g, pm = grid_of_cells(slam, ctx, c)
            before = counters(g)
            want = C.answer(c, pm)
            got = slam.grid_distance_field_host(g, c["cap"])
            assert got.dtype == np.int16 and got.shape == want.shape, tag(c)
            assert np.array_equal(got, want), tag(c) + (np.argwhere(got != want)[:4].tolist(),)
            if device_form(c):
                d2 = torch.full(want.shape, -7, dtype=torch.int16, device=torch.device("cuda", ctx.device))
                torch.cuda.synchronize()
                d1 = g.distance_field(c["cap"])
                assert g.distance_field(c["cap"], out=d2) is d2
                ctx.synchronize()
                assert np.array_equal(d1.cpu().numpy(), want) and np.array_equal(d2.cpu().numpy(), want), tag(c)
            untouched(g, before, c)
            g.close()
    ctx.check_status()


# ------------------------------------------------------------------ the window matcher
def match_host(slam, g, c, sel=None):
    """grid_match_host of the case's hypotheses ``sel`` (a slice or index array; None: all)."""
    pick = (lambda a: a) if sel is None else (lambda a: None if a is None else np.ascontiguousarray(a[sel]))
    r = c["ranges"] if c["ranges"].ndim == 1 else pick(c["ranges"])
    return slam.grid_match_host(g, r, pick(c["centres"]), c["cos_t"], c["sin_t"], pick(c["rot_cs"]), c["nx"], c["ny"], c["step"],
                                max_range=c["max_range"], cap=c["cap"], grid_of_batch=pick(c["maps"]), return_costs=True)


def test_match(slam, ctx):
    for seed in C.seeds():
        c = C.case_of("match", seed)
        with named(c):
            g, pm = grid_of_cells(slam, ctx, c)
            before = counters(g)
            want = C.answer(c, pm)
            got = match_host(slam, g, c)
            for a, b, name in zip(got, want, ("best", "cost", "used", "costs")):
                assert a.dtype == np.int32 and a.shape == b.shape and np.array_equal(a, b), tag(c) + (name,)
            if not c["costs"]:                                             # the cost volume not asked for: the same three
                r = c["ranges"]
                three = slam.grid_match_host(g, r, c["centres"], c["cos_t"], c["sin_t"], c["rot_cs"], c["nx"], c["ny"], c["step"],
                                             max_range=c["max_range"], cap=c["cap"], grid_of_batch=c["maps"])
                assert len(three) == 3 and all(np.array_equal(a, b) for a, b in zip(three, want)), tag(c)
            # batch invariance: reversed, and the first hypothesis alone
            for a, b in zip(match_host(slam, g, c, slice(None, None, -1)), got):
                assert np.array_equal(a[::-1], b), tag(c) + ("reversed",)
            for a, b in zip(match_host(slam, g, c, slice(0, 1)), got):
                assert np.array_equal(a, b[:1]), tag(c) + ("alone",)
            if device_form(c):
                d = [up(c[k], ctx) for k in ("ranges", "centres", "cos_t", "sin_t", "rot_cs")]
                maps = up(c["maps"], ctx)
                import torch
                torch.cuda.synchronize()
                kw = dict(max_range=c["max_range"], cap=c["cap"], grid_of_batch=maps)
                o1 = g.match(*d, c["nx"], c["ny"], c["step"], return_costs=True, **kw)
                o2 = g.match(*d, c["nx"], c["ny"], c["step"], **kw)
                ctx.synchronize()
                assert len(o1) == 4 and len(o2) == 3, tag(c)
                for a, b in zip(o1 + o2, got + got[:3]):
                    assert np.array_equal(a.cpu().numpy(), b), tag(c) + ("device form",)
            untouched(g, before, c)
            g.close()
    ctx.check_status()


# ------------------------------------------------------------------ global localisation
def locate_host(slam, g, c, sel=None):
    pick = (lambda a: a) if sel is None else (lambda a: None if a is None else np.ascontiguousarray(a[sel]))
    B = c["B"] if sel is None else len(np.arange(c["B"])[sel])
    r = c["ranges"] if c["ranges"].ndim == 1 else pick(c["ranges"])
    return slam.grid_locate_host(g, r, c["cos_t"], c["sin_t"], c["rot_cs"], levels=c["H"], region=pick(c["regions"]), max_range=c["max_range"],
                                 cap=c["cap"], grid_of_batch=pick(c["maps"]), B=B, return_stats=True)


def test_locate(slam, ctx):
    import torch
    for seed in C.seeds():
        c = C.case_of("locate", seed)
        with named(c):
            g, pm = grid_of_cells(slam, ctx, c)
            before = counters(g)
            fields = LC.fields_of(slam, g, c["cap"])                      # the device's own field is the restatement's
            mb, _ = C.locate_plan(c)
            with option(ctx, "locate_ws_mb", mb, 64):
                got = LC.check(slam, g, fields, c["scale"], c["ranges"], c["cos_t"], c["sin_t"], c["rot_cs"], c["H"], c["max_range"], c["cap"],
                               maps=c["maps"], regions=c["regions"], B=c["B"])
                for name, sel in (("reversed", slice(None, None, -1)), ("alone", slice(0, 1))):
                    part = locate_host(slam, g, c, sel)
                    for a, b in zip(part, got):
                        assert a.dtype == b.dtype and np.array_equal(a, b[sel]), tag(c) + (name,)
            if device_form(c):
                d = dict(cos_t=up(c["cos_t"], ctx), sin_t=up(c["sin_t"], ctx), rot_cs=up(c["rot_cs"], ctx))
                r, reg, maps = up(c["ranges"], ctx), up(c["regions"], ctx), up(c["maps"], ctx)
                torch.cuda.synchronize()
                kw = dict(levels=c["H"], region=reg, max_range=c["max_range"], cap=c["cap"], grid_of_batch=maps, B=c["B"])
                o1 = g.locate(r, return_stats=True, **kw, **d)
                o2 = g.locate(r, **kw, **d)
                ctx.synchronize()
                assert len(o1) == 4 and len(o2) == 3, tag(c)
                for a, b in zip(o1 + o2, got + got[:3]):
                    assert np.array_equal(a.cpu().numpy(), b), tag(c) + ("device form",)
            untouched(g, before, c)
            g.close()
    ctx.set_option("locate_ws_mb", 64)
    ctx.check_status()


# ------------------------------------------------------------------ frontiers
def frontiers_host(slam, g, c, maps, B, labels=True):
    return slam.grid_frontiers_host(g, grid_of_batch=maps, B=B, radius=c["radius"], min_unknown=c["min_unknown"], min_clear2=c["min_clear2"],
                                    cap=c["cap"], min_size=c["min_size"], max_clusters=c["M"], labels=labels)


def test_frontiers(slam, ctx):
    import torch
    for seed in C.seeds():
        c = C.case_of("frontiers", seed)
        with named(c):
            g, pm = FC.grid_of(slam, ctx, c["pmaps"])
            before = counters(g)
            fields = C.fields_of(pm, c["cap"]) if c["min_clear2"] > 0 else None
            mb, _ = C.frontier_plan(c)
            with option(ctx, "frontier_ws_mb", mb, 256):
                got = FC.check(slam, g, pm, maps=c["maps"], B=c["B"], radius=c["radius"], min_unknown=c["min_unknown"], min_size=c["min_size"],
                               M=c["M"], fields=fields, min_clear2=c["min_clear2"], cap=c["cap"])
                if not c["labels"]:                                        # labels not asked for: the same counts and tables
                    FC.same(frontiers_host(slam, g, c, c["maps"], c["B"], labels=False), got[:3])
                maps = np.arange(c["B"], dtype=np.int32) if c["maps"] is None else c["maps"]
                for name, sel in (("reversed", slice(None, None, -1)), ("alone", slice(0, 1))):
                    part = frontiers_host(slam, g, c, np.ascontiguousarray(maps[sel]), len(maps[sel]))
                    for a, b in zip(part, got):
                        assert a.dtype == b.dtype and np.array_equal(a, b[sel]), tag(c) + (name,)
            if device_form(c):
                dm = up(c["maps"], ctx)
                torch.cuda.synchronize()
                kw = dict(B=c["B"], radius=c["radius"], min_unknown=c["min_unknown"], min_clear2=c["min_clear2"], cap=c["cap"],
                          min_size=c["min_size"], max_clusters=c["M"])
                o1 = g.frontiers(dm, labels=True, **kw)
                o2 = g.frontiers(dm, **kw)
                ctx.synchronize()
                assert len(o1) == 4 and len(o2) == 3, tag(c)
                FC.same([t.cpu().numpy() for t in o1], got)
                FC.same([t.cpu().numpy() for t in o2], got[:3])
            untouched(g, before, c)
            g.close()
    ctx.set_option("frontier_ws_mb", 256)
    ctx.check_status()


# ------------------------------------------------------------------ the weighs
def weigh_dev(slam, ctx, g, c):
    """slam_mcl_weigh_dev / slam_mcl_weigh_maps_dev twice back to back on copies of the inputs; the outputs of both."""
    import torch
    abi = pkg("_abi")
    L = abi.lib()
    fn = L.slam_mcl_weigh_maps_dev if c["own_maps"] else L.slam_mcl_weigh_dev
    F, P, n = c["F"], c["P"], c["n"]
    dev = torch.device("cuda", ctx.device)
    fixed = [up(c[k], ctx) for k in ("motion", "noise", "ranges", "cos_t", "sin_t", "maps")]
    runs = []
    for _ in range(2):
        runs.append(dict(poses=up(c["poses"], ctx), acc=up(c["acc"], ctx), cost=torch.full((F, P), -9, dtype=torch.int32, device=dev),
                         used=torch.full((F,), -9, dtype=torch.int32, device=dev)))
    torch.cuda.synchronize()
    for r in runs:
        abi.check(fn(ctx.handle, g._h, abi.ptr(r["poses"]), abi.ptr(fixed[0]), abi.ptr(fixed[1]), abi.ptr(fixed[2]), abi.ptr(fixed[3]),
                     abi.ptr(fixed[4]), abi.ptr(fixed[5]), F, P, n, c["max_range"], c["cap"], None, abi.ptr(r["acc"]), abi.ptr(r["cost"]),
                     abi.ptr(r["used"])))
    ctx.synchronize()
    return [(r["poses"].cpu().numpy(), r["cost"].cpu().numpy(), None if r["acc"] is None else r["acc"].cpu().numpy(), r["used"].cpu().numpy())
            for r in runs]


def test_weigh(slam, ctx):
    for seed in C.seeds():
        c = C.case_of("weigh", seed)
        with named(c):
            g, pm = grid_of_cells(slam, ctx, c)
            before = counters(g)
            fields = C.fields_of(pm, c["cap"])
            geom = (c["scale"], c["off_x"], c["off_y"])
            kw = dict(max_range=c["max_range"], cap=c["cap"], motion=c["motion"], noise=c["noise"], acc=c["acc"], fields=fields, tag=tag(c),
                      maps=None if c["own_maps"] else c["maps"], pmaps=c["maps"] if c["own_maps"] else None)
            with option(ctx, "mcl_shape", c["mcl_shape"], -1):
                got = check_weigh(slam, g, pm, geom, c["poses"], c["ranges"], c["cos_t"], c["sin_t"], **kw)
                if device_form(c):
                    for dev in weigh_dev(slam, ctx, g, c):
                        check_weigh(slam, g, pm, geom, c["poses"], c["ranges"], c["cos_t"], c["sin_t"], got=dev, **kw)
                        for a, b in zip(dev, got):                         # the same kernels: the same bits
                            assert (a is None and b is None) or same_bits(a, b), tag(c) + ("device form",)
            untouched(g, before, c)
            g.close()
    ctx.set_option("mcl_shape", -1)
    ctx.check_status()


# ------------------------------------------------------------------ resampling
def resample_dev(slam, ctx, c):
    import torch
    abi = pkg("_abi")
    F, P = c["F"], c["P"]
    dev = torch.device("cuda", ctx.device)
    poses, table, u0 = up(c["poses"], ctx), up(c["table"].view(np.int32), ctx), up(c["u0"], ctx)
    runs = [dict(acc=up(c["acc"], ctx), poses=torch.empty_like(poses), anc=torch.full((F, P), -9, dtype=torch.int32, device=dev),
                 est=torch.empty((F, 4), dtype=torch.float64, device=dev), info=torch.empty((F, 4), dtype=torch.int32, device=dev)) for _ in range(2)]
    torch.cuda.synchronize()
    for r in runs:
        abi.check(abi.lib().slam_mcl_resample_dev(ctx.handle, abi.ptr(poses), abi.ptr(r["acc"]), abi.ptr(table), c["T"], c["shift"], abi.ptr(u0),
                                                  c["ess_frac"], F, P, abi.ptr(r["poses"]), abi.ptr(r["anc"]), abi.ptr(r["est"]), abi.ptr(r["info"])))
    ctx.synchronize()
    return [tuple(r[k].cpu().numpy() for k in ("poses", "acc", "anc", "est", "info")) for r in runs]


def test_resample(slam, ctx):
    for seed in C.seeds():
        c = C.case_of("resample", seed)
        with named(c):
            args = (c["poses"], c["acc"], c["table"], c["u0"])
            kw = dict(shift=c["shift"], ess_frac=c["ess_frac"], tag=tag(c))
            clamped = int(c["table"].max()) > (1 << 20)                    # the host form rejects such a table; the device form clamps it
            if clamped:
                with pytest.raises(slam.SlamError, match="table entry above 2\\^20"):
                    slam.mcl_resample_host(ctx, *args, shift=c["shift"], ess_frac=c["ess_frac"])
            else:
                got = check_resample(slam, ctx, *args, **kw)
            if clamped or device_form(c):
                for dev in resample_dev(slam, ctx, c):
                    check_resample(slam, ctx, *args, got=dev, **kw)
                    if not clamped:
                        assert all(same_bits(a, b) for a, b in zip(dev, got)), tag(c) + ("device form",)
    ctx.check_status()


# ------------------------------------------------------------------ settle
def test_settle(slam, ctx):
    import torch
    abi = pkg("_abi")
    dev = torch.device("cuda", ctx.device)
    for seed in C.seeds():
        c = C.case_of("settle", seed)
        with named(c):
            want = C.answer(c)
            F, P = c["F"], c["P"]
            settled, poses, map_src, moved = slam.mcl_settle_host(ctx, c["ancestors"], c["poses"], map0=c["map0"])
            for a, name in ((settled, "settled"), (map_src, "map_src"), (moved, "moved")):
                assert a.dtype == np.int32 and np.array_equal(a, want[name]), tag(c) + (name,)
            assert (poses is None and want["poses"] is None) or same_bits(poses, want["poses"]), tag(c)
            if device_form(c):
                anc, src = up(c["ancestors"], ctx), up(c["poses"], ctx)
                runs = [dict(settled=torch.full((F, P), -9, dtype=torch.int32, device=dev), map_src=torch.full((F, P), -9, dtype=torch.int32, device=dev),
                             moved=torch.full((F,), -9, dtype=torch.int32, device=dev), poses=None if src is None else torch.empty_like(src))
                        for _ in range(2)]
                torch.cuda.synchronize()
                for r in runs:
                    abi.check(abi.lib().slam_mcl_settle_dev(ctx.handle, abi.ptr(anc), abi.ptr(src), F, P, c["map0"], abi.ptr(r["settled"]),
                                                            abi.ptr(r["poses"]), abi.ptr(r["map_src"]), abi.ptr(r["moved"])))
                ctx.synchronize()
                for r in runs:
                    for name in ("settled", "map_src", "moved"):
                        assert np.array_equal(r[name].cpu().numpy(), want[name]), tag(c) + (name, "device form")
                    assert src is None or same_bits(r["poses"].cpu().numpy(), want["poses"]), tag(c)
    ctx.check_status()


# ------------------------------------------------------------------ the in-place map copy
def set_counters(g, c):
    import torch
    g._ctx.synchronize()
    p, h = g.counters_torch()
    p.copy_(torch.from_numpy(c["pass_cnt"].view(np.int32)).to(p.device))
    h.copy_(torch.from_numpy(c["hit_cnt"].view(np.int32)).to(h.device))
    torch.cuda.synchronize()


def test_copy(slam, ctx):
    import torch
    for seed in C.seeds():
        c = C.case_of("copy", seed)
        with named(c):
            want = C.answer(c)
            g = slam.DeviceGrid(c["G"], c["xw"], c["yw"], 1.0, 0.0, 0.0, context=ctx)
            set_counters(g, c)
            got = slam.grid_copy_maps_host(g, c["src"], c["first"])
            assert got.dtype == np.int32 and np.array_equal(got, want["copied"]), tag(c)
            p, h = counters(g)
            assert np.array_equal(p, want["pass_cnt"]) and np.array_equal(h, want["hit_cnt"]), tag(c)   # copies, prefix and suffix alike
            if device_form(c):
                set_counters(g, c)
                src = up(c["src"], ctx)
                torch.cuda.synchronize()
                o1 = g.copy_maps(src, c["first"])
                o2 = g.copy_maps(src, c["first"])                          # again on the copied maps: nothing more changes
                ctx.synchronize()
                assert np.array_equal(o1.cpu().numpy(), want["copied"]) and np.array_equal(o2.cpu().numpy(), want["copied"]), tag(c)
                p, h = counters(g)
                assert np.array_equal(p, want["pass_cnt"]) and np.array_equal(h, want["hit_cnt"]), tag(c) + ("device form",)
            g.close()
    ctx.check_status()
