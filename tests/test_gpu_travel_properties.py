"""The seeded cases of slam_grid_travel (tests/travel_cases.py) on the device: every output of every case against the
restatement on the map and the field read back, with array_equal; SLAM_HYP_EXAMPLES turns the sweep into a soak run.
'travel' is one query a call.  'travel_batch' is B queries routed over G maps in the host form on every seed; on every
third seed the batch reversed, its first query alone and the call without cost_out, which must all equal the batch (no new
reference answer); on every third seed the device form twice back to back, the second call with through_unknown flipped;
on every fourth seed the budget cut to two chunks.  Every assertion message carries the seed."""
import time

import numpy as np
import pytest

import frontier_cases as FC
import travel_cases as TC
import travel_ref as T
from conftest import pkg

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


@pytest.fixture(autouse=True)
def _clock(request):
    t = time.perf_counter()
    yield
    print("%s: %.1f s over %d seeds" % (request.node.name, time.perf_counter() - t, len(TC.seeds())))


@pytest.mark.parametrize("lot", range(6))
def test_seeded_cases(slam, ctx, lot):
    seeds = [s for s in TC.seeds() if s % 6 == lot]
    for seed in seeds:
        case = TC.case_of("travel", seed)
        g, pm = FC.grid_of(slam, ctx, case["pmap"])
        field = slam.grid_distance_field_host(g, case["cap"])[0] if case["min_clear2"] > 0 else None
        want = TC.answer(case, pm[0], field)
        got = slam.grid_travel_host(g, case["sources"][None], goals=case["goals"][None], foot=case["foot"],
                                    through_unknown=case["through_unknown"], min_clear2=case["min_clear2"], cap=case["cap"],
                                    path_cap=case["path_cap"], dirs=True)
        if case["path_cap"] == 0:
            got["path"] = np.full((1,) + want["path"].shape, -1, dtype=np.int32)
        assert got["status"].tolist() == [0], seed
        TC.same({k: v[0] for k, v in got.items() if k != "status"}, {k: v for k, v in want.items() if k not in ("status", "T")}, tag=seed)
        g.close()
    ctx.check_status()


# ------------------------------------------------------------------ batches
def keys_of(case, cost=True):
    return [k for k in TC.KEYS if not (k == "path" and case["path_cap"] == 0) and (cost or k != "cost")]


def host_form(slam, g, case, rows=slice(None), **kw):
    a = dict(grid_of_batch=np.ascontiguousarray(case["maps"][rows]), goals=np.ascontiguousarray(case["goals"][rows]), cap=case["cap"],
             dirs=True, **TC.rule_of(case))
    a.update(kw)
    return slam.grid_travel_host(g, np.ascontiguousarray(case["sources"][rows]), **a)


def query(name, a=0, b=0, c=0):
    import ctypes as C
    abi = pkg("_abi")
    out = C.c_int64()
    abi.check(abi.lib().slam_plan_query(name.encode(), int(a), int(b), int(c), -1, C.byref(out)))
    return int(out.value)


@pytest.mark.parametrize("lot", range(6))
def test_seeded_batches(slam, ctx, lot):
    import torch
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    for seed in [s for s in TC.seeds() if s % 6 == lot]:
        case = TC.case_of("travel_batch", seed)
        g, pm = FC.grid_of(slam, ctx, case["pmaps"])
        G, B = len(pm), len(case["maps"])
        fields = slam.grid_distance_field_host(g, case["cap"]) if case["min_clear2"] > 0 else None
        want = TC.answer_batch(case, pm, fields)
        want = {k: want[k] for k in keys_of(case)}
        named = (case["maps"] >= 0) & (case["maps"] < G)
        batch = host_form(slam, g, case)
        TC.same(batch, want, tag=(seed, "host form"))
        assert np.array_equal(batch["status"], np.where(named, 0, -1)), seed
        if seed % 3 == 0:
            rev = host_form(slam, g, case, slice(None, None, -1))
            TC.same({k: v[::-1] for k, v in rev.items()}, batch, tag=(seed, "reversed"))
            TC.same(host_form(slam, g, case, slice(0, 1)), {k: v[:1] for k, v in batch.items()}, tag=(seed, "the first query alone"))
            TC.same(host_form(slam, g, case, cost=False), {k: batch[k] for k in keys_of(case, cost=False)}, tag=(seed, "cost=False"))
        if seed % 3 == 1:
            flipped = dict(TC.rule_of(case, through_unknown=not case["through_unknown"]))
            want2 = T.batch(pm, case["sources"], maps=case["maps"], fields=fields, goals=case["goals"], **flipped)
            src, maps, goals = up(case["sources"]), up(case["maps"]), up(case["goals"])
            torch.cuda.synchronize()
            o1 = g.travel(src, maps, goals=goals, cap=case["cap"], dirs=True, **TC.rule_of(case))
            o2 = g.travel(src, maps, goals=goals, cap=case["cap"], dirs=True, **flipped)
            ctx.synchronize()
            TC.same({k: v.cpu().numpy() for k, v in o1.items()}, want, tag=(seed, "device form"))
            TC.same({k: v.cpu().numpy() for k, v in o2.items()}, {k: want2[k] for k in keys_of(case)}, tag=(seed, "device form, second call"))
        if seed % 4 == 0 and B >= 2:
            per = -(-B // 2)
            try:
                ctx.set_option("travel_ws_mb", per * query("travel_query_bytes", g.xw, g.yw, 0) / 1048576.0)     # exactly `per` queries fit
                TC.same(host_form(slam, g, case), batch, tag=(seed, "two chunks"))
            finally:
                ctx.set_option("travel_ws_mb", 256)
        g.close()
    ctx.check_status()
