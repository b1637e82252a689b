"""The seeded cases of slam_grid_view_gain (tests/view_cases.py) on the device, under both engines: the host form on
every seed, counts and seen words bit-equal to tests/view_ref.py on the pmaps read back; on every third seed the device
form, the batch reversed and the first view alone, which must all equal the batch.  SLAM_HYP_EXAMPLES turns the sweep
into a soak run.  Every assertion message carries the seed."""
import time

import numpy as np
import pytest

import view_cases as VC
from conftest import pkg
from test_gpu_view import check, dev, grid_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def slam():
    p = pkg()
    p._abi.default_context()   # fails loudly when there is no gfx950 device
    return p


@pytest.fixture(scope="module", params=[0, 1], ids=["global", "lds"])
def ctx(request, slam):
    c = slam.Context(0)
    c.set_option("gain_lds", request.param)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _clock(request):
    t = time.perf_counter()
    yield
    print("%s: %.1f s over %d seeds" % (request.node.name, time.perf_counter() - t, len(VC.seeds())))


def host_form(slam, g, case, rows=slice(None)):
    return slam.grid_view_gain_host(g, case["poses"][rows], case["ct"], case["st"], max_range=case["max_range"], skip=case["skip"],
                                    grid_of_batch=np.ascontiguousarray(case["maps"][rows]), return_seen=True)


@pytest.mark.parametrize("lot", range(3))
def test_seeded_cases(slam, ctx, lot):
    for seed in [s for s in VC.seeds() if (s // 7) % 3 == lot]:
        case = VC.case_of("view", seed)
        g = grid_of(slam, ctx, case["pmaps"], case["scale"], case["off_x"], case["off_y"])
        pm = np.stack([g.read(i)["pmap"] for i in range(g.G)])
        want = VC.answer(case, pm)
        ok = VC.named(case)
        if ok.all():
            batch = host_form(slam, g, case)
            check(batch, want, "seed %d, host form" % seed)
        else:                                            # the host form rejects the entry that names no map, and answers the rest
            with pytest.raises(slam.SlamError, match="grid_of_batch"):
                host_form(slam, g, case)
            rows = np.flatnonzero(ok)
            if len(rows):
                check(host_form(slam, g, case, rows), (want[0][rows], want[1][rows]), "seed %d, host form of the named rows" % seed)
        if seed % 3 == 0:
            a = dict(max_range=case["max_range"], skip=case["skip"])
            check(dev(g, ctx, case["poses"], case["ct"], case["st"], gob=case["maps"], **a), want, "seed %d, device form" % seed)
            rev = dev(g, ctx, case["poses"][::-1], case["ct"], case["st"], gob=case["maps"][::-1], **a)
            check((rev[0][::-1], rev[1][::-1]), want, "seed %d, reversed" % seed)
            check(dev(g, ctx, case["poses"][:1], case["ct"], case["st"], gob=case["maps"][:1], **a), (want[0][:1], want[1][:1]),
                  "seed %d, the first view alone" % seed)
        g.close()
    ctx.check_status()
