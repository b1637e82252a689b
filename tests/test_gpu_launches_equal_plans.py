"""The launchers shape their launches by the planners and nothing else, by observation: what a launch reports of itself -
the window kernel's residency line (SLAM_WIN_RESIDENCY: threads, LDS, window, workgroups) and the timing slots of the
kernel families - is what slam_plan_win / slam_plan_icp answer for the same request, and the results are the oracle's."""
import re

import numpy as np
import pytest

import icp_shapes as sh
import win_shapes as ws
from conftest import pkg
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu
FTOL = 1e-9
AMIN, AMAX = -3.14159, 3.14159
REPORT = re.compile(r"k_grid_update_win: (\d+) threads, (\d+) bytes of LDS \(window (\d+) cells\), (\d+) workgroups: ")


@pytest.fixture(scope="module")
def slam():
    p = pkg()
    p._abi.default_context()
    return p


def test_replay_and_batch_launch_what_the_plans_say(slam, syn, capfd, monkeypatch):
    # a replay of 40 scans of 90 beams: 39 pairs matched, 39 scans cast in groups of 8 by the shared-map window kernel
    rep = syn.make_replay(40, 90, seed=11, stride=5)
    monkeypatch.setenv("SLAM_WIN_RESIDENCY", "1")
    dr = slam.DeviceReplay(rep.ranges, AMIN, AMAX)
    dr.ctx.set_option("grid_mode", 3)
    dr.ctx.set_option("grid_group", 8)
    grid = dr.make_grid(1, 400, 400, 0.05)
    dr.ctx.timing_enable(True)
    dr.ctx.timing_read()
    capfd.readouterr()
    dr.run()
    poses, T, it = dr.results()
    timing = dr.ctx.timing_read()
    reports = REPORT.findall(capfd.readouterr().err)
    dr.ctx.timing_enable(False)

    p = ws.plan_win(39, 90, 8, L=1, pmap_live=True, guard=-1)         # (guard -1: of the build that is loaded)
    assert p.form == "Win" and p.split == 1 and p.wgs == 10 and p.threads == 512
    assert [tuple(int(v) for v in r) for r in reports] == [(p.threads, p.lds, p.win_cells, p.wgs)]
    m = sh.plan_icp(39, 90, 90, True, guard=-1)
    assert m.form == "Workgroup" and (m.qpt, m.block) == (1, 128)
    assert {k: n for k, (_, n) in timing.items() if n} == {"icp": 1, "compose": 1, "grid": 1}
    assert timing["grid"][0] > 0 and timing["icp"][0] > 0

    og = co.Grid(400, 400, 20.0, 10.0, 10.0)
    oposes, oT, oit, visits = co.replay(rep.ranges, AMIN, AMAX, og, threads=8)
    assert np.array_equal(it[0], oit)
    assert np.max(np.abs(poses[0] - oposes)) < FTOL and np.max(np.abs(T[0] - oT)) < FTOL
    r = grid.read(0, want=("pmap", "pass", "hit"))
    assert np.array_equal(r["pass"], og.pass_cnt) and np.array_equal(r["hit"], og.hit_cnt)
    assert np.array_equal(r["pmap"], og.pmap) and grid.visits() == visits

    # a batch of 65 pairs of 129 points: the preference applies (two queries per lane), one workgroup launch
    rng = np.random.default_rng(65)
    B, n = 65, 129
    tar = rng.normal(0, 3, size=(B, 2, n))
    th = rng.uniform(-0.1, 0.1, size=B)
    src = np.empty((B, 2, n))
    for b in range(B):
        c, s = np.cos(th[b]), np.sin(th[b])
        x, y = tar[b, 0] + rng.normal(0, 0.02, n), tar[b, 1] + rng.normal(0, 0.02, n)
        src[b, 0], src[b, 1] = c * x - s * y + 0.05, s * x + c * y - 0.03
    ctx = slam.Context(0)
    ctx.timing_enable(True)
    ctx.timing_read()
    Tb, itb, errb = slam.icp_batch_host(tar, src, 12, 1e-4, context=ctx)
    timing = ctx.timing_read()
    ctx.close()
    m = sh.plan_icp(B, n, n, False, guard=-1)
    assert m.form == "Workgroup" and (m.qpt, m.block, m.preferred) == (2, 128, 1) and not m.raise_attr
    assert {k: n for k, (_, n) in timing.items() if n} == {"icp": 1} and timing["icp"][0] > 0
    oT, oit, oerr = co.icp_batch(tar, src, 12, 1e-4)
    assert np.array_equal(itb, oit)
    assert np.max(np.abs(Tb - oT)) < FTOL and np.max(np.abs(errb - oerr)) < FTOL
