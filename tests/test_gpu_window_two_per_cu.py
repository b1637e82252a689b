"""The shared-map window kernel (k_grid_update_win) in launches of more workgroups than the chip has CUs, where the
window is carved so that two workgroups share a CU (33 216 cells for groups of 16 scans of 360 beams instead of
36 864), and the phases of a group are decided per direction half.

Every case (tests/win_cases.py): grid_mode 3, groups of 16 scans of 360 beams, scans 2 - 3 cells apart, 304 groups (19
distinct ones, 16 times over) cast into ONE map twice, with one and with two workgroups per group (grid_split).  The
boxes sit at the edges of the capacity tests/win_shapes.py gives for that launch: a box one cell row under and one over
it, one half over, both halves over, a quadrant over (sub-rectangle + direct atomics), rows of an odd number of cells,
rays leaving the map (tests/test_win_shapes_cpu.py asserts the phases each group takes).  Counters, pmap and the visit
count must equal the oracle's.  The same scans in two launches of 152 groups (at most one workgroup per CU) keep the old
capacity and give the same map.  Which capacity a launch took, and how many of its workgroups the runtime holds on a
CU, is read from the library's SLAM_WIN_RESIDENCY report."""
import re

import numpy as np
import pytest

import win_cases as wc
import win_shapes as ws
from conftest import pkg
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu

_REFERENCE = {}


def _reference(case):
    """The oracle's map after one and after two passes over the case's scans (computed once, never changed)."""
    if case not in _REFERENCE:
        xw, yw, scale, off_x, off_y = wc.CASES[case][0]
        OX, OY, CX, CY = wc.scans(case)
        og = co.Grid(xw, yw, scale, off_x, off_y)
        snaps = []
        for _ in range(2):
            for b in range(wc.SCANS):
                og.update(OX[b], OY[b], CX[b], CY[b])
            snaps.append({"pass": og.pass_cnt.copy(), "hit": og.hit_cnt.copy(), "pmap": og.pmap.copy(), "visits": og.visits})
        for s in snaps:
            for name in ("pass", "hit", "pmap"):
                s[name].setflags(write=False)
        _REFERENCE[case] = snaps
    return _REFERENCE[case]


@pytest.fixture(scope="module")
def slam():
    p = pkg()
    p._abi.default_context()
    return p


REPORT = re.compile(r"k_grid_update_win: 1024 threads, (\d+) bytes of LDS \(window (\d+) cells\), (\d+) workgroups: (-?\d+) resident per CU\n")


def _cast(slam, case, split, pieces, capfd, monkeypatch):
    """Cast the case's scans twice, each time in `pieces` launches of equal size; compare with the oracle after each pass.
    Returns the library's residency reports, one per launch: (two per CU by the rule, workgroups, resident per CU)."""
    xw, yw, scale, off_x, off_y = wc.CASES[case][0]
    OX, OY, CX, CY = wc.scans(case)
    ref = _reference(case)
    monkeypatch.setenv("SLAM_WIN_RESIDENCY", "1")
    ctx = slam.Context(0)
    ctx.set_option("grid_mode", 3)
    ctx.set_option("grid_group", wc.GROUP)
    ctx.set_option("grid_split", split)
    g = slam.DeviceGrid(1, xw, yw, scale, off_x, off_y, context=ctx)
    capfd.readouterr()
    per = wc.SCANS // pieces
    for k in range(2):
        for p in range(pieces):
            sl = slice(p * per, (p + 1) * per)
            g.update_host(OX[sl], OY[sl], CX[sl], CY[sl])
        ctx.check_status()
        r = g.read(0, want=("pmap", "pass", "hit"))
        assert np.array_equal(r["pass"], ref[k]["pass"]), (k, int(np.sum(r["pass"] != ref[k]["pass"])))
        assert np.array_equal(r["hit"], ref[k]["hit"]), k
        assert np.array_equal(r["pmap"], ref[k]["pmap"]), (k, int(np.sum(r["pmap"] != ref[k]["pmap"])))
        assert g.visits() == ref[k]["visits"], k
    err = capfd.readouterr().err
    g.close()
    ctx.close()
    out = []
    for lds, cells, wgs, per_cu in (tuple(int(v) for v in m) for m in REPORT.findall(err)):
        # (the LDS-guard debug build asks for 512 bytes more and carves the window out of what is left)
        guard = lds - ws.win_lds_bytes(wc.GROUP, wc.NEW.sort_cap, cells)
        assert guard in (0, 512), (lds, cells)
        two = wgs > ws.CUS
        assert cells == ws.win_cells_for(wc.GROUP, wc.NEW.sort_cap, two, guard=guard)
        assert (cells < ws.WIN_CELLS) == two and (guard or cells == (wc.CAP if two else ws.WIN_CELLS))
        out.append((two, wgs, per_cu))
    return out


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("case", list(wc.CASES))
def test_chip_filling_launch(slam, case, split, capfd, monkeypatch):
    """304 groups in one launch, twice: the window carved for two workgroups per CU, and the runtime grants two."""
    reports = _cast(slam, case, split, 1, capfd, monkeypatch)
    assert reports == [(True, 304 * (split + 1), 2)] * 2


@pytest.mark.parametrize("case", ["row_over", "one_half_over"])
def test_same_scans_in_launches_of_one_workgroup_per_cu(slam, case, capfd, monkeypatch):
    """The same scans in two launches of 152 groups each: the old capacity, one workgroup per CU, the same map."""
    reports = _cast(slam, case, 0, 2, capfd, monkeypatch)
    assert reports == [(False, 152, 1)] * 4
