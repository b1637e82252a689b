"""tests/win_shapes.py against the source text of csrc/grid_kernels.hip, the window's capacity over every group size,
and the phases of the benchmark trajectory under the old and the new capacity.  No GPU."""
import importlib
import re
from collections import Counter

import pytest

import win_shapes as ws

BEAMS = (90, 360, 720, 1080)


@pytest.fixture(scope="module")
def text():
    with open(ws.SOURCE) as f:
        return f.read()


def test_constants_are_the_sources(text):
    for name, value in ws.source_constants(text).items():
        assert getattr(ws, name) == value, name
    assert "double px, py, c, s;" in text and "int pcx, pcy, cbad, pad;" in text       # ScanConst: 48 bytes


def test_rules_are_the_sources(text):
    """The lines the restatement stands for, as they are written."""
    flat = re.sub(r"\s+", " ", text)
    for line in (
        "return win_sc_bytes(group) + kWinBoxInts * 4 + 4 * kSortBins * 4 + (size_t)sort_cap * 2 + (size_t)win_cells * 2 + kLdsGuard;",
        "return rays <= kMaxSortRays ? (int)((rays + 7) & ~7L) : 0;",
        "const long half = lds_per_cu / 2 - kWinHalfSlack;",
        "long cells = ((half - other) / 2) & ~15L;",
        "if (cells > kWinCells) return (int)cells;",
        "return two_per_cu && cells >= kWinTwoFloor ? (int)cells : kWinCells;",
        "(!exclusive && sort_cap > 0 && wgs > chip.cus) ? win_cells_for(group, sort_cap, true, chip.lds_per_cu) : own_cells;",
        "const long wgs = (long)(split ? 2 * groups : groups) * L;",
        "if (left && right) { part[0] = 0x5u; part[1] = 0xAu; nph = 2; }",
        "else if (left) { part[0] = 0x5u; part[1] = 2u; part[2] = 8u; nph = 3; }",
        "else if (right) { part[0] = 1u; part[1] = 4u; part[2] = 0xAu; nph = 3; }",
        "else { part[0] = 1u; part[1] = 2u; part[2] = 4u; part[3] = 8u; nph = 4; }",
        "return (long)(o[2] - o[0] + 1) * ((o[3] - o[1] + 2) & ~1) <= win_cells;",
    ):
        assert line in flat, line


def test_benchmark_shape():
    """Group 16 x 360 beams: 88 704 bytes (one per CU) at kWinCells, 33 216 cells and two per CU in a chip-filling launch."""
    assert ws.win_lds_bytes(16, 5760, ws.WIN_CELLS) == 88704
    assert ws.win_lds_bytes(8, 2880, ws.WIN_CELLS) == 82560
    bench = ws.launch(999, 360, 16, L=32, split_pref=0)
    assert bench.wgs == 2016 and bench.two_per_cu and bench.win_cells == 33216
    assert 2 * bench.lds <= ws.LDS_PER_CU - 2 * ws.HALF_SLACK
    lone = ws.launch(999, 360, 16, L=1)                              # 63 groups: split, spread, today's window
    assert lone.split == 1 and lone.wgs == 126 and not lone.two_per_cu and lone.win_cells == ws.WIN_CELLS
    assert ws.launch(999, 360, 16, L=4, split_pref=0).win_cells == ws.WIN_CELLS         # 252 workgroups: one per CU
    assert ws.launch(999, 360, 16, L=5, split_pref=0).win_cells == 33216                # 315


@pytest.mark.parametrize("guard", [0, 512])
def test_capacity_sweep(guard):
    """Group 1..64 x beams 90 / 360 / 720 / 1080, with and without the chip-filling rule (and the debug build's guard)."""
    seen_two = 0
    for n in BEAMS:
        for group in range(1, ws.WIN_MAX_GROUP + 1):
            if group * n > 65535:
                continue
            cap = ws.win_sort_cap(group * n)
            old = ws.win_cells_for(group, cap, False, guard=guard)
            assert old >= ws.WIN_CELLS and old % 16 == 0
            for two in (False, True):
                cells = ws.win_cells_for(group, cap, two, guard=guard)
                assert cells % 16 == 0                               # whole 16-cell pieces (an even number: whole dwords)
                assert cells >= ws.TWO_FLOOR
                assert cells >= ws.win_sort_cap(group * n)           # pass 1 parks a 16-bit key per sorted ray in the window
                lds = ws.win_lds_bytes(group, cap, cells, guard)
                assert lds <= ws.LDS_PER_CU
                if cells != ws.WIN_CELLS:                            # carved for two per CU
                    assert 2 * (lds + ws.HALF_SLACK) <= ws.LDS_PER_CU, (group, n, cells)
                    seen_two += cells < ws.WIN_CELLS
                if not two:
                    assert cells == old
            # the launch rule: two per CU only for sorted rays in a launch of more workgroups than CUs
            for L, split in ((1, 0), (40, 0), (40, 1)):
                la = ws.launch(640, n, group, L=L, split_pref=split, guard=guard)
                if la.win_cells < ws.WIN_CELLS:
                    assert la.sort_cap > 0 and la.wgs > ws.CUS and la.two_per_cu
                    assert 2 * (la.lds + ws.HALF_SLACK) <= ws.LDS_PER_CU
                if la.sort_cap == 0 or la.wgs <= ws.CUS:
                    assert la.win_cells == ws.win_cells_for(group, la.sort_cap, False, guard=guard)
    assert seen_two > 50


def test_floor_is_reachable_and_binding():
    """The smallest carving any sorted launch can ask for (64 scans of 128 beams: 8 192 rays) is the floor itself, so every
    sorted chip-filling launch takes two per CU; one byte of LDS more per workgroup and it would not."""
    cells = ws.win_cells_for(64, ws.win_sort_cap(8192), True)
    assert cells == ws.TWO_FLOOR
    assert ws.win_cells_for(64, ws.win_sort_cap(8192), True, guard=512) == ws.WIN_CELLS     # (the guard build: below the floor)
    assert ws.win_cells_for(20, ws.win_sort_cap(7200), True) == 31680
    unsorted = ws.launch(9990, 360, 24, split_pref=0)                # 8 640 rays: not sorted, so not shrunk either
    assert unsorted.sort_cap == 0 and unsorted.wgs > ws.CUS and unsorted.win_cells == ws.win_cells_for(24, 0) >= ws.WIN_CELLS


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_benchmark_trajectory_phases(seed):
    """Groups of 16 scans of the benchmark trajectory, true poses: phase histogram under the old and the new capacity,
    with the two-then-four rule and the per-half rule.  Every part of every group fits its window."""
    slam = importlib.import_module("a-2d-lidar-based-slam-system-for-wheeled-mobile-robots_amd")
    rep = slam.synthetic.make_replay(1000, 360, seed=seed, stride=5)
    new_cells = ws.launch(999, 360, 16, L=32, split_pref=0).win_cells
    orgs, ends = ws.replay_cells(rep)
    boxes = [ws.box_cells(ws.plan(orgs[s:s + 16], ends[s:s + 16].reshape(-1, 2), 400, 400, 1 << 30).boxes[0]) for s in range(0, 999, 16)]
    print("seed %d: %d groups, boxes %d .. %d cells" % (seed, len(boxes), min(boxes), max(boxes)))
    hist = {}
    for cells in (ws.WIN_CELLS, new_cells, 32768):
        for name, rule in (("two-then-four", ws.plan_two_then_four), ("per-half", ws.plan)):
            plans = ws.replay_plans(rep, 16, cells, rule=rule)
            assert len(plans) == 63
            hist[cells, name] = Counter(len(p.parts) for p in plans)
            print("  window %5d cells, %-13s: %s" % (cells, name, dict(sorted(hist[cells, name].items()))))
            assert all(all(p.fits) for p in plans), "a part does not fit its window"
    assert min(boxes) > ws.WIN_CELLS                                 # every group is cut already
    if seed == 1:
        assert hist[ws.WIN_CELLS, "two-then-four"] == {2: 63}
        assert hist[33216, "two-then-four"] == {2: 46, 4: 17}
        assert hist[32768, "two-then-four"] == {2: 32, 4: 31}
    for cells in (ws.WIN_CELLS, new_cells, 32768):
        old, new = hist[cells, "two-then-four"], hist[cells, "per-half"]
        assert new[2] == old[2] and new[3] + new[4] == old[4]        # the per-half rule only turns fours into threes


def test_gpu_cases_launch_shapes():
    """What the cases of tests/test_gpu_window_two_per_cu.py rely on: 304 groups take the carving for two workgroups per CU,
    152 the old one."""
    import win_cases as wc
    assert wc.NEW.two_per_cu and wc.NEW.wgs == 304 and wc.CAP == 33216 and 2 * wc.NEW.lds <= ws.LDS_PER_CU
    assert not wc.OLD.two_per_cu and wc.OLD.wgs == 152 and wc.OLD.win_cells == ws.WIN_CELLS and 2 * wc.OLD.lds > ws.LDS_PER_CU
    assert wc.ROWS * 192 <= wc.CAP < (wc.ROWS + 1) * 192


@pytest.mark.parametrize("case", ["row_under", "row_over", "one_half_over", "both_halves_over", "quadrant_over",
                                  "odd_rows_one_half_over", "leaves_map"])
def test_gpu_cases_take_the_phases_they_are_about(case):
    """Every distinct group of a case: phases with the new and the old capacity, every part but the quadrants of
    quadrant_over fits its window, and the two workgroups of grid_split take one or two phases each."""
    import win_cases as wc
    assert list(wc.CASES) == ["row_under", "row_over", "one_half_over", "both_halves_over", "quadrant_over",
                              "odd_rows_one_half_over", "leaves_map"]
    (xw, yw, *_), _, _, (new_ph, old_ph) = wc.CASES[case]
    orgs, ends = wc.groups(case)
    for d in range(wc.DISTINCT):
        new, old = ws.plan(orgs[d], ends[d], xw, yw, wc.CAP), ws.plan(orgs[d], ends[d], xw, yw, ws.WIN_CELLS)
        assert (len(new.parts), len(old.parts)) == (new_ph, old_ph), (d, new, old)
        assert all(new.fits) == (case != "quadrant_over")
        halves = [ws.plan(orgs[d], ends[d], xw, yw, wc.CAP, half=h) for h in (0, 1)]
        assert sorted(len(h.parts) for h in halves) == {1: [1, 1], 2: [1, 1], 3: [1, 2], 4: [2, 2]}[new_ph]
        whole = ws.plan(orgs[d], ends[d], xw, yw, 1 << 30).boxes[0]
        if case in ("row_under", "row_over"):
            assert ws.box_cells(whole) == (wc.ROWS + (case == "row_over")) * 192
        if case == "leaves_map":
            assert whole[2] == xw - 1 and whole[3] == yw - 1
