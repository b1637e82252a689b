"""The window ray cast's launch decision and phase rule as the library answers for them (tests/win_shapes.py: slam_plan_win,
slam_plan_win_phases, slam_plan_query): the kernel form of a launch, the window's capacity over every group size, and
the phases of the benchmark trajectory under the old and the new capacity.  No GPU."""
import importlib
from collections import Counter

import pytest

import win_shapes as ws

BEAMS = (90, 360, 720, 1080)


@pytest.mark.parametrize("yw", [400, 401])
@pytest.mark.parametrize("redo", [False, True])
def test_forms_of_the_maps_only_writer(yw, redo):
    """One scan into a map that is the workgroup's own (live pmap, a map per stream, one hit occupies): the byte-window
    kernel with its re-do launch up to 384 beams where the grid has a re-do list, one ray per lane up to 512 beams, two up
    to 1 024, the general owner kernel beyond - and for rows that are no multiple of 16 cells (401)."""
    want = {384: "Owner8ThenRedo" if redo else "Owner1", 385: "Owner1", 512: "Owner1", 513: "Owner2", 1024: "Owner2", 1025: "Own"}
    for n, form in want.items():
        p = ws.plan_win(1, n, 1, L=32, pmap_live=True, private=True, hit_levels=1, xw=400, yw=yw, redo=redo)
        assert p.form == (form if yw == 400 else "Own"), (n, p)
        assert p.exclusive and not p.live_dirty and not p.split and not p.lds_hits
        if p.form == "Own":
            assert (p.grid_x, p.grid_y, p.threads) == (1, 32, ws.MIN_THREADS)
        else:
            assert (p.grid_x, p.grid_y, p.threads) == (1, 32, ws.query("kOwnerThreads")) and p.lds_attr == 0
            assert p.win_cells == ws.win_cells_for(1, p.sort_cap) >= yw and p.lds == ws.win_lds_bytes(1, p.sort_cap, p.win_cells)
        if p.form == "Owner8ThenRedo":
            assert p.redo_grid == 32 and p.own8_lds == ws.query("kOwn8LdsBytes") == ws.LDS_PER_CU // 2
            assert p.own8_win == p.own8_lds - ws.query("own8_fixed_bytes", ws.query("kOwn8Threads"))
            assert ws.plan_win(1, n, 1, L=1000, pmap_live=True, private=True, xw=400, yw=yw, redo=True).redo_grid == 256
    # three hit levels, or several scans to the workgroup: the general owner kernel
    assert ws.plan_win(1, 360, 1, pmap_live=True, hit_levels=3, redo=redo).form == "Own"
    assert ws.plan_win(4, 360, 4, pmap_live=True, redo=redo).form == "Own"


def test_launches_that_are_not_exclusive():
    """Three hit levels alone do not make a launch shared; a map named by the caller, or several streams into one map, do:
    the shared-map kernel, and the live pmap is left behind."""
    own = dict(pmap_live=True, xw=400, yw=400)
    assert ws.plan_win(1, 360, 1, L=8, private=True, hit_levels=2, **own).form == "Own"
    for p in (ws.plan_win(1, 360, 1, L=8, private=True, hit_levels=2, got=True, **own), ws.plan_win(1, 360, 1, got=True, **own),
              ws.plan_win(1, 360, 1, L=2, private=False, **own), ws.plan_win(2, 360, 1, **own)):
        assert p.form == "Win" and not p.exclusive and p.live_dirty
    assert ws.plan_win(1, 360, 1, L=2, private=True, **own).exclusive and ws.plan_win(1, 360, 1, L=1, **own).exclusive
    assert not ws.plan_win(1, 360, 1, L=2).live_dirty                  # (no live pmap: nothing to leave behind)


def test_threads_hits_and_the_spreading_request():
    """Threads: a lane per four rays in whole waves, 512 at least (one scan of 90 beams), 1 024 at most (from 4 096 rays).
    Hits in the window: by default exactly in sorted launches of more workgroups than CUs; "win_lds_hits" 1 in every
    sorted launch, 0 in none.  The spreading request, half a CU's LDS and 512 bytes, exactly in split launches of at most
    a workgroup per CU whose own need is at most half a CU's."""
    assert ws.plan_win(1, 90, 1).threads == ws.plan_win(8, 256, 8).threads == 512 and ws.plan_win(9, 228, 9).threads == 576
    assert ws.plan_win(16, 256, 16).threads == ws.plan_win(64, 1000, 64).threads == 1024
    half = ws.LDS_PER_CU // 2
    seen = Counter()
    for n in BEAMS:
        for group in (1, 2, 7, 8, 16, 22, 24, 64):
            if group * n > 65535:
                continue
            for scans, L in ((group, 1), (40 * group, 1), (192 * group, 1), (193 * group, 1), (256 * group, 1), (257 * group, 1), (999, 32)):
                for split_pref in (-1, 0, 1):
                    p = ws.plan_win(scans, n, group, L=L, split_pref=split_pref)
                    groups = -(-scans // group)
                    assert p.split == int(p.sort_cap > 0 and (split_pref > 0 or (split_pref < 0 and groups * L <= 3 * ws.CUS // 4)))
                    assert p.wgs == (2 if p.split else 1) * groups * L == p.grid_x * p.grid_y
                    assert p.lds_hits == int(p.sort_cap > 0 and p.wgs > ws.CUS)
                    for pref in (0, 1):
                        q = ws.plan_win(scans, n, group, L=L, split_pref=split_pref, hits_pref=pref)
                        assert q.lds_hits == int(pref and p.sort_cap > 0) and q._replace(lds_hits=p.lds_hits) == p
                    need = ws.win_lds_bytes(group, p.sort_cap, p.win_cells)
                    spread = bool(p.split) and p.wgs <= ws.CUS and need <= half
                    assert p.lds == (half + 512 if spread else need) and p.lds_attr == (p.lds if p.lds > ws.query("win_lds_max") else 0)
                    seen[spread, bool(p.lds_hits), bool(p.lds_attr)] += 1
    assert all(seen[k] for k in ((True, False, False), (False, True, False), (False, False, False))) and len(seen) == 3, seen
    # on this chip no launch needs more than the standing allowance; the spreading request of a chip with more LDS does
    big = ws.plan_win(40 * 8, 360, 8, lds_per_cu=256 * 1024)
    assert big.split and big.lds == big.lds_attr == 128 * 1024 + 512 > ws.query("win_lds_max")


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
