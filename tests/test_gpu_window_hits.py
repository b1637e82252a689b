"""Hits of the shared-map window kernel (k_grid_update_win) counted per end cell in the LDS window: context option
"win_lds_hits".  Sorted groups (up to 8 192 rays) park every ray's end cell while they walk, count the parked hits in
the window once the pass counts have left it, and send one global add per distinct end cell; everything else - end
cells outside a window that does not cover the rays' box, rays of a wave that walks the checked way, unsorted groups -
still adds its hits directly.

Every case is cast twice into the same map (grid_mode 3, no live pmap: the shared-map kernel), with the option at 0
and at 1 and with one and two workgroups per group (grid_split); pass, hit, pmap and the visit count must equal the
oracle's after each pass - one frozen reference per case, so the four variants are bit-equal to each other as well.

Small cases (tests/win_hit_cases.py), one group in one launch: all rays of 16 x 360 and of 64 x 128 (the largest
sorted group) ending in one cell; end cells that other rays pass through, and empty paths (end cell = origin cell: no
hit); end cells on the window's first and last row and column, with the window's first column at an even and at an odd
y; half the end cells outside the map; a NaN beam mid-scan (the beams behind it leave no hit, the error is the same);
24 x 360 rays, unsorted; three hit levels (hit_inc 4) with cells of 1, 2 and 16 hits a pass.
Chip-filling cases (tests/win_cases.py: 304 groups of 16 x 360, the window carved for two workgroups per CU): boxes a
row under and over the capacity, one half over, both halves over - groups of 1, 2, 3 and 4 phases -, a quadrant over
(sub-rectangle: end cells outside the window), odd rows (32-bit flush), rays that leave the map.
A replay of two trajectories routed crosswise into two 601 x 601 maps: odd rows, and the second map starts at an odd
cell, so no 64-bit pair flush anywhere."""
import numpy as np
import pytest

import test_gpu_window_two_per_cu as two_per_cu                     # (its frozen references of the win_cases launches)
import win_cases as wc
import win_hit_cases as hc
from conftest import pkg
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu

AMIN, AMAX = -3.14159, 3.14159
VARIANTS = [(hits, split) for hits in (0, 1) for split in (0, 1)]


@pytest.fixture(scope="module")
def slam():
    p = pkg()
    p._abi.default_context()
    return p


def _context(slam, group, hits, split):
    ctx = slam.Context(0)
    ctx.set_option("grid_mode", 3)
    ctx.set_option("grid_group", group)
    ctx.set_option("grid_split", split)
    ctx.set_option("win_lds_hits", hits)
    return ctx


def _cast(slam, dims, scans, group, hits, split, ref, hit_inc=20.0, raises=False):
    """Cast the scans twice into one map and compare everything with the reference after each pass."""
    xw, yw, scale, off_x, off_y = dims
    OX, OY, CX, CY = scans
    ctx = _context(slam, group, hits, split)
    g = slam.DeviceGrid(1, xw, yw, scale, off_x, off_y, hit_inc=hit_inc, context=ctx)
    for k in range(2):
        if raises:
            with pytest.raises(ValueError):
                g.update_host(OX, OY, CX, CY)
        else:
            g.update_host(OX, OY, CX, CY)
            ctx.check_status()
        r = g.read(0, want=("pmap", "pass", "hit"))
        assert np.array_equal(r["pass"], ref[k]["pass"]), (k, int(np.sum(r["pass"] != ref[k]["pass"])))
        assert np.array_equal(r["hit"], ref[k]["hit"]), (k, int(np.sum(r["hit"] != ref[k]["hit"])))
        assert np.array_equal(r["pmap"], ref[k]["pmap"]), (k, int(np.sum(r["pmap"] != ref[k]["pmap"])))
        assert g.visits() == ref[k]["visits"], k
    g.close()
    ctx.close()


@pytest.mark.parametrize("hits,split", VARIANTS)
@pytest.mark.parametrize("case", list(hc.SMALL))
def test_one_group(slam, case, hits, split):
    make, group = hc.SMALL[case]
    scans = make()
    ref = hc.reference(case, hc.STD, scans)
    if case.startswith("pile_up"):
        rays = scans[0].size
        assert ref[0]["hit"].max() == rays and np.count_nonzero(ref[0]["hit"]) == 1 and ref[1]["hit"].max() == 2 * rays
    if case == "shared_cells":
        assert np.count_nonzero((ref[0]["hit"] > 0) & (ref[0]["pass"] > 0)) >= 300     # cells that are both
        assert ref[0]["hit"].sum() == 16 * 355                                          # five empty paths a scan
    if case == "ends_outside_map":
        assert 16 * 100 < ref[0]["hit"].sum() < 16 * 260
    _cast(slam, hc.STD, scans, group, hits, split, ref)


@pytest.mark.parametrize("hits,split", VARIANTS)
def test_nan_beam(slam, hits, split):
    """A NaN coordinate in the middle of the sixth scan: ValueError with or without the option, and of that scan only
    the beams before it are applied."""
    OX, OY, CX, CY = hc.scans(hc.STD, hc.origins(16), hc.EDGES_EVEN)
    OY = OY.copy()
    OY[5, 180] = np.nan
    OY[5, 187] = np.nan                                             # never reached
    stops = [hc.BEAMS] * 16
    stops[5] = 180
    ref = hc.reference("nan_beam", hc.STD, (OX, OY, CX, CY), stops=stops)
    assert ref[0]["hit"].sum() == 16 * hc.BEAMS - 180
    _cast(slam, hc.STD, (OX, OY, CX, CY), 16, hits, split, ref, raises=True)


@pytest.mark.parametrize("hits,split", VARIANTS)
def test_three_hit_levels(slam, hits, split):
    """hit_inc 4: a cell is occupied from its third hit on, so pmap depends on the exact hit counts."""
    scans = hc.hit_levels()
    ref = hc.reference("hit_levels", hc.STD, scans, hit_inc=4.0)
    counts = set(np.unique(ref[0]["hit"]))
    assert {1, 2, 16} <= counts
    _cast(slam, hc.STD, scans, 16, hits, split, ref, hit_inc=4.0)


@pytest.mark.parametrize("hits,split", VARIANTS)
@pytest.mark.parametrize("case", list(wc.CASES))
def test_chip_filling_launch(slam, case, hits, split):
    """304 groups in one launch: the window of 33 216 cells, groups of one to four phases, sub-rectangles."""
    _cast(slam, wc.CASES[case][0], wc.scans(case), wc.GROUP, hits, split, two_per_cu._reference(case))


_REPLAY = {}


def _replay_reference(syn):
    if not _REPLAY:
        ranges = np.stack([syn.make_replay(49, 360, seed=40 + l, stride=5).ranges for l in range(2)])
        p0 = np.array([[0.0, 0.0, 0.0], [0.5, -0.5, 0.7]])
        ogs = [co.Grid(601, 601, 20.0, 15.0, 15.0) for _ in range(2)]
        snaps = []
        for _ in range(2):
            for l, gi in enumerate((1, 0)):
                co.replay(ranges[l], AMIN, AMAX, ogs[gi], pose0=p0[l])
            snaps.append([{"pass": og.pass_cnt.copy(), "hit": og.hit_cnt.copy(), "pmap": og.pmap.copy()} for og in ogs])
        _REPLAY.update(ranges=ranges, p0=p0, snaps=snaps)
    return _REPLAY


@pytest.mark.parametrize("hits,split", VARIANTS)
def test_odd_maps_routed_crosswise(slam, syn, hits, split):
    """Two trajectories of 48 scans, groups of 16, trajectory 0 into map 1 and trajectory 1 into map 0 of 601 x 601."""
    ref = _replay_reference(syn)
    ctx = _context(slam, 16, hits, split)
    grid = slam.DeviceGrid(2, 601, 601, 20.0, 15.0, 15.0, context=ctx)
    for k in range(2):
        slam.replay_host(ref["ranges"], AMIN, AMAX, grid=grid, pose0=ref["p0"], grid_of_traj=[1, 0], context=ctx)
        ctx.check_status()
        for gi in range(2):
            r = grid.read(gi, want=("pmap", "pass", "hit"))
            want = ref["snaps"][k][gi]
            assert np.array_equal(r["pass"], want["pass"]), (k, gi)
            assert np.array_equal(r["hit"], want["hit"]), (k, gi, int(np.sum(r["hit"] != want["hit"])))
            assert np.array_equal(r["pmap"], want["pmap"]), (k, gi)
    grid.close()
    ctx.close()
