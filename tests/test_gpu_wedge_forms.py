"""The two casts for maps much larger than an LDS window at their class, band and part edges: the direction wedges
(grid_mode 4, and 1 where the map is large enough for the library to pick them) and the recorded-walk tiles (2), with the
deterministic inputs of tests/wedge_cases.py (what those inputs reach is checked without a GPU in test_wedge_cases.py).

A: slopes on and one cell either side of every class boundary, exact diagonals, lengths 0, 1 .. 400, both walk directions.
B: several bands of the full 512 rows; bands cut down to what the window holds; bands by direct atomics before bands that
fit.  C: units of 2 048, 2 064 and 4 160 rays (1, 2, 3 parts) and groups of 7 and 2 scans.  D: rows of an odd number of
cells (the per-cell flush), the map's corners and its last row and column.  E: sides of 65 535 (the last the wedges take)
and 65 536 (tiles under every mode).  F: a map per trajectory where the maps hold an odd number of cells, so that map 1
starts at 4 mod 8 bytes (the 64-bit pair flush must go by the parity of the address, not of the cell in its map).

Every case on a context of its own, two passes (the second adds to non-zero counters), the status checked after every
call; pass, hit and pmap bit-equal to the oracle's, the visit counts equal; for F iteration counts exact, poses and
transforms to 1e-9, the maps that no trajectory names untouched."""
import functools

import numpy as np
import pytest

import wedge_cases as K
from conftest import pkg
from oracle import c_oracle as co
from oracle import checks

pytestmark = pytest.mark.gpu
FTOL = 1e-9
PASSES = 2

CASES = {
    "A_class_boundaries": K.case_a,
    "B1_full_bands": K.case_b1,
    "B1_full_bands_steep": lambda: K.transposed(K.case_b1()),
    "B2_cut_bands": K.case_b2,
    "B3_direct_then_fit": K.case_b3,
    "C_one_part": lambda: K.case_c(*K.C_CASES["one_part"]),
    "C_two_parts": lambda: K.case_c(*K.C_CASES["two_parts"]),
    "C_three_parts": lambda: K.case_c(*K.C_CASES["three_parts"]),
    "C_ragged_groups": lambda: K.case_c(*K.C_CASES["ragged_groups"]),
    "D_601x601": lambda: K.case_d(601, 601),
    "D_600x601": lambda: K.case_d(600, 601),
    "D_601x600": lambda: K.case_d(601, 600),
    "E_side_65535": lambda: K.case_e(65535),
    "E_side_65536": lambda: K.case_e(65536),
}


def modes_of(case):
    """4 always; 1 where the map is large (the library then picks the wedges itself); 2: the tiles, same inputs."""
    xw, yw = case["dims"][:2]
    return [4] + ([1] if xw * yw > 8 * K.KWIN_CELLS else []) + [2]


PARAMS = [(name, mode) for name, build in CASES.items() for mode in modes_of(build())]


@pytest.fixture(scope="module")
def slam():
    p = pkg()
    p._abi.default_context()
    return p


@functools.lru_cache(maxsize=1)
def reference(name):
    """The case, its coordinates, and the oracle's (pass, hit, pmap, visits) after each pass."""
    case = CASES[name]()
    xw, yw, scale, off_x, off_y = case["dims"]
    OX, OY, CX, CY = K.world(case)
    og = co.Grid(xw, yw, scale, off_x, off_y)
    after = []
    for _ in range(PASSES):
        for b in range(len(CX)):
            og.update(OX[b], OY[b], CX[b], CY[b])
        after.append((og.pass_cnt.copy(), og.hit_cnt.copy(), og.pmap.copy(), og.visits))
    return case, (OX, OY, CX, CY), after


@pytest.mark.parametrize("name,mode", PARAMS, ids=["%s-mode%d" % p for p in PARAMS])
def test_explicit_scans(slam, name, mode):
    case, (OX, OY, CX, CY), after = reference(name)
    xw, yw, scale, off_x, off_y = case["dims"]
    ctx = slam.Context(0)
    ctx.set_option("grid_mode", mode)
    ctx.set_option("grid_group", case["group"])
    g = slam.DeviceGrid(1, xw, yw, scale, off_x, off_y, context=ctx)
    try:
        for k, (opass, ohit, opmap, ovisits) in enumerate(after):
            g.update_host(OX, OY, CX, CY)
            ctx.check_status()                                       # (an LDS-guard overrun of a mis-sized band shows here)
            r = g.read(0, want=("pmap", "pass", "hit"))
            bad = np.argwhere(r["pass"] != opass)
            assert len(bad) == 0, (k, len(bad), bad[:4].tolist(), r["pass"][tuple(bad[0])], opass[tuple(bad[0])])
            assert np.array_equal(r["hit"], ohit), (k, int(np.sum(r["hit"] != ohit)))
            assert np.array_equal(r["pmap"], opmap), (k, int(np.sum(r["pmap"] != opmap)))
            assert g.visits() == ovisits, (k, g.visits(), ovisits)
    finally:
        g.close()
        ctx.close()


@functools.lru_cache(maxsize=1)
def reference_f(route):
    """Per map the oracle's counters after each pass ({map: [(pass, hit, pmap)]}), per trajectory (poses, T, iters), and
    the visits of all trajectories after each pass."""
    ranges = K.case_f(pkg("synthetic"))
    grids = {m: checks.metric_grid(K.F_SIDE, K.F_SIDE, K.F_RESO) for m in range(K.F_MAPS)}
    after, traj, visits, total = {m: [] for m in grids}, {}, [], 0
    for _ in range(PASSES):
        for l, m in enumerate(route):
            op, oT, oit, v = checks.replay_reference(ranges[l], K.F_AMIN, K.F_AMAX, grids[m], pose0=tuple(K.F_POSE0[l]), threads=4)
            traj[l] = (op, oT, oit)
            total += v
        visits.append(total)
        for m, og in grids.items():
            after[m].append((og.pass_cnt.copy(), og.hit_cnt.copy(), og.pmap.copy()))
    return ranges, after, traj, visits


@pytest.mark.parametrize("mode", [1, 4])
@pytest.mark.parametrize("route", [tuple(r) for r in K.F_ROUTES], ids=["maps_2_1_0", "maps_1_1_0"])
def test_map_per_trajectory_at_odd_offsets(slam, route, mode):
    ranges, after, traj, visits = reference_f(route)
    ctx = slam.Context(0)
    ctx.set_option("grid_mode", mode)
    grid = slam.DeviceGrid.metric(K.F_MAPS, K.F_SIDE, K.F_SIDE, K.F_RESO, context=ctx)
    try:
        for k in range(PASSES):
            poses, T, it = slam.replay_host(ranges, K.F_AMIN, K.F_AMAX, grid=grid, pose0=K.F_POSE0, grid_of_traj=list(route), context=ctx)
            ctx.check_status()
            for l in range(K.F_MAPS):
                op, oT, oit = traj[l]
                assert np.array_equal(it[l], oit), (k, l)
                assert np.max(np.abs(poses[l] - op)) < FTOL and np.max(np.abs(T[l] - oT)) < FTOL, (k, l)
            for m in range(K.F_MAPS):
                opass, ohit, opmap = after[m][k]
                r = grid.read(m, want=("pmap", "pass", "hit"))
                # a count that leaks over a map's boundary lands in its neighbour's first or last cell
                for cell in ((0, 0), (K.F_SIDE - 1, K.F_SIDE - 1)):
                    assert r["pass"][cell] == opass[cell] and r["hit"][cell] == ohit[cell], (k, m, cell)
                assert np.array_equal(r["pass"], opass), (k, m, int(np.sum(r["pass"] != opass)))
                assert np.array_equal(r["hit"], ohit), (k, m, int(np.sum(r["hit"] != ohit)))
                assert np.array_equal(r["pmap"], opmap), (k, m)
                if m not in route:                                   # a map that no trajectory names stays as it was made
                    assert not r["pass"].any() and not r["hit"].any() and np.all(r["pmap"] == 50), (k, m)
            assert grid.visits() == visits[k], (k, grid.visits(), visits[k])
    finally:
        grid.close()
        ctx.close()
