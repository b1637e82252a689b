"""The two LDS-window group kernels (grid_mode 3), one deterministic case per form they take.

Shared map (k_grid_update_win: several workgroups write one map): one window, two direction halves, four
quadrants, a quadrant that does not fit (sub-rectangle + direct atomics), rays that leave the map, an origin
outside it, rows of an odd number of cells (32-bit flush), more rays than are sorted (one window, no
quadrants), a NaN beam, and a live pmap that the launch cannot keep current; each with one and with two
workgroups per group (grid_split).

Owned map (k_grid_update_own: live pmap, one workgroup is the map's only writer, and the launch is not one the
single-scan owner kernels take): several scans with the fused and with the scalar sweep, a box larger than the
window, and single scans of 1 204 rays (> 1 024) in the strip form - one strip, several, rays that leave the
map, an origin outside it -, with three hit levels (no strip form), and across the pass threshold.

The window holds 36 864 .. 40 288 cells; the boxes below are chosen against that.  Endpoints lie on rings
around the origins so that every octant, the endpoint swap and lines stepping towards -x occur.  Counters, pmap
and the visit count must equal the oracle's after each of two passes."""
import numpy as np
import pytest

from conftest import pkg
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu

STD = (440, 400, 20.0, 11.0, 10.0)                                 # xw, yw, scale, off_x, off_y
ODD = (440, 401, 20.0, 11.0, 10.0)                                 # rows of an odd number of cells
BIG = (640, 640, 20.0, 16.0, 16.0)


@pytest.fixture(scope="module")
def slam():
    p = pkg()
    p._abi.default_context()
    return p


def _ring(x_lo, x_hi, y_lo, y_hi, step=1):
    """Cells on the border of the box, all four sides."""
    cells = [(x, y_lo) for x in range(x_lo, x_hi + 1, step)] + [(x, y_hi) for x in range(x_lo, x_hi + 1, step)]
    cells += [(x_lo, y) for y in range(y_lo, y_hi + 1, step)] + [(x_hi, y) for y in range(y_lo, y_hi + 1, step)]
    return cells


def _fit(cells, n):
    """Exactly n end cells: the list repeated as often as it takes."""
    return (cells * (n // len(cells) + 1))[:n]


def _scans(dims, orgs, cells):
    """One scan per origin to the same end cells, each scan's beams rotated by its number: ox, oy [B, n], cx, cy [B]."""
    _, _, scale, off_x, off_y = dims
    ox = np.array([(c[0] + 0.5) / scale - off_x for c in cells])
    oy = np.array([(c[1] + 0.5) / scale - off_y for c in cells])
    OX = np.stack([np.roll(ox, -b) for b in range(len(orgs))])
    OY = np.stack([np.roll(oy, -b) for b in range(len(orgs))])
    CX = np.array([(o[0] + 0.5) / scale - off_x for o in orgs])
    CY = np.array([(o[1] + 0.5) / scale - off_y for o in orgs])
    return OX, OY, CX, CY


def _near(org, count):
    """`count` origins a few cells apart, the first one at org."""
    d = [(0, 0), (2, -2), (-2, 1), (1, 3), (-3, -1), (3, 2), (-1, -3), (2, 1), (-2, -2)]
    return [(org[0] + d[k][0], org[1] + d[k][1]) for k in range(count)]


def _box(r):
    t = r["pass"].astype(np.int64) + r["hit"]
    bx, by = np.nonzero(t.sum(axis=1))[0], np.nonzero(t.sum(axis=0))[0]
    return int(bx[-1] - bx[0] + 1), int(by[-1] - by[0] + 1)


def _cast(slam, dims, scans, group, split=-1, live=False, hit_inc=20.0, passes=2, box=None, stops=None):
    """Cast the scans `passes` times and compare everything with the oracle after each pass; returns the last
    read-back.  stops: beams of every scan that the reference applies before it raises (ValueError expected)."""
    xw, yw, scale, off_x, off_y = dims
    OX, OY, CX, CY = scans
    ctx = slam.Context(0)
    ctx.set_option("grid_mode", 3)
    ctx.set_option("grid_group", group)
    ctx.set_option("grid_split", split)
    g = slam.DeviceGrid(1, xw, yw, scale, off_x, off_y, hit_inc=hit_inc, context=ctx)
    if live:
        g.live_pmap()
    og = co.Grid(xw, yw, scale, off_x, off_y, hit_inc=hit_inc)
    for k in range(passes):
        if stops is None:
            g.update_host(OX, OY, CX, CY)
            ctx.check_status()
        else:
            with pytest.raises(ValueError):
                g.update_host(OX, OY, CX, CY)
        for b in range(len(CX)):
            stop = OX.shape[1] if stops is None else stops[b]
            og.update(OX[b, :stop], OY[b, :stop], CX[b], CY[b])
        r = g.read(0, want=("pmap", "pass", "hit"))
        assert np.array_equal(r["pass"], og.pass_cnt), (k, int(np.sum(r["pass"] != og.pass_cnt)))
        assert np.array_equal(r["hit"], og.hit_cnt), k
        assert np.array_equal(r["pmap"], og.pmap), (k, int(np.sum(r["pmap"] != og.pmap)))
        assert g.visits() == og.visits, k
    if box is not None:
        assert _box(r) == box                                       # the rays' box really has the stated shape
    g.close()
    ctx.close()
    return r


# name: map, first origin, end cells, box of the touched cells
SHARED = {
    "one_window": (STD, (215, 203), _ring(150, 290, 120, 280, 2), (141, 161)),
    "two_halves": (STD, (195, 195), _ring(60, 330, 90, 300, 3), (271, 211)),               # 271 x 212 > window, 136 x 212 fits
    "four_quadrants": (STD, (220, 200), _ring(20, 420, 30, 370, 4), (401, 341)),           # 201 x 342 > window, 201 x 172 fits
    "quadrant_too_large": (BIG, (320, 320), _ring(20, 620, 20, 620, 5), (601, 601)),       # 301 x 302 > window: sub-rectangle
    "leaves_map_two_sides": (STD, (304, 294), _ring(169, 500, 189, 460, 3), (271, 211)),   # clipped at x = 439 and y = 399: two halves
    "origin_outside": (STD, (-30, 180), _ring(40, 300, 100, 320, 4) + [(-50, 181), (-30, 181)], None),
    "odd_rows_one_window": (ODD, (215, 203), _ring(150, 290, 120, 280, 2), (141, 161)),
    "odd_rows_two_halves": (ODD, (195, 195), _ring(60, 330, 90, 300, 3), (271, 211)),
}


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("case", list(SHARED))
def test_shared_map_group_of_three(slam, case, split):
    """Three scans, one group, no live pmap: with grid_split 1 two workgroups share the group (by beam parity when its
    box fits one window, else by direction half, a half that does not fit cut again at the origins' row)."""
    dims, org, cells, box = SHARED[case]
    assert 200 <= len(cells) <= 800
    _cast(slam, dims, _scans(dims, _near(org, 3), cells), 3, split, box=box)


@pytest.mark.parametrize("case", ["one_window", "four_quadrants"])
def test_shared_map_unsorted_group(slam, case):
    """9 scans x 1 000 beams in one group: more rays than are sorted, so one window and no quadrants (a box larger
    than the window keeps a sub-rectangle), and grid_split changes nothing."""
    dims, org, cells, box = SHARED[case]
    dense = _ring(*{"one_window": (150, 290, 120, 280), "four_quadrants": (20, 420, 30, 370)}[case], 1)
    scans = _scans(dims, _near(org, 9), _fit(cells + dense, 1000))
    maps = [_cast(slam, dims, scans, 9, split, box=box) for split in (0, 1)]
    for name in ("pass", "hit", "pmap"):
        assert np.array_equal(maps[0][name], maps[1][name]), name


@pytest.mark.parametrize("split", [0, 1])
def test_shared_map_nan_beam(slam, split):
    """A NaN coordinate in the middle of the second scan: ValueError, and that scan's beams before it are applied."""
    dims, org, cells, _ = SHARED["two_halves"]
    OX, OY, CX, CY = _scans(dims, _near(org, 3), cells)
    n = OX.shape[1]
    OY[1, n // 2] = np.nan
    OY[1, n // 2 + 7] = np.nan                                      # never reached
    _cast(slam, dims, (OX, OY, CX, CY), 3, split, stops=[n, n // 2, n])


@pytest.mark.parametrize("split", [0, 1])
def test_shared_map_with_live_pmap(slam, split):
    """Six scans in two groups into a map with a live pmap: no workgroup owns the map, and the pmap read afterwards
    (brought up to date by the read) equals the oracle's."""
    dims, org, cells, box = SHARED["two_halves"]
    _cast(slam, dims, _scans(dims, _near(org, 6), cells), 3, split, live=True, box=box)


OWN_YW402 = (440, 402, 20.0, 11.0, 10.0)
OWNED_GROUP = {
    "fused_sweep": (STD, (215, 203), _ring(150, 290, 120, 280, 2), (141, 161)),            # rows of a multiple of 4 cells
    "scalar_sweep": (OWN_YW402, (215, 203), _ring(150, 290, 120, 280, 2), (141, 161)),
    "box_too_large": (STD, (220, 200), _ring(20, 420, 30, 370, 4), (401, 341)),            # sub-rectangle, sweep over the whole box
}


@pytest.mark.parametrize("case", list(OWNED_GROUP))
def test_owned_map_group_of_three(slam, case):
    """Three scans in one group (grid_group 64) into a map with a live pmap: one window, flush, then the sweep that
    re-thresholds pmap over the rays' whole box."""
    dims, org, cells, box = OWNED_GROUP[case]
    _cast(slam, dims, _scans(dims, _near(org, 3), cells), 64, live=True, box=box)


OWNED_SCAN = {
    "one_strip": ((215, 203), _ring(150, 290, 120, 280, 1), (141, 161)),
    "several_strips": ((220, 200), _ring(20, 420, 30, 370, 2) + _ring(21, 419, 31, 369, 3), (401, 341)),
    "leaves_map": ((215, 203), _ring(-60, 500, -40, 450, 2), None),
    "origin_outside": ((-30, 180), _ring(40, 300, 100, 320, 1) + [(-50, 181), (-30, 181)], None),
}


@pytest.mark.parametrize("case", list(OWNED_SCAN))
def test_owned_map_single_scan_strips(slam, case):
    """One scan of 1 204 rays - more than the single-scan owner kernels take - into a map with a live pmap: the strip
    form of the group kernel."""
    org, cells, box = OWNED_SCAN[case]
    _cast(slam, STD, _scans(STD, [org], _fit(cells, 1204)), 1, live=True, box=box)


def test_owned_map_single_scan_three_hit_levels(slam):
    """hit_inc 4: one hit does not occupy, so the strip form (which relies on that) is not taken: window, flush
    and fused sweep for a single scan of 1 204 rays."""
    org, cells, box = OWNED_SCAN["one_strip"]
    _cast(slam, STD, _scans(STD, [org], _fit(cells, 1204)), 1, live=True, hit_inc=4.0, box=box)


def test_owned_map_single_scan_pass_threshold(slam):
    """The strip sweep decides pmap from the live pmap's previous value and the new pass count: 300 rays along one line,
    so its cells cross the 1 001-pass threshold during the 4th scan, in scans padded to 1 204 rays by 904 copies of a
    short ray elsewhere; a cell hit once stays occupied when later only passed through."""
    ctx = slam.Context(0)
    ctx.set_option("grid_mode", 3)
    g = slam.DeviceGrid(1, 208, 208, 10.0, 10.0, 10.0, context=ctx)
    g.live_pmap()
    og = co.Grid(208, 208, 10.0, 10.0, 10.0)

    def step(ex, ey, count):
        ox = np.concatenate([np.full(count, ex), np.full(1204 - count, -0.25)])
        oy = np.concatenate([np.full(count, ey), np.full(1204 - count, -0.15)])
        g.update_host(ox, oy, 0.0, 0.0)
        og.update(ox, oy, 0.0, 0.0)
        r = g.read(0, want=("pmap", "pass", "hit"))
        assert np.array_equal(r["pass"], og.pass_cnt) and np.array_equal(r["hit"], og.hit_cnt)
        assert np.array_equal(r["pmap"], og.pmap) and g.visits() == og.visits
        return r

    for k in range(5):
        r = step(3.05, 1.55, 300)
        assert (r["pmap"][110, 105] == 100) == (k >= 3)              # a pass-through cell of the line
    # a shorter ray now ends (hits) in a cell that so far was only passed through, then longer rays pass through
    # that cell again: it stays occupied
    for ex in (-2.05, -3.05, -3.05):
        r = step(ex, 0.0, 1)
        assert r["pmap"][79, 100] == 100 and r["pmap"][85, 100] == 0
    assert r["hit"][79, 100] == 1 and r["pass"][79, 100] == 2 and r["hit"][69, 100] == 2
    ctx.check_status()
    g.close()
    ctx.close()
