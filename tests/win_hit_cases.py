"""The small cases of tests/test_gpu_window_hits.py: explicit end cells for the shared-map window kernel
(k_grid_update_win) that are about where the HITS of a group fall - piled up in one cell, in cells other rays pass
through, on the window's edges, outside the window or the map, nowhere (an empty path) - and the oracle's map for any
case, computed once.  Test infrastructure only; the chip-filling cases come from tests/win_cases.py."""
import numpy as np

from oracle import c_oracle as co

STD = (440, 400, 20.0, 11.0, 10.0)                                 # xw, yw, scale, off_x, off_y
ORG = (212, 190)
BEAMS = 360


def origins(count, org=ORG):
    """`count` origin cells 2 - 3 cells apart, four to a row."""
    return [(org[0] + 2 * (k % 4) + (k // 4) % 2, org[1] + 3 * (k // 4)) for k in range(count)]


def ring(x_lo, x_hi, y_lo, y_hi, step):
    """Cells on the border of the box, all four sides; the corners are in it when step divides both sides."""
    xs, ys = range(x_lo, x_hi + 1, step), range(y_lo, y_hi + 1, step)
    return [(x, y_lo) for x in xs] + [(x, y_hi) for x in xs] + [(x_lo, y) for y in ys] + [(x_hi, y) for y in ys]


def fit(cells, n):
    """Exactly n end cells: the list repeated as often as it takes."""
    return (cells * (n // len(cells) + 1))[:n]


def scans(dims, orgs, ends):
    """ends: [n] cells shared by every scan (each scan's beams rotated by its number), or [B][n] cells as they stand.
    World coordinates of the cell centres: ox, oy [B, n], cx, cy [B]."""
    _, _, scale, off_x, off_y = dims
    e = np.array(ends)
    if e.ndim == 2:
        e = np.stack([np.roll(e, -b, axis=0) for b in range(len(orgs))])
    o = np.array(orgs)
    return ((e[..., 0] + 0.5) / scale - off_x, (e[..., 1] + 0.5) / scale - off_y,
            (o[:, 0] + 0.5) / scale - off_x, (o[:, 1] + 0.5) / scale - off_y)


def pile_up(count, beams, cell):
    """Every ray of `count` scans ends in one cell."""
    return scans(STD, origins(count), [[cell] * beams] * count)


def shared_cells():
    """16 scans to end cells 10 .. 54 cells from the first origin in eight directions: the longer rays of a direction
    pass through the end cells of the shorter ones (exactly so for the first scan's axis-parallel and diagonal rays).
    Five beams of every scan end in the scan's own origin cell: an empty path, no hit."""
    orgs = origins(16)
    dirs = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]
    cells = [(ORG[0] + d * ux, ORG[1] + d * uy) for d in range(10, 55) for ux, uy in dirs]
    ends = [list(np.roll(np.array(cells), -b, axis=0)) for b in range(16)]
    for b in range(16):
        for i in range(40, 360, 70):
            ends[b][i] = orgs[b]
    return scans(STD, orgs, [[tuple(c) for c in e] for e in ends])


def hit_levels():
    """16 scans whose end cells take 16 hits, 2 hits and 1 hit a pass (three hit levels: hit_inc 4)."""
    orgs = origins(16)
    ends = [[(260, 130 + i) if i < 120 else (270 + b // 2, 130 + i - 120) if i < 240 else (285 + b, 130 + i - 240)
             for i in range(BEAMS)] for b in range(16)]
    return scans(STD, orgs, ends)


# name: (scans, grid_group).  Windows are the clamped box of origins and end cells, its first column moved to an even y.
EDGES_EVEN = fit(ring(150, 290, 120, 280, 2), BEAMS)                # 141 x 161 cells: one window, hits on all four edges
EDGES_ODD = fit(ring(151, 289, 121, 281, 2), BEAMS)                 # first column y = 121: the window starts at 120
OUTSIDE = fit(ring(-60, 500, -40, 450, 10) + ring(150, 290, 120, 280, 4), BEAMS)   # half the ends beyond the map
SMALL = {
    "pile_up_16x360": (lambda: pile_up(16, 360, (262, 231)), 16),
    "pile_up_64x128": (lambda: pile_up(64, 128, (150, 171)), 64),   # 8 192 rays: the largest sorted group
    "shared_cells": (shared_cells, 16),
    "edges_even": (lambda: scans(STD, origins(16), EDGES_EVEN), 16),
    "edges_odd": (lambda: scans(STD, origins(16), EDGES_ODD), 16),
    "ends_outside_map": (lambda: scans(STD, origins(16), OUTSIDE), 16),
    "unsorted_24x360": (lambda: scans(STD, origins(24), EDGES_EVEN), 24),   # 8 640 rays: not sorted, hits added directly
}

_REFERENCE = {}


def reference(key, dims, sc, hit_inc=20.0, stops=None):
    """The oracle's map after one and after two passes over the scans (computed once per key, never changed).
    stops: beams of every scan that the reference applies before it raises."""
    if key not in _REFERENCE:
        xw, yw, scale, off_x, off_y = dims
        OX, OY, CX, CY = sc
        og = co.Grid(xw, yw, scale, off_x, off_y, hit_inc=hit_inc)
        snaps = []
        for _ in range(2):
            for b in range(len(CX)):
                stop = OX.shape[1] if stops is None else stops[b]
                og.update(OX[b, :stop], OY[b, :stop], CX[b], CY[b])
            snaps.append({"pass": og.pass_cnt.copy(), "hit": og.hit_cnt.copy(), "pmap": og.pmap.copy(), "visits": og.visits})
        for s in snaps:
            for name in ("pass", "hit", "pmap"):
                s[name].setflags(write=False)
        _REFERENCE[key] = snaps
    return _REFERENCE[key]
