"""The cases of tests/test_gpu_window_two_per_cu.py: groups of 16 scans of 360 beams whose boxes sit at the edges of the
window that a chip-filling launch carves for two workgroups per CU (tests/win_shapes.py).  Test infrastructure only;
tests/test_win_shapes_cpu.py asserts, without a GPU, that every group takes the phases its case is about.

A launch is 304 groups - 19 distinct ones, 16 times over - of scans 2 - 3 cells apart; the end cells lie on a ring
around the origins, so that every octant occurs, and the ring's corners pin the box."""
import numpy as np

import win_shapes as ws

GROUP, BEAMS, DISTINCT, REPEAT = 16, 360, 19, 16
SCANS = GROUP * DISTINCT * REPEAT                                    # 4 864 scans, 304 groups
STD = (440, 400, 20.0, 11.0, 10.0)                                 # xw, yw, scale, off_x, off_y
ODD = (440, 401, 20.0, 11.0, 10.0)                                 # rows of an odd number of cells
BIG = (640, 640, 20.0, 16.0, 16.0)
NEW = ws.launch(SCANS, BEAMS, GROUP, split_pref=0)                  # 304 workgroups: carved for two per CU
OLD = ws.launch(SCANS // 2, BEAMS, GROUP, split_pref=0)             # 152: one per CU, the old capacity
CAP = NEW.win_cells
ROWS = CAP // 192                                                    # window rows of 192 cells that fit: 173

# the 16 origins of a group, relative to its first: 2 - 3 cells apart, 8 x 10 cells in all
OFFS = [(2 * (k % 4) + (k // 4) % 2, 3 * (k // 4)) for k in range(GROUP)]


def _border(x_lo, x_hi, y_lo, y_hi, step):
    """Cells on the border of the box, all four sides, corners included."""
    xs, ys = sorted(set(range(x_lo, x_hi, step)) | {x_hi}), sorted(set(range(y_lo, y_hi, step)) | {y_hi})
    return [(x, y_lo) for x in xs] + [(x, y_hi) for x in xs] + [(x_lo, y) for y in ys] + [(x_hi, y) for y in ys]


def ring(org, x_lo, x_hi, y_lo, y_hi, step):
    """BEAMS end cells: the border of the box, every step-th cell and the corners - these pin the group's box -, and for the
    rest of the beams the border of a small box around the origins (12 cells from their middle: short rays, which keep
    the reference's work down; the long ones still reach every part of the box from 16 origins)."""
    far = _border(x_lo, x_hi, y_lo, y_hi, step)
    near = _border(org[0] - 8, org[0] + 16, org[1] - 7, org[1] + 17, 1)
    assert 80 <= len(far) < BEAMS
    cells = far + (near * (BEAMS // len(near) + 1))[:BEAMS - len(far)]
    return [cells[(k * 7) % BEAMS] for k in range(BEAMS)]           # (7 and 360 are coprime: long and short rays interleaved)


# name: map, first origin of the first group, end cells, phases of a group cast by one workgroup (new capacity, old capacity)
ORG = (212, 190)
CASES = {
    "row_under": (STD, ORG, ring(ORG, 130, 130 + ROWS - 1, 100, 291, 3), (1, 1)),        # 173 x 192 = the capacity
    "row_over": (STD, ORG, ring(ORG, 130, 130 + ROWS, 100, 291, 3), (2, 1)),             # 174 x 192: two halves
    "one_half_over": (STD, ORG, ring(ORG, 40, 303, 100, 291, 6), (3, 2)),                # left of the origins ~180 x 192, right ~90
    "both_halves_over": (STD, ORG, ring(ORG, 24, 414, 100, 291, 8), (4, 4)),
    "quadrant_over": (BIG, (316, 315), ring((316, 315), 20, 620, 20, 620, 28), (4, 4)),  # ~300 x 300 a quadrant: sub-rectangle
    "odd_rows_one_half_over": (ODD, ORG, ring(ORG, 40, 303, 100, 291, 6), (3, 2)),
    "leaves_map": (STD, (300, 290), ring((300, 290), 169, 500, 189, 460, 8), (2, 2)),    # clipped at x = 439 and y = 399
}


def groups(case):
    """Origin cells [DISTINCT, GROUP, 2] and end cells [DISTINCT, BEAMS, 2]: group d is the first one moved by a cell or
    two, its beams rotated by 7 d."""
    _, org, cells, _ = CASES[case]
    orgs = np.array([[(org[0] + d % 3 + dx, org[1] + d % 2 + dy) for dx, dy in OFFS] for d in range(DISTINCT)])
    ends = np.array([np.roll(np.array(cells), -7 * d, axis=0) for d in range(DISTINCT)])
    return orgs, ends


def scans(case):
    """Every scan of the launch, in world coordinates (cell centres): ox, oy [SCANS, BEAMS], cx, cy [SCANS]; scan s of
    a group has its beams rotated by s."""
    _, _, scale, off_x, off_y = CASES[case][0]
    orgs, ends = groups(case)
    ends = np.stack([np.stack([np.roll(ends[d], -s, axis=0) for s in range(GROUP)]) for d in range(DISTINCT)])   # [D, G, n, 2]
    OX = np.tile(((ends[..., 0] + 0.5) / scale - off_x).reshape(-1, BEAMS), (REPEAT, 1))
    OY = np.tile(((ends[..., 1] + 0.5) / scale - off_y).reshape(-1, BEAMS), (REPEAT, 1))
    CX = np.tile(((orgs[..., 0] + 0.5) / scale - off_x).reshape(-1), REPEAT)
    CY = np.tile(((orgs[..., 1] + 0.5) / scale - off_y).reshape(-1), REPEAT)
    return OX, OY, CX, CY
