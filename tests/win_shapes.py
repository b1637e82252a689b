"""Plain-Python restatement of how the LDS-window ray cast (launch_win / k_grid_update_win in csrc/grid_kernels.hip)
sizes its window and cuts a group's rays into phases.  Test infrastructure only: tests/test_win_shapes_cpu.py checks
it against the source text and sweeps it, tests/test_gpu_window_two_per_cu.py takes its box sizes from it.

What is restated:
  win_lds_bytes    dynamic LDS of a window workgroup: scan constants, control block, histogram, sorted order, window
  win_cells_for    the window's capacity in 16-bit cells: kWinCells; more for small groups (two workgroups still share
                   a CU); and, for a launch that wants two per CU (two_per_cu), the same carving even where it comes
                   out below kWinCells, down to kWinTwoFloor
  launch           which of the two a shared-map launch gets: two per CU only for sorted rays (sort_cap > 0) in a
                   launch of more workgroups than the chip has CUs
  plan             the phases of one workgroup: the box of everything if it fits, else per direction half (left /
                   right of the origins' column) one phase if the half fits and two (cut at the origins' row) if not
"""
from __future__ import annotations

import os
import re
from collections import namedtuple

import numpy as np

SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                      "a-2d-lidar-based-slam-system-for-wheeled-mobile-robots_amd", "csrc", "grid_kernels.hip")

WIN_CELLS = 36864              # kWinCells
WIN_MAX_GROUP = 64             # kWinMaxGroup
SORT_BINS = 128                # kSortBins
MAX_SORT_RAYS = 8192           # kMaxSortRays
WIN_BOX_INTS = 160             # kWinBoxInts
HALF_SLACK = 512               # kWinHalfSlack
TWO_FLOOR = 29632              # kWinTwoFloor
SCAN_CONST = 4 * 8 + 4 * 4     # sizeof(ScanConst): four doubles, four ints
LDS_PER_CU = 160 * 1024
CUS = 256

NAMES = {"kWinCells": "WIN_CELLS", "kWinMaxGroup": "WIN_MAX_GROUP", "kSortBins": "SORT_BINS", "kMaxSortRays": "MAX_SORT_RAYS",
         "kWinBoxInts": "WIN_BOX_INTS", "kWinHalfSlack": "HALF_SLACK", "kWinTwoFloor": "TWO_FLOOR"}


def source_constants(text=None):
    """The constants above as csrc/grid_kernels.hip states them: {Python name: value}."""
    if text is None:
        with open(SOURCE) as f:
            text = f.read()
    out = {}
    for c_name, py_name in NAMES.items():
        m = re.findall(r"constexpr int %s = (\d+);" % c_name, text)
        assert len(m) == 1, c_name
        out[py_name] = int(m[0])
    return out


def win_sc_bytes(group):
    return (group * SCAN_CONST + 15) & ~15


def win_sort_cap(rays):
    return (rays + 7) & ~7 if rays <= MAX_SORT_RAYS else 0


def win_lds_bytes(group, sort_cap, win_cells, guard=0):
    return win_sc_bytes(group) + WIN_BOX_INTS * 4 + 4 * SORT_BINS * 4 + sort_cap * 2 + win_cells * 2 + guard


def win_cells_for(group, sort_cap, two_per_cu=False, lds_per_cu=LDS_PER_CU, guard=0):
    half = lds_per_cu // 2 - HALF_SLACK
    cells = ((half - win_lds_bytes(group, sort_cap, 0, guard)) // 2) & ~15
    if cells > WIN_CELLS:
        return cells
    return cells if two_per_cu and cells >= TWO_FLOOR else WIN_CELLS


Launch = namedtuple("Launch", "group sort_cap split wgs two_per_cu win_cells lds")


def launch(scans, n, group, L=1, split_pref=-1, cus=CUS, lds_per_cu=LDS_PER_CU, guard=0):
    """A shared-map launch (k_grid_update_win) of L streams of `scans` scans of n beams in groups of `group`."""
    groups = (scans + group - 1) // group
    sort_cap = win_sort_cap(group * n)
    split = int(sort_cap > 0 and (split_pref > 0 or (split_pref < 0 and groups * L <= 3 * cus // 4)))
    wgs = (2 * groups if split else groups) * L
    two = sort_cap > 0 and wgs > cus
    cells = win_cells_for(group, sort_cap, two, lds_per_cu, guard)
    lds = win_lds_bytes(group, sort_cap, cells, guard)
    half_cu = lds_per_cu // 2
    if split and wgs <= cus and lds <= half_cu and half_cu + 512 <= lds_per_cu:
        lds = half_cu + 512                                          # the spreading request of a lone launch
    return Launch(group, sort_cap, split, wgs, two, cells, lds)


# ---- phases -------------------------------------------------------------------------------------------------------

def _clamp(box, xw, yw, ymask):
    """clamp_box: None where nothing of the box is in the map."""
    x0, y0, x1, y1 = max(box[0], 0), max(box[1], 0), min(box[2], xw - 1), min(box[3], yw - 1)
    y0 &= ~ymask
    return (x0, y0, x1, y1) if x0 <= x1 and y0 <= y1 else None


def box_cells(box):
    """Window cells a clamped box takes: rows are stored padded to an even height."""
    return (box[2] - box[0] + 1) * ((box[3] - box[1] + 2) & ~1)


Plan = namedtuple("Plan", "parts boxes fits")      # per phase: quadrant mask, clamped box (None: empty), whether it fits


def plan(orgs, ends, xw, yw, win_cells, half=None, sorted_rays=True, even_rows=None, per_half=True):
    """Phases of a workgroup for scans with origin cells orgs [S, 2] and end cells ends [R, 2] (all of the group's valid
    rays).  half: None for one workgroup per group, 0 / 1 for the two of grid_split.  per_half False: the earlier rule
    of the unsplit form (both halves fit, or four quadrants)."""
    orgs, ends = np.asarray(orgs), np.asarray(ends)
    ymask = 1 if (yw % 2 == 0 if even_rows is None else even_rows) else 0
    bb = (min(orgs[:, 0].min(), ends[:, 0].min()), min(orgs[:, 1].min(), ends[:, 1].min()),
          max(orgs[:, 0].max(), ends[:, 0].max()), max(orgs[:, 1].max(), ends[:, 1].max()))
    ox0, oy0, ox1, oy1 = orgs[:, 0].min(), orgs[:, 1].min(), orgs[:, 0].max(), orgs[:, 1].max()
    qbox = []
    for q in range(4):
        qbox.append((max(ox0, bb[0]) if q & 1 else bb[0], max(oy0, bb[1]) if q & 2 else bb[1],
                     bb[2] if q & 1 else min(ox1, bb[2]), bb[3] if q & 2 else min(oy1, bb[3])))

    def box_of(mask):
        bs = [qbox[q] for q in range(4) if mask >> q & 1 and qbox[q][0] <= qbox[q][2]]
        if not bs:
            return None
        return _clamp((min(b[0] for b in bs), min(b[1] for b in bs), max(b[2] for b in bs), max(b[3] for b in bs)), xw, yw, ymask)

    def fits(mask):
        b = box_of(mask)
        return b is None or box_cells(b) <= win_cells

    if half is not None:
        mine = 0xA if half else 0x5
        if fits(0xF):
            parts = [0xF]
        elif fits(mine):
            parts = [mine]
        else:
            parts = [mine & 0x3, mine & 0xC]
    elif not sorted_rays or fits(0xF):
        parts = [0xF]
    else:
        left, right = fits(0x5), fits(0xA)
        if left and right:
            parts = [0x5, 0xA]
        elif left and per_half:
            parts = [0x5, 0x2, 0x8]
        elif right and per_half:
            parts = [0x1, 0x4, 0xA]
        else:
            parts = [0x1, 0x2, 0x4, 0x8]
    return Plan(parts, [box_of(p) for p in parts], [fits(p) for p in parts])


def plan_two_then_four(orgs, ends, xw, yw, win_cells):
    """The rule before the halves were decided one by one: both halves fit, or four quadrants."""
    return plan(orgs, ends, xw, yw, win_cells, per_half=False)


# ---- the benchmark trajectory ---------------------------------------------------------------------------------------

def replay_cells(rep, xw=400, yw=400, reso=0.05):
    """Origin cells [S, 2] and end cells [S, n, 2] of scans 1.. of a synthetic replay, cast from its TRUE poses taken
    relative to the first (the benchmark's map rule: scale 1 / reso, offsets half the map), as ReplaySource::ray does."""
    scale, off_x, off_y = round(1.0 / reso), xw * reso / 2.0, yw * reso / 2.0
    p = rep.poses_true
    c0, s0 = np.cos(p[0, 2]), np.sin(p[0, 2])
    dx, dy = p[1:, 0] - p[0, 0], p[1:, 1] - p[0, 1]
    px, py, th = c0 * dx + s0 * dy, -s0 * dx + c0 * dy, p[1:, 2] - p[0, 2]
    n = rep.ranges.shape[1]
    ang = np.linspace(rep.angle_min, rep.angle_max, n)
    r = rep.ranges[1:].astype(np.float64)
    r = np.where(np.isinf(r), 30.0, r)
    lx, ly = np.cos(ang)[None] * r, np.sin(ang)[None] * r
    c, s = np.cos(th)[:, None], np.sin(th)[:, None]
    x, y = c * lx - s * ly + px[:, None], s * lx + c * ly + py[:, None]
    cell = lambda v, off: np.trunc(scale * (v + off)).astype(np.int64)
    return (np.stack([cell(px, off_x), cell(py, off_y)], axis=1),
            np.stack([cell(x, off_x), cell(y, off_y)], axis=2))


def replay_plans(rep, group, win_cells, xw=400, yw=400, reso=0.05, rule=plan):
    orgs, ends = replay_cells(rep, xw, yw, reso)
    return [rule(orgs[s0:s0 + group], ends[s0:s0 + group].reshape(-1, 2), xw, yw, win_cells)
            for s0 in range(0, len(orgs), group)]
