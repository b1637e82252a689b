"""How the LDS-window ray cast sizes its window and shapes a shared-map launch, asked of the library itself (plan_win and
the size functions of csrc/launch_shapes.h, through slam_plan_win / slam_plan_query of the C ABI: no GPU needed), and
how k_grid_update_win cuts a group's rays into phases.  Test infrastructure only: tests/test_win_shapes_cpu.py sweeps it,
tests/test_gpu_window_two_per_cu.py takes its box sizes from it.

  win_lds_bytes    dynamic LDS of a window workgroup: scan constants, control block, histogram, sorted order, window
  win_cells_for    the window's capacity in 16-bit cells: kWinCells; more for small groups (two workgroups still share
                   a CU); and, for a launch that wants two per CU (two_per_cu), the same carving even where it comes
                   out below kWinCells, down to kWinTwoFloor
  launch           the shape of a shared-map launch: two per CU only for sorted rays (sort_cap > 0) in a launch of more
                   workgroups than the chip has CUs
  plan_win         every field of slam_plan_win's answer, for any request
  plan             the phases of one workgroup: the box of everything if it fits, else per direction half (left /
                   right of the origins' column) one phase if the half fits and two (cut at the origins' row) if not
"""
from __future__ import annotations

import ctypes as C
import importlib
from collections import namedtuple

import numpy as np

PKG = "a-2d-lidar-based-slam-system-for-wheeled-mobile-robots_amd"


def query(name, a=0, b=0, c=0, guard=0):
    """slam_plan_query: a constant or a size function of csrc/launch_shapes.h by its name there."""
    abi = importlib.import_module(PKG + "._abi")
    out = C.c_int64()
    abi.check(abi.lib().slam_plan_query(name.encode(), int(a), int(b), int(c), int(guard), C.byref(out)))
    return out.value


WIN_CELLS = query("kWinCells")
WIN_MAX_GROUP = query("kWinMaxGroup")
SORT_BINS = query("kSortBins")
MAX_SORT_RAYS = query("kMaxSortRays")
WIN_BOX_INTS = query("kWinBoxInts")
HALF_SLACK = query("kWinHalfSlack")
TWO_FLOOR = query("kWinTwoFloor")
MIN_THREADS = query("kWinMinThreads")
SCAN_CONST = query("kScanConstBytes")
LDS_PER_CU = query("kLdsPerCu")
CUS = query("kChipCus")
FORMS = ("Win", "Own", "Owner1", "Owner2", "Owner8ThenRedo")        # SLAM_WIN_FORM_*


def win_sort_cap(rays):
    return query("win_sort_cap", rays)


def win_lds_bytes(group, sort_cap, win_cells, guard=0):
    return query("win_lds_bytes", group, sort_cap, win_cells, guard)


def win_cells_for(group, sort_cap, two_per_cu=False, guard=0):
    """(for a CU of LDS_PER_CU bytes; launch() takes another chip's)"""
    return query("win_cells_for", group, sort_cap, two_per_cu, guard)


WinPlan = namedtuple("WinPlan", "form grid_x grid_y threads lds lds_attr exclusive sort_cap win_cells split lds_hits two_per_cu wgs "
                                "own8_lds own8_win redo_grid live_dirty")


def plan_win(scans, n, group, L=1, got=False, pmap_live=False, private=False, hit_levels=1, xw=400, yw=400, redo=False,
             split_pref=-1, hits_pref=-1, cus=CUS, lds_per_cu=LDS_PER_CU, guard=0):
    """slam_plan_win's answer for a launch of L streams of `scans` scans of n beams in groups of `group`; form by name."""
    abi = importlib.import_module(PKG + "._abi")
    out = (C.c_int * len(WinPlan._fields))()
    abi.check(abi.lib().slam_plan_win(L, scans, n, group, int(got), int(pmap_live), int(private), hit_levels, xw, yw, int(redo),
                                      split_pref, hits_pref, cus, lds_per_cu, guard, out))
    p = WinPlan(*out)
    return p._replace(form=FORMS[p.form])


Launch = namedtuple("Launch", "group sort_cap split wgs two_per_cu win_cells lds")


def launch(scans, n, group, L=1, split_pref=-1, cus=CUS, lds_per_cu=LDS_PER_CU, guard=0):
    """A shared-map launch (k_grid_update_win) of L streams of `scans` scans of n beams in groups of `group`."""
    p = plan_win(scans, n, group, L=L, split_pref=split_pref, cus=cus, lds_per_cu=lds_per_cu, guard=guard)
    assert p.form == "Win"
    return Launch(group, p.sort_cap, p.split, p.wgs, bool(p.two_per_cu), p.win_cells, p.lds)


# ---- phases -------------------------------------------------------------------------------------------------------

def box_cells(box):
    """Window cells a clamped box takes: rows are stored padded to an even height."""
    return (box[2] - box[0] + 1) * ((box[3] - box[1] + 2) & ~1)


Plan = namedtuple("Plan", "parts boxes fits")      # per phase: quadrant mask, clamped box (None: empty), whether it fits


class _Phases(C.Structure):                         # slam_win_phases
    _fields_ = [("nph", C.c_int), ("parity", C.c_int), ("part", C.c_int * 4), ("box", (C.c_int * 4) * 4), ("any", C.c_int * 4),
                ("fits", C.c_int * 4)]


def plan(orgs, ends, xw, yw, win_cells, half=None, sorted_rays=True, even_rows=None, per_half=True):
    """Phases of a workgroup (slam_plan_win_phases) for scans with origin cells orgs [S, 2] and end cells ends [R, 2] (all
    of the group's valid rays).  half: None for one workgroup per group, 0 / 1 for the two of grid_split.  per_half False:
    the earlier rule of the unsplit form (both halves fit, or four quadrants), which the library no longer has."""
    orgs, ends = np.asarray(orgs), np.asarray(ends)
    ymask = 1 if (yw % 2 == 0 if even_rows is None else even_rows) else 0
    bb = (C.c_int * 4)(min(orgs[:, 0].min(), ends[:, 0].min()), min(orgs[:, 1].min(), ends[:, 1].min()),
                       max(orgs[:, 0].max(), ends[:, 0].max()), max(orgs[:, 1].max(), ends[:, 1].max()))
    org = (C.c_int * 4)(orgs[:, 0].min(), orgs[:, 1].min(), orgs[:, 0].max(), orgs[:, 1].max())
    abi = importlib.import_module(PKG + "._abi")

    def ask(cells, half):
        p = _Phases()
        abi.check(abi.lib().slam_plan_win_phases(bb, org, xw, yw, ymask, min(cells, 2 ** 31 - 1), int(sorted_rays),
                                                 -1 if half is None else half, C.byref(p)))
        return Plan(list(p.part[:p.nph]), [tuple(p.box[k]) if p.any[k] else None for k in range(p.nph)],
                    [bool(p.fits[k]) for k in range(p.nph)])

    got = ask(win_cells, half)
    if per_half or half is not None or len(got.parts) != 3:
        return got
    # one half fits, the other does not: the earlier rule cut both.  The quadrants' boxes are what the two workgroups of a
    # split launch get when nothing fits (a half that is empty altogether stays one part, with no box)
    left, right = ([q.boxes[0], q.boxes[1]] if len(q.parts) == 2 else [None, None] for q in (ask(0, 0), ask(0, 1)))
    boxes = [left[0], right[0], left[1], right[1]]
    return Plan([0x1, 0x2, 0x4, 0x8], boxes, [b is None or box_cells(b) <= win_cells for b in boxes])


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
