"""Where the map reset that rides on the scan-matching launch could go wrong (test infrastructure only; no GPU needed).

Context option "replay_reset": slam_replay_dev hands the grid object's state - the pass and hit counters of every map and
the visit slots, ``state_bytes`` in all - to its scan-matching launch, whose lanes clear it 16 bytes at a time in a
grid-stride loop (icp_clear_on_the_way, csrc/icp_kernels.hip).  A launch has ``lanes = pairs x block`` and
``n16 = state_bytes / 16`` words to clear, so the loop makes ``ceil(n16 / lanes)`` trips.  The cases below put the lane
count where that loop changes: far below the word count (many trips), one block short of it, on it, one block past it,
and at four times as many (one trip, most lanes idle) - for each launch form the scan matcher has.  Both sizes are asked of
the library (slam_plan_icp, slam_plan_query "grid_state_bytes"); tests/test_replay_reset_cases.py holds the table to the
edges it is there for, tests/test_gpu_replay_reset.py runs it."""
from __future__ import annotations

from collections import namedtuple

import icp_shapes

BEAMS = 360
XW = YW = 64                      # one map of 64 x 64 cells: 2 x 16 KiB of counters and the visit slots, 3 072 words
RESO = 0.2                        # 12.8 m across: the 10 m x 8 m room lies inside
N16 = 3072

# name: (context options, the same as arguments of plan_icp, the form plan_icp answers)
FORMS = {
    "workgroup_qpt1": ({"icp_qpt": 1}, dict(icp_qpt=1), "Workgroup"),
    "workgroup_qpt2": ({"icp_qpt": 2}, dict(icp_qpt=2), "Workgroup"),
    "workgroup_qpt3": ({"icp_qpt": 3}, dict(icp_qpt=3), "Workgroup"),
    "wave_f32": ({"icp_one_wave": 1, "icp_f32_filter": 1}, dict(one_wave=1, f32_filter=1), "WaveF32"),
    "wave_f64": ({"icp_one_wave": 1, "icp_f32_filter": 0}, dict(one_wave=1, f32_filter=0), "WaveF64"),
}
KINDS = ("many_trips", "below", "equal", "above", "one_trip")

Case = namedtuple("Case", "form kind pairs block lanes n16 trips options")


def grid_state_bytes(G, xw, yw):
    """Bytes of a grid object's state as slam_grid_create lays it out: what a reset clears."""
    return icp_shapes.query("grid_state_bytes", G, xw, yw)


def plan(form, pairs):
    """The launch of ``pairs`` scan pairs of a replay in that form, as the library shapes it."""
    kw = dict(icp_qpt=0, one_wave=-1, f32_filter=-1)
    kw.update(FORMS[form][1])
    return icp_shapes.plan_icp(pairs, BEAMS, BEAMS, True, kw["icp_qpt"], one_wave=kw["one_wave"], f32_filter=kw["f32_filter"])


def trips(n16, lanes):
    return -(-n16 // lanes)


def case(form, kind, xw=XW, yw=YW):
    """The pair count of (form, kind).  The block follows the batch - the preferred queries per lane replace the
    size-derived ones only in launches of more than 64 pairs - so the pair count and the block it is computed from are
    settled together: the block is the one the plan gives AT that pair count."""
    n16 = grid_state_bytes(1, xw, yw) // 16
    want = {"below": lambda b: n16 // b - 1, "equal": lambda b: n16 // b, "above": lambda b: n16 // b + 1}
    if kind in ("many_trips", "preferred_trips"):
        pairs = 1 if kind == "many_trips" else PREFERRED_PAIRS
    elif kind in want:
        pairs = want[kind](plan(form, 1).block)
        for _ in range(4):                        # (a fixed point: one step where the block does not follow the batch)
            pairs = want[kind](plan(form, pairs).block)
        assert pairs == want[kind](plan(form, pairs).block), "no pair count agrees with its own block"
    else:                                         # one_trip: the fewest pairs, in the form's own shape where the batch rule lets it
        asked = FORMS[form][1].get("icp_qpt", 0)
        first = next(p for p in range(1, 4 * n16 + 1) if not asked or plan(form, p).qpt == asked)
        pairs = next(p for p in range(first, 4 * n16 + 1) if p * plan(form, p).block >= 4 * n16)
    p = plan(form, pairs)
    return Case(form, kind, pairs, p.block, pairs * p.block, n16, trips(n16, pairs * p.block), dict(FORMS[form][0]))


def cases():
    return [case(f, k) for f in FORMS for k in KINDS]


# The 64 x 64 map is too small to meet two and three queries per lane below its word count: at 65 pairs, the fewest that
# take the preference, their launches already have four and nearly three times as many lanes as words.  One case each
# on a map of 256 x 256 cells puts those two kernels through several trips as well.
PREFERRED_PAIRS = 65
PREFERRED_MAP = 256


def preferred_cases():
    return [case(f, "preferred_trips", PREFERRED_MAP, PREFERRED_MAP) for f in ("workgroup_qpt2", "workgroup_qpt3")]


def case_id(c):
    return "%s-%s-%dpairs" % (c.form, c.kind, c.pairs)


def max_pairs():
    """The largest pair count of both tables: the scans the GPU test draws once."""
    return max(c.pairs for c in cases() + preferred_cases())


# several maps: a trajectory routes to maps 2 and 0, map 1 is nobody's
MANY = dict(G=3, xw=37, yw=53, reso=0.2, L=2, n_scan=6, grid_of_traj=(2, 0))
