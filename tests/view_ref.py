"""NumPy reference of the view gain (include/slam_hip.h, "view gain"), written from its stated semantics on the
pieces of tests/raycast_ref.py: ``trace``, ``_beams`` and ``table_points`` (and through them the oracle's
``bresenham_path`` and ``world_points``).

    view(pmap, scale, off_x, off_y, pose, cos_t, sin_t, max_range, skip)
        -> (counts int32 [4] = (unknown, free, occupied cells of the seen set, open beams),
            seen uint32 [xw, ceil(yw / 32)]: bit y & 31 of word y >> 5 in row x)
        a row of -1 and zero words for a pose that cannot be a cell (or pmap None: the view names no map)

Plus the inputs the CPU and the GPU tests share (the gap map, the view that leaves the map)."""
import numpy as np

import raycast_ref as R
from oracle import oracle_np as O

UNKNOWN, FREE, OCCUPIED, OPEN = range(4)


def words_of(cells, xw, yw):
    w = np.zeros((xw, (yw + 31) // 32), dtype=np.uint32)
    for x, y in cells:
        w[x, y >> 5] |= np.uint32(1 << (y & 31))
    return w


def cells_of(words, yw):
    """The set of cells of bit words [xw, wpr]; asserts that no bit is set at y >= yw."""
    out = set()
    for x, w in zip(*np.nonzero(words)):
        for b in range(32):
            if (int(words[x, w]) >> b) & 1:
                assert 32 * w + b < yw, (x, w, b)
                out.add((int(x), int(32 * w + b)))
    return out


def detail(pmap, scale, off_x, off_y, pose, cos_t, sin_t, max_range, skip=1, walk_order=False):
    """dict(counts, seen (a set of cells), marks (in-bounds path cells seen, with repeats), open) or None for a bad view.
    ``walk_order``: the MISTAKE of taking, on a reversed line, the first find in walk order (the last in path order)."""
    n = len(cos_t)
    pc = R.table_points(np.full(n, np.float32(max_range)), cos_t, sin_t)
    start, ends = R._beams(pose, pc, scale, off_x, off_y) if pmap is not None else (None, [None] * n)
    if start is None:
        return None
    xw, yw = pmap.shape
    seen, marks, n_open = set(), 0, 0
    for e in ends:
        if e is None:
            continue
        path = O.bresenham_path(start, e)
        j, lp, _ = R.trace(pmap, start, e, skip)
        if walk_order and j >= 0 and R.is_flagged(start, e):
            j = max(k for k, (cx, cy) in enumerate(path) if k >= skip and 0 <= cx < xw and 0 <= cy < yw and pmap[cx][cy] == 100)
        n_open += j < 0
        for k in range(skip, (j if j >= 0 else lp - 1) + 1):
            cx, cy = path[k]
            if 0 <= cx < xw and 0 <= cy < yw:
                seen.add((cx, cy))
                marks += 1
    counts = np.zeros(4, dtype=np.int32)
    for c in seen:
        counts[{50: UNKNOWN, 0: FREE, 100: OCCUPIED}[int(pmap[c])]] += 1
    counts[OPEN] = n_open
    return dict(counts=counts, seen=seen, marks=marks)


def view(pmap, scale, off_x, off_y, pose, cos_t, sin_t, max_range, skip=1):
    d = detail(pmap, scale, off_x, off_y, pose, cos_t, sin_t, max_range, skip)
    if d is None:
        shape = (0, 0) if pmap is None else (pmap.shape[0], (pmap.shape[1] + 31) // 32)
        return np.full(4, -1, dtype=np.int32), np.zeros(shape, dtype=np.uint32)
    return d["counts"], words_of(d["seen"], *pmap.shape)


def views(pmaps, scale, off_x, off_y, poses, cos_t, sin_t, max_range, skip=1, gob=None):
    """(counts [B, 4], seen [B, xw, wpr]) of a batch: view b reads pmaps[gob[b]] (None: map 0); an entry outside the
    maps gives a bad view."""
    xw, yw = pmaps[0].shape
    cs, ss = [], []
    for b, p in enumerate(poses):
        g = 0 if gob is None else int(gob[b])
        c, s = view(pmaps[g] if 0 <= g < len(pmaps) else None, scale, off_x, off_y, p, cos_t, sin_t, max_range, skip)
        cs.append(c)
        ss.append(s if s.size else np.zeros((xw, (yw + 31) // 32), dtype=np.uint32))
    return np.stack(cs), np.stack(ss)


# ---------------------------------------------------------------- shared inputs
def counters_of(pmap):
    """(pass, hit) int32 counters that finalize to ``pmap`` under the reference's rule (one hit occupies): occupied =
    one hit, free = one pass, unknown = untouched."""
    pm = np.asarray(pmap)
    return (pm == 0).astype(np.int32), (pm == 100).astype(np.int32)


GAP_INNER = [(40, y) for y in range(30, 35)]        # cells of the radius-8 ring opened
GAP_OUTER = [(48, y) for y in range(28, 37)]        # cells of the radius-16 ring opened


def gap_pmap():
    """The ring map with a gap in both rings towards +x: a view from the centre sees out through it."""
    pm = R.ring_pmap().copy()
    for c in GAP_INNER + GAP_OUTER:
        assert pm[c] == 100
        pm[c] = 0
    return pm


LEAVE_CELL = (3, 60)                                # a view near the map's corner: most of ring(20) lies outside
LEAVE_POSE = np.array([3.5, 60.5, 0.0])


def pose_at(cell):
    return np.array([cell[0] + 0.5, cell[1] + 0.5, 0.0])


# The two-room map of the goal tests: a walled room (free cells 10 .. 30 squared) in unknown space with two ways out.
# West, near the robot: a five-cell slit into a walled-in pocket of 25 unknown cells.  East, farther away: a mouth of
# 17 cells onto an unexplored hall.  Nearest-frontier rules pick the slit; a view from the mouth reveals far more.
ROOM_ROBOT = (12, 20)
ROOM_SLIT, ROOM_MOUTH = (7, 20), (31, 20)            # the representatives of the two frontier clusters
ROOM_FRONTIERS = dict(radius=2, min_unknown=8, min_size=3)


def two_room_pmap():
    pm = np.full((64, 64), 50, dtype=np.int8)
    pm[9:32, 9:32] = 100
    pm[10:31, 10:31] = 0
    pm[1:9, 17:24] = 100
    pm[7:10, 18:23] = 0
    pm[2:7, 18:23] = 50
    pm[31, 12:29] = 0
    return pm
