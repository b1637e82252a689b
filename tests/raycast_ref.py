"""NumPy reference of the two operators that read a map along rays (include/slam_hip.h, "rays traced through a
map"), written from their stated semantics on the oracle's pinned pieces: ``bresenham_path`` (the reference's own
rasteriser, golden g1), ``world_points`` (obs = u2T(pose).dot(pc)) and ``laser_to_numpy`` (inf -> 30 m).

    trace(pmap, start, end, skip)  smallest path index j >= skip whose cell is in bounds and has pmap == 100,
                                   else -1; and the path length Lp
    raycast(...)                   the scan the map would give: range to the found cell's centre, inf, or NaN
    score(...)                     a measured scan's beams in seven classes, and their tallies

Plus the inputs the CPU and the GPU tests share (ring maps, beam tables, the room)."""
import math

import numpy as np

from oracle import oracle_np as O

EMPTY, HIT, BLOCKED, FREE, UNKNOWN, OUT, BAD = range(7)
MAX_CELL = 1 << 20


def to_cell(v, scale, off):
    """int(scale * (v + off)) (mapping.py:33-36); None where Python's int() raises (NaN, inf) or the index is
    beyond 2^20 (the library's bound on a ray)."""
    c = scale * (v + off)
    if c != c or not abs(c) < MAX_CELL:
        return None
    return int(c)


def trace(pmap, start, end, skip):
    path = O.bresenham_path(start, end)
    xw, yw = pmap.shape
    for j, (cx, cy) in enumerate(path):
        if j >= skip and 0 <= cx < xw and 0 <= cy < yw and pmap[cx][cy] == 100:
            return j, len(path), (cx, cy)
    return -1, len(path), None


def table_points(ranges, cos_t, sin_t):
    """laser_to_numpy for given beam tables: the same products, inf -> 30 m (slam_ekf.py:115-123)."""
    r = np.array(ranges, dtype=np.float64)
    r[r == np.inf] = O.MAX_LASER_RANGE
    pc = np.ones((3, len(r)))
    pc[0] = np.asarray(cos_t, dtype=np.float64) * r
    pc[1] = np.asarray(sin_t, dtype=np.float64) * r
    return pc


def _beams(pose, pc, scale, off_x, off_y):
    """(start cell, [end cell or None per beam]) or None when the pose itself cannot be a cell."""
    pose = np.asarray(pose, dtype=np.float64).reshape(3)
    n = pc.shape[1]
    if not np.all(np.isfinite(pose)):
        return None, [None] * n
    with np.errstate(all="ignore"):
        obs = O.world_points(pose, pc)
    sx, sy = to_cell(pose[0], scale, off_x), to_cell(pose[1], scale, off_y)
    if sx is None or sy is None:
        return None, [None] * n
    ends = []
    for i in range(n):
        ex, ey = to_cell(obs[0][i], scale, off_x), to_cell(obs[1][i], scale, off_y)
        ends.append(None if ex is None or ey is None else (ex, ey))
    return (sx, sy), ends


def raycast(pmap, scale, off_x, off_y, pose, cos_t, sin_t, max_range, skip=1):
    """ranges float32 [n], cells int32 [n, 2] of one pose (pmap None: the hypothesis names no map)."""
    n = len(cos_t)
    pc = table_points(np.full(n, np.float32(max_range)), cos_t, sin_t)
    start, ends = _beams(pose, pc, scale, off_x, off_y) if pmap is not None else (None, [None] * n)
    ranges = np.full(n, np.nan, dtype=np.float32)
    cells = np.full((n, 2), -1, dtype=np.int32)
    for i, e in enumerate(ends):
        if start is None or e is None:
            continue
        j, _, cell = trace(pmap, start, e, skip)
        if j < 0:
            ranges[i] = np.inf
            continue
        dx = (cell[0] + 0.5) / scale - off_x - float(pose[0])
        dy = (cell[1] + 0.5) / scale - off_y - float(pose[1])
        ranges[i] = np.float32(math.sqrt(dx * dx + dy * dy))
        cells[i] = cell
    return ranges, cells


def score(pmap, scale, off_x, off_y, pose, pc, skip=1):
    """counts int32 [7], classes int8 [n] of one pose; pc [3, n] the scan's points (laser_to_numpy with
    clip_inf=True, or table_points)."""
    n = pc.shape[1]
    start, ends = _beams(pose, pc, scale, off_x, off_y) if pmap is not None else (None, [None] * n)
    cls = np.full(n, BAD, dtype=np.int8)
    for i, e in enumerate(ends):
        if start is None or e is None:
            continue
        j, lp, _ = trace(pmap, start, e, skip)
        if lp == 0:
            cls[i] = EMPTY
        elif j == lp - 1:
            cls[i] = HIT
        elif j >= 0:
            cls[i] = BLOCKED
        elif 0 <= e[0] < pmap.shape[0] and 0 <= e[1] < pmap.shape[1]:
            cls[i] = UNKNOWN if pmap[e[0]][e[1]] == 50 else FREE
        else:
            cls[i] = OUT
    return np.bincount(cls, minlength=7).astype(np.int32), cls


# ---------------------------------------------------------------- shared inputs
CENTRE = (32, 32)                       # of the 64 x 64 ring map: scale 1, offsets 0, pose at the cell's middle
RING_POSE = np.array([32.5, 32.5, 0.0])


def ring(r, c=CENTRE):
    """Every cell at Chebyshev distance r of c."""
    return [(c[0] + i, c[1] + j) for i in range(-r, r + 1) for j in range(-r, r + 1) if max(abs(i), abs(j)) == r]


def ring_updates():
    """The two Mapping.update calls that put hits on the rings of radius 8 and 16: (ox, oy, cx, cy) each, the
    endpoints the rings' cell centres."""
    out = []
    for r in (8, 16):
        cells = ring(r)
        out.append((np.array([x + 0.5 for x, _ in cells]), np.array([y + 0.5 for _, y in cells]),
                    CENTRE[0] + 0.5, CENTRE[1] + 0.5))
    return out


def ring_pmap():
    m = O.Mapping(64, 64, 1.0, scale=1.0, offset_x=0.0, offset_y=0.0)
    for ox, oy, cx, cy in ring_updates():
        m.update(ox, oy, cx, cy)
    return m.pmap.astype(np.int8)


def tables_to(cells, c=CENTRE):
    """Beam tables with which a beam of range 1 from the middle of cell c, heading 0, ends in the middle of
    cells[i] (all exact in float64): cos_t = dx, sin_t = dy."""
    return (np.array([float(x - c[0]) for x, _ in cells]), np.array([float(y - c[1]) for _, y in cells]))


def near_tie_ends(c=CENTRE):
    """The near-tie lines of g1 - ends (10, 3) and (12, 1) - in all eight octants."""
    out = []
    for a, b in ((10, 3), (12, 1)):
        for u, v in ((a, b), (b, a)):
            for sx in (1, -1):
                for sy in (1, -1):
                    out.append((c[0] + sx * u, c[1] + sy * v))
    return out


def is_flagged(start, end):
    """bresenham.py:14-19: the walk runs end -> start."""
    (x0, y0), (x1, y1) = start, end
    steep = abs(y1 - y0) > abs(x1 - x0)
    return (y0 > y1) if steep else (x0 > x1)


AMIN, AMAX = -3.14159, 3.14159


def room(syn):
    """The 6-pose, 120-beam room at 400 x 400, scale 20: (ranges [6, 120] float32, poses [6, 3]) that build the
    map, and the B = 5 hypotheses scored against it with the last scan: the true pose, two offsets, one outside the
    map looking in, one NaN."""
    rep = syn.make_replay(6, 120, seed=4)
    poses = np.asarray(rep.poses_true, dtype=np.float64)
    true = poses[-1]
    hyp = np.stack([true, true + np.array([0.3, 0.2, 0.0]), true + np.array([0.0, 0.0, 0.2]),
                    np.array([-12.0, 0.5, 0.0]), np.array([np.nan, 0.0, 0.0])])
    return np.asarray(rep.ranges, dtype=np.float32), poses, hyp


def room_pmap(ranges, poses):
    m = O.Mapping(400, 400, 0.05, scale=20.0, offset_x=10.0, offset_y=10.0)
    for r, p in zip(ranges, poses):
        obs = O.world_points(p, O.laser_to_numpy(r, AMIN, AMAX, clip_inf=True))
        m.update(obs[0], obs[1], p[0], p[1])
    return m.pmap.astype(np.int8)
