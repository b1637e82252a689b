"""Inputs of test_gpu_raycast_bounds.py and the reference's answers on them, all on the CPU: maps written as
(pass, hit) counters on non-square, ragged shapes under both occupied rules, batches that take the pack kernel and
the two trace engines past one pass of their loops, staged blocks that hold several hypotheses of several maps, the
LDS fit boundary and `skip` at the ends of a scored line.  test_raycast_bound_cases.py checks without a GPU that
these inputs reach what they are there for.

The pmap is computed here, in NumPy, from the counters (`pmap_of`, on oracle_np.occupied_rule); the reference
(raycast_ref.raycast / raycast_ref.score) reads that pmap.  Every builder is cached: an answer is computed once
and shared by every test, and nobody writes into it."""
import functools
import math

import numpy as np

import raycast_ref as R
from oracle import oracle_np as O

FREE_INC, THRESH = 0.01, 10.0
HIT_INCS = (20, 4)                      # one hit level (pass threshold 1001) and three (1001 / 601 / 201)
CLASSES6 = (R.EMPTY, R.HIT, R.BLOCKED, R.FREE, R.UNKNOWN, R.OUT)


def table(hit_inc):
    return O.occupied_rule(FREE_INC, float(hit_inc), THRESH)


def pmap_of(pass_, hit, hit_inc):
    """50 where pass | hit == 0, else 100 where h >= len(table) or p >= table[h], else 0."""
    t = table(hit_inc)
    occ = hit >= len(t)
    for h, th in enumerate(t):
        occ = occ | ((hit == h) & (pass_ >= th))
    return np.where((pass_ | hit) == 0, 50, np.where(occ, 100, 0)).astype(np.int8)


def trig(n):
    ang = np.linspace(R.AMIN, R.AMAX, n)                      # _abi.trig_tables
    return np.ascontiguousarray(np.cos(ang)), np.ascontiguousarray(np.sin(ang))


def world(cell, scale, off):
    """The world coordinate whose cell coordinate is `cell` (a float: x.5 is the middle of cell x)."""
    return cell / scale - off


def beam_cells(pose, ct, st, ranges, scale, ox, oy):
    """(start cell, end cells) as the reference forms them."""
    return R._beams(pose, R.table_points(ranges, ct, st), scale, ox, oy)


def ref_raycast(pmaps, geom, poses, gob, ct, st, max_range, skip=1):
    """ranges [B, n], cells [B, n, 2]; pmaps a list, gob[b] the map of pose b (outside the list: no map)."""
    scale, ox, oy = geom
    out = [R.raycast(pmaps[g] if 0 <= g < len(pmaps) else None, scale, ox, oy, p, ct, st, max_range, skip) for p, g in zip(poses, gob)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def ref_score(pmaps, geom, poses, gob, ct, st, ranges, skip=1):
    """counts [B, 7], classes [B, n]; ranges [n] shared or [B, n]."""
    scale, ox, oy = geom
    ranges = np.asarray(ranges, dtype=np.float32)
    out = []
    for b, (p, g) in enumerate(zip(poses, gob)):
        pc = R.table_points(ranges if ranges.ndim == 1 else ranges[b], ct, st)
        out.append(R.score(pmaps[g] if 0 <= g < len(pmaps) else None, scale, ox, oy, p, pc, skip))
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def flagged_of(poses, ct, st, max_range, geom):
    """[B, n] bool: the cast line of beam i of pose b is walked end -> start (False too where there is no line)."""
    out = np.zeros((len(poses), len(ct)), dtype=bool)
    for b, p in enumerate(poses):
        start, ends = beam_cells(p, ct, st, np.full(len(ct), np.float32(max_range)), *geom)
        for i, e in enumerate(ends):
            out[b, i] = start is not None and e is not None and R.is_flagged(start, e)
    return out


# ================================================================== A. non-square, ragged maps, both rules
N_A = 37
SHAPES = ((37, 300), (300, 37), (65, 33), (5, 257), (64, 95), (1, 70))
# (xw, yw, scale, off_x, off_y): every shape at scale 1, offsets 0, and one with an index rule of its own
A_GEOMS = tuple((xw, yw, 1.0, 0.0, 0.0) for xw, yw in SHAPES) + ((64, 95, 2.5, 3.0, 7.0),)
A_MULTI = ((37, 300), (65, 33))         # run as G = 3 grids too
A_GOB = np.array([2, 0, 1, 1, 0, 2, 0, 1], dtype=np.int32)            # neither monotone nor sorted
N_AIMED = 12                            # aimed beams per aim pose and kind of cell (occupied, free, untouched)
AIM_POSES = (0, 2)


def aim_cells(xw, yw):
    return ((xw // 2, yw // 2), (-3, yw // 3))


def a_poses(xw, yw, scale, ox, oy, seed):
    """8 poses: the middle of a cell near the centre and of one three cells outside the map, both with heading 0 (the
    aimed beams start there: AIM_POSES), the far corner, three more from one to three cells outside the map looking
    in, two seeded; headings over (-pi, pi)."""
    rng = np.random.default_rng(100 + seed)
    c = [(xw // 2 + 0.5, yw // 2 + 0.5, 0.0),
         (max(xw - 3, 0) + 0.5, max(yw - 4, 0) + 0.5, 0.7),
         (-3.5, yw // 3 + 0.5, 0.0),             # cell -3: int() truncates towards zero
         (xw + 1.5, yw + 2.5, -2.4),
         (xw / 2.0 + 0.25, -1.5, 1.6),
         (0.5, yw + 0.75, -1.5),
         (rng.uniform(0, xw), rng.uniform(0, yw), rng.uniform(-math.pi, math.pi)),
         (rng.uniform(0, xw), rng.uniform(0, yw), rng.uniform(-math.pi, math.pi))]
    return np.array([[world(x, scale, ox), world(y, scale, oy), h] for x, y, h in c])


def forced_cells(xw, yw):
    """Occupied whatever the draw: the corners, row 0, and the columns at both ends of a mask word - at every third
    row and the last one, so that rays get past them.  (With xw = 1 row 0 is the whole map; there it keeps only
    its cells in those columns, or no beam could end on a free or an untouched cell.)"""
    cells = {(0, 0), (0, yw - 1), (xw - 1, 0), (xw - 1, yw - 1)}
    if xw > 1:
        cells |= {(0, ly) for ly in range(yw)}
    for ly in (31, 32, 63, 64, 255, 256, yw - 1):
        if ly < yw:
            cells |= {(lx, ly) for lx in range(xw) if lx % 3 == 0 or lx == xw - 1}
    return sorted(cells)


def crossed_cells(poses, ct, st, max_range, geom, xw, yw):
    """The in-bounds cells from path index 1 on of every cast line, in first-met order."""
    seen = {}
    for p in poses:
        start, ends = beam_cells(p, ct, st, np.full(len(ct), np.float32(max_range)), *geom)
        for e in ends:
            for cx, cy in O.bresenham_path(start, e)[1:]:
                if 0 <= cx < xw and 0 <= cy < yw:
                    seen.setdefault((cx, cy), None)
    return list(seen)


def draw_counters(xw, yw, hit_inc, seed, crossed=()):
    """(pass, hit) int32 [xw, yw]: about 10 % of the cells touched, hit over 0 .. len(table), pass over
    {0, 1, table[h] - 1, table[h], table[h] + 1, 5}; the forced cells occupied by their hit level; the eight cells
    nearest the first aim pose free (so that the smallest map has eight beams that end FREE); and, on cells
    taken from `crossed` (cells some cast line crosses), every (h, table[h] + {-1, 0, 1}) once more.  Returns also
    those threshold cells as {(h, d): cell}."""
    rng = np.random.default_rng(seed)
    t = table(hit_inc)
    touched = rng.random((xw, yw)) < 0.10
    hit = np.where(touched, rng.integers(0, len(t) + 1, (xw, yw)), 0)
    th = np.array(t + [t[-1]])[hit]
    cand = np.stack([0 * th, 0 * th + 1, th - 1, th, th + 1, 0 * th + 5])
    pass_ = np.where(touched, np.take_along_axis(cand, rng.integers(0, 6, (1, xw, yw)), 0)[0], 0)
    forced = forced_cells(xw, yw)
    for c in forced:
        hit[c], pass_[c] = len(t), 0
    forced, c0 = set(forced), aim_cells(xw, yw)[0]
    near = sorted((max(abs(x - c0[0]), abs(y - c0[1])), x, y) for x in range(xw) for y in range(yw) if (x, y) != c0 and (x, y) not in forced)
    for _, x, y in near[:8]:                                           # around the first aim pose: passed, never hit
        hit[x, y], pass_[x, y] = 0, 5
    forced |= {(x, y) for _, x, y in near[:8]}
    free = [c for c in crossed if c not in forced]
    thresh_cells = {}
    if free:
        pick = rng.permutation(len(free))[:3 * len(t)]
        for k, (h, d) in zip(pick, [(h, d) for h in range(len(t)) for d in (-1, 0, 1)]):
            hit[free[k]], pass_[free[k]] = h, t[h] + d
            thresh_cells[(h, d)] = free[k]
    return pass_.astype(np.int32), hit.astype(np.int32), thresh_cells


@functools.lru_cache(maxsize=None)
def case_a(xw, yw, scale, ox, oy, hit_inc):
    geom = (scale, ox, oy)
    seed = 7 * xw + yw + hit_inc
    poses = a_poses(xw, yw, scale, ox, oy, seed)
    ct, st = trig(N_A)
    max_range = float(np.float32(0.75 * max(xw, yw) / scale))
    crossed = crossed_cells(poses, ct, st, max_range, geom, xw, yw)
    maps = [draw_counters(xw, yw, hit_inc, seed + 1000 * k, crossed) for k in range(3 if (xw, yw) in A_MULTI and scale == 1.0 else 1)]
    pmaps = [pmap_of(p, h, hit_inc) for p, h, _ in maps]
    # the scan: seeded ranges with a few zeros (EMPTY) and one inf, then beams of range 1 from each aim pose (the middle
    # of its cell, heading 0) to the middle of the nearest occupied, free and untouched cells, as raycast_ref.tables_to
    rng = np.random.default_rng(seed + 5)
    scan = rng.uniform(0.0, max_range, N_A).astype(np.float32)
    scan[::9], scan[5] = 0.0, np.inf
    aimed, adx, ady = [], [], []
    for c0 in aim_cells(xw, yw):
        order = sorted(((max(abs(x - c0[0]), abs(y - c0[1])), x, y) for x in range(xw) for y in range(yw) if (x, y) != c0))
        mine = [c for v in (100, 0, 50) for c in [(x, y) for _, x, y in order if pmaps[0][x, y] == v][:N_AIMED]]
        aimed.append(mine)
        # from the pose's coordinate to the middle of the cell (cell -3 is entered at -3.5: int() truncates towards zero)
        px, py = (c0[0] + 0.5 if c0[0] >= 0 else c0[0] - 0.5), c0[1] + 0.5
        adx += [(x + 0.5 - px) / scale for x, _ in mine]
        ady += [(y + 0.5 - py) / scale for _, y in mine]
    sct, sst = np.concatenate([ct, adx]), np.concatenate([st, ady])
    sscan = np.concatenate([scan, np.ones(len(adx), dtype=np.float32)])
    return dict(xw=xw, yw=yw, geom=geom, hit_inc=hit_inc, maps=maps, pmaps=pmaps, poses=poses, ct=ct, st=st, max_range=max_range,
                sct=sct, sst=sst, scan=sscan, aimed=aimed, crossed=set(crossed))


@functools.lru_cache(maxsize=None)
def ref_a(xw, yw, scale, ox, oy, hit_inc, multi=False):
    """(ranges, cells, counts, classes) of the 8 poses on map 0, or with `multi` on maps A_GOB."""
    c = case_a(xw, yw, scale, ox, oy, hit_inc)
    gob = A_GOB if multi else np.zeros(8, dtype=np.int32)
    return ref_raycast(c["pmaps"], c["geom"], c["poses"], gob, c["ct"], c["st"], c["max_range"]) + \
        ref_score(c["pmaps"], c["geom"], c["poses"], gob, c["sct"], c["sst"], c["scan"])


# ================================================================== B. pack past one pass of rows
B_G, B_XW, B_YW = 1025, 1024, 3         # 1 049 600 rows of three cells: 1 024 more than the pack kernel's 2^20 blocks
B_MAPS = (0, 1023, 1024, 512)           # three maps with occupied cells and an empty one
N_B = 8


@functools.lru_cache(maxsize=None)
def case_b():
    """{map: [(lx, ly, pass, hit)]}: in map 1024 only rows 0, 1 and 1023 - global rows 2^20, 2^20 + 1, 2^20 + 1023."""
    cells = {0: [(3, 1, 0, 1), (700, 0, 1001, 0), (700, 2, 1000, 0), (1023, 1, 0, 1)],
             1023: [(0, 2, 0, 2), (512, 1, 0, 1), (1023, 0, 2000, 0), (520, 1, 7, 0)],
             1024: [(0, 1, 0, 1), (1, 0, 1001, 0), (1, 2, 0, 1), (1023, 1, 0, 1), (1023, 2, 3, 1)],
             512: []}
    pmaps = {}
    for g, cs in cells.items():
        p, h = np.zeros((B_XW, B_YW), dtype=np.int32), np.zeros((B_XW, B_YW), dtype=np.int32)
        for lx, ly, pv, hv in cs:
            p[lx, ly], h[lx, ly] = pv, hv
        pmaps[g] = pmap_of(p, h, 20)
    poses = np.array([[6.5, 1.5, 3.1], [1017.5, 1.5, 0.05], [6.5, 1.5, 3.1], [1017.5, 1.5, 0.05], [5.5, 0.5, 2.9], [600.5, 1.5, 0.0],
                      [515.5, 1.5, 3.14], [1020.5, 2.5, -0.1], [6.5, 1.5, 3.1], [300.5, 1.5, 0.0]])
    gob = np.array([1024, 1024, 0, 0, 1024, 0, 1023, 1023, 512, 512], dtype=np.int32)
    ct, st = np.cos(np.linspace(-0.3, 0.3, N_B)), np.sin(np.linspace(-0.3, 0.3, N_B))
    scan = np.array([5.0, 6.0, 5.5, 6.5, 3.0, 0.0, 110.0, 7.0], dtype=np.float32)
    return dict(cells=cells, pmaps=pmaps, poses=poses, gob=gob, ct=ct, st=st, scan=scan, max_range=120.0)


@functools.lru_cache(maxsize=None)
def ref_b():
    c = case_b()
    pmaps = [c["pmaps"].get(g) for g in range(B_G)]
    return ref_raycast(pmaps, (1.0, 0.0, 0.0), c["poses"], c["gob"], c["ct"], c["st"], c["max_range"]) + \
        ref_score(pmaps, (1.0, 0.0, 0.0), c["poses"], c["gob"], c["ct"], c["st"], c["scan"])


# ================================================================== C. staged blocks of several hypotheses and maps
STAGED_BLOCKS = 2048                    # kRaycastStagedBlocks: hyps_per_block = ceil(B / 2048)
C_SHAPE = (37, 300)                     # 370 mask words a map: staging takes every lane twice
C_BS = (2048, 2049, 4097)               # hyps_per_block 1, 2, and 3 with a partial last block
C_NS = (1, 37, 65, 100)
# maps of twelve consecutive hypotheses: in threes AAA, AAB, ABC, ABA; in twos AA, AB, BC, AB, CC, AC
C_GOB12 = (0, 0, 0, 1, 1, 2, 0, 1, 2, 2, 0, 2)
C_POSES, C_ROWS, C_ROW_PERIOD = 6, 4, 7                               # pose b % 6, range row (b % 7) % 4
C_PERIOD = 84                           # lcm(12, 6, 7)


def hyps_per_block(B):
    return (B + STAGED_BLOCKS - 1) // STAGED_BLOCKS


def c_gob(B):
    return np.array(C_GOB12, dtype=np.int32)[np.arange(B) % 12]


def run_patterns(gob, hpb):
    """The shapes of the staged blocks: for each block of `hpb` consecutive hypotheses the tuple of its runs' maps,
    renamed in order of first appearance ((0,) one map, (0, 1, 0) A-B-A, ...), with the block's length."""
    out = set()
    for b0 in range(0, len(gob), hpb):
        blk, runs, names = list(gob[b0:b0 + hpb]), [], {}
        for g in blk:
            k = names.setdefault(g, len(names))
            if not runs or runs[-1] != k:
                runs.append(k)
        out.add((len(blk), tuple(runs)))
    return out


def c_invalid(B):
    """grid_of_batch with invalid entries: between two runs of one map, at a block's first and last slot, two
    different ones side by side (inside a block and across blocks), and on the batch's last hypothesis.  The blocks
    meant are those of three hypotheses; at one or two a block the same rows are simply invalid."""
    gob = c_gob(B)
    for b, v in ((1, 3), (12, -1), (14, 3), (24, 3), (25, 100), (38, -1), (39, 3), (49, -1), (B - 1, -1), (B - 4, 3)):
        gob[b] = v
    return gob


@functools.lru_cache(maxsize=None)
def case_c(n):
    xw, yw = C_SHAPE
    a = case_a(xw, yw, 1.0, 0.0, 0.0, 4)                               # the G = 3 maps of A, three hit levels
    poses = a["poses"][[0, 2, 1, 6, 3, 5]]
    ct, st = (np.array([1.0]), np.array([0.0])) if n == 1 else trig(n)
    rng = np.random.default_rng(40 + n)
    rows = np.stack([rng.uniform(0.0, a["max_range"], n), rng.uniform(0.5, 3.5, n), rng.uniform(20.0, 60.0, n),
                     rng.uniform(0.0, 12.0, n)]).astype(np.float32)
    rows[0, ::9], rows[3, ::7] = 0.0, np.nan
    rows[2, n // 2] = np.inf
    if n == 1:
        # one beam along the heading: the start cell (EMPTY); one cell on - from pose 0 a cell made free; four on - from
        # pose 1, three cells outside, the occupied row 0; 30 m - through the map or past it
        rows = np.array([[0.0], [1.0], [4.0], [np.inf]], dtype=np.float32)
    return dict(xw=xw, yw=yw, geom=a["geom"], hit_inc=4, maps=a["maps"], pmaps=a["pmaps"], poses=poses, ct=ct, st=st, rows=rows,
                max_range=a["max_range"])


@functools.lru_cache(maxsize=None)
def ref_c(n):
    """The reference on one period of the batch: (ranges, cells) [12, ...] by b % 12, (counts, classes) [84, ...]
    by b % 84."""
    c = case_c(n)
    b12, b84 = np.arange(12), np.arange(C_PERIOD)
    cast = ref_raycast(c["pmaps"], c["geom"], c["poses"][b12 % C_POSES], np.array(C_GOB12), c["ct"], c["st"], c["max_range"])
    score = ref_score(c["pmaps"], c["geom"], c["poses"][b84 % C_POSES], np.array(C_GOB12)[b84 % 12], c["ct"], c["st"],
                      c["rows"][(b84 % C_ROW_PERIOD) % C_ROWS])
    return cast + score


def c_batch(n, B):
    """(poses [B, 3], ranges [B, n], grid_of_batch [B]) of the tiled batch."""
    c, b = case_c(n), np.arange(B)
    return c["poses"][b % C_POSES], c["rows"][(b % C_ROW_PERIOD) % C_ROWS], c_gob(B)


def c_expected(n, B, gob=None):
    """The reference's rows for the batch; rows whose grid_of_batch entry names no map are NaN / (-1, -1) / BAD."""
    r, cells, counts, cls = ref_c(n)
    b = np.arange(B)
    r, cells, counts, cls = r[b % 12], cells[b % 12], counts[b % C_PERIOD], cls[b % C_PERIOD]
    if gob is not None:
        bad = (gob < 0) | (gob >= 3)
        r[bad], cells[bad], cls[bad] = np.nan, -1, R.BAD
        counts[bad] = [0, 0, 0, 0, 0, 0, n]
    return r, cells, counts, cls


# ================================================================== D. the direct engine past 2^28 rays
D_B, D_N = 65537, 4096                  # 2^28 + 4096 rays: the last hypothesis alone is the second pass
D_MAX_RANGE = 3.0
D_FIVE = np.array([[38.5, 32.5, 0.0], [32.5, 25.5, 0.4], [47.5, 46.5, -2.0], [15.5, 30.5, 1.0], [32.5, 32.5, 0.3]])
D_SIXTH = np.array([24.5, 41.5, 2.5])


@functools.lru_cache(maxsize=None)
def case_d():
    ct, st = trig(D_N)
    scan = np.random.default_rng(9).uniform(0.0, 3.0, D_N).astype(np.float32)
    six = np.vstack([D_FIVE, D_SIXTH])
    pm = R.ring_pmap()
    r, _ = ref_raycast([pm], (1.0, 0.0, 0.0), six, np.zeros(6, dtype=int), ct, st, D_MAX_RANGE)
    counts, _ = ref_score([pm], (1.0, 0.0, 0.0), six, np.zeros(6, dtype=int), ct, st, scan)
    return dict(ct=ct, st=st, scan=scan, six=six, ranges=r, counts=counts)


def d_index():
    idx = np.arange(D_B) % 5
    idx[-1] = 5
    return idx


# ================================================================== E. the LDS fit boundary
LDS_BYTES = 64 * 1024                   # kRaycastLdsBytes
E_SHAPES = ((512, 1024), (513, 1024))   # mask of exactly 65 536 bytes, and one row more
N_E = 64


def mask_bytes(xw, yw):
    return xw * ((yw + 31) // 32) * 4


@functools.lru_cache(maxsize=None)
def case_e(xw, yw):
    rng = np.random.default_rng(xw)
    hit = (rng.random((xw, yw)) < 0.01).astype(np.int32)
    pass_ = np.where(rng.random((xw, yw)) < 0.05, rng.integers(1, 1003, (xw, yw)), 0).astype(np.int32)
    hit[xw - 1, ::5] = 1                                               # the last row, the one a short staging copy would lose
    pm = pmap_of(pass_, hit, 20)
    poses = np.array([[xw - 6.5, 500.5, 0.2], [505.5, 1020.5, -1.0], [256.5, 31.5, 1.5], [xw + 1.5, 700.5, 3.0]])
    ct, st = trig(N_E)
    scan = rng.uniform(0.0, 150.0, N_E).astype(np.float32)
    return dict(xw=xw, yw=yw, geom=(1.0, 0.0, 0.0), hit_inc=20, maps=[(pass_, hit, {})], pmaps=[pm], poses=poses, ct=ct, st=st, scan=scan,
                max_range=200.0)


@functools.lru_cache(maxsize=None)
def ref_e(xw, yw):
    c = case_e(xw, yw)
    gob = np.zeros(len(c["poses"]), dtype=int)
    return ref_raycast(c["pmaps"], c["geom"], c["poses"], gob, c["ct"], c["st"], c["max_range"]) + \
        ref_score(c["pmaps"], c["geom"], c["poses"], gob, c["ct"], c["st"], c["scan"])


# ================================================================== F. skip at the ends of a scored line
# (start cell, end cell, what the end cell is) on the ring map (rings of radius 8 and 16 around (32, 32))
F_BEAMS = (((32, 32), (48, 35), "occupied"),       # unflagged, ends on the outer ring
           ((32, 32), (16, 29), "occupied"),       # flagged
           ((40, 28), (40, 36), "occupied"),       # unflagged, along the inner ring's wall: the cell before the end is occupied too
           ((40, 36), (40, 28), "occupied"),       # flagged, the same wall
           ((32, 32), (52, 35), "untouched"),
           ((32, 32), (12, 29), "untouched"),
           ((32, 32), (70, 36), "outside"),
           ((32, 32), (30, 68), "outside"))


def f_case(k):
    """(pose [1, 3], cos_t, sin_t, scan, Lp) of beam k: range 1 from the middle of its start cell, heading 0."""
    s, e, _ = F_BEAMS[k]
    ct, st = R.tables_to([e], s)
    return np.array([[s[0] + 0.5, s[1] + 0.5, 0.0]]), ct, st, np.ones(1, dtype=np.float32), len(O.bresenham_path(s, e))


def f_expected(k, skip):
    """(class, ranges, cells) of beam k at `skip` by the reference."""
    pose, ct, st, scan, _ = f_case(k)
    pm = R.ring_pmap()
    cls = R.score(pm, 1.0, 0.0, 0.0, pose[0], R.table_points(scan, ct, st), skip)[1][0]
    r, cells = R.raycast(pm, 1.0, 0.0, 0.0, pose[0], ct, st, 1.0, skip)
    return cls, r, cells
