"""Deterministic inputs for the two ray casts of maps much larger than an LDS window - the direction wedges
(k_wedge_sort / k_wedge_order / k_wedge_cast: grid_mode 4, and 1 on a large map) and the recorded-walk tiles
(grid_mode 2) - and an integer model of how the wedges deal rays to workgroups.  NumPy only.

What the inputs reach is asserted without a GPU in test_wedge_cases.py; test_gpu_wedge_forms.py casts them.

The model is a port of csrc/grid_walk.h (ray_setup) and csrc/grid_kernels.hip (wedge_class, wedge_shear, the group rule
of launch_wedges, plan_cast): a ray is one of 16 classes - (steep?, walk runs towards the origin?) x four equal parts
of minor / major in [-1, 1] -; a (group of scans, class) UNIT is cut into PARTS of 2 048 rays; a part sweeps its rays
in BANDS of at most 512 rows of the walk axis, fewer where the band's parallelogram (width Hw in the sheared coordinate
v = y - M a) would not fit the 37 888 window cells, and a band wider than half the window goes by direct atomics.

A case is a dict: dims (xw, yw, scale, off_x, off_y), orgs [B, 2] origin cells, ends [B, n, 2] end cells, group (the
grid_group option).  world(case) gives the coordinates of the cell centres, (cell + 0.5) / scale - off."""
import numpy as np

CLASSES = 16
SLOPES = 4
PART_RAYS = 2048
BAND_ROWS = 512
WIN_CELLS = 37888
LEN_BIN = 16
KWIN_CELLS = 36864                 # a map is "large" past 8 of these (plan_cast)
MAX_SIDE = 65535                   # end cells travel as 16-bit pairs
TILE_MAX_BEAMS = 8192
SCALE = 20.0                       # 0.05 m cells


# ------------------------------------------------------------------ the model
def ray_setup(sx, sy, ex, ey):
    """grid_walk.h ray_setup on integer arrays: dict of valid, steep, flag, x0, y0, dx, dy, ystep (walk coordinates)."""
    sx, sy, ex, ey = (np.asarray(v, dtype=np.int64) for v in (sx, sy, ex, ey))
    valid = ~((sx == ex) & (sy == ey))
    steep = np.abs(ey - sy) > np.abs(ex - sx)
    sx, sy, ex, ey = np.where(steep, sy, sx), np.where(steep, sx, sy), np.where(steep, ey, ex), np.where(steep, ex, ey)
    flag = sx > ex
    sx, ex, sy, ey = np.where(flag, ex, sx), np.where(flag, sx, ex), np.where(flag, ey, sy), np.where(flag, sy, ey)
    return dict(valid=valid, steep=steep, flag=flag, x0=sx, y0=sy, dx=ex - sx, dy=np.abs(ey - sy), ystep=np.where(sy < ey, 1, -1))


def wedge_class(steep, flag, ddx, ddy):
    """wedge_class: ddx, ddy = end cell - origin cell (before any swap).  Rays with ddx == ddy == 0 have no class."""
    maj, mnr = np.where(steep, ddy, ddx).astype(np.int64), np.where(steep, ddx, ddy).astype(np.int64)
    amaj = np.maximum(np.abs(maj), 1)
    q = np.minimum(SLOPES - 1, ((mnr * np.where(maj < 0, -1, 1) + amaj) * SLOPES) // (2 * amaj))   # (the numerator is >= 0)
    return (np.where(steep, 2, 0) + np.where(flag, 1, 0)) * SLOPES + q


def wedge_shear(cls):
    mid2 = 2 * (2 * (np.asarray(cls) % SLOPES) + 1 - SLOPES)
    return np.where(mid2 >= SLOPES, 1, np.where(mid2 <= -SLOPES, -1, 0))


def group_size(group, n, scans):
    """launch_wedges / launch_tiles: scans per group."""
    return min(group if group > 0 else 16, max(1, 65535 // n), scans)


def plan_cast(xw, yw, mode, n, maps=False):
    """plan_cast for slam_grid_update without grid_of_batch and for the replay entries (maps: grid_of_traj given)."""
    big = xw * yw > 8 * KWIN_CELLS
    wok = mode != 2 and xw <= MAX_SIDE and yw <= MAX_SIDE
    if mode in (1, 2, 4) and n <= TILE_MAX_BEAMS and (big or mode in (2, 4)) and (not maps or wok):
        return "wedges" if wok else "tiles"
    return "window" if mode != 0 and n <= 65535 else "direct"


def classify(case):
    """Per ray [B, n]: the ray_setup fields, cls (-1: no ray - end cell = origin cell), and unit = group * 16 + cls."""
    orgs, ends = case["orgs"], case["ends"]
    B, n = ends.shape[:2]
    r = ray_setup(orgs[:, None, 0], orgs[:, None, 1], ends[..., 0], ends[..., 1])
    cls = wedge_class(r["steep"], r["flag"], ends[..., 0] - orgs[:, None, 0], ends[..., 1] - orgs[:, None, 1])
    r["cls"] = np.where(r["valid"], cls, -1)
    G = group_size(case["group"], n, B)
    r["G"] = G
    r["unit"] = np.where(r["valid"], (np.arange(B)[:, None] // G) * CLASSES + cls, -1)
    return r


def unit_rays(case):
    """{unit: rays} of the case's launch."""
    u = classify(case)["unit"]
    vals, counts = np.unique(u[u >= 0], return_counts=True)
    return dict(zip(vals.tolist(), counts.tolist()))


def parts_of(rays):
    return [min(PART_RAYS, rays - k) for k in range(0, rays, PART_RAYS)]


def walk_coords(cells, steep):
    """(a, y): walk axis and the other axis of map cells [k, 2]."""
    return (cells[:, 1], cells[:, 0]) if steep else (cells[:, 0], cells[:, 1])


def band_model(a, v):
    """Fewest bands any sweep of a part can take, from the part's true pass cells (a: walk axis, v: sheared coordinate):
    greedy bands of the most rows that the cells' own extent allows - every sub-range of a feasible band is feasible, so
    the greedy count is a lower bound on the kernel's, whose widths (predicted, rounded to even) are no smaller.
    Returns [(a_lo, rows, Hw_lb, direct)]: Hw_lb the v extent of the true cells in the band (0: none), direct: not even
    two rows of it fit (Hw_lb * 2 > 37 888), so the kernel certainly casts the band by direct atomics."""
    a, v = np.asarray(a), np.asarray(v)
    out, a_lo, a_end = [], int(a.min()) & ~1, int(a.max())
    while a_lo <= a_end:
        rows = (min(a_end - a_lo + 1, BAND_ROWS) + 1) & ~1
        for _ in range(2):
            m = (a >= a_lo) & (a < a_lo + rows)
            hw = int(v[m].max() - v[m].min() + 1) if m.any() else 0
            fit = (WIN_CELLS // hw) & ~1 if hw else rows
            if fit < 2 or rows <= fit:
                break
            rows = fit
        m = (a >= a_lo) & (a < a_lo + rows)
        hw = int(v[m].max() - v[m].min() + 1) if m.any() else 0
        out.append((a_lo, rows, hw, hw * 2 > WIN_CELLS))
        a_lo += rows
    return out


def float_walk_ties(dx, dy):
    """Walk steps at which the reference's float error term is exactly 0.5 after the add (bresenham.py:51-53)."""
    if dx == 0:
        return 0
    derr, error, ties = dy / dx, 0.0, 0
    for _ in range(dx + 1):
        error += derr
        ties += error == 0.5
        if error >= 0.5:
            error -= 1.0
    return ties


# ------------------------------------------------------------------ builders
def dims_of(xw, yw):
    return (xw, yw, SCALE, xw / (2.0 * SCALE), yw / (2.0 * SCALE))


def make(dims, orgs, ends, group=0):
    orgs, ends = np.asarray(orgs, dtype=np.int64), np.asarray(ends, dtype=np.int64)
    assert orgs.ndim == 2 and ends.ndim == 3 and len(orgs) == len(ends)
    return dict(dims=dims, orgs=orgs, ends=ends, group=group)


def world(case):
    """OX, OY [B, n], CX, CY [B]: the centres of the end and origin cells."""
    _, _, scale, off_x, off_y = case["dims"]
    e, o = case["ends"], case["orgs"]
    return (e[..., 0] + 0.5) / scale - off_x, (e[..., 1] + 0.5) / scale - off_y, (o[:, 0] + 0.5) / scale - off_x, (o[:, 1] + 0.5) / scale - off_y


def to_cell(v, scale, off):
    """mapping.py:33-36, int(scale * (v + off))."""
    return np.trunc(scale * (np.asarray(v) + off)).astype(np.int64)


def transposed(case):
    xw, yw, scale, off_x, off_y = case["dims"]
    return make((yw, xw, scale, off_y, off_x), case["orgs"][:, ::-1], case["ends"][..., ::-1], case["group"])


def _fit(cells, n):
    return (list(cells) * (n // len(cells) + 1))[:n]


def _ring(x_lo, x_hi, y_lo, y_hi, step=1):
    cells = [(x, y_lo) for x in range(x_lo, x_hi + 1, step)] + [(x, y_hi) for x in range(x_lo, x_hi + 1, step)]
    return cells + [(x_lo, y) for y in range(y_lo, y_hi + 1, step)] + [(x_hi, y) for y in range(y_lo, y_hi + 1, step)]


# A. class boundaries
A_LENGTHS = (1, 2, 3, 4, 40, 400)
A_RATIOS = tuple((k, 4) for k in range(-4, 5))          # minor / major = k / 4
A_ORG = (450, 450)


def case_a():
    """Scan 0: from one origin, for either major axis and either sign of it, major lengths 1 .. 400 and every minor
    offset that gives minor / major in {-1, -3/4, .., 1} exactly, and one cell of minor either side of each (|minor| =
    major + 1 turns the ray to the other steepness; |minor| == major is adx == ady: not steep); 16 rays of no length.
    Scan 1: rays of length 1 only, the eight neighbours of the origin."""
    rays = []
    for L in A_LENGTHS:
        minors = sorted({k * L // 4 + d for k, q in A_RATIOS if (k * L) % q == 0 for d in (-1, 0, 1)})
        for sgn in (1, -1):
            for m in minors:
                rays.append((sgn * L, m))                 # major axis x
                rays.append((m, sgn * L))                 # major axis y
    rays += [(0, 0)] * 16
    n = len(rays)
    near = [(dx, dy) for dx in (-1, 0, 1) for dy in (-1, 0, 1) if (dx, dy) != (0, 0)]
    ends = np.array([rays, _fit(near, n)]) + np.array(A_ORG)
    return make(dims_of(900, 900), [A_ORG, A_ORG], ends)


# B. bands
def case_b1():
    """One class (not steep, away from the origin, slopes 0.03 .. 0.05: a pencil narrow enough for bands of the full 512
    rows) with rays 520, 1 030 and 1 540 cells long from one origin: they end in the 2nd, 3rd and 4th band."""
    org = (30, 350)
    ends = [(org[0] + L, org[1] + m) for L in (520, 1030, 1540) for m in range(-(-3 * L // 100), 5 * L // 100 + 1)]
    return make(dims_of(1600, 700), [org], [ends])


def case_b2():
    """16 scans of one group from origins 20 cells apart across the minor axis, every scan with the same pencil of rays
    600 cells long: the class is 300 cells wide plus the pencil, so a band is cut down to about 37 888 / 330 rows."""
    orgs = [(20, 100 + 20 * s) for s in range(16)]
    ends = [[(o[0] + 600, o[1] + m) for m in range(18, 31)] for o in orgs]
    return make(dims_of(700, 500), orgs, ends)


B3_DIMS = dims_of(640, 20000)


def case_b3():
    """Scans 0 and 1 cast the same class from origins 19 200 cells apart on the minor axis (rays up to 500 cells long from
    x = 4: the first band of 512 rows is wider than any window); scan 2 casts that class from x = 604 next to scan 0: the
    band from row 516 on holds its rays alone and fits.  The walk axis needs 600 cells and more for this, so the map is
    640 x 20 000."""
    orgs = [(4, 300), (4, 19500), (604, 320)]
    pencil = [(L, m) for L in (100, 200, 300, 400, 500) for m in range(L // 10, L // 4, max(1, L // 50))]
    far = _fit([(L, m) for L in (20, 28, 35) for m in range(1, L // 3)], len(pencil))
    ends = [[(o[0] + L, o[1] + m) for L, m in (far if k == 2 else pencil)] for k, o in enumerate(orgs)]
    return make(B3_DIMS, orgs, ends)


# C. parts
def case_c(scans, n, group=0):
    """Every beam of every scan in ONE class: not steep, away from the origin, slopes 0.06 .. 0.44 (strictly inside the
    quarter [0, 1/2)), lengths 40 .. 399, from origins a few cells apart."""
    i = np.arange(n)
    L = 40 + (i * 7) % 360
    m = (L * (0.06 + 0.38 * ((i * 131) % 997) / 997.0)).astype(np.int64)
    orgs = np.array([(100 + s % 5, 280 + (s * 3) % 17) for s in range(scans)])
    ends = np.stack([np.stack([o[0] + np.roll(L, -s), o[1] + np.roll(m, -s)], axis=1) for s, o in enumerate(orgs)])
    return make(dims_of(600, 600), orgs, ends, group)


C_CASES = {"one_part": (16, 128, 0), "two_parts": (16, 129, 0), "three_parts": (64, 65, 64), "ragged_groups": (9, 8192, 64)}
C_UNIT_RAYS = {"one_part": [2048], "two_parts": [2064], "three_parts": [4160], "ragged_groups": [7 * 8192, 2 * 8192]}


# D. rows of an odd length
D_MAPS = ((601, 601), (600, 601), (601, 600))


def case_d(xw, yw):
    """Full-circle fans to the map's border (every third cell and the four corners) from an origin with an even and one
    with an odd pcx, and from origins in the last row (x = xw - 1) and the last column (y = yw - 1)."""
    ends = _ring(0, xw - 1, 0, yw - 1, 3) + [(0, 0), (xw - 1, yw - 1), (0, yw - 1), (xw - 1, 0)]
    orgs = [(300, 301), (301, 298), (xw - 1, 250), (251, yw - 1)]
    return make(dims_of(xw, yw), orgs, [ends] * len(orgs))


# E. sides
def case_e(xw):
    """Origins and ends in the 300 columns below x = 65 535 of an xw x 8 map."""
    ends = _ring(65236, 65534, 0, 7) + [(x, 3 + (x % 3)) for x in range(65240, 65534, 5)]
    orgs = [(65400, 3), (65534, 7), (65237, 0)]
    return make(dims_of(xw, 8), orgs, [ends] * len(orgs))


# F. a map per trajectory at odd cell offsets
F_SIDE, F_RESO, F_MAPS, F_SCANS, F_BEAMS = 601, 0.05, 3, 5, 90
F_ROUTES = ([2, 1, 0], [1, 1, 0])
F_POSE0 = np.array([[0.0, 0.0, 0.0], [0.4, -0.3, 0.5], [-0.6, 0.5, -1.1]])
F_AMIN, F_AMAX = -3.14159, 3.14159


def case_f(syn):
    """ranges [3, 5, 90]: three trajectories of synthetic.make_replay."""
    return np.stack([syn.make_replay(F_SCANS, F_BEAMS, seed=41 + l).ranges for l in range(F_MAPS)])
