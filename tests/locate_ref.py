"""NumPy restatement of global scan localisation (include/slam_hip.h, "global scan localisation: exact branch and
bound on a pyramid of the field"), written from its stated semantics:

    offsets(...)     the scan discretised for one rotation: (ax, ay) of the used beams that are on, the number that are off
    volume(...)      the definition by brute force: shifted adds of the field, the whole cost volume [K, ni, nj]
    brute(...)       (best (k, i, j), cost, used) of that volume: the smallest (cost, flat)
    level(...)       P_h with its padding, from the definition (a min over 2^h x 2^h cells; min is separable)
    search(...)      the two-step search with Python / NumPy integers: incumbent by descent, then the sweep; stats included
    locate_batch(..) the batch, hypothesis by hypothesis

The field is tests/match_ref.field; the inputs are those of tests/raycast_ref.py and tests/match_ref.py plus the ragged maps."""
import numpy as np

import match_ref as M

LIM = float(1 << 20)


def offsets(ranges, cos_t, sin_t, c, s, scale, max_range):
    """(ax int64 [m], ay int64 [m], off, used) of one rotation."""
    r32 = np.asarray(ranges, dtype=np.float32)
    rr = r32.astype(np.float64)
    use = np.isfinite(rr) & (r32 < np.float32(max_range))
    rr = rr[use]
    with np.errstate(all="ignore"):
        lx, ly = np.asarray(cos_t, dtype=np.float64)[use] * rr, np.asarray(sin_t, dtype=np.float64)[use] * rr
        vx = float(scale) * (float(c) * lx + (-float(s)) * ly)
        vy = float(scale) * (float(s) * lx + float(c) * ly)
        on = (np.abs(vx) < LIM) & (np.abs(vy) < LIM)                 # NaN and inf compare false
        ax, ay = np.floor(vx[on] + 0.5).astype(np.int64), np.floor(vy[on] + 0.5).astype(np.int64)
    return ax, ay, int(np.count_nonzero(~on)), int(np.count_nonzero(use))


def whole(fld):
    return (0, 0, fld.shape[0], fld.shape[1])


def volume(fld, scale, ranges, cos_t, sin_t, rot_cs, region, max_range, cap):
    """costs int64 [K, ni, nj] and used: every candidate by the definition, one shifted add of the field per beam."""
    fld = np.asarray(fld).astype(np.int64)
    xw, yw = fld.shape
    i0, j0, ni, nj = (int(v) for v in region)
    rot_cs = np.asarray(rot_cs, dtype=np.float64).reshape(-1, 2)
    out = np.zeros((len(rot_cs), ni, nj), dtype=np.int64)
    used = 0
    for k, (c, s) in enumerate(rot_cs):
        ax, ay, off, used = offsets(ranges, cos_t, sin_t, c, s, scale, max_range)
        out[k] += off * cap
        for dx, dy in zip(ax.tolist(), ay.tolist()):
            e = np.full((ni, nj), cap, dtype=np.int64)
            lo_i, hi_i = max(i0, -dx), min(i0 + ni, xw - dx)         # robot cells i with 0 <= i + dx < xw
            lo_j, hi_j = max(j0, -dy), min(j0 + nj, yw - dy)
            if lo_i < hi_i and lo_j < hi_j:
                e[lo_i - i0:hi_i - i0, lo_j - j0:hi_j - j0] = fld[lo_i + dx:hi_i + dx, lo_j + dy:hi_j + dy]
            out[k] += e
    return out, used


def brute(fld, scale, ranges, cos_t, sin_t, rot_cs, region, max_range, cap):
    """((k, i, j), cost, used): the first smallest of the flattened volume is the smallest (cost, flat)."""
    vol, used = volume(fld, scale, ranges, cos_t, sin_t, rot_cs, region, max_range, cap)
    i0, j0, ni, nj = (int(v) for v in region)
    if used == 0:
        return (0, i0, j0), 0, 0
    flat = int(np.argmin(vol.reshape(-1)))
    return (flat // (ni * nj), i0 + flat // nj % ni, j0 + flat % nj), int(vol.reshape(-1)[flat]), used


def level(fld, h, cap):
    """P_h stored from -(2^h - 1): out[x + pad][y + pad] = min over 0 <= a, b < 2^h of E(x + a, y + b)."""
    fld = np.asarray(fld).astype(np.int64)
    xw, yw = fld.shape
    s = 1 << h
    pad = s - 1
    e = np.full((xw + 2 * pad, yw + 2 * pad), cap, dtype=np.int64)   # E for -pad <= x < xw + pad
    e[pad:pad + xw, pad:pad + yw] = fld
    rows = e[:xw + pad].copy()
    for a in range(1, s):
        np.minimum(rows, e[a:a + xw + pad], out=rows)
    out = rows[:, :yw + pad].copy()
    for b in range(1, s):
        np.minimum(out, rows[:, b:b + yw + pad], out=out)
    return out


def level_at(P, h, x, y, cap):
    pad = (1 << h) - 1
    u, v = np.asarray(x) + pad, np.asarray(y) + pad
    ok = (u >= 0) & (u < P.shape[0]) & (v >= 0) & (v < P.shape[1])
    return np.where(ok, P[np.where(ok, u, 0), np.where(ok, v, 0)], cap)


def pyramid(fld, H, cap):
    return [level(fld, h, cap) for h in range(H + 1)]


def search(pyr, scale, ranges, cos_t, sin_t, rot_cs, region, H, max_range, cap):
    """((k, i, j), cost, used, stats int64 [H + 2]) of one hypothesis on its pyramid ``pyr`` = [P_0 .. P_H]."""
    i0, j0, ni, nj = (int(v) for v in region)
    rot_cs = np.asarray(rot_cs, dtype=np.float64).reshape(-1, 2)
    K = len(rot_cs)
    offs = [offsets(ranges, cos_t, sin_t, c, s, scale, max_range) for c, s in rot_cs]
    used = offs[0][3]
    stats = np.zeros(H + 2, dtype=np.int64)
    if used == 0:
        return (0, i0, j0), 0, 0, stats
    nI = [-(-ni // (1 << h)) for h in range(H + 1)]
    nJ = [-(-nj // (1 << h)) for h in range(H + 1)]

    def bound(h, k, I, J):
        ax, ay, off, _ = offs[k]
        x = i0 + np.asarray(I, dtype=np.int64)[:, None] * (1 << h) + ax[None, :]
        y = j0 + np.asarray(J, dtype=np.int64)[:, None] * (1 << h) + ay[None, :]
        return level_at(pyr[h], h, x, y, cap).sum(axis=1) + off * cap

    def kids(h, I, J):                                               # children at level h of the nodes (I, J) of level h + 1
        cI = (2 * I[:, None] + np.array([0, 0, 1, 1])).reshape(-1)
        cJ = (2 * J[:, None] + np.array([0, 1, 0, 1])).reshape(-1)
        ok = (cI < nI[h]) & (cJ < nJ[h])
        return cI[ok], cJ[ok]

    tI, tJ = (a.reshape(-1) for a in np.meshgrid(np.arange(nI[H]), np.arange(nJ[H]), indexing="ij"))
    top = np.stack([bound(H, k, tI, tJ) for k in range(K)])
    # 1. the incumbent: the smallest (LB, node index), then down by the smallest (LB, I, J)
    node = int(np.argmin(top.reshape(-1)))
    k, I, J = node // (nI[H] * nJ[H]), int(tI[node % (nI[H] * nJ[H])]), int(tJ[node % (nI[H] * nJ[H])])
    U = int(top.reshape(-1)[node])
    for h in range(H - 1, -1, -1):
        cI, cJ = kids(h, np.array([I]), np.array([J]))               # in (I, J) order
        lb = bound(h, k, cI, cJ)
        w = int(np.argmin(lb))
        I, J, U = int(cI[w]), int(cJ[w]), int(lb[w])
    # 2. the sweep, U fixed
    stats[H], stats[H + 1] = K * nI[H] * nJ[H], U
    best = None
    for k in range(K):
        keep = top[k] <= U
        I, J, lb = tI[keep], tJ[keep], top[k][keep]
        for h in range(H - 1, -1, -1):
            I, J = kids(h, I, J)
            stats[h] += len(I)
            lb = bound(h, k, I, J)
            keep = lb <= U
            I, J, lb = I[keep], J[keep], lb[keep]
        if len(I):
            keys = (lb.astype(np.int64) << 32) | ((k * ni + I) * nj + J)
            best = int(keys.min()) if best is None else min(best, int(keys.min()))
    flat, cost = best & 0xffffffff, best >> 32
    return (flat // (ni * nj), i0 + flat // nj % ni, j0 + flat % nj), cost, used, stats


def locate_batch(fields, scale, ranges, cos_t, sin_t, rot_cs, H, max_range, cap, maps=None, regions=None, B=None):
    """fields [G, xw, yw]; ranges [n] (shared) or [B, n]; maps None or [B]; regions None or [B, 4].  Returns best int32
    [B, 3], cost int32 [B], used int32 [B], stats int64 [B, H + 2]; a hypothesis whose map entry is outside [0, G), or
    whose region is empty or not inside the map, gets -1 / -1 / 0 and stats of 0."""
    ranges = np.asarray(ranges, dtype=np.float32)
    if B is None:
        B = len(ranges) if ranges.ndim == 2 else len(maps) if maps is not None else len(regions) if regions is not None else 1
    best, cost, used = np.full((B, 3), -1, dtype=np.int32), np.full(B, -1, dtype=np.int32), np.zeros(B, dtype=np.int32)
    stats = np.zeros((B, H + 2), dtype=np.int64)
    pyrs = {}
    for b in range(B):
        gi = 0 if maps is None else int(maps[b])
        if not 0 <= gi < len(fields):
            continue
        xw, yw = fields[gi].shape
        reg = (0, 0, xw, yw) if regions is None else tuple(int(v) for v in regions[b])
        if reg[0] < 0 or reg[1] < 0 or reg[2] < 1 or reg[3] < 1 or reg[0] + reg[2] > xw or reg[1] + reg[3] > yw:
            continue
        if gi not in pyrs:
            pyrs[gi] = pyramid(fields[gi], H, cap)
        out = search(pyrs[gi], scale, ranges if ranges.ndim == 1 else ranges[b], cos_t, sin_t, rot_cs, reg, H, max_range, cap)
        best[b], cost[b], used[b], stats[b] = out
    return best, cost, used, stats


def rotations(n_rot):
    th = -np.pi + np.arange(int(n_rot)) * (2.0 * np.pi / int(n_rot))
    return th, np.stack([np.cos(th), np.sin(th)], axis=-1)


def pose_of(best, scale, off_x, off_y, rot_cs):
    k, i, j = (int(v) for v in best)
    return np.array([(i + 0.5) / scale - off_x, (j + 0.5) / scale - off_y, np.arctan2(rot_cs[k][1], rot_cs[k][0])])


# ---------------------------------------------------------------- shared inputs
RAGGED = ((33, 35), (70, 33), (40, 70))


def ragged_pmap(xw, yw, seed=0):
    """An xw x yw map with occupied cells in the four corners, down the last column and scattered inside."""
    rng = np.random.default_rng(100 + seed)
    pm = np.full((xw, yw), 50, dtype=np.int8)
    cells = [(0, 0), (0, yw - 1), (xw - 1, 0), (xw - 1, yw - 1)] + [(x, yw - 1) for x in range(3, xw, 7)]
    cells += [(int(x), int(y)) for x, y in zip(rng.integers(0, xw, 25), rng.integers(0, yw, 25))]
    for x, y in cells:
        pm[x, y] = 100
    return pm, cells


def ragged_scan(n, seed=0, reach=24.0):
    """Beam tables over the full circle and ranges (cells at scale 1) up to ``reach``."""
    rng = np.random.default_rng(200 + seed)
    ang = np.linspace(-3.0, 3.1, n)
    return np.cos(ang), np.sin(ang), rng.uniform(2.0, reach, n).astype(np.float32)


ROOM_K, ROOM_H = 256, 5
ROOM_ARGS = dict(max_range=30.0, cap=64)
_room = {}


def room_case(syn):
    """The room of tests/match_ref.py located globally: the last scan, K = 256, H = 5, the whole map; computed once per
    process.  A dict of match_ref's case plus rot_cs [K, 2], thetas and the restatement's (best, cost, used, stats)."""
    if not _room:
        case = dict(M.room_case(syn))
        th, rot = rotations(ROOM_K)
        pyr = pyramid(case["field"], ROOM_H, ROOM_ARGS["cap"])
        ref = search(pyr, 20.0, case["scan"], case["cos_t"], case["sin_t"], rot, whole(case["field"]), ROOM_H, **ROOM_ARGS)
        case.update(loc_thetas=th, loc_rot=rot, loc_ref=ref)
        _room.update(case)
    return _room
