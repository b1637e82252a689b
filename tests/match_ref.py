"""NumPy reference of the distance field of the grid and of the window matcher on it (include/slam_hip.h,
"distance field of the map and the window scan-to-map matcher"), written from their stated semantics:

    field(pmap, cap)    min(cap, min over cells with pmap == 100 of (x-u)^2 + (y-v)^2), by brute force
    match(...)          one hypothesis: the cost of every candidate of its window, the best flat index (the first
                        smallest), its cost and the number of used beams

The cost loop is the header's expression, beam by beam, on ``raycast_ref.to_cell``; the inputs are those of
tests/raycast_ref.py (ring_pmap, room, room_pmap)."""
import numpy as np

import raycast_ref as R


def field(pmap, cap):
    pmap = np.asarray(pmap)
    xw, yw = pmap.shape
    occ = np.argwhere(pmap == 100).astype(np.int64)
    out = np.full((xw, yw), int(cap), dtype=np.int64)
    xs, ys = np.arange(xw, dtype=np.int64)[:, None], np.arange(yw, dtype=np.int64)[None, :]
    for u, v in occ:
        np.minimum(out, (xs - u) ** 2 + (ys - v) ** 2, out=out)
    return out.astype(np.int16)


def rotations(theta, n_rot, rot_step):
    """(angles [K], rot_cs [K, 2]) as Mapping.match_scan forms them."""
    th = float(theta) + (np.arange(int(n_rot)) - int(n_rot) // 2) * float(rot_step)
    return th, np.stack([np.cos(th), np.sin(th)], axis=-1)


def match(fld, scale, off_x, off_y, ranges, centre, cos_t, sin_t, rot_cs, nx, ny, step, max_range, cap):
    """(best, best cost, used, costs int32 [K, 2 nx + 1, 2 ny + 1]) of one hypothesis; fld None: it names no map."""
    rot_cs = np.asarray(rot_cs, dtype=np.float64).reshape(-1, 2)
    K, wx, wy = rot_cs.shape[0], 2 * nx + 1, 2 * ny + 1
    cx, cy = float(centre[0]), float(centre[1])
    costs = np.full((K, wx, wy), -1, dtype=np.int32)
    if (fld is None or not (np.isfinite(cx) and np.isfinite(cy)) or R.to_cell(cx, scale, off_x) is None
            or R.to_cell(cy, scale, off_y) is None):
        return -1, -1, 0, costs
    ranges = np.asarray(ranges, dtype=np.float32)
    mr = np.float32(max_range)
    beams = []
    for t in range(len(ranges)):
        rr = float(ranges[t])
        if np.isfinite(rr) and ranges[t] < mr:
            beams.append((float(cos_t[t]) * rr, float(sin_t[t]) * rr))
    xw, yw = fld.shape
    for k in range(K):
        c, s = float(rot_cs[k][0]), float(rot_cs[k][1])
        for i in range(wx):
            px = cx + float(i - nx) * step
            for j in range(wy):
                py = cy + float(j - ny) * step
                cost = 0
                for lx, ly in beams:
                    x = c * lx + (-s) * ly + px * 1.0
                    y = s * lx + c * ly + py * 1.0
                    ex, ey = R.to_cell(x, scale, off_x), R.to_cell(y, scale, off_y)
                    if ex is not None and ey is not None and 0 <= ex < xw and 0 <= ey < yw:
                        cost += int(fld[ex][ey])
                    else:
                        cost += cap
                costs[k, i, j] = cost
    best = int(np.argmin(costs.reshape(-1)))            # the first smallest: the lowest flat index
    return best, int(costs.reshape(-1)[best]), len(beams), costs


def match_batch(fields, scale, off_x, off_y, ranges, centres, cos_t, sin_t, rot_cs, nx, ny, step, max_range, cap, maps=None):
    """The batch, hypothesis by hypothesis: fields [G, xw, yw], ranges [n] (shared) or [B, n], maps None or [B]
    (an entry outside [0, G): no map).  Returns best [B], cost [B], used [B], costs [B, K, wx, wy], all int32."""
    ranges = np.asarray(ranges, dtype=np.float32)
    out = []
    for b, ctr in enumerate(np.asarray(centres, dtype=np.float64).reshape(-1, 2)):
        gi = 0 if maps is None else int(maps[b])
        fld = fields[gi] if 0 <= gi < len(fields) else None
        out.append(match(fld, scale, off_x, off_y, ranges if ranges.ndim == 1 else ranges[b], ctr, cos_t, sin_t, rot_cs[b], nx, ny,
                         step, max_range, cap))
    return (np.array([o[0] for o in out], dtype=np.int32), np.array([o[1] for o in out], dtype=np.int32),
            np.array([o[2] for o in out], dtype=np.int32), np.stack([o[3] for o in out]))


def pose_of(centre, thetas, best, nx, ny, step):
    """The pose of flat index ``best``: the reference's own restatement of match_pose."""
    wx, wy = 2 * nx + 1, 2 * ny + 1
    k, i, j = best // (wx * wy), best // wy % wx, best % wy
    return np.array([centre[0] + float(i - nx) * step, centre[1] + float(j - ny) * step, thetas[k]])


# ---------------------------------------------------------------- the recovery case (issue text; room map)
ROOM_OFFSET = np.array([0.12, -0.08, 0.05])
ROOM_ARGS = dict(nx=4, ny=4, step=0.05, max_range=30.0, cap=64)
ROOM_K, ROOM_ROT_STEP = 11, 0.01


_room = {}


def room_case(syn):
    """The recovery case and the reference's answer to it, computed once per process: a dict of the scans and poses
    that build the map, pmap, field, the last scan, the true pose, the start pose, angles [K], rot_cs [K, 2], the beam
    tables and (best, cost, used, costs) of the reference."""
    if not _room:
        ranges, poses, _ = R.room(syn)
        pm = R.room_pmap(ranges, poses)
        true = poses[-1]
        start = true + ROOM_OFFSET
        th, rot = rotations(start[2], ROOM_K, ROOM_ROT_STEP)
        ang = np.linspace(R.AMIN, R.AMAX, ranges.shape[1])
        ct, st = np.cos(ang), np.sin(ang)
        fld = field(pm, ROOM_ARGS["cap"])
        ref = match(fld, 20.0, 10.0, 10.0, ranges[-1], start[:2], ct, st, rot, **ROOM_ARGS)
        _room.update(ranges=ranges, poses=poses, pmap=pm, field=fld, scan=ranges[-1], true=true, start=start, thetas=th, rot_cs=rot,
                     cos_t=ct, sin_t=st, ref=ref)
    return _room
