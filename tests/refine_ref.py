"""slam_grid_refine (include/slam_refine.h) restated twice from its contract (test infrastructure only):

    refine(...)       NumPy float64: the beams of an evaluation as arrays, elementwise operations in the contract's order
                      (NumPy fuses nothing), the ten sums by numpy.sum; math.cos / math.sin of the heading
    refine_mp(...)    the same, operation by operation, in mpmath at 50 digits: every input enters as the float64 (or
                      float32) it is, the pose is carried at full precision from step to step, and the closest that any
                      u or v of any evaluation comes to an integer is returned with the answer ("sure" cases)

Both take one hypothesis: fld int16 [xw, yw] or None (the entry names no map), the index rule, ranges float32 [n], the
pose [3], the beam tables, iters, damping, step_cells, step_rad, max_range, cap.  Both return a dict: pose [3], cost [2],
used, normal [9] = (Hxx, Hxy, Hxt, Hyy, Hyt, Htt, gx, gy, gt), status; refine_mp adds ``margin``.  ``batch`` runs a batch
hypothesis by hypothesis."""
import math

import numpy as np
from mpmath import mp, mpf

DIGITS = 50
mp.dps = DIGITS
OFF = 2.0 ** 20
OK, BAD_POSE, NO_MAP = 0, 1, 2


def used_beams(ranges, cos_t, sin_t, max_range):
    """(indices of the used beams, rr float64 of them): isfinite(rr) and ranges[t] < max_range as float32."""
    r = np.asarray(ranges, dtype=np.float32)
    keep = np.isfinite(r) & (r < np.float32(max_range))
    t = np.flatnonzero(keep)
    return t, r[t].astype(np.float64)


def status_of(fld, scale, off_x, off_y, pose):
    if fld is None:
        return NO_MAP
    px, py, th = (float(v) for v in pose)
    if not (math.isfinite(px) and math.isfinite(py) and math.isfinite(th)):
        return BAD_POSE
    if not (abs(scale * (px + off_x) - 0.5) < OFF and abs(scale * (py + off_y) - 0.5) < OFF):
        return BAD_POSE
    return OK


def unanswered(pose, status):
    return dict(pose=np.array(pose, dtype=np.float64), cost=np.array([-1.0, -1.0]), used=0, normal=np.zeros(9), status=status,
                margin=math.inf)


def evaluate(d, sd, scale, off_x, off_y, lx, ly, px, py, th):
    """The ten sums at a pose, NumPy float64: d float64 [xw, yw] the distances in cells, lx, ly the used beams."""
    c, s = math.cos(th), math.sin(th)
    x = c * lx + (-s) * ly + px
    y = s * lx + c * ly + py
    u = scale * (x + off_x) - 0.5
    v = scale * (y + off_y) - 0.5
    with np.errstate(invalid="ignore"):
        on = (np.abs(u) < OFF) & (np.abs(v) < OFF)
    uu, vv = np.where(on, u, 0.0), np.where(on, v, 0.0)
    fi, fj = np.floor(uu), np.floor(vv)
    a, b = uu - fi, vv - fj
    i, j = fi.astype(np.int64), fj.astype(np.int64)
    xw, yw = d.shape

    def at(i, j):
        inside = (i >= 0) & (i < xw) & (j >= 0) & (j < yw)
        return np.where(inside, d[np.clip(i, 0, xw - 1), np.clip(j, 0, yw - 1)], sd)
    d00, d10, d01, d11 = at(i, j), at(i + 1, j), at(i, j + 1), at(i + 1, j + 1)
    r = (1.0 - b) * ((1.0 - a) * d00 + a * d10) + b * ((1.0 - a) * d01 + a * d11)
    mx = scale * ((1.0 - b) * (d10 - d00) + b * (d11 - d01))
    my = scale * ((1.0 - a) * (d01 - d00) + a * (d11 - d10))
    r, mx, my = np.where(on, r, sd), np.where(on, mx, 0.0), np.where(on, my, 0.0)
    jt = mx * (-s * lx - c * ly) + my * (c * lx - s * ly)
    return [float(np.sum(t)) for t in (r * r, mx * mx, mx * my, mx * jt, my * my, my * jt, jt * jt, mx * r, my * r, jt * r)]


def step_of(S, damping, zero=0.0, eps=1e-9):
    """delta = -A^-1 g by the adjugate of A = H + damping diag(H) + 1e-9 I; S the ten sums (any number type)."""
    p, q, r = (S[1] + damping * S[1]) + eps, S[2], S[3]
    u, v, w = (S[4] + damping * S[4]) + eps, S[5], (S[6] + damping * S[6]) + eps
    c00, c01, c02 = u * w - v * v, r * v - q * w, q * v - r * u
    c11, c12, c22 = p * w - r * r, q * r - p * v, p * u - q * q
    det = p * c00 + q * c01 + r * c02
    return (-((c00 * S[7] + c01 * S[8] + c02 * S[9]) / det), -((c01 * S[7] + c11 * S[8] + c12 * S[9]) / det),
            -((c02 * S[7] + c12 * S[8] + c22 * S[9]) / det))


def clamp(v, lim):
    return -lim if v < -lim else lim if v > lim else v


def refine(fld, scale, off_x, off_y, ranges, pose, cos_t, sin_t, iters, damping, step_cells, step_rad, max_range, cap):
    st = status_of(fld, scale, off_x, off_y, pose)
    if st != OK:
        return unanswered(pose, st)
    t, rr = used_beams(ranges, cos_t, sin_t, max_range)
    lx, ly = np.asarray(cos_t, dtype=np.float64)[t] * rr, np.asarray(sin_t, dtype=np.float64)[t] * rr
    d, sd = np.sqrt(np.asarray(fld).astype(np.float64)), math.sqrt(float(cap))
    px, py, th = (float(v) for v in pose)
    lim = float(step_cells) / float(scale)
    for it in range(int(iters) + 1):
        S = evaluate(d, sd, float(scale), float(off_x), float(off_y), lx, ly, px, py, th)
        if it == 0:
            cost0 = S[0]
        if it == int(iters):
            break
        dx, dy, dt = step_of(S, float(damping))
        px, py, th = px + clamp(dx, lim), py + clamp(dy, lim), th + clamp(dt, float(step_rad))
    return dict(pose=np.array([px, py, th]), cost=np.array([cost0, S[0]]), used=len(t), normal=np.array(S[1:]), status=OK)


def refine_mp(fld, scale, off_x, off_y, ranges, pose, cos_t, sin_t, iters, damping, step_cells, step_rad, max_range, cap):
    st = status_of(fld, scale, off_x, off_y, pose)
    if st != OK:
        return unanswered(pose, st)
    t, rr = used_beams(ranges, cos_t, sin_t, max_range)
    lxy = [(mpf(float(cos_t[k])) * mpf(float(r)), mpf(float(sin_t[k])) * mpf(float(r))) for k, r in zip(t, rr)]
    fld = np.asarray(fld)
    xw, yw = fld.shape
    sd = mp.sqrt(mpf(int(cap)))
    roots = {}

    def at(i, j):
        if not (0 <= i < xw and 0 <= j < yw):
            return sd
        f = int(fld[i, j])
        if f not in roots:
            roots[f] = mp.sqrt(mpf(f))
        return roots[f]
    sc, ox, oy, half, one, zero = mpf(float(scale)), mpf(float(off_x)), mpf(float(off_y)), mpf(0.5), mpf(1), mpf(0)
    px, py, th = (mpf(float(v)) for v in pose)
    lim, lim_t, damp, eps, off = mpf(float(step_cells)) / sc, mpf(float(step_rad)), mpf(float(damping)), mpf(1e-9), mpf(OFF)
    margin = math.inf
    for it in range(int(iters) + 1):
        c, s = mp.cos(th), mp.sin(th)
        S = [zero] * 10
        for lx, ly in lxy:
            x, y = c * lx + (-s) * ly + px, s * lx + c * ly + py
            u, v = sc * (x + ox) - half, sc * (y + oy) - half
            r, mx, my = sd, zero, zero
            if abs(u) < off and abs(v) < off:
                fi, fj = mp.floor(u), mp.floor(v)
                a, b = u - fi, v - fj
                margin = min(margin, float(min(a, one - a, b, one - b)))
                i, j = int(fi), int(fj)
                d00, d10, d01, d11 = at(i, j), at(i + 1, j), at(i, j + 1), at(i + 1, j + 1)
                r = (one - b) * ((one - a) * d00 + a * d10) + b * ((one - a) * d01 + a * d11)
                mx = sc * ((one - b) * (d10 - d00) + b * (d11 - d01))
                my = sc * ((one - a) * (d01 - d00) + a * (d11 - d10))
            else:
                margin = min(margin, abs(float(abs(u) - off)), abs(float(abs(v) - off)))      # the off test is discrete too
            jt = mx * (-s * lx - c * ly) + my * (c * lx - s * ly)
            for k, term in enumerate((r * r, mx * mx, mx * my, mx * jt, my * my, my * jt, jt * jt, mx * r, my * r, jt * r)):
                S[k] += term
        if it == 0:
            cost0 = S[0]
        if it == int(iters):
            break
        dx, dy, dt = step_of(S, damp, zero, eps)
        px, py, th = px + clamp(dx, lim), py + clamp(dy, lim), th + clamp(dt, lim_t)
    return dict(pose=np.array([float(px), float(py), float(th)]), cost=np.array([float(cost0), float(S[0])]), used=len(t),
                normal=np.array([float(v) for v in S[1:]]), status=OK, margin=margin)


def batch(fn, fields, scale, off_x, off_y, ranges, poses, cos_t, sin_t, iters, damping, step_cells, step_rad, max_range, cap, maps=None):
    """``fn`` (refine or refine_mp) over a batch: fields [G, xw, yw], ranges [n] (shared) or [B, n], maps None or [B] (an
    entry outside [0, G): no map).  A dict of stacked arrays: pose [B, 3], cost [B, 2], used [B], normal [B, 9], status
    [B] and, from refine_mp, margin [B]."""
    ranges = np.asarray(ranges, dtype=np.float32)
    out = []
    for b, pose in enumerate(np.asarray(poses, dtype=np.float64).reshape(-1, 3)):
        gi = 0 if maps is None else int(maps[b])
        fld = fields[gi] if 0 <= gi < len(fields) else None
        out.append(fn(fld, scale, off_x, off_y, ranges if ranges.ndim == 1 else ranges[b], pose, cos_t, sin_t, iters, damping,
                      step_cells, step_rad, max_range, cap))
    keys = [k for k in ("pose", "cost", "used", "normal", "status", "margin") if all(k in o for o in out)]
    return {k: np.array([o[k] for o in out], dtype=np.int32 if k in ("used", "status") else np.float64) for k in keys}
