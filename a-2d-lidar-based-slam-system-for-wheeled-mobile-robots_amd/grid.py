"""The occupancy maps on the device and every query on them (``slam_grid_*``).

    DeviceGrid       G maps resident on the device; its methods take torch device tensors and only enqueue
    grid_*_host      the same queries on NumPy arrays, batched: query b reads map ``grid_of_batch[b]``
    match_* / locate_* / frontier_* / view_*, nearest_goal / travel_goal / gain_goal
                     pure helpers around them: rotation tables, answers to poses, goal rules

``Mapping`` holds a one-map ``DeviceGrid`` and answers its one-map queries through ``grid_*_host``; ``GridSLAM`` and
``DeviceGridSLAM`` hold one of P and of F * P maps.  Each ``slam_grid_*`` query symbol is called from one place here.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _abi


def clearance_cells2(clearance, scale, cap):
    """``min_clear2`` of a clearance in metres on a grid of ``scale`` cells per metre: ``ceil((clearance * scale)^2)``
    squared cells, 0 for none; an error beyond ``cap``, which is as far as the distance field measures."""
    c2 = int(math.ceil((float(clearance) * scale) ** 2)) if clearance > 0 else 0
    if c2 > int(cap):
        raise ValueError("clearance of %g m is %d squared cells, beyond cap = %d" % (clearance, c2, cap))
    return c2


def pose_cell(pose, scale, off_x, off_y):
    """The cell of a pose by the map's own rule, ``int(scale * (v + off))``, truncated toward zero.  A torch tensor
    [..., 2] of positions gives an int32 tensor [..., 2] on its device (clamped to +-2^30, no synchronise); anything else
    is one pose and gives (x, y) as Python ints, raising where ``int()`` does."""
    if type(pose).__module__.split(".")[0] == "torch":
        import torch
        off = torch.tensor([off_x, off_y], dtype=torch.float64, device=pose.device)
        return (scale * (pose + off)).clamp(-2.0 ** 30, 2.0 ** 30).trunc().to(torch.int32)
    p = np.asarray(pose, dtype=np.float64).reshape(-1)
    return (int(scale * (p[0] + off_x)), int(scale * (p[1] + off_y)))


def _one_or_many(pose_or_poses):
    """(poses float64 [B, 3], one): ``one`` when a single pose [3] was given, whose answer :func:`_first` unwraps."""
    p = np.asarray(pose_or_poses, dtype=np.float64)
    return p.reshape(-1, 3), p.ndim == 1


def _first(out, one=True):
    """Row 0 of a batched answer - of every part of a tuple, None staying None - for a single query; else ``out``."""
    if not one:
        return out
    return tuple(None if o is None else o[0] for o in out) if isinstance(out, tuple) else out[0]


def _locate_batch(ranges, grid_of_batch, region, B):
    """B of a locate call: as given, else the rows of ranges [B, n], else - one shared scan [n] - those of
    ``grid_of_batch``, of ``region``, or 1."""
    if B is None:
        B = ranges.shape[0] if ranges.ndim != 1 else grid_of_batch.shape[0] if grid_of_batch is not None else region.shape[0] if region is not None else 1
    return int(B)


def _frontiers_batch(grid, grid_of_batch, B):
    """B of a frontiers call: as given, else the rows of ``grid_of_batch``, else one query per map."""
    return int((grid.G if grid_of_batch is None else grid_of_batch.shape[0]) if B is None else B)


def _batch_args(poses, grid_of_batch):
    p = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 3))
    gob = None if grid_of_batch is None else np.ascontiguousarray(np.asarray(grid_of_batch, dtype=np.int32).reshape(p.shape[0]))
    return p, gob


def _tables(cos_t, sin_t):
    ct = np.ascontiguousarray(np.asarray(cos_t, dtype=np.float64).reshape(-1))
    st = np.ascontiguousarray(np.asarray(sin_t, dtype=np.float64).reshape(ct.shape[0]))
    return ct, st


def grid_raycast_host(grid, poses, cos_t, sin_t, max_range=30.0, skip=1, grid_of_batch=None, return_cells=False):
    """The scan the map would give (``slam_grid_raycast``): every beam of every pose [B, 3] cast to ``max_range``
    through its map of ``grid`` (a :class:`DeviceGrid`) along the line ``Mapping.update`` would walk.  ``cos_t``,
    ``sin_t`` [n]: the beam tables (``_abi.trig_tables``).  Returns ranges float32 [B, n] to the centre of the first
    occupied cell from path index ``skip`` on - inf: none, NaN: a pose or cell index the reference would raise on -
    and with ``return_cells`` also those cells int32 [B, n, 2], (-1, -1) where there is none."""
    p, gob = _batch_args(poses, grid_of_batch)
    ct, st = _tables(cos_t, sin_t)
    B, n = p.shape[0], ct.shape[0]
    r = np.empty((B, n), dtype=np.float32)
    cells = np.empty((B, n, 2), dtype=np.int32) if return_cells else None
    _abi.check(_abi.lib().slam_grid_raycast(grid._ctx.handle, grid._h, _abi.ptr(p), B, _abi.ptr(gob), _abi.ptr(ct), _abi.ptr(st),
                                            n, float(max_range), int(skip), _abi.ptr(r), _abi.ptr(cells)))
    return (r, cells) if return_cells else r


def grid_score_host(grid, ranges, poses, cos_t, sin_t, skip=1, grid_of_batch=None, return_classes=False):
    """How measured scans sit in the map (``slam_grid_scan_score``): ranges float32 [B, n], or one [n] shared by
    every pose; each beam is formed as ``update_scans`` forms it and traced to its own end cell.  Returns counts
    int32 [B, 7] per class (``_abi.RAY_*``) and with ``return_classes`` also the classes int8 [B, n]."""
    p, gob = _batch_args(poses, grid_of_batch)
    ct, st = _tables(cos_t, sin_t)
    B, n = p.shape[0], ct.shape[0]
    r = np.ascontiguousarray(np.asarray(ranges, dtype=np.float32))
    shared = r.ndim == 1
    if r.shape != ((n,) if shared else (B, n)):
        raise ValueError("ranges must be [n] or [B, n]")
    counts = np.empty((B, _abi.RAY_CLASSES), dtype=np.int32)
    cls = np.empty((B, n), dtype=np.int8) if return_classes else None
    _abi.check(_abi.lib().slam_grid_scan_score(grid._ctx.handle, grid._h, _abi.ptr(r), int(shared), _abi.ptr(p), B, _abi.ptr(gob),
                                               _abi.ptr(ct), _abi.ptr(st), n, int(skip), _abi.ptr(counts), _abi.ptr(cls)))
    return (counts, cls) if return_classes else counts


def grid_view_gain_host(grid, poses, cos_t, sin_t, max_range=30.0, skip=1, grid_of_batch=None, return_seen=False):
    """What a scan from each pose would reveal (``slam_grid_view_gain``): the beams of every pose [B, 3] are cast to
    ``max_range`` as :func:`grid_raycast_host` casts them, and the SET of in-bounds cells they see - up to and
    including each beam's first occupied cell, or to its end - is counted against the map.  ``grid_of_batch`` None:
    every view reads map 0.  Returns counts int32 [B, 4] = (unknown, free, occupied cells of the set, beams that found
    nothing) (``_abi.VIEW_*``; a row of -1 for a pose the index rule rejects) and with ``return_seen`` also the set as
    bit words uint32 [B, xw, ceil(yw / 32)], bit ``y & 31`` of word ``y >> 5`` in row x."""
    p, gob = _batch_args(poses, grid_of_batch)
    ct, st = _tables(cos_t, sin_t)
    B, n = p.shape[0], ct.shape[0]
    counts = np.empty((B, _abi.VIEW_COUNTS), dtype=np.int32)
    seen = np.empty((B, grid.xw, (grid.yw + 31) // 32), dtype=np.uint32) if return_seen else None
    _abi.check(_abi.lib().slam_grid_view_gain(grid._ctx.handle, grid._h, _abi.ptr(p), B, _abi.ptr(gob), _abi.ptr(ct), _abi.ptr(st),
                                              n, float(max_range), int(skip), _abi.ptr(counts), _abi.ptr(seen)))
    return (counts, seen) if return_seen else counts


def view_poses(cells, scale, off_x, off_y):
    """Poses [..., 3] at the CENTRES of cells [..., 2], heading 0, on a grid of index rule (scale, off_x, off_y): x =
    (i + 0.5) / scale - off_x, y alike (:func:`frontier_points`).  A torch tensor gives a float64 tensor on its device
    (no synchronise); anything else a NumPy array."""
    if type(cells).__module__.split(".")[0] == "torch":
        import torch
        c = cells.to(torch.float64)
        return torch.stack([(c[..., 0] + 0.5) / float(scale) - float(off_x), (c[..., 1] + 0.5) / float(scale) - float(off_y),
                            torch.zeros_like(c[..., 0])], dim=-1).contiguous()
    pts = frontier_points(cells, scale, off_x, off_y)
    return np.ascontiguousarray(np.concatenate([pts, np.zeros(pts.shape[:-1] + (1,))], axis=-1))


def view_tables(n):
    """(cos_t, sin_t) float64 [n] of ``n`` beams over the full circle, theta_i = -pi + i * 2 pi / n
    (:func:`locate_rotations`): the beams a goal's view is counted with."""
    rot = locate_rotations(n)[1]
    return np.ascontiguousarray(rot[:, 0]), np.ascontiguousarray(rot[:, 1])


def _window_ok(K, nx, ny):
    """The window sizes ``slam_grid_match`` takes (a cost volume is only allocated for those; the library rejects the rest)."""
    return K >= 1 and nx >= 0 and ny >= 0 and K * (2 * int(nx) + 1) * (2 * int(ny) + 1) <= 1 << 24


def grid_distance_field_host(grid, cap=64):
    """The distance field of every map of ``grid`` (``slam_grid_distance_field``): int16 [G, xw, yw], the squared
    cell distance to the nearest occupied cell (pmap == 100 as the counters stand now), capped at ``cap``
    (1 .. 32767).  Rebuilt on every call."""
    out = np.empty((grid.G, grid.xw, grid.yw), dtype=np.int16)
    _abi.check(_abi.lib().slam_grid_distance_field(grid._ctx.handle, grid._h, int(cap), _abi.ptr(out)))
    return out


def grid_match_host(grid, ranges, centres, cos_t, sin_t, rot_cs, nx, ny, step, max_range=30.0, cap=64, grid_of_batch=None,
                    return_costs=False):
    """The window matcher on the distance field (``slam_grid_match``): ranges float32 [B, n] or one shared [n],
    centres [B, 2], rot_cs [B, K, 2] the cos / sin of every rotation; the window is (2 nx + 1) x (2 ny + 1)
    translations of ``step`` around each centre.  Returns (best int32 [B] flat candidate index, cost int32 [B],
    used int32 [B]) and with ``return_costs`` also the cost volume int32 [B, K, 2 nx + 1, 2 ny + 1];
    :func:`match_pose` turns ``best`` into poses.  The field is rebuilt on every call."""
    ctr = np.ascontiguousarray(np.asarray(centres, dtype=np.float64).reshape(-1, 2))
    B = ctr.shape[0]
    gob = None if grid_of_batch is None else np.ascontiguousarray(np.asarray(grid_of_batch, dtype=np.int32).reshape(B))
    ct, st = _tables(cos_t, sin_t)
    n = ct.shape[0]
    rot = np.ascontiguousarray(np.asarray(rot_cs, dtype=np.float64))
    if rot.ndim != 3 or rot.shape[0] != B or rot.shape[2] != 2:
        raise ValueError("rot_cs must be [B, K, 2]")
    K = rot.shape[1]
    r = np.ascontiguousarray(np.asarray(ranges, dtype=np.float32))
    shared = r.ndim == 1
    if r.shape != ((n,) if shared else (B, n)):
        raise ValueError("ranges must be [n] or [B, n]")
    best, cost, used = (np.empty(B, dtype=np.int32) for _ in range(3))
    vol = np.empty((B, K, 2 * int(nx) + 1, 2 * int(ny) + 1), dtype=np.int32) if return_costs and _window_ok(K, nx, ny) else None
    _abi.check(_abi.lib().slam_grid_match(grid._ctx.handle, grid._h, _abi.ptr(r), int(shared), _abi.ptr(ctr), B, _abi.ptr(gob),
                                          _abi.ptr(ct), _abi.ptr(st), n, _abi.ptr(rot), K, int(nx), int(ny), float(step),
                                          float(max_range), int(cap), _abi.ptr(best), _abi.ptr(cost), _abi.ptr(used),
                                          _abi.ptr(vol)))
    return (best, cost, used, vol) if return_costs else (best, cost, used)


def grid_refine_host(grid, ranges, poses, cos_t, sin_t, iters=10, damping=1e-3, step_cells=0.5, step_rad=0.02, max_range=30.0,
                     cap=64, grid_of_batch=None, field=None, return_normal=False):
    """Poses refined below the cell (``slam_grid_refine``, include/slam_refine.h): ``iters`` damped Gauss-Newton steps of
    every pose [B, 3] on the bilinear interpolation of the square root of its map's distance field, each step clamped to
    ``step_cells`` cells in x and y and ``step_rad`` radians.  ranges float32 [B, n] or one shared [n]; ``field`` None:
    the field is rebuilt by the call, else int16 [G, xw, yw] of :func:`grid_distance_field_host` at the same ``cap``.
    Returns (poses [B, 3], cost float64 [B, 2] at the start and at the end, used int32 [B], status int32 [B]
    (``_abi.REFINE_*``)) and with ``return_normal`` also normal float64 [B, 9] = (Hxx, Hxy, Hxt, Hyy, Hyt, Htt, gx, gy,
    gt) of the last evaluation.  The call never chooses between start and end; the costs let the caller."""
    p, gob = _batch_args(poses, grid_of_batch)
    ct, st = _tables(cos_t, sin_t)
    B, n = p.shape[0], ct.shape[0]
    r = np.ascontiguousarray(np.asarray(ranges, dtype=np.float32))
    shared = r.ndim == 1
    if r.shape != ((n,) if shared else (B, n)):
        raise ValueError("ranges must be [n] or [B, n]")
    f = None if field is None else np.ascontiguousarray(np.asarray(field, dtype=np.int16))
    if f is not None and f.shape != (grid.G, grid.xw, grid.yw):
        raise ValueError("field must be [G, xw, yw]")
    out, cost = np.empty((B, 3), dtype=np.float64), np.empty((B, 2), dtype=np.float64)
    used, status = np.empty(B, dtype=np.int32), np.empty(B, dtype=np.int32)
    normal = np.empty((B, _abi.REFINE_NORMAL_LEN), dtype=np.float64) if return_normal else None
    _abi.check(_abi.lib().slam_grid_refine(grid._ctx.handle, grid._h, _abi.ptr(r), int(shared), _abi.ptr(p), B, _abi.ptr(gob),
                                           _abi.ptr(ct), _abi.ptr(st), n, int(iters), float(damping), float(step_cells),
                                           float(step_rad), float(max_range), int(cap), _abi.ptr(f), _abi.ptr(out), _abi.ptr(cost),
                                           _abi.ptr(used), _abi.ptr(normal), _abi.ptr(status)))
    return (out, cost, used, status, normal) if return_normal else (out, cost, used, status)


def refine_normal(normal):
    """(H [..., 3, 3] symmetric, g [..., 3]) of ``normal`` [..., 9] = (Hxx, Hxy, Hxt, Hyy, Hyt, Htt, gx, gy, gt)."""
    v = np.asarray(normal, dtype=np.float64)
    return v[..., [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(v.shape[:-1] + (3, 3)), v[..., 6:9].copy()


def grid_locate_host(grid, ranges, cos_t, sin_t, rot_cs, levels=5, region=None, max_range=30.0, cap=64, grid_of_batch=None,
                     B=None, return_stats=False):
    """Global scan localisation (``slam_grid_locate``): the best pose of every scan over its whole map, or over
    ``region`` int32 [B, 4] = (i0, j0, ni, nj) robot cells, and the rotations ``rot_cs`` [K, 2]
    (:func:`locate_rotations`), exact, by branch and bound on a ``levels``-deep pyramid of the distance field.  ranges
    float32 [B, n], or one shared [n] (then ``B`` comes from ``grid_of_batch`` / ``region`` / ``B``, default 1).
    Returns (best int32 [B, 3] = (k, i, j), cost int32 [B], used int32 [B]) and with ``return_stats`` also stats int64
    [B, levels + 2]: the nodes evaluated per level and the incumbent U.  :func:`locate_pose` turns ``best`` into poses."""
    ct, st = _tables(cos_t, sin_t)
    n = ct.shape[0]
    r = np.ascontiguousarray(np.asarray(ranges, dtype=np.float32))
    shared = r.ndim == 1
    gob = None if grid_of_batch is None else np.ascontiguousarray(np.asarray(grid_of_batch, dtype=np.int32).reshape(-1))
    reg = None if region is None else np.ascontiguousarray(np.asarray(region, dtype=np.int32).reshape(-1, 4))
    B = _locate_batch(r, gob, reg, B)
    if r.shape != ((n,) if shared else (B, n)) or (gob is not None and gob.shape[0] != B) or (reg is not None and reg.shape[0] != B):
        raise ValueError("ranges must be [n] or [B, n], grid_of_batch [B], region [B, 4]")
    rot = np.ascontiguousarray(np.asarray(rot_cs, dtype=np.float64))
    if rot.ndim != 2 or rot.shape[1] != 2:
        raise ValueError("rot_cs must be [K, 2]")
    H = int(levels)
    best = np.empty((max(B, 0), 3), dtype=np.int32)
    cost, used = (np.empty(max(B, 0), dtype=np.int32) for _ in range(2))
    stats = np.empty((max(B, 0), max(H, 0) + 2), dtype=np.int64) if return_stats else None
    _abi.check(_abi.lib().slam_grid_locate(grid._ctx.handle, grid._h, _abi.ptr(r), int(shared), B, _abi.ptr(gob), _abi.ptr(ct),
                                           _abi.ptr(st), n, _abi.ptr(rot), rot.shape[0], _abi.ptr(reg), H, float(max_range),
                                           int(cap), _abi.ptr(best), _abi.ptr(cost), _abi.ptr(used), _abi.ptr(stats)))
    return (best, cost, used, stats) if return_stats else (best, cost, used)


def locate_rotations(n_rot):
    """(angles [K], rot_cs [K, 2]) of a full circle of ``n_rot`` rotations: theta_k = -pi + k * 2 pi / n_rot, cosine and
    sine by NumPy."""
    th = -np.pi + np.arange(int(n_rot)) * (2.0 * np.pi / int(n_rot))
    return th, np.ascontiguousarray(np.stack([np.cos(th), np.sin(th)], axis=-1))


def locate_pose(best, scale, off_x, off_y, rot_cs):
    """Poses [B, 3] of the answers ``best`` [B, 3] = (k, i, j) of a global localisation on a grid of index rule
    (scale, off_x, off_y): the CENTRE of cell (i, j), x = (i + 0.5) / scale - off_x, y alike, theta = atan2(sin_k, cos_k);
    NaN rows where best is -1."""
    best = np.asarray(best).reshape(-1, 3).astype(np.int64)
    rot = np.asarray(rot_cs, dtype=np.float64).reshape(-1, 2)
    ok = best[:, 0] >= 0
    k = np.where(ok, best[:, 0], 0)
    out = np.stack([(best[:, 1].astype(np.float64) + 0.5) / float(scale) - float(off_x),
                    (best[:, 2].astype(np.float64) + 0.5) / float(scale) - float(off_y), np.arctan2(rot[k, 1], rot[k, 0])], axis=1)
    out[~ok] = np.nan
    return out


def grid_frontiers_host(grid, grid_of_batch=None, B=None, radius=2, min_unknown=13, min_clear2=0, cap=64, min_size=5,
                        max_clusters=256, labels=False):
    """Map frontiers (``slam_grid_frontiers``) on NumPy arrays: query b reads map ``grid_of_batch[b]`` (None: map b, B
    defaults to G).  Returns (count int32 [B, 2] = (kept clusters, frontier cells), clusters int32 [B, M, 8] = (label,
    size, rep_x, rep_y, x0, y0, x1, y1), sums int64 [B, M, 2] = (sx, sy)) and with ``labels`` also int32 [B, xw, yw].
    The defaults (2, 13, 5) come from one experiment on the synthetic room; they are not tuned."""
    gob = None if grid_of_batch is None else np.ascontiguousarray(np.asarray(grid_of_batch, dtype=np.int32).reshape(-1))
    B = _frontiers_batch(grid, gob, B)
    if gob is not None and gob.shape[0] != B:
        raise ValueError("grid_of_batch must be [B]")
    M = int(max_clusters)
    count = np.empty((max(B, 0), 2), dtype=np.int32)
    clusters = np.empty((max(B, 0), max(M, 0), 8), dtype=np.int32)
    sums = np.empty((max(B, 0), max(M, 0), 2), dtype=np.int64)
    lab = np.empty((max(B, 0), grid.xw, grid.yw), dtype=np.int32) if labels else None
    _abi.check(_abi.lib().slam_grid_frontiers(grid._ctx.handle, grid._h, B, _abi.ptr(gob), int(radius), int(min_unknown),
                                              int(min_clear2), int(cap), int(min_size), M, _abi.ptr(count),
                                              _abi.ptr(clusters) if M > 0 else None, _abi.ptr(sums) if M > 0 else None,
                                              _abi.ptr(lab)))
    return (count, clusters, sums, lab) if labels else (count, clusters, sums)


def frontier_points(cells, scale, off_x, off_y):
    """World coordinates [..., 2] of the CENTRES of cells [..., 2] on a grid of index rule (scale, off_x, off_y):
    x = (i + 0.5) / scale - off_x, y alike, as :func:`locate_pose` places a cell."""
    c = np.asarray(cells, dtype=np.float64)
    return np.stack([(c[..., 0] + 0.5) / float(scale) - float(off_x), (c[..., 1] + 0.5) / float(scale) - float(off_y)], axis=-1)


def frontier_dict(count, clusters, sums, scale, off_x, off_y):
    """One query's outputs of ``slam_grid_frontiers`` as the dict :meth:`Mapping.frontiers` returns."""
    K = max(0, min(int(count[0]), clusters.shape[0]))
    cl, sm = clusters[:K], sums[:K].astype(np.float64)
    size = cl[:, 1].astype(np.float64).reshape(-1, 1)
    return dict(label=cl[:, 0].copy(), size=cl[:, 1].copy(), cell=cl[:, 2:4].copy(), point=frontier_points(cl[:, 2:4], scale, off_x, off_y),
                centroid=frontier_points(sm / np.maximum(size, 1.0), scale, off_x, off_y), bbox=cl[:, 4:8].copy(),
                count=int(count[0]), n_frontier=int(count[1]))


def nearest_goal(fr, pose):
    """The representative point of the kept cluster nearest to the pose's (x, y) - squared distance in float64, ties to
    the lowest label (the rows are in label order) - or None when no cluster is kept."""
    if fr["point"].shape[0] == 0:
        return None
    p = np.asarray(pose, dtype=np.float64).reshape(-1)
    d = (fr["point"][:, 0] - p[0]) ** 2 + (fr["point"][:, 1] - p[1]) ** 2
    return fr["point"][int(np.argmin(d))].copy()


def _travel_shapes(grid, sources, grid_of_batch, goals):
    """(B, S, Q) of a travel call from the shapes of its arguments: sources [B, S, 2] (or [S, 2] for B = 1), goals
    [B, Q, 2] or None."""
    if sources.ndim == 2:
        sources = sources.reshape((1,) + tuple(sources.shape))
    if sources.ndim != 3 or sources.shape[2] != 2:
        raise ValueError("sources must be [B, S, 2]")
    B, S = int(sources.shape[0]), int(sources.shape[1])
    if grid_of_batch is not None and int(grid_of_batch.shape[0]) != B:
        raise ValueError("grid_of_batch must be [B]")
    Q = 0
    if goals is not None:
        if goals.ndim == 2:
            goals = goals.reshape((1,) + tuple(goals.shape))
        if goals.ndim != 3 or goals.shape[0] != B or goals.shape[2] != 2:
            raise ValueError("goals must be [B, Q, 2]")
        Q = int(goals.shape[1])
    return sources, goals, B, S, Q


def grid_travel_host(grid, sources, grid_of_batch=None, goals=None, foot=0, through_unknown=False, min_clear2=0, cap=64, path_cap=0,
                     cost=True, dirs=False):
    """The travel-cost field (``slam_grid_travel``) on NumPy arrays: sources int32 [B, S, 2] cells, query b on map
    ``grid_of_batch[b]`` (None: map b), goals int32 [B, Q, 2] or None.  Returns a dict: ``status`` int32 [B], with ``cost``
    ``cost`` int32 [B, xw, yw], with ``dirs`` ``dir`` int8 [B, xw, yw], with goals ``goal_cost`` and ``path_len`` int32
    [B, Q] and, when ``path_cap`` > 0, ``path`` int32 [B, Q, path_cap, 2]."""
    gob = None if grid_of_batch is None else np.ascontiguousarray(np.asarray(grid_of_batch, dtype=np.int32).reshape(-1))
    src = np.ascontiguousarray(np.asarray(sources, dtype=np.int32))
    gl = None if goals is None else np.ascontiguousarray(np.asarray(goals, dtype=np.int32))
    src, gl, B, S, Q = _travel_shapes(grid, src, gob, gl)
    P = int(path_cap)
    out = dict(status=np.empty((B,), dtype=np.int32))
    if cost:
        out["cost"] = np.empty((B, grid.xw, grid.yw), dtype=np.int32)
    if dirs:
        out["dir"] = np.empty((B, grid.xw, grid.yw), dtype=np.int8)
    if gl is not None:
        out["goal_cost"], out["path_len"] = np.empty((B, Q), dtype=np.int32), np.empty((B, Q), dtype=np.int32)
        if P > 0:
            out["path"] = np.empty((B, Q, P, 2), dtype=np.int32)
    ptr = lambda k: _abi.ptr(out[k]) if k in out and out[k].size else None
    _abi.check(_abi.lib().slam_grid_travel(grid._ctx.handle, grid._h, B, _abi.ptr(gob), _abi.ptr(src), S, int(foot), int(bool(through_unknown)),
                                           int(min_clear2), int(cap), _abi.ptr(gl) if Q > 0 else None, Q, P, _abi.ptr(out["status"]),
                                           ptr("cost"), ptr("dir"), ptr("goal_cost"), ptr("path_len"), ptr("path")))
    return out


def travel_goal(fr, goal_cost):
    """Index of the kept cluster of ``fr`` (:func:`frontier_dict`) with the smallest travel cost >= 0 in ``goal_cost``
    [K], ties to the lowest label (the rows are in label order); None when none is reachable."""
    c = np.asarray(goal_cost)[:fr["point"].shape[0]].astype(np.int64)
    if c.size == 0 or not np.any(c >= 0):
        return None
    return int(np.argmin(np.where(c >= 0, c, np.iinfo(np.int64).max)))


def gain_goal(fr, goal_cost, unknown, bias=100):
    """Index of the kept cluster of ``fr`` (:func:`frontier_dict`) that reveals the most unknown cells per unit of
    travel, or None.  Candidates are the clusters with travel cost c >= 0 in ``goal_cost`` [K] and u > 0 in
    ``unknown`` [K] (the ``VIEW_UNKNOWN`` count of a view from the cluster's representative); k beats l iff
    u_k * (c_l + bias) > u_l * (c_k + bias), in exact Python integers; ties go to the lower cost, then to the lower
    label (the rows are in label order).  ``bias`` is in travel-cost units (10 per straight cell step); its default of
    100 is a starting value, not a tuned one."""
    K = fr["point"].shape[0]
    c = [int(v) for v in np.asarray(goal_cost).reshape(-1)[:K]]
    u = [int(v) for v in np.asarray(unknown).reshape(-1)[:K]]
    bias = int(bias)
    if bias < 1:
        raise ValueError("bias must be >= 1")
    best = None
    for k in range(min(K, len(c), len(u))):
        if c[k] < 0 or u[k] <= 0:
            continue
        if best is None:
            best = k
            continue
        lhs, rhs = u[k] * (c[best] + bias), u[best] * (c[k] + bias)
        if lhs > rhs or (lhs == rhs and c[k] < c[best]):
            best = k
    return best


def grid_copy_maps_host(grid, src, first=0):
    """``slam_grid_copy_maps`` on a NumPy array: map ``first + k`` of ``grid`` becomes a copy of map ``src[k]``.  Returns
    int32 [count]: 1 copied, 0 kept (its own map, or no map).  A source that is itself a destination raises."""
    s = np.ascontiguousarray(np.asarray(src, dtype=np.int32).reshape(-1))
    out = np.empty(s.shape[0], dtype=np.int32)
    _abi.check(_abi.lib().slam_grid_copy_maps(grid._ctx.handle, grid._h, _abi.ptr(s), int(first), s.shape[0], _abi.ptr(out)))
    return out


def grid_update_particles_host(grid, ranges, cos_t, sin_t, poses, acc=None, map0=0):
    """``slam_grid_update_particles`` on NumPy arrays: ranges [F, n], poses [F, P, 3], acc int32 [F, P] or None."""
    p = np.ascontiguousarray(np.asarray(poses, dtype=np.float64))
    F, P = p.shape[:2]
    ct, st = _tables(cos_t, sin_t)
    r = np.ascontiguousarray(np.asarray(ranges, dtype=np.float32).reshape(F, ct.shape[0]))
    a = None if acc is None else np.ascontiguousarray(np.asarray(acc, dtype=np.int32).reshape(F, P))
    _abi.check(_abi.lib().slam_grid_update_particles(grid._ctx.handle, grid._h, _abi.ptr(r), _abi.ptr(ct), _abi.ptr(st), _abi.ptr(p),
                                                     _abi.ptr(a), F, P, ct.shape[0], int(map0)))


def match_rotations(thetas, n_rot=11, rot_step=0.01):
    """(angles [B, K], rot_cs [B, K, 2]) of the matcher's rotations: theta + (k - n_rot // 2) * rot_step, cosine
    and sine by NumPy."""
    th = np.asarray(thetas, dtype=np.float64).reshape(-1, 1) + (np.arange(int(n_rot)) - int(n_rot) // 2) * float(rot_step)
    return th, np.ascontiguousarray(np.stack([np.cos(th), np.sin(th)], axis=-1))


def match_pose(centres, thetas, best, nx, ny, step):
    """Poses [B, 3] of the flat candidate indices ``best`` [B] of a window match: ``thetas`` [B, K] the angles the
    rotation tables were made from, x = cx + (i - nx) * step, y = cy + (j - ny) * step; NaN rows where best is -1."""
    ctr = np.asarray(centres, dtype=np.float64).reshape(-1, 2)
    th = np.asarray(thetas, dtype=np.float64).reshape(ctr.shape[0], -1)
    best = np.asarray(best).reshape(-1).astype(np.int64)
    wx, wy = 2 * int(nx) + 1, 2 * int(ny) + 1
    ok = best >= 0
    idx = np.where(ok, best, 0)
    k, i, j = idx // (wx * wy), idx // wy % wx, idx % wy
    out = np.stack([ctr[:, 0] + (i - int(nx)).astype(np.float64) * float(step),
                    ctr[:, 1] + (j - int(ny)).astype(np.float64) * float(step), th[np.arange(len(idx)), k]], axis=1)
    out[~ok] = np.nan
    return out


class DeviceGrid:
    """G occupancy maps resident on the device (``slam_grid_*``)."""

    def __init__(self, G, xw, yw, scale, off_x, off_y, free_inc=0.01, hit_inc=20.0, thresh=10.0, context=None):
        self._ctx = context or _abi.default_context()
        self.G, self.xw, self.yw = int(G), int(xw), int(yw)
        self.scale, self.off_x, self.off_y = float(scale), float(off_x), float(off_y)
        h = C.c_void_p()
        _abi.check(_abi.lib().slam_grid_create(self._ctx.handle, self.G, self.xw, self.yw, float(scale), float(off_x),
                                               float(off_y), float(free_inc), float(hit_inc), float(thresh), C.byref(h)))
        self._h = h

    @classmethod
    def metric(cls, G, xw, yw, reso, **kw):
        """Index rule from the resolution: scale = 1/reso, offsets = half the map width
        (400x400 @ 0.05 -> scale 20, offset 10; the reference is 200x200 @ 0.1 -> 10, 10)."""
        s = 1.0 / reso
        s = float(round(s)) if abs(round(s) - s) < 1e-9 else s
        return cls(G, xw, yw, s, xw / (2.0 * s), yw / (2.0 * s), **kw)

    def close(self):
        if getattr(self, "_h", None) is not None and self._ctx._h is not None:
            _abi.lib().slam_grid_destroy(self._ctx.handle, self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        _abi.check(_abi.lib().slam_grid_reset(self._ctx.handle, self._h))

    def counters_torch(self):
        """(pass, hit) as torch int32 tensors [G, xw, yw] that ALIAS the device counters (the
        uint32 bits viewed as int32: sums wrap identically) - for checkpoint / restore
        (``.clone()`` / ``.copy_()``) and for ``torch.distributed.all_reduce`` across ranks."""
        import torch
        p, h = C.c_void_p(), C.c_void_p()
        _abi.check(_abi.lib().slam_grid_counters_dev(self._ctx.handle, self._h, C.byref(p), C.byref(h)))

        class _View:                      # minimal __cuda_array_interface__ carrier
            def __init__(self, ptr, shape):
                self.__cuda_array_interface__ = {"shape": shape, "typestr": "<i4", "data": (int(ptr), False), "version": 2}
        shape = (self.G, self.xw, self.yw)
        dev = torch.device("cuda", self._ctx.device)
        return (torch.as_tensor(_View(p.value, shape), device=dev), torch.as_tensor(_View(h.value, shape), device=dev))

    def live_pmap(self):
        """Keep ``pmap`` [G, xw, yw] int8 resident and current on the device
        (``slam_grid_live_pmap``); returns its device address."""
        p = C.c_void_p()
        _abi.check(_abi.lib().slam_grid_live_pmap(self._ctx.handle, self._h, C.byref(p)))
        return int(p.value)

    def update_host(self, ox, oy, cx, cy, grid_of_batch=None):
        ox = np.ascontiguousarray(np.asarray(ox, dtype=np.float64))
        oy = np.ascontiguousarray(np.asarray(oy, dtype=np.float64))
        if ox.ndim == 1:
            ox, oy = ox[None], oy[None]
        B, n = ox.shape
        cx = np.ascontiguousarray(np.asarray(cx, dtype=np.float64).reshape(B))
        cy = np.ascontiguousarray(np.asarray(cy, dtype=np.float64).reshape(B))
        gob = None if grid_of_batch is None else np.ascontiguousarray(np.asarray(grid_of_batch, dtype=np.int32))
        _abi.check(_abi.lib().slam_grid_update(self._ctx.handle, self._h, _abi.ptr(ox), _abi.ptr(oy), _abi.ptr(cx),
                                               _abi.ptr(cy), B, n, _abi.ptr(gob)))

    def raycast(self, poses, cos_t, sin_t, max_range=30.0, skip=1, grid_of_batch=None, ranges_out=None, cells_out=None,
                return_cells=False):
        """``slam_grid_raycast_dev`` on torch device tensors: poses float64 [B, 3], cos_t / sin_t float64 [n],
        grid_of_batch int32 [B] or None.  Writes ranges float32 [B, n] (and cells int32 [B, n, 2]) into the tensors
        given or into fresh ones; enqueued on the context's stream, no synchronise."""
        import torch
        B, n = int(poses.shape[0]), int(cos_t.shape[0])
        if ranges_out is None:
            ranges_out = torch.empty((B, n), dtype=torch.float32, device=poses.device)
        if cells_out is None and return_cells:
            cells_out = torch.empty((B, n, 2), dtype=torch.int32, device=poses.device)
        _abi.check(_abi.lib().slam_grid_raycast_dev(self._ctx.handle, self._h, _abi.ptr(poses), B, _abi.ptr(grid_of_batch),
                                                    _abi.ptr(cos_t), _abi.ptr(sin_t), n, float(max_range), int(skip),
                                                    _abi.ptr(ranges_out), _abi.ptr(cells_out)))
        return ranges_out if cells_out is None else (ranges_out, cells_out)

    def score(self, ranges, poses, cos_t, sin_t, skip=1, grid_of_batch=None, counts_out=None, class_out=None,
              return_classes=False):
        """``slam_grid_scan_score_dev`` on torch device tensors: ranges float32 [B, n] or a shared [n].  Writes counts
        int32 [B, 7] (and classes int8 [B, n]) into the tensors given or into fresh ones; no synchronise."""
        import torch
        B, n = int(poses.shape[0]), int(cos_t.shape[0])
        if counts_out is None:
            counts_out = torch.empty((B, _abi.RAY_CLASSES), dtype=torch.int32, device=poses.device)
        if class_out is None and return_classes:
            class_out = torch.empty((B, n), dtype=torch.int8, device=poses.device)
        _abi.check(_abi.lib().slam_grid_scan_score_dev(self._ctx.handle, self._h, _abi.ptr(ranges), int(ranges.dim() == 1),
                                                       _abi.ptr(poses), B, _abi.ptr(grid_of_batch), _abi.ptr(cos_t),
                                                       _abi.ptr(sin_t), n, int(skip), _abi.ptr(counts_out), _abi.ptr(class_out)))
        return counts_out if class_out is None else (counts_out, class_out)

    def view_gain(self, poses, cos_t, sin_t, max_range=30.0, skip=1, grid_of_batch=None, counts_out=None, seen_out=None,
                  return_seen=False):
        """``slam_grid_view_gain_dev`` on torch device tensors: poses float64 [B, 3], cos_t / sin_t float64 [n],
        grid_of_batch int32 [B] or None (every view reads map 0).  Writes counts int32 [B, 4] (``_abi.VIEW_*``; and the
        seen set as int32 bit words [B, xw, ceil(yw / 32)]) into the tensors given or into fresh ones; enqueued on the
        context's stream, no synchronise."""
        import torch
        B, n = int(poses.shape[0]), int(cos_t.shape[0])
        if counts_out is None:
            counts_out = torch.empty((B, _abi.VIEW_COUNTS), dtype=torch.int32, device=poses.device)
        if seen_out is None and return_seen:
            seen_out = torch.empty((B, self.xw, (self.yw + 31) // 32), dtype=torch.int32, device=poses.device)
        _abi.check(_abi.lib().slam_grid_view_gain_dev(self._ctx.handle, self._h, _abi.ptr(poses), B, _abi.ptr(grid_of_batch),
                                                      _abi.ptr(cos_t), _abi.ptr(sin_t), n, float(max_range), int(skip),
                                                      _abi.ptr(counts_out), _abi.ptr(seen_out)))
        return counts_out if seen_out is None else (counts_out, seen_out)

    def distance_field(self, cap=64, out=None):
        """``slam_grid_distance_field_dev``: the capped squared cell distance to the nearest occupied cell of every
        map, into the torch int16 tensor [G, xw, yw] given or a fresh one on the context's device; rebuilt on every
        call, enqueued on the context's stream, no synchronise."""
        import torch
        if out is None:
            out = torch.empty((self.G, self.xw, self.yw), dtype=torch.int16, device=torch.device("cuda", self._ctx.device))
        _abi.check(_abi.lib().slam_grid_distance_field_dev(self._ctx.handle, self._h, int(cap), _abi.ptr(out)))
        return out

    def match(self, ranges, centres, cos_t, sin_t, rot_cs, nx, ny, step, max_range=30.0, cap=64, grid_of_batch=None,
              best_out=None, cost_out=None, used_out=None, costs_out=None, return_costs=False):
        """``slam_grid_match_dev`` on torch device tensors: ranges float32 [B, n] or a shared [n], centres float64
        [B, 2], cos_t / sin_t float64 [n], rot_cs float64 [B, K, 2].  Writes best / cost / used int32 [B] (and the
        cost volume int32 [B, K, 2 nx + 1, 2 ny + 1]) into the tensors given or into fresh ones; no synchronise."""
        import torch
        B, n, K = int(centres.shape[0]), int(cos_t.shape[0]), int(rot_cs.shape[1])
        new = lambda *shape: torch.empty(shape, dtype=torch.int32, device=centres.device)
        best_out = new(B) if best_out is None else best_out
        cost_out = new(B) if cost_out is None else cost_out
        used_out = new(B) if used_out is None else used_out
        if costs_out is None and return_costs:
            costs_out = new(B, K, 2 * int(nx) + 1, 2 * int(ny) + 1)
        _abi.check(_abi.lib().slam_grid_match_dev(self._ctx.handle, self._h, _abi.ptr(ranges), int(ranges.dim() == 1),
                                                  _abi.ptr(centres), B, _abi.ptr(grid_of_batch), _abi.ptr(cos_t), _abi.ptr(sin_t),
                                                  n, _abi.ptr(rot_cs), K, int(nx), int(ny), float(step), float(max_range),
                                                  int(cap), _abi.ptr(best_out), _abi.ptr(cost_out), _abi.ptr(used_out),
                                                  _abi.ptr(costs_out)))
        return (best_out, cost_out, used_out) if costs_out is None else (best_out, cost_out, used_out, costs_out)

    def refine(self, ranges, poses, cos_t, sin_t, iters=10, damping=1e-3, step_cells=0.5, step_rad=0.02, max_range=30.0, cap=64,
               grid_of_batch=None, field=None, out=None, return_normal=False):
        """``slam_grid_refine_dev`` on torch device tensors: ranges float32 [B, n] or a shared [n], poses float64 [B, 3],
        cos_t / sin_t float64 [n], grid_of_batch int32 [B] or None, field int16 [G, xw, yw] of :meth:`distance_field` at
        the same ``cap`` or None (rebuilt by the call).  Writes poses float64 [B, 3], cost float64 [B, 2], used int32 [B]
        and status int32 [B] (and normal float64 [B, 9]) into the tensors of ``out`` (a tuple in that order) or into fresh
        ones and returns them; enqueued on the context's stream, no synchronise."""
        import torch
        B, n = int(poses.shape[0]), int(cos_t.shape[0])
        if out is None:
            new = lambda dtype, *shape: torch.empty(shape, dtype=dtype, device=poses.device)
            out = (new(torch.float64, B, 3), new(torch.float64, B, 2), new(torch.int32, B), new(torch.int32, B))
            if return_normal:
                out += (new(torch.float64, B, _abi.REFINE_NORMAL_LEN),)
        normal = out[4] if len(out) > 4 else None
        _abi.check(_abi.lib().slam_grid_refine_dev(self._ctx.handle, self._h, _abi.ptr(ranges), int(ranges.dim() == 1), _abi.ptr(poses),
                                                   B, _abi.ptr(grid_of_batch), _abi.ptr(cos_t), _abi.ptr(sin_t), n, int(iters),
                                                   float(damping), float(step_cells), float(step_rad), float(max_range), int(cap),
                                                   _abi.ptr(field), _abi.ptr(out[0]), _abi.ptr(out[1]), _abi.ptr(out[2]),
                                                   _abi.ptr(normal), _abi.ptr(out[3])))
        return out

    def locate(self, ranges, cos_t, sin_t, rot_cs, levels=5, region=None, max_range=30.0, cap=64, grid_of_batch=None, B=None,
               best_out=None, cost_out=None, used_out=None, stats_out=None, return_stats=False):
        """``slam_grid_locate_dev`` on torch device tensors: ranges float32 [B, n] or a shared [n] (then ``B`` comes from
        ``grid_of_batch`` / ``region`` / ``B``, default 1), cos_t / sin_t float64 [n], rot_cs float64 [K, 2], region int32
        [B, 4] or None, grid_of_batch int32 [B] or None.  Writes best int32 [B, 3] = (k, i, j), cost / used int32 [B]
        (and stats int64 [B, levels + 2]) into the tensors given or into fresh ones; no synchronise."""
        import torch
        n, K, H = int(cos_t.shape[0]), int(rot_cs.shape[0]), int(levels)
        B = _locate_batch(ranges, grid_of_batch, region, B)
        new = lambda dtype, *shape: torch.empty(shape, dtype=dtype, device=cos_t.device)
        best_out = new(torch.int32, B, 3) if best_out is None else best_out
        cost_out = new(torch.int32, B) if cost_out is None else cost_out
        used_out = new(torch.int32, B) if used_out is None else used_out
        if stats_out is None and return_stats:
            stats_out = new(torch.int64, B, max(H, 0) + 2)
        _abi.check(_abi.lib().slam_grid_locate_dev(self._ctx.handle, self._h, _abi.ptr(ranges), int(ranges.dim() == 1), B,
                                                   _abi.ptr(grid_of_batch), _abi.ptr(cos_t), _abi.ptr(sin_t), n, _abi.ptr(rot_cs), K,
                                                   _abi.ptr(region), H, float(max_range), int(cap), _abi.ptr(best_out),
                                                   _abi.ptr(cost_out), _abi.ptr(used_out), _abi.ptr(stats_out)))
        return (best_out, cost_out, used_out) if stats_out is None else (best_out, cost_out, used_out, stats_out)

    def frontiers(self, grid_of_batch=None, B=None, radius=2, min_unknown=13, min_clear2=0, cap=64, min_size=5, max_clusters=256,
                  labels=False, out=None):
        """``slam_grid_frontiers_dev`` on torch device tensors: grid_of_batch int32 [B] or None (query b reads map b, B
        defaults to G).  Writes count int32 [B, 2], clusters int32 [B, M, 8], sums int64 [B, M, 2] (and with ``labels``
        int32 [B, xw, yw]) into the tensors of ``out`` (a tuple in that order) or into fresh ones and returns them; no
        synchronise.  The defaults (2, 13, 5) come from one experiment on the synthetic room; they are not tuned."""
        import torch
        B = _frontiers_batch(self, grid_of_batch, B)
        M = int(max_clusters)
        if out is None:
            dev = grid_of_batch.device if grid_of_batch is not None else torch.device("cuda", self._ctx.device)
            new = lambda dtype, *shape: torch.empty(shape, dtype=dtype, device=dev)
            out = (new(torch.int32, max(B, 0), 2), new(torch.int32, max(B, 0), max(M, 0), 8), new(torch.int64, max(B, 0), max(M, 0), 2))
            if labels:
                out += (new(torch.int32, max(B, 0), self.xw, self.yw),)
        lab = out[3] if len(out) > 3 else None
        _abi.check(_abi.lib().slam_grid_frontiers_dev(self._ctx.handle, self._h, B, _abi.ptr(grid_of_batch), int(radius),
                                                      int(min_unknown), int(min_clear2), int(cap), int(min_size), M, _abi.ptr(out[0]),
                                                      _abi.ptr(out[1]) if M > 0 else None, _abi.ptr(out[2]) if M > 0 else None,
                                                      _abi.ptr(lab)))
        return out

    def travel(self, sources, grid_of_batch=None, goals=None, foot=0, through_unknown=False, min_clear2=0, cap=64, path_cap=0,
               cost=True, dirs=False, out=None):
        """``slam_grid_travel_dev`` on torch device tensors: sources int32 [B, S, 2] cells, grid_of_batch int32 [B] or None
        (query b reads map b), goals int32 [B, Q, 2] or None (rows of -1 are legal: the ``rep_x, rep_y`` columns of
        :meth:`frontiers`' table go straight in once made contiguous).  Writes into the tensors of the dict ``out`` or
        into fresh ones and returns the dict: ``status`` int32 [B], with ``cost`` ``cost`` int32 [B, xw, yw], with
        ``dirs`` ``dir`` int8 [B, xw, yw], with goals ``goal_cost`` / ``path_len`` int32 [B, Q] and, when ``path_cap``
        > 0, ``path`` int32 [B, Q, path_cap, 2].  No synchronise."""
        import torch
        sources, goals, B, S, Q = _travel_shapes(self, sources, grid_of_batch, goals)
        P = int(path_cap)
        if not sources.is_contiguous() or (goals is not None and not goals.is_contiguous()):
            raise ValueError("sources and goals must be contiguous")
        if out is None:
            new = lambda dtype, *shape: torch.empty(shape, dtype=dtype, device=sources.device)
            out = dict(status=new(torch.int32, B))
            if cost:
                out["cost"] = new(torch.int32, B, self.xw, self.yw)
            if dirs:
                out["dir"] = new(torch.int8, B, self.xw, self.yw)
            if goals is not None:
                out["goal_cost"], out["path_len"] = new(torch.int32, B, Q), new(torch.int32, B, Q)
                if P > 0:
                    out["path"] = new(torch.int32, B, Q, P, 2)
        ptr = lambda k: _abi.ptr(out[k]) if k in out and out[k].numel() else None
        _abi.check(_abi.lib().slam_grid_travel_dev(self._ctx.handle, self._h, B, _abi.ptr(grid_of_batch), _abi.ptr(sources), S, int(foot),
                                                   int(bool(through_unknown)), int(min_clear2), int(cap),
                                                   _abi.ptr(goals) if Q > 0 else None, Q, P, _abi.ptr(out["status"]), ptr("cost"),
                                                   ptr("dir"), ptr("goal_cost"), ptr("path_len"), ptr("path")))
        return out

    def copy_maps(self, src, first=0, out=None):
        """``slam_grid_copy_maps_dev``: map ``first + k`` becomes a copy of map ``src[k]`` (torch int32 device tensor
        [count]), counters and live pmap, in place.  An entry that names its own map or no map keeps it (0 in the
        result); a source that is itself a destination of the call leaves that destination alone (-1); otherwise 1.
        Writes int32 [count] into ``out`` or a fresh tensor; no synchronise."""
        import torch
        count = int(src.shape[0])
        if out is None:
            out = torch.empty((count,), dtype=torch.int32, device=src.device)
        _abi.check(_abi.lib().slam_grid_copy_maps_dev(self._ctx.handle, self._h, _abi.ptr(src), int(first), count, _abi.ptr(out)))
        return out

    def update_particles(self, ranges, cos_t, sin_t, poses, acc=None, map0=0):
        """``slam_grid_update_particles_dev`` on torch device tensors: ranges float32 [F, n], poses float64 [F, P, 3],
        acc int32 [F, P] or None.  Scan f is integrated from every pose of filter f into map ``map0 + f * P + p`` as
        ``slam_grid_update_scans`` would; a particle whose acc is ``MCL_DEAD`` casts nothing.  No synchronise."""
        F, P, n = int(poses.shape[0]), int(poses.shape[1]), int(cos_t.shape[0])
        _abi.check(_abi.lib().slam_grid_update_particles_dev(self._ctx.handle, self._h, _abi.ptr(ranges), _abi.ptr(cos_t),
                                                             _abi.ptr(sin_t), _abi.ptr(poses), _abi.ptr(acc), F, P, n, int(map0)))

    def read(self, g=0, want=("pmap",)):
        out = {}
        if "pmap" in want:
            out["pmap"] = np.empty((self.xw, self.yw), dtype=np.int8)
        if "datamap" in want:
            out["datamap"] = np.empty((self.xw, self.yw), dtype=np.float64)
        if "pass" in want:
            out["pass"] = np.empty((self.xw, self.yw), dtype=np.uint32)
        if "hit" in want:
            out["hit"] = np.empty((self.xw, self.yw), dtype=np.uint32)
        _abi.check(_abi.lib().slam_grid_read(self._ctx.handle, self._h, int(g), _abi.ptr(out.get("pmap")),
                                             _abi.ptr(out.get("datamap")), _abi.ptr(out.get("pass")),
                                             _abi.ptr(out.get("hit"))))
        return out

    def occupancy_grid_data(self, g=0):
        out = np.empty(self.xw * self.yw, dtype=np.int8)
        _abi.check(_abi.lib().slam_grid_occupancy_data(self._ctx.handle, self._h, int(g), _abi.ptr(out)))
        return out

    def visits(self):
        v = C.c_uint64(0)
        _abi.check(_abi.lib().slam_grid_visits(self._ctx.handle, self._h, C.byref(v)))
        return int(v.value)
