"""slam_grid_travel restated on the host (test infrastructure only): the traversable set, a heap Dijkstra over it with the
header's move rule, and ``dir`` and the paths from the final costs.  A second, independent statement - Bellman-Ford by
shifted arrays, run to its fixed point - and a cell-by-cell check of the definition hold it (tests/test_travel_ref.py)."""
import heapq

import numpy as np

STRAIGHT, DIAGONAL = 10, 14
MOVES = ((1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1))
WEIGHTS = (STRAIGHT,) * 4 + (DIAGONAL,) * 4


def valid_sources(shape, sources):
    xw, yw = shape
    return [(int(x), int(y)) for x, y in np.asarray(sources).reshape(-1, 2) if 0 <= x < xw and 0 <= y < yw]


def traversable(pmap, field, sources, foot, through_unknown, min_clear2):
    """bool [xw, yw]: the set T of the header."""
    pm = np.asarray(pmap)
    T = pm == 0
    if through_unknown:
        T |= pm == 50
    if min_clear2 > 0:
        T &= np.asarray(field) >= min_clear2
    xw, yw = pm.shape
    for x, y in valid_sources(pm.shape, sources):
        T[max(x - foot, 0):min(x + foot, xw - 1) + 1, max(y - foot, 0):min(y + foot, yw - 1) + 1] = True
    return T


def allowed(T):
    """bool [8, xw, yw]: the move from each cell in each direction is allowed."""
    xw, yw = T.shape
    P = np.zeros((xw + 2, yw + 2), dtype=bool)
    P[1:-1, 1:-1] = T
    at = lambda dx, dy: P[1 + dx:1 + dx + xw, 1 + dy:1 + dy + yw]
    out = np.zeros((8, xw, yw), dtype=bool)
    for d, (dx, dy) in enumerate(MOVES):
        ok = T & at(dx, dy)
        if d >= 4:
            ok = ok & at(dx, 0) & at(0, dy)
        out[d] = ok
    return out


def costs(T, sources):
    """int32 [xw, yw]: heap Dijkstra from the valid sources over T; -1 where nothing arrives."""
    xw, yw = T.shape
    ok = allowed(T)
    dist = np.full((xw, yw), -1, dtype=np.int64)
    heap = []
    for s in set(valid_sources(T.shape, sources)):
        dist[s] = 0
        heap.append((0, s[0], s[1]))
    heapq.heapify(heap)
    while heap:
        c, x, y = heapq.heappop(heap)
        if c != dist[x, y]:
            continue
        for d, (dx, dy) in enumerate(MOVES):
            if ok[d, x, y]:
                n = c + WEIGHTS[d]
                if dist[x + dx, y + dy] < 0 or n < dist[x + dx, y + dy]:
                    dist[x + dx, y + dy] = n
                    heapq.heappush(heap, (n, x + dx, y + dy))
    return dist.astype(np.int32)


def costs_bellman_ford(T, sources):
    """The same by shifted arrays: every cell takes the minimum over its allowed moves until nothing changes."""
    xw, yw = T.shape
    ok = allowed(T)
    BIG = np.int64(1) << 40
    dist = np.full((xw, yw), BIG, dtype=np.int64)
    for s in valid_sources(T.shape, sources):
        dist[s] = 0
    while True:
        P = np.full((xw + 2, yw + 2), BIG, dtype=np.int64)
        P[1:-1, 1:-1] = dist
        new = dist.copy()
        for d, (dx, dy) in enumerate(MOVES):
            new = np.where(ok[d], np.minimum(new, P[1 + dx:1 + dx + xw, 1 + dy:1 + dy + yw] + WEIGHTS[d]), new)
        if np.array_equal(new, dist):
            return np.where(dist >= BIG, -1, dist).astype(np.int32)
        dist = new


def dirs(T, cost):
    """int8 [xw, yw]: the lowest code whose move is allowed and whose neighbour's cost + weight is the cell's."""
    xw, yw = T.shape
    ok = allowed(T)
    P = np.full((xw + 2, yw + 2), -1, dtype=np.int64)
    P[1:-1, 1:-1] = cost
    out = np.full((xw, yw), -1, dtype=np.int8)
    for d in range(7, -1, -1):
        dx, dy = MOVES[d]
        n = P[1 + dx:1 + dx + xw, 1 + dy:1 + dy + yw]
        hit = ok[d] & (cost > 0) & (n >= 0) & (n + WEIGHTS[d] == cost)
        out[hit] = d
    return out


def path(cost, direction, goal):
    """The cells from the goal along ``dir`` to a source, SOURCE FIRST; [] for a goal outside the map or without a cost."""
    xw, yw = cost.shape
    x, y = int(goal[0]), int(goal[1])
    if not (0 <= x < xw and 0 <= y < yw) or cost[x, y] < 0:
        return []
    cells = [(x, y)]
    while direction[x, y] >= 0:
        dx, dy = MOVES[direction[x, y]]
        x, y = x + dx, y + dy
        cells.append((x, y))
    return cells[::-1]


def answer(pmap, field, sources, foot=0, through_unknown=False, min_clear2=0, goals=None, path_cap=0):
    """One query: dict(status, cost, dir[, goal_cost, path_len, path]) with the dtypes and the -1 padding of the operator."""
    T = traversable(pmap, field, sources, foot, through_unknown, min_clear2)
    cost = costs(T, sources)
    direction = dirs(T, cost)
    out = dict(status=np.int32(0), cost=cost, dir=direction, T=T)
    if goals is not None:
        gl = np.asarray(goals).reshape(-1, 2)
        Q = gl.shape[0]
        out["goal_cost"], out["path_len"] = np.full(Q, -1, dtype=np.int32), np.zeros(Q, dtype=np.int32)
        out["path"] = np.full((Q, path_cap, 2), -1, dtype=np.int32)
        for j, g in enumerate(gl):
            cells = path(cost, direction, g)
            if cells:
                out["goal_cost"][j], out["path_len"][j] = cost[g[0], g[1]], len(cells)
                n = min(len(cells), path_cap)
                out["path"][j, :n] = np.asarray(cells[:n], dtype=np.int32).reshape(n, 2)
    return out


def no_map(shape, goals=None, path_cap=0):
    """What a query whose map entry is outside [0, G) answers."""
    out = dict(status=np.int32(-1), cost=np.full(shape, -1, dtype=np.int32), dir=np.full(shape, -1, dtype=np.int8))
    if goals is not None:
        Q = np.asarray(goals).reshape(-1, 2).shape[0]
        out.update(goal_cost=np.full(Q, -1, dtype=np.int32), path_len=np.zeros(Q, dtype=np.int32),
                   path=np.full((Q, path_cap, 2), -1, dtype=np.int32))
    return out


def batch(pmaps, sources, maps=None, fields=None, goals=None, path_cap=0, **kw):
    """Queries b on maps[b] (None: map b) stacked: the arrays of ``grid_travel_host``."""
    pmaps = np.asarray(pmaps)
    src = np.asarray(sources)
    B = src.shape[0]
    maps = range(B) if maps is None else maps
    rows = []
    for b, gi in enumerate(maps):
        gl = None if goals is None else np.asarray(goals)[b]
        if 0 <= gi < pmaps.shape[0]:
            rows.append(answer(pmaps[gi], None if fields is None else fields[gi], src[b], goals=gl, path_cap=path_cap, **kw))
        else:
            rows.append(no_map(pmaps.shape[1:], gl, path_cap))
    keys = ["status", "cost", "dir"] + (["goal_cost", "path_len", "path"] if goals is not None else [])
    return {k: np.stack([r[k] for r in rows]) for k in keys}
