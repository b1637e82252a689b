"""NumPy / heap restatement of the reference's A* global planner (course_agv_nav
global_planner.py, find_path.start_find :148-179 with append_around_open :181-204,
append_path :206-213 and find_min_cost_f :216-223).  Test infrastructure only: the CPU oracle
of tests/test_astar_ref_golden.py and the GPU tests.

Two restatements make it fast and keep it exact:
  - inflation: the in-place loop of :149-155 written as the greedy trigger set it computes.  A
    cell in rows / columns [r, span - r) triggers iff it holds 100 or -1 in the original map and
    no earlier trigger (scan order) has its (2r+1)^2 window over it; every trigger writes 99
    over its window.  This is not a dilation.
  - search: the open list's pop (the first index of the smallest f below 100 000, else index 0)
    is the smallest (min(f, 100000), seq) key, where seq numbers the cells in the order they
    were first appended (a replacement keeps its list position, a removal keeps the order).
Statuses are those of include/slam_hip.h (SLAM_ASTAR_*).
"""
from __future__ import annotations

import heapq

import numpy as np

OK, INVALID_START, INVALID_GOAL, NO_PATH, EDGE, TRUNCATED, BAD_MAP = range(7)
STATUS_NAMES = ("OK", "INVALID_START", "INVALID_GOAL", "NO_PATH", "EDGE", "TRUNCATED", "BAD_MAP")
CLAMP = 100000
# append_around_open's neighbour order (:182-185): row offset outer, column offset inner
MOVES = [(di, dj) for di in (-1, 0, 1) for dj in (-1, 0, 1) if (di, dj) != (0, 0)]


def inflate(m, span=129, r=2, counters=None):
    """The map start_find leaves behind (:149-155): a row-major int array [H][W].  ``counters``: a dict that
    receives what the trigger rule met on the way - candidates (cells of 100 or -1 in [r, span - r)^2), triggers,
    blocked_above (candidates under the window of a trigger of an earlier row), blocked_left (candidates within r
    columns of the last trigger of their own row) and blocked_left_far (those whose trigger lies in another
    64-column word); the answer is the same with or without it."""
    out = np.array(m, dtype=np.int64, copy=True)
    src = out.copy()
    H, W = out.shape
    if span > min(H, W) or r < 0:
        raise ValueError("span must be <= min(H, W) and r >= 0")
    trig = np.zeros((H, W), dtype=bool)
    stats = dict(candidates=0, triggers=0, blocked_above=0, blocked_left=0, blocked_left_far=0)
    lo, hi = r, span - r
    for i in range(lo, hi):
        above = trig[max(lo, i - r):i]
        cov = np.zeros(W, dtype=bool)
        if above.size:                          # horizontal reach of the rows above: any trigger in columns [j - r, j + r]
            c = np.concatenate([[0], np.cumsum(above.any(axis=0))])
            j = np.arange(W)
            cov = c[np.minimum(j + r + 1, W)] - c[np.maximum(j - r, 0)] > 0
        holds = (src[i] == 100) | (src[i] == -1)
        cand = holds & ~cov
        last = -(1 << 40)
        for j in np.nonzero(cand[lo:hi])[0] + lo:
            if j > last + r:                    # no earlier trigger of this row reaches j
                trig[i, j] = True
                last = j
            else:
                stats["blocked_left"] += 1
                stats["blocked_left_far"] += int(j // 64 != last // 64)
        stats["candidates"] += int(holds[lo:hi].sum())
        stats["blocked_above"] += int((holds & cov)[lo:hi].sum())
    for i, j in zip(*np.nonzero(trig)):
        out[i - r:i + r + 1, j - r:j + r + 1] = 99
    if counters is not None:
        counters.update(stats, triggers=int(trig.sum()))
    return out


def to_rows(m, wire_layout=True):
    """Row-major [H][W] view of a map given as OccupancyGrid data (wire, [H][W]) or as
    Mapping.pmap ([x][y] = [W][H])."""
    m = np.asarray(m)
    return m if wire_layout else m.T


def plan(imap, start, goal, path_cap=None, counters=False):
    """One query on an inflated row-major map.  start / goal as find_path receives them
    ([row, col] before its -1, :137-142).  Returns dict(status, path [L][2] start -> goal
    (row, col), length, expansions = len(close_list)); with ``counters`` also replacements (open
    entries replaced by a cheaper one, :200-201) and max_open (the longest the open list was when
    find_min_cost_f read it).  The other entries are the same with or without them."""
    H, W = imap.shape
    sr, sc = int(start[0]) - 1, int(start[1]) - 1
    gr, gc = int(goal[0]) - 1, int(goal[1]) - 1
    res = dict(status=OK, path=np.zeros((0, 2), np.int32), length=0, expansions=0)
    count = dict(replacements=0, max_open=0, n_open=0)

    def done(d):
        return dict(d, replacements=count["replacements"], max_open=count["max_open"]) if counters else d

    if not (0 <= sr < H and 0 <= sc < W):
        return done(dict(res, status=EDGE))
    if imap[sr, sc] != 0:
        return done(dict(res, status=INVALID_START))
    if not (0 <= gr < H and 0 <= gc < W):
        return done(dict(res, status=EDGE))
    if imap[gr, gc] != 0:
        return done(dict(res, status=INVALID_GOAL))
    free = np.asarray(imap).reshape(-1) == 0
    state = np.zeros(H * W, np.int8)      # 0 new, 1 open, 2 closed
    g, seq, parent = {}, {}, {}
    heap = []
    nseq = 0

    def expand(cell, gv):
        nonlocal nseq
        r0, c0 = divmod(cell, W)
        if r0 == 0 or r0 == H - 1 or c0 == 0 or c0 == W - 1:
            return False                  # a neighbour index would leave the map
        for di, dj in MOVES:
            n = cell + di * W + dj
            if not free[n] or state[n] == 2:
                continue
            ng = gv + 10
            f = ng + 10 * (abs(gr - (r0 + di)) + abs(gc - (c0 + dj)))
            if state[n] == 1:
                if g[n] <= ng:            # replaced only if the open f is strictly larger
                    continue
                count["replacements"] += 1
            else:
                state[n] = 1
                seq[n] = nseq
                nseq += 1
                count["n_open"] += 1
            g[n] = ng
            parent[n] = cell
            heapq.heappush(heap, (min(f, CLAMP), seq[n], n))
        return True

    s = sr * W + sc
    if not expand(s, 0):
        return done(dict(res, status=EDGE))
    state[s] = 2
    closed = 1
    goal_c = gr * W + gc
    while True:
        count["max_open"] = max(count["max_open"], count["n_open"])
        while heap:
            k, q, n = heapq.heappop(heap)
            h = 10 * (abs(gr - n // W) + abs(gc - n % W))
            if state[n] == 1 and k == min(g[n] + h, CLAMP):
                break
        else:
            return done(dict(res, status=NO_PATH, expansions=closed))
        if n == goal_c:
            cells = [n]
            while cells[-1] != s:
                cells.append(parent[cells[-1]])
            cells.reverse()
            path = np.array([divmod(c, W) for c in cells], dtype=np.int32)
            L = len(path)
            st = OK if path_cap is None or L <= path_cap else TRUNCATED
            return done(dict(status=st, path=path, length=L, expansions=closed))
        count["n_open"] -= 1                  # open_list.remove (:178)
        if not expand(n, g[n]):
            return done(dict(res, status=EDGE, expansions=closed))
        state[n] = 2
        closed += 1


def world_path(path_rc, resolution, origin_x, origin_y):
    """publisher_path / mapToWorld (:81-85, :100-121): x = col * res + origin_y + 0.25,
    y = row * res + origin_x + 0.25 - the origins swapped, a constant 0.25 offset."""
    p = np.asarray(path_rc, dtype=np.float64).reshape(-1, 2)
    x = p[:, 1] * resolution + origin_y + 0.25
    y = p[:, 0] * resolution + origin_x + 0.25
    return np.stack([x, y], axis=1)


def map_from_png(rgb, negate=True, occupied_thresh=0.65, free_thresh=0.196):
    """map_server's trinary rule: OccupancyGrid data [H][W] (row 0 = the image's bottom row)."""
    a = np.asarray(rgb)
    avg = a[..., :3].astype(np.int64).sum(axis=2) // 3 if a.ndim == 3 else a.astype(np.int64)
    if negate:
        avg = 255 - avg
    occ = (255 - avg) / 255.0
    out = np.where(occ > occupied_thresh, 100, np.where(occ < free_thresh, 0, -1)).astype(np.int8)
    return out[::-1].copy()
