"""slam_grid_frontiers restated with NumPy and Python integers (include/slam_hip.h is the definition): the frontier mask
from shifted arrays and shifted adds, the 8-connected components by a union-find over the frontier cells only, the
statistics, the representative cell, the table in label order and the per-query outputs, which no chunking can change
because nothing here knows of chunks.  Test infrastructure only."""
import numpy as np


def unknown_count(pmap, radius):
    """The number of cells equal to 50 in the (2 radius + 1)^2 window of every cell, over the cells inside the map."""
    xw, yw = pmap.shape
    r = int(radius)
    pad = np.zeros((xw + 2 * r, yw + 2 * r), dtype=np.int32)
    pad[r:r + xw, r:r + yw] = pmap == 50
    rows = np.zeros((xw + 2 * r, yw), dtype=np.int32)
    for d in range(2 * r + 1):
        rows += pad[:, d:d + yw]
    out = np.zeros((xw, yw), dtype=np.int32)
    for d in range(2 * r + 1):
        out += rows[d:d + xw]
    return out


def mask(pmap, radius=0, min_unknown=0, field=None, min_clear2=0):
    """F [xw, yw] bool."""
    pm = np.asarray(pmap)
    unk = pm == 50
    near = np.zeros(pm.shape, dtype=bool)
    near[1:] |= unk[:-1]
    near[:-1] |= unk[1:]
    near[:, 1:] |= unk[:, :-1]
    near[:, :-1] |= unk[:, 1:]
    f = (pm == 0) & near
    if min_unknown > 0:
        f &= unknown_count(pm, radius) >= int(min_unknown)
    if min_clear2 > 0:
        f &= np.asarray(field).astype(np.int64) >= int(min_clear2)
    return f


def label(f):
    """labels int32 [xw, yw]: the smallest flat index of the 8-connected component of every frontier cell, -1 elsewhere.
    A union-find over the frontier cells in flat order: a cell meets the four neighbours before it."""
    xw, yw = f.shape
    flat = np.flatnonzero(f.reshape(-1))
    slot = {int(c): k for k, c in enumerate(flat)}
    parent = list(range(len(flat)))

    def find(k):
        root = k
        while parent[root] != root:
            root = parent[root]
        while parent[k] != root:
            parent[k], k = root, parent[k]
        return root

    for k, c in enumerate(flat):
        c = int(c)
        x, y = divmod(c, yw)
        for dx, dy in ((0, -1), (-1, -1), (-1, 0), (-1, 1)):
            nx, ny = x + dx, y + dy
            if 0 <= nx < xw and 0 <= ny < yw:
                j = slot.get(nx * yw + ny)
                if j is not None:
                    a, b = find(k), find(j)
                    if a != b:
                        parent[max(a, b)] = min(a, b)
    out = np.full(xw * yw, -1, dtype=np.int32)
    for k, c in enumerate(flat):
        out[c] = flat[find(k)]          # slots are in flat order, so the smallest slot is the smallest flat index
    return out.reshape(xw, yw)


def clusters_of(labels):
    """Every cluster in label order: rows (label, size, rep_x, rep_y, x0, y0, x1, y1) int64 and (sx, sy) int64."""
    xw, yw = labels.shape
    flat = np.flatnonzero(labels.reshape(-1) >= 0)
    lab = labels.reshape(-1)[flat]
    order = np.argsort(lab, kind="stable")
    flat, lab = flat[order], lab[order]
    rows, sums = [], []
    cuts = np.flatnonzero(np.diff(lab)) + 1
    for cells in np.split(flat, cuts) if len(flat) else []:
        xs, ys = [int(v) for v in cells // yw], [int(v) for v in cells % yw]
        size, sx, sy = len(xs), sum(xs), sum(ys)
        cxr, cyr = (2 * sx + size) // (2 * size), (2 * sy + size) // (2 * size)
        _, rep = min(((x - cxr) ** 2 + (y - cyr) ** 2, int(c)) for x, y, c in zip(xs, ys, cells))
        rows.append((int(cells.min()), size, rep // yw, rep % yw, min(xs), min(ys), max(xs), max(ys)))
        sums.append((sx, sy))
    return np.array(rows, dtype=np.int64).reshape(-1, 8), np.array(sums, dtype=np.int64).reshape(-1, 2)


def frontiers(pmap, radius=2, min_unknown=13, min_size=5, M=256, field=None, min_clear2=0):
    """One query: (count int32 [2], clusters int32 [M, 8], sums int64 [M, 2], labels int32 [xw, yw])."""
    labels = label(mask(pmap, radius, min_unknown, field, min_clear2))
    rows, sums = clusters_of(labels)
    keep = rows[:, 1] >= int(min_size)
    rows, sums = rows[keep], sums[keep]
    count = np.array([len(rows), int((labels >= 0).sum())], dtype=np.int32)
    table = np.full((M, 8), -1, dtype=np.int32)
    stab = np.full((M, 2), -1, dtype=np.int64)
    k = min(len(rows), M)
    table[:k], stab[:k] = rows[:k], sums[:k]
    return count, table, stab, labels


def frontiers_batch(pmaps, maps=None, B=None, fields=None, **kw):
    """The batch: query b reads pmaps[maps[b]] (maps None: b); an entry outside [0, G) answers (-1, -1), rows and labels
    of -1.  Every distinct map is worked out once.  Returns (count [B, 2], clusters [B, M, 8], sums [B, M, 2], labels)."""
    G = len(pmaps)
    maps = list(range(G if B is None else B)) if maps is None else [int(m) for m in maps]
    M = kw.get("M", 256)
    xw, yw = pmaps[0].shape
    done, out = {}, []
    for gi in maps:
        if not 0 <= gi < G:
            out.append((np.full(2, -1, np.int32), np.full((M, 8), -1, np.int32), np.full((M, 2), -1, np.int64),
                        np.full((xw, yw), -1, np.int32)))
            continue
        if gi not in done:
            done[gi] = frontiers(pmaps[gi], field=None if fields is None else fields[gi], **kw)
        out.append(done[gi])
    return tuple(np.stack([o[k] for o in out]) for k in range(4))


def flood(f):
    """The same labels by an independent flood fill: a stack, 8 neighbours, seeds in flat order."""
    xw, yw = f.shape
    out = np.full((xw, yw), -1, dtype=np.int32)
    for x0, y0 in zip(*np.nonzero(f)):
        if out[x0, y0] >= 0:
            continue
        seed = int(x0) * yw + int(y0)
        out[x0, y0] = seed
        stack = [(int(x0), int(y0))]
        while stack:
            x, y = stack.pop()
            for dx in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    nx, ny = x + dx, y + dy
                    if 0 <= nx < xw and 0 <= ny < yw and f[nx, ny] and out[nx, ny] < 0:
                        out[nx, ny] = seed
                        stack.append((nx, ny))
    return out


def sizes_by_rank(labels):
    """Cluster sizes, largest first."""
    lab = labels[labels >= 0]
    return sorted(np.unique(lab, return_counts=True)[1].tolist(), reverse=True)
