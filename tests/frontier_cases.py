"""The maps that the CPU and the GPU tests of slam_grid_frontiers share (test infrastructure only): patterns at which a
labelling kernel can still go wrong, as pmaps of 0 (free), 50 (unknown) and 100 (occupied), and the helpers that write
them straight into a grid's counters and compare every output with the restatement (tests/frontier_ref.py)."""
import numpy as np

import frontier_ref as F

A, B = (130, 67), (67, 130)        # lines cross every multiple of 8, 16, 32 and 64 in both axes


def blank(shape):
    return np.full(shape, 50, dtype=np.int8)


def serpentine(xw=70, yw=65):
    """A one-cell-wide path through unknown space: every second row, joined at alternating ends.  One component whose
    label lies at one end."""
    pm = blank((xw, yw))
    pm[0::2] = 0
    for k, x in enumerate(range(1, xw - 1, 2)):
        pm[x, yw - 1 if k % 2 == 0 else 0] = 0
    return pm


def spiral(xw, yw):
    """A square spiral inward, one cell wide, one unknown cell between its arms: a walk from (0, 0) that turns when the
    cell two ahead is free already."""
    pm = blank((xw, yw))
    x, y, d = 0, 0, 0
    pm[0, 0] = 0
    inside = lambda i, j: 0 <= i < xw and 0 <= j < yw
    while True:
        dx, dy = ((0, 1), (1, 0), (0, -1), (-1, 0))[d]
        moved = 0
        while inside(x + dx, y + dy) and not (inside(x + 2 * dx, y + 2 * dy) and pm[x + 2 * dx, y + 2 * dy] == 0):
            x, y, moved = x + dx, y + dy, moved + 1
            pm[x, y] = 0
        if moved == 0:
            return pm
        d = (d + 1) % 4


def comb(shape):
    """Teeth along x in every second column, joined only in the last row."""
    pm = blank(shape)
    pm[:, 0::2] = 0
    pm[-1, :] = 0
    return pm


def u_shapes(shape):
    """Pairs of arms that meet in the last row only: every U is one component, and its arms carry two labels until then."""
    pm = blank(shape)
    xw, yw = shape
    for y in range(0, yw - 2, 4):
        pm[:, y] = 0
        pm[:, y + 2] = 0
        pm[-1, y + 1] = 0
    return pm


def checkerboard(shape):
    pm = blank(shape)
    xs, ys = np.indices(shape)
    pm[(xs + ys) % 2 == 0] = 0
    return pm


def diagonal_blobs():
    """64 pairs of 2 x 2 blobs that touch only diagonally, the touching point at every residue of (x mod 8, y mod 8)."""
    pm = blank((72, 72))
    for i in range(8):
        for j in range(8):
            x, y = 9 * i, 9 * j
            pm[x:x + 2, y:y + 2] = 0
            pm[x + 2:x + 4, y + 2:y + 4] = 0
    return pm


def lattice(shape):
    """Isolated cells on a stride-2 lattice: ceil(xw / 2) * ceil(yw / 2) clusters of one cell."""
    pm = blank(shape)
    pm[0::2, 0::2] = 0
    return pm


def rules():
    """A free 9 x 11 map with unknown and occupied cells placed so that every clause of the cell rule decides somewhere."""
    pm = np.zeros((9, 11), dtype=np.int8)
    pm[0, 1] = 50           # corner (0, 0) has an unknown neighbour inside the map; corner (8, 10) has none
    pm[4, 0] = 50           # on the edge y = 0: (3, 0) and (5, 0) qualify
    pm[8, 5] = 50           # on the edge x = 8
    pm[6, 3] = 50           # (5, 2), (7, 4), (5, 4), (7, 2) have only this diagonal neighbour
    pm[3, 7] = 50
    pm[3, 8] = 100          # (2, 8) and (4, 8) are next to an occupied cell; (3, 6) next to the unknown one only
    pm[2, 6] = 100          # (2, 7) and (3, 6) are next to an occupied cell AND the unknown (3, 7): they qualify
    pm[3, 9] = 50           # (3, 10): an edge cell between an unknown cell and the map's edge
    return pm


def crescent():
    """Half a ring, two cells thick: its centroid lies outside it."""
    pm = blank((40, 40))
    xs, ys = np.indices(pm.shape)
    d2 = (xs - 20) ** 2 + (ys - 20) ** 2
    pm[(d2 >= 100) & (d2 < 169) & (ys <= 20)] = 0
    return pm


def ties():
    """Four free cells around an occupied one: one 8-connected cluster, the centroid is the occupied cell and all four
    members are as near; and a pair whose rounded centroid is its second cell."""
    pm = blank((12, 12))
    pm[5, 5] = 100
    for x, y in ((4, 5), (5, 4), (5, 6), (6, 5)):
        pm[x, y] = 0
    pm[9, 2] = pm[9, 3] = 0
    return pm


def random_map(shape, density, seed):
    """Free cells at `density` in unknown space, 5 % occupied."""
    rng = np.random.default_rng(seed)
    u = rng.random(shape)
    pm = blank(shape)
    pm[u < density] = 0
    pm[rng.random(shape) < 0.05] = 100
    return pm


def patterns():
    """name -> pmap: every pattern above at the sizes the tests use."""
    out = {"serpentine": serpentine(), "serpentine_t": np.ascontiguousarray(serpentine().T)}
    for tag, shape in (("a", A), ("b", B)):
        out["spiral_" + tag] = spiral(*shape)
        out["comb_" + tag] = comb(shape)
        out["u_" + tag] = u_shapes(shape)
        out["checker_" + tag] = checkerboard(shape)
    out.update(diagonal=diagonal_blobs(), rules=rules(), crescent=crescent(), ties=ties())
    for shape in ((65, 63), A):
        for k, density in enumerate((0.3, 0.5, 0.6)):
            out["random_%dx%d_%g" % (shape + (density,))] = random_map(shape, density, 100 * shape[0] + k)
    return out


# ------------------------------------------------------------------ the device side
class MapGrid:
    """A Mapping's one map seen as a grid of G = 1, for the helpers here and for grid_frontiers_host."""

    def __init__(self, m):
        self._ctx, self._h, self.G, self.xw, self.yw = m._ctx, m.grid._h, 1, m.xw, m.yw

    def read(self, gi, want=("pmap",)):
        from conftest import pkg
        abi = pkg("_abi")
        out = np.empty((self.xw, self.yw), dtype=np.int8)
        abi.check(abi.lib().slam_grid_read(self._ctx.handle, self._h, 0, abi.ptr(out), None, None, None))
        return {"pmap": out}


def counters(g):
    """(pass, hit): torch int32 views [G, xw, yw] of the grid's device counters."""
    import ctypes as C
    import torch
    from conftest import pkg
    abi = pkg("_abi")
    p, h = C.c_void_p(), C.c_void_p()
    abi.check(abi.lib().slam_grid_counters_dev(g._ctx.handle, g._h, C.byref(p), C.byref(h)))

    class View:
        def __init__(self, ptr):
            self.__cuda_array_interface__ = {"shape": (g.G, g.xw, g.yw), "typestr": "<i4", "data": (int(ptr), False), "version": 2}
    dev = torch.device("cuda", g._ctx.device)
    return torch.as_tensor(View(p.value), device=dev), torch.as_tensor(View(h.value), device=dev)


def pmaps_of(g):
    return np.stack([g.read(gi, want=("pmap",))["pmap"] for gi in range(g.G)])


def write(g, pmaps):
    """pmaps [G, xw, yw] written straight into the counters: pass = 1 frees a cell, hit = 1 occupies it, nothing leaves
    it unknown.  Returns the pmaps read back, which are the ones given."""
    import torch
    g._ctx.synchronize()
    p, h = counters(g)
    pm = np.asarray(pmaps).reshape(g.G, g.xw, g.yw)
    p.copy_(torch.from_numpy((pm == 0).astype(np.int32)).to(p.device))
    h.copy_(torch.from_numpy((pm == 100).astype(np.int32)).to(h.device))
    torch.cuda.synchronize()
    back = pmaps_of(g)
    assert np.array_equal(back, pm)
    return back


def grid_of(slam, ctx, pmaps, scale=1.0):
    pm = np.asarray(pmaps)
    pm = pm[None] if pm.ndim == 2 else pm
    g = slam.DeviceGrid(pm.shape[0], pm.shape[1], pm.shape[2], scale, 0.0, 0.0, context=ctx)
    return g, write(g, pm)


DTYPES = (np.int32, np.int32, np.int64, np.int32)


def same(got, want):
    assert len(got) == len(want)
    for a, b, dt in zip(got, want, DTYPES):
        assert a.dtype == dt and a.shape == b.shape, (a.dtype, a.shape, b.shape)
        assert np.array_equal(a, b), (np.argwhere(a != b)[:5], a[a != b][:5], b[a != b][:5])


def check(slam, g, pmaps, maps=None, B=None, radius=0, min_unknown=0, min_size=1, M=64, fields=None, min_clear2=0, cap=64):
    """The host form, labels included, against the restatement on the pmaps read back."""
    want = F.frontiers_batch(pmaps, maps=maps, B=B, fields=fields, radius=radius, min_unknown=min_unknown, min_size=min_size, M=M,
                             min_clear2=min_clear2)
    got = slam.grid_frontiers_host(g, grid_of_batch=maps, B=B, radius=radius, min_unknown=min_unknown, min_clear2=min_clear2, cap=cap,
                                   min_size=min_size, max_clusters=M, labels=True)
    same(got, want)
    return got
