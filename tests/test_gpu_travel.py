"""slam_grid_travel on the device against tests/travel_ref.py, every output with array_equal (dtype, shape and the -1
padding included) and status 0 wherever a map is named: the patterns at which a relaxation by tiles can go wrong, written
straight into the counters at the smallest shapes where it can - one cell, one row, one column, one tile of 64 x 64
exactly and one more in each axis, 130 x 67 and 67 x 130 whose walls cross every multiple of 8, 16, 32 and 64; 260 x 200
and 200 x 260, where interior tiles have all eight neighbours; sources on a tile's border, by hand; the rule clause by clause; sources; goals and paths; the room built by update_scans; one map of 1 000 x 1 000; and every Python
surface."""
import numpy as np
import pytest

import frontier_cases as FC
import frontier_ref as F
import match_ref as M
import raycast_ref as R
import travel_cases as TC
import travel_ref as T
from conftest import pkg

pytestmark = pytest.mark.gpu

PATTERNS = FC.patterns()
SHAPES = sorted({pm.shape for pm in PATTERNS.values()})
TILE = 64


@pytest.fixture(scope="module")
def slam():
    p = pkg()
    p._abi.default_context()   # fails loudly when there is no gfx950 device
    return p


@pytest.fixture(scope="module")
def ctx(slam):
    c = slam.Context(0)
    yield c
    c.close()


def first_free(pm):
    free = np.argwhere(pm == 0)
    return free[0] if len(free) else np.array([0, 0])


def spread_goals(pm, n=6):
    free = np.argwhere(pm == 0)
    xw, yw = pm.shape
    picks = free[:: max(len(free) // n, 1)][:n] if len(free) else np.zeros((0, 2), dtype=np.int64)
    picks = np.concatenate([picks, np.zeros((n - len(picks), 2), dtype=np.int64)])
    return np.concatenate([picks, [[-1, -1], [xw, 0], [xw - 1, yw - 1], first_free(pm)]]).astype(np.int32)


# ------------------------------------------------------------------ patterns
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_pattern_of_a_shape_in_one_batch(slam, ctx, shape):
    """The patterns of one size are the maps of one grid: query b reads map b (NULL routing, B = G), from the first free
    cell - the end of the serpentine, the spiral and the comb, so the wavefront re-enters every tile many times - with
    goals spread over the free cells and paths in full."""
    names = [n for n in sorted(PATTERNS) if PATTERNS[n].shape == shape]
    g, pm = FC.grid_of(slam, ctx, np.stack([PATTERNS[n] for n in names]))
    src = np.stack([[first_free(p)] for p in pm]).astype(np.int32)
    goals = np.stack([spread_goals(p) for p in pm])
    got = TC.check(slam, g, pm, src, goals=goals, path_cap=shape[0] * shape[1])
    for k, n in enumerate(names):
        kind = n.split("_")[0]
        if kind in ("serpentine", "spiral", "comb"):                      # one path: every free cell is reached
            assert np.array_equal(got["cost"][k] >= 0, pm[k] == 0), n
        if kind == "checker":                                             # no move exists at all under the no-corner-cut rule
            assert (got["cost"][k] >= 0).sum() == 1, n
        if n == "serpentine":
            assert got["cost"][k].max() == 10 * ((pm[k] == 0).sum() - 1) and got["path_len"][k].max() > 1500
    TC.check(slam, g, pm, src, through_unknown=True, foot=1)             # the unknown cells open: an open room with pillars
    g.close()


@pytest.mark.parametrize("shape", ((1, 1), (1, 70), (70, 1), (TILE, TILE), (TILE + 1, TILE), (TILE, TILE + 1), (TILE + 1, TILE + 1)),
                         ids=lambda s: "%dx%d" % s)
def test_open_room_and_random_maps_at_the_tile_edges(slam, ctx, shape):
    maps = [np.zeros(shape, dtype=np.int8)] + [FC.random_map(shape, d, 7 + k) for k, d in enumerate((0.3, 0.5, 0.6))]
    maps.append(FC.serpentine(*shape) if min(shape) >= 3 else np.zeros(shape, dtype=np.int8))
    g, pm = FC.grid_of(slam, ctx, np.stack(maps))
    last = np.array([shape[0] - 1, shape[1] - 1])
    src = np.stack([[first_free(p), last] for p in pm]).astype(np.int32)
    goals = np.stack([spread_goals(p) for p in pm])
    got = TC.check(slam, g, pm, src, goals=goals, path_cap=min(8, shape[0] * shape[1]))
    assert np.all(got["cost"][0] >= 0)                                   # the open room: every cell is reached
    TC.check(slam, g, pm, src[:, :1], through_unknown=True)
    TC.check(slam, g, pm, src, foot=8, goals=goals, path_cap=shape[0] * shape[1])
    g.close()


def test_diagonal_blobs_are_walls_at_every_residue(slam, ctx):
    g, pm = FC.grid_of(slam, ctx, PATTERNS["diagonal"])
    src = np.array([[[9 * i, 9 * j] for i in range(8) for j in range(8)]], dtype=np.int32)        # S = 64: a source in every first blob
    got = TC.check(slam, g, pm, src)
    assert (got["cost"][0] >= 0).sum() == 64 * 4                          # the second blob of a pair touches only diagonally
    TC.check(slam, g, pm, src, through_unknown=True)
    g.close()


# ------------------------------------------------------------------ many tiles
def walled_rooms(shape):
    """Free, cut by walls two cells thick ON the rows each side of a tile border - 63 | 64 and 127 | 128 - with one-cell
    doors through both rows at y = 0 and at the tile's corner cells y = 63 (first wall), y = 64 and the last column (second)."""
    pm = np.zeros(shape, dtype=np.int8)
    for rows, doors in (((63, 64), (0, 63)), ((127, 128), (64, shape[1] - 1))):
        for x in rows:
            pm[x, :] = 100
            pm[x, list(doors)] = 0
    return pm


def staircase(shape):
    """Occupied but for the band |x - y| <= 1: the diagonal steps (63, 63) -> (64, 64) and (127, 127) -> (128, 128) go
    through the corner shared by four tiles, between two cells that lie in the other two."""
    xs, ys = np.indices(shape)
    return np.where(np.abs(xs - ys) <= 1, 0, 100).astype(np.int8)


def in_tile(pm, tx, ty):
    """The first free cell of tile (tx, ty), or the tile's first cell."""
    free = np.argwhere(pm[tx * TILE:(tx + 1) * TILE, ty * TILE:(ty + 1) * TILE] == 0)
    return np.array([tx * TILE, ty * TILE]) + (free[0] if len(free) else 0)


@pytest.mark.parametrize("shape", ((260, 200), (200, 260)), ids=lambda s: "%dx%d" % s)
def test_many_tiles_with_every_interior_tile_loaded(slam, ctx, shape):
    """5 x 4 and 4 x 5 tiles, the last ones 4 and 8 cells wide: interior tiles have all eight neighbours.  Six maps in one
    grid, each queried three times in one routed call: from one end of its path, from the centre tile's corner cell, and
    from three sources in three different tiles."""
    xw, yw = shape
    names = ["serpentine", "serpentine_t", "spiral", "random_0.6", "rooms", "staircase"]
    maps = [FC.serpentine(xw, yw), np.ascontiguousarray(FC.serpentine(yw, xw).T), TC.spiral(xw, yw), FC.random_map(shape, 0.6, 19),
            walled_rooms(shape), staircase(shape)]
    g, pm = FC.grid_of(slam, ctx, np.stack(maps))
    G = len(pm)
    centre = np.array([(xw // TILE // 2) * TILE, (yw // TILE // 2) * TILE])           # the first cell of the centre tile
    src = np.empty((3 * G, 3, 2), dtype=np.int32)
    for k, p in enumerate(pm):
        src[k] = first_free(p)                                                        # S = 3 with one cell three times is S = 1
        src[G + k] = centre
        src[2 * G + k] = [in_tile(p, 0, 0), in_tile(p, 1, 2), in_tile(p, 2, 1)]
    assert all(len({(int(x) // TILE, int(y) // TILE) for x, y in s}) == 3 for s in src[2 * G:])
    goals = np.stack([spread_goals(p) for p in pm] * 3)
    got = TC.check(slam, g, pm, src, maps=np.tile(np.arange(G, dtype=np.int32), 3), goals=goals, path_cap=64)
    cost = dict(zip(names, got["cost"][:G]))
    assert cost["serpentine"].max() == 10 * ((pm[0] == 0).sum() - 1) and cost["serpentine_t"].max() == 10 * ((pm[1] == 0).sum() - 1)
    assert np.array_equal(cost["spiral"] >= 0, pm[2] == 0) and np.all(cost["rooms"][pm[4] == 0] >= 0)
    stairs = cost["staircase"]
    assert stairs[64, 64] - stairs[63, 63] == 14 and stairs[128, 128] - stairs[127, 127] == 14 and stairs[0, 0] == 0
    assert got["path_len"].max() > 64                                                  # paths longer than path_cap among them
    g.close()


# ------------------------------------------------------------------ the ring rule
def corridors():
    """name -> (cells [n, 2] in walking order, the index of the last cell before the tile border): occupied maps of
    130 x 130 with one corridor one cell wide across a tile border."""
    line = lambda lo, hi: np.arange(lo, hi + 1)
    along_x = lambda lo, hi, y: np.stack([line(lo, hi), np.full(hi - lo + 1, y)], axis=1)
    along_y = lambda x, lo, hi: np.stack([np.full(hi - lo + 1, x), line(lo, hi)], axis=1)
    return {"x 63|64": (along_x(60, 70, 20), 3), "x 127|128": (along_x(121, 129, 90), 6), "y 63|64": (along_y(20, 60, 70), 3),
            "y 127|128": (along_y(90, 121, 129), 6)}


def test_a_source_on_a_tile_border_tells_the_tile_across_it(slam, ctx):
    """The ring rule by hand: a source in the last or first row or column of its tile never goes down, so the tile across
    the border is dirty from the start or never hears of it.  Straight corridors with the source on either side of the
    border, an L whose corner (63, 63) is the source and whose way out is (64, 63), and a foot square that lies in two
    tiles with nothing else free."""
    cor = corridors()
    names = list(cor)
    pm = np.full((len(names) + 2, 130, 130), 100, dtype=np.int8)
    for k, n in enumerate(names):
        pm[k][tuple(cor[n][0].T)] = 0
    L = np.concatenate([np.stack([np.full(9, 63), np.arange(55, 64)], axis=1), np.stack([np.arange(64, 71), np.full(7, 63)], axis=1)])
    pm[len(names)][tuple(L.T)] = 0                                                    # map len(names) + 1 stays occupied throughout
    g, pm = FC.grid_of(slam, ctx, pm)
    maps, src = [], []
    for k, n in enumerate(names):
        cells, last = cor[n]
        maps += [k, k]
        src += [[cells[last]], [cells[last + 1]]]
    maps.append(len(names))
    src.append([[63, 63]])
    maps, src = np.array(maps, dtype=np.int32), np.array(src, dtype=np.int32)
    got = TC.check(slam, g, pm, src, maps=maps, goals=np.stack([cor[names[min(m, len(names) - 1)]][0][[0, -1]] for m in maps]), path_cap=16)
    for b, (m, s) in enumerate(zip(maps[:-1], src[:-1])):
        cells = cor[names[m]][0]
        assert np.array_equal(got["cost"][b][tuple(cells.T)], 10 * np.abs(cells - s[0]).sum(axis=1)), (names[m], s)
        assert (got["cost"][b] >= 0).sum() == len(cells)
    assert np.array_equal(got["cost"][-1][tuple(L.T)], 10 * np.abs(L - [63, 63]).sum(axis=1)) and (got["cost"][-1] >= 0).sum() == len(L)
    # the foot square across a border: the source two cells from it, in the corridors and on the map with nothing free
    blank = len(names) + 1
    fmaps, fsrc = [], []
    for k, n in enumerate(names):
        cells, last = cor[n]
        for s in (cells[last - 1], cells[last + 2]):
            fmaps += [k, blank]
            fsrc += [[s], [s]]
    fmaps, fsrc = np.array(fmaps, dtype=np.int32), np.array(fsrc, dtype=np.int32)
    got = TC.check(slam, g, pm, fsrc, maps=fmaps, foot=2)
    for b, m in enumerate(fmaps):
        reached = got["cost"][b] >= 0
        if m == blank:
            lo, hi = np.maximum(fsrc[b, 0] - 2, 0), np.minimum(fsrc[b, 0] + 2, 129)
            assert reached.sum() == np.prod(hi - lo + 1), (b, fsrc[b])                # the whole square, clipped by the map alone
            assert len({(x // TILE, y // TILE) for x, y in np.argwhere(reached)}) == 2
        else:
            assert np.all(reached[tuple(cor[names[m]][0].T)]), (b, fsrc[b])
    g.close()


# ------------------------------------------------------------------ the rule
def test_foot_clipped_in_a_corner_and_over_occupied_cells(slam, ctx):
    pm = np.full((3, 20, 23), 100, dtype=np.int8)
    pm[1, 5:15, 5:15] = 0
    pm[2] = FC.random_map((20, 23), 0.5, 3)
    g, pm = FC.grid_of(slam, ctx, pm)
    for src in ([0, 0], [19, 22], [10, 10], [4, 4]):
        s = np.tile(np.array(src, dtype=np.int32), (3, 1, 1))
        for foot in (0, 1, 8):
            got = TC.check(slam, g, pm, s, foot=foot)
            if src == [0, 0]:                                            # map 0 is occupied throughout: the clipped square alone
                assert (got["cost"][0] >= 0).sum() == (foot + 1) ** 2
    g.close()


def test_through_unknown_and_sources(slam, ctx):
    """S = 1, 3 and 64; sources outside the map, duplicated, on occupied cells; a query with no valid source."""
    g, pm = FC.grid_of(slam, ctx, np.stack([PATTERNS["random_65x63_0.5"], PATTERNS["random_65x63_0.6"]]))
    rng = np.random.default_rng(5)
    free = np.argwhere(pm[1] == 0)
    occupied = np.argwhere(pm[0] == 100)
    for S in (1, 3, 64):
        src = np.stack([free[rng.integers(0, len(free), S)], free[rng.integers(0, len(free), S)]]).astype(np.int32)
        src[0, -1] = occupied[0]
        if S > 1:
            src[:, 1] = src[:, 0]                                        # a duplicate
            src[1, 2 % S] = (65, 0)                                      # outside
            src[0, 0] = (-1, -1)
        for through in (False, True):
            TC.check(slam, g, pm, src, through_unknown=through)
    none = np.array([[[-1, 0], [65, 62], [0, 63]], [[64, 62], [0, -1], [70, 70]]], dtype=np.int32)
    got = TC.check(slam, g, pm, none, goals=np.zeros((2, 2, 2), dtype=np.int32), path_cap=3, through_unknown=True)
    assert np.all(got["cost"][0] == -1) and np.all(got["dir"][0] == -1) and got["status"].tolist() == [0, 0]
    assert got["goal_cost"][0].tolist() == [-1, -1] and got["path_len"][0].tolist() == [0, 0] and got["cost"][1, 64, 62] == 0
    g.close()


def test_clearance_at_its_thresholds_and_no_field_without_it(slam, ctx):
    cap = 16
    g, pm = FC.grid_of(slam, ctx, PATTERNS["random_65x63_0.6"])
    fields = np.stack([M.field(pm[0], cap)])
    assert np.array_equal(slam.grid_distance_field_host(g, cap), fields)
    cell = tuple(np.argwhere((pm[0] == 0) & (fields[0] >= 2) & (fields[0] < cap))[0])
    v = int(fields[0][cell])
    src = np.array([[cell]], dtype=np.int32)
    ctx.timing_enable(True)
    ctx.timing_read()
    TC.check(slam, g, pm, src, fields=fields, min_clear2=0, cap=cap)
    t = ctx.timing_read()
    assert t["finalize"][1] == 0 and t["grid"][1] == 1                  # no field without a clearance
    far = np.array([[[64, 62]]], dtype=np.int32)
    for c2 in (1, 4, v, v + 1, cap):
        got = TC.check(slam, g, pm, far, fields=fields, min_clear2=c2, cap=cap, through_unknown=True, foot=1)
        assert got["cost"][0, 64, 62] == 0
        assert T.traversable(pm[0], fields[0], far[0], 1, True, c2)[cell] == (c2 <= v), (c2, v)
    assert ctx.timing_read()["finalize"][1] == 5
    ctx.timing_enable(False)
    TC.check(slam, g, pm, src, fields=fields, min_clear2=1, cap=1)
    g.close()


# ------------------------------------------------------------------ goals and paths
def test_goals_and_path_cap_around_the_length(slam, ctx):
    g, pm = FC.grid_of(slam, ctx, PATTERNS["spiral_a"])
    src = np.array([[first_free(pm[0])]], dtype=np.int32)
    free = np.argwhere(pm[0] == 0)
    goals = np.array([[src[0, 0], free[40], free[-1], [1, 1], [-1, -1], [130, 0], [0, 67], [-1, 5]]], dtype=np.int32)
    full = TC.check(slam, g, pm, src, goals=goals, path_cap=130 * 67)
    n = int(full["path_len"][0, 1])
    assert full["path_len"][0, 0] == 1 and full["goal_cost"][0, 0] == 0 and n > 3 and pm[0, 1, 1] != 0
    assert full["path_len"][0, 3:].tolist() == [0] * 5 and full["goal_cost"][0, 3:].tolist() == [-1] * 5
    for cap in (0, n - 1, n, n + 1):
        got = TC.check(slam, g, pm, src, goals=goals, path_cap=cap)
        assert got["path_len"][0, 1] == n                                # the TRUE length, also beyond path_cap
    only = slam.grid_travel_host(g, src, goals=goals, path_cap=0, cost=False)                       # the goal outputs alone
    assert sorted(only) == ["goal_cost", "path_len", "status"] and np.array_equal(only["goal_cost"], full["goal_cost"])
    g.close()


def test_frontier_table_goes_in_device_to_device(slam, ctx):
    import torch
    names = ["random_130x67_0.5", "u_a", "random_130x67_0.6"]
    g, pm = FC.grid_of(slam, ctx, np.stack([PATTERNS[n] for n in names]))
    dev = torch.device("cuda", 0)
    src_h = np.stack([[first_free(p)] for p in pm]).astype(np.int32)
    src = torch.from_numpy(src_h).to(dev)
    torch.cuda.synchronize()
    table = g.frontiers(radius=0, min_unknown=0, min_size=2, max_clusters=24)[1]
    ctx.stream_order(torch.cuda.current_stream(dev).cuda_stream, 0)    # torch's copy waits for the table, the next call for the copy
    reps = table[:, :, 2:4].contiguous()
    ctx.stream_order(torch.cuda.current_stream(dev).cuda_stream, 1)
    out = g.travel(src, goals=reps, path_cap=5, dirs=True)
    ctx.synchronize()
    want_reps = F.frontiers_batch(pm, radius=0, min_unknown=0, min_size=2, M=24)[1][:, :, 2:4]
    assert np.array_equal(reps.cpu().numpy(), want_reps) and (want_reps == -1).any() and (want_reps >= 0).any()
    TC.same({k: v.cpu().numpy() for k, v in out.items()}, T.batch(pm, src_h, goals=want_reps, path_cap=5))
    g.close()


# ------------------------------------------------------------------ real maps
@pytest.mark.parametrize("scans", (1, 3, 6))
def test_room_built_by_update_scans(slam, ctx, syn, scans):
    rep = syn.make_replay(6, 120, seed=4)
    ranges, poses = np.asarray(rep.ranges, dtype=np.float32), np.asarray(rep.poses_true, dtype=np.float64)
    m = slam.Mapping.metric(400, 400, 0.05, context=ctx)
    g = FC.MapGrid(m)
    m.update_scans(ranges[:scans], R.AMIN, R.AMAX, poses[:scans])
    pm = FC.pmaps_of(g)
    assert np.array_equal(pm[0], m.pmap.astype(np.int8))
    cell = m.pose_cell(poses[scans - 1])
    src = np.array([[cell]], dtype=np.int32)
    fr = m.frontiers()
    goals = np.concatenate([fr["cell"][:12], [[0, 0]]]).astype(np.int32)[None]
    got = TC.check(slam, g, pm, src, goals=goals, path_cap=64, foot=1)
    assert (got["cost"][0] >= 0).sum() > 1000
    assert np.array_equal(m.travel_field(poses[scans - 1], foot=1), got["cost"][0])
    if scans == 3:
        TC.check(slam, g, pm, src, through_unknown=True, min_clear2=4, cap=16, fields=np.stack([M.field(pm[0], 16)]))


def test_one_map_of_1000_x_1000(slam, ctx):
    """Free but for a wall across it with one door: the costs are octile distances, to the door and on from it."""
    n, wall, door = 1000, 600, 300
    big = np.zeros((n, n), dtype=np.int8)
    big[wall, :] = 100
    big[wall, door] = 0
    g, pm = FC.grid_of(slam, ctx, big)
    s = (450, 520)
    octile = lambda x, y, ax, ay: 10 * np.maximum(abs(x - ax), abs(y - ay)) + 4 * np.minimum(abs(x - ax), abs(y - ay))
    xs, ys = np.indices((n, n))
    want = octile(xs, ys, *s)
    through = octile(wall - 1, door, *s) + 20                            # straight through the door: its corners are cut off
    want = np.where(xs > wall, through + octile(xs, ys, wall + 1, door), want)
    want[wall, :] = -1
    want[wall, door] = through - 10
    goals = np.array([[[999, 999], [0, 0], [wall, 0]]], dtype=np.int32)
    got = slam.grid_travel_host(g, np.array([[s]], dtype=np.int32), goals=goals, path_cap=4, dirs=True)
    assert got["status"].tolist() == [0] and np.array_equal(got["cost"][0], want.astype(np.int32))
    assert got["goal_cost"][0].tolist() == [want[999, 999], want[0, 0], -1] and got["path_len"][0, 2] == 0
    steps = np.abs(np.diff(got["path"][0, 0], axis=0))
    assert got["path"][0, 0, 0].tolist() == [450, 520] and got["path_len"][0, 0] > 500 and steps.max() == 1 and np.all(steps.sum(axis=1) > 0)
    d = got["dir"][0]
    assert d[s] == -1 and np.all(d[wall, np.arange(n) != door] == -1) and np.all(d[want > 0] >= 0)
    g.close()


# ------------------------------------------------------------------ Python surfaces
def u_room(closed=False):
    """Free, with a wall between the robot at cell (10, 20) and a block of unknown cells 8 cells away that leaves the way
    round by y >= 50 - unless closed - and a second block of unknown cells in a corner, further off but in the open."""
    pm = np.zeros((40, 60), dtype=np.int8)
    pm[14, :50 if not closed else 60] = 100
    pm[18:23, 18:23] = 50
    pm[0:2, 0:6] = 50
    return pm


def test_u_shaped_room_distance_and_travel_name_different_goals(slam, ctx):
    kw = dict(radius=0, min_unknown=0, min_size=1)
    m = slam.Mapping(40, 60, 0.1, context=ctx)
    g = FC.MapGrid(m)
    pm = FC.write(g, u_room()[None])
    pose = np.array([(10 + 0.5) / 10.0 - 10.0, (20 + 0.5) / 10.0 - 10.0, 0.3])
    assert m.pose_cell(pose) == (10, 20)
    fr = m.frontiers(**kw)
    assert fr["count"] == 2
    near, far = m.next_goal(pose, **kw), m.next_goal(pose, by="travel", **kw)
    assert np.array_equal(near, m.next_goal(pose, by="distance", **kw)) and not np.array_equal(near, far)
    want = T.answer(pm[0], None, [[10, 20]], goals=fr["cell"], path_cap=0)
    k = int(np.argmin(want["goal_cost"]))
    assert want["goal_cost"].min() > 0 and np.array_equal(far, fr["point"][k]) and np.array_equal(near, fr["point"][1 - k])
    assert fr["cell"][1 - k, 0] > 14 > fr["cell"][k, 0]                   # the near one lies behind the wall
    for cap in (256, 2):                                                  # path_cap is grown when the path is longer
        points, cost = m.travel_path(pose, far, path_cap=cap)
        ref = T.answer(pm[0], None, [[10, 20]], goals=[fr["cell"][k]], path_cap=4096)
        n = int(ref["path_len"][0])
        assert cost == ref["goal_cost"][0] and np.array_equal(points, slam.frontier_points(ref["path"][0, :n], 10.0, 10.0, 10.0))
        assert np.array_equal(points[-1], far) and np.array_equal(points[0], slam.frontier_points([10, 20], 10.0, 10.0, 10.0))
    round_the_wall = m.travel_path(pose, near)
    assert round_the_wall is not None and round_the_wall[1] == want["goal_cost"][1 - k] > 2 * want["goal_cost"][k]
    assert np.array_equal(m.travel_field(pose), T.answer(pm[0], None, [[10, 20]])["cost"])
    with pytest.raises(ValueError):
        m.travel_field(pose, clearance=1.0, cap=64)                       # 10 cells squared is beyond the cap
    with pytest.raises(ValueError):
        m.next_goal(pose, by="bearing")
    assert (m.travel_field(pose, clearance=0.2) >= 0).sum() < (m.travel_field(pose) >= 0).sum()
    # the wall closed: the near frontier cannot be reached, and from behind it nothing else can
    pm = FC.write(g, u_room(closed=True)[None])
    assert m.travel_path(pose, near) is None and np.array_equal(m.next_goal(pose, by="travel", **kw), far)
    behind = np.array([(30 + 0.5) / 10.0 - 10.0, (40 + 0.5) / 10.0 - 10.0, 0.0])
    assert np.array_equal(m.next_goal(behind, by="travel", **kw), near)
    pm[0, 18:23, 18:23] = 0
    FC.write(g, pm)
    assert m.next_goal(behind, by="travel", **kw) is None and m.next_goal(behind, **kw) is not None    # frontiers exist behind walls


def test_robot_on_its_own_occupied_cell_needs_the_foot(slam, ctx):
    m = slam.Mapping(30, 30, 0.1, context=ctx)
    pm = np.zeros((1, 30, 30), dtype=np.int8)
    pm[0, 14:17, 14:17] = 100
    FC.write(FC.MapGrid(m), pm)
    pose = ((15 + 0.5) / 10.0 - 10.0, (15 + 0.5) / 10.0 - 10.0, 0.0)
    assert (m.travel_field(pose) >= 0).sum() == 1 and np.all(m.travel_field(pose, foot=1) >= 0)


def test_gridslam_next_goal_by_travel(slam, ctx, syn):
    rep = syn.make_replay(3, 120, seed=4)
    s = slam.GridSLAM(200, 200, 0.1, 4, np.random.default_rng(3), context=ctx)
    s.init(rep.poses_true[0])
    for r in np.asarray(rep.ranges, dtype=np.float32)[:2]:
        s.update(r, R.AMIN, R.AMAX)
    kw = dict(radius=1, min_unknown=3, min_size=2, max_clusters=64)
    fr = s.frontiers(**kw)
    p = s.best_pose
    cell = [int(s.grid.scale * (p[0] + s.grid.off_x)), int(s.grid.scale * (p[1] + s.grid.off_y))]
    want = T.answer(s.pmap, None, [cell], foot=1, goals=fr["cell"])["goal_cost"].astype(np.int64)
    goal = s.next_goal(by="travel", foot=1, **kw)
    assert (want >= 0).any() and np.array_equal(goal, fr["point"][int(np.argmin(np.where(want >= 0, want, 1 << 40)))])
    assert np.array_equal(s.next_goal(**kw), s.next_goal(by="distance", **kw))


def test_device_gridslam_travel_and_next_goals(slam, ctx):
    import torch
    d = slam.DeviceGridSLAM(3, 2, 65, 63, 0.1, angle_min=R.AMIN, angle_max=R.AMAX, n=8, context=ctx)
    names = ["random_65x63_0.6", "random_65x63_0.5", "random_65x63_0.6", "random_65x63_0.5", "random_65x63_0.3", "random_65x63_0.6"]
    pm = FC.write(d.grid, np.stack([PATTERNS[n] for n in names]))
    scale, ox, oy = d.grid.scale, d.grid.off_x, d.grid.off_y
    free = np.argwhere(pm[1] == 0)[5]
    poses = np.zeros((3, 2, 3))
    poses[0, 1, :2] = ((free[0] + 0.25) / scale - ox, (free[1] + 0.75) / scale - oy)
    poses[2, 0, :2] = (-0.4 / scale - ox, 7.5 / scale - oy)                # truncation toward zero: cell (0, 7), not (-1, 7)
    d.set_particles(poses)
    d.info[:, 0] = torch.tensor([1, -1, 0], dtype=torch.int32, device=d.dev)   # filter 1 has no live particle: no map, not map 3
    torch.cuda.synchronize()
    cells = np.array([[[int(scale * (poses[0, 1, 0] + ox)), int(scale * (poses[0, 1, 1] + oy))]], [[-1, -1]],
                      [[int(scale * (poses[2, 0, 0] + ox)), int(scale * (poses[2, 0, 1] + oy))]]], dtype=np.int32)
    assert cells[0, 0].tolist() == free.tolist() and cells[2, 0].tolist() == [0, 7]
    maps = [1, -1, 4]
    out = d.travel(foot=1, dirs=True)
    ctx.synchronize()
    TC.same({k: v.cpu().numpy() for k, v in out.items()}, T.batch(pm, cells, maps=maps, foot=1))
    assert out["status"].cpu().tolist() == [0, -1, 0]
    kw = dict(radius=1, min_unknown=2, min_size=2)
    cell, cost, status = d.next_goals(foot=1, max_clusters=32, **kw)
    ctx.synchronize()
    reps = F.frontiers_batch(pm, maps=maps, M=32, **kw)[1][:, :, 2:4]
    want = T.batch(pm, cells, maps=maps, foot=1, goals=reps)["goal_cost"].astype(np.int64)
    assert status.cpu().tolist() == [0, -1, 0]
    for f in range(3):
        k = int(np.argmin(np.where(want[f] >= 0, want[f], 1 << 40)))
        if want[f, k] >= 0:
            assert cell[f].cpu().tolist() == reps[f, k].tolist() and cost[f].item() == want[f, k], f
        else:
            assert cell[f].cpu().tolist() == [-1, -1] and cost[f].item() == -1, f
    assert (want[0] >= 0).any() and not (want[1] >= 0).any()
