"""slam_grid_frontiers on the device against tests/frontier_ref.py, every output with array_equal (dtype, shape and the -1
padding included): the patterns at which a labelling kernel can go wrong, written straight into the counters at sizes
whose lines cross every multiple of 8, 16, 32 and 64; the cell rule clause by clause; the window and the clearance at
their thresholds; counts far above the table; statistics; random maps near the percolation threshold; the ragged maps and
the room built by update_scans; batches routed, alone, reversed and with entries that name no map; and every Python
surface."""
import numpy as np
import pytest

import frontier_cases as FC
import frontier_ref as F
import locate_ref as L
import match_ref as M
import raycast_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu

PATTERNS = FC.patterns()
SHAPES = sorted({pm.shape for pm in PATTERNS.values()})


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


# ------------------------------------------------------------------ labelling
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_pattern_of_a_shape_in_one_batch(slam, ctx, shape):
    """The patterns of one size are the maps of one grid: query b reads map b (NULL routing, B = G)."""
    names = [n for n in sorted(PATTERNS) if PATTERNS[n].shape == shape]
    g, pm = FC.grid_of(slam, ctx, np.stack([PATTERNS[n] for n in names]))
    got = FC.check(slam, g, pm, M=512)                                   # the plain rule, every cluster, none beyond the table
    assert got[0][:, 0].max() <= 512
    for k, n in enumerate(names):                                        # one component, its label at its first cell
        if n.split("_")[0] in ("serpentine", "spiral", "comb", "checker", "crescent"):
            assert got[0][k, 0] == 1 and got[1][k, 0, 0] == np.flatnonzero(F.mask(pm[k]).reshape(-1))[0], n
    FC.check(slam, g, pm, radius=1, min_unknown=3, min_size=2, M=64)
    FC.check(slam, g, pm, radius=2, min_unknown=13, min_size=5, M=256)   # the defaults


def test_diagonal_touch_at_every_tile_corner(slam, ctx):
    g, pm = FC.grid_of(slam, ctx, PATTERNS["diagonal"])
    got = FC.check(slam, g, pm, M=64)
    assert got[0][0].tolist() == [64, 511] and got[1][0, 1:, 1].tolist() == [8] * 63 and got[1][0, 0, 1] == 7


def test_counts_far_above_the_table(slam, ctx):
    lat = FC.lattice(FC.A)
    g, pm = FC.grid_of(slam, ctx, lat)
    n = 65 * 34
    for Mx in (0, 1, n - 1, n, n + 1):
        count, table, sums, labels = FC.check(slam, g, pm, M=Mx)
        assert count[0].tolist() == [n, n] and table.shape == (1, Mx, 8)
        k = min(Mx, n)
        assert np.all(np.diff(table[0, :k, 0]) > 0) and np.all(table[0, k:] == -1) and np.all(sums[0, k:] == -1)
        assert np.array_equal(table[0, :k, 0], np.flatnonzero(lat.reshape(-1) == 0)[:k])
    count, table, _ = slam.grid_frontiers_host(g, radius=0, min_unknown=0, min_size=1, max_clusters=0)   # NULL tables
    assert count.tolist() == [[n, n]] and table.shape == (1, 0, 8)


# ------------------------------------------------------------------ the cell rule
def test_cell_rule_clause_by_clause(slam, ctx):
    g, pm = FC.grid_of(slam, ctx, PATTERNS["rules"])
    labels = FC.check(slam, g, pm, M=16)[3][0]
    f = labels >= 0
    assert f[0, 0] and not f[8, 10] and f[3, 0] and f[5, 0] and f[8, 4] and f[8, 6] and f[7, 5]
    assert not (f[5, 2] or f[7, 4] or f[5, 4] or f[7, 2])               # only a diagonal unknown neighbour
    assert f[2, 7] and f[3, 6] and f[3, 10] and not f[3, 8] and not f[2, 8]


@pytest.mark.parametrize("radius", (0, 1, 2, 8))
def test_window_rule_at_its_thresholds(slam, ctx, radius):
    """A 9 x 11 map: the window of radius 8 exceeds it.  For a corner cell (its window clipped on two sides) and an inner
    cell: min_unknown at 0, 1, exactly the number present, one more, and (2r + 1)^2."""
    g, pm = FC.grid_of(slam, ctx, PATTERNS["rules"])
    full = (2 * radius + 1) ** 2
    present = F.unknown_count(pm[0], radius)
    for cell in ((0, 0), (7, 5)):
        n = int(present[cell])
        for mu in sorted({0, 1, n, n + 1, full}):
            if mu > full:
                continue
            labels = FC.check(slam, g, pm, radius=radius, min_unknown=mu, M=16)[3][0]
            assert (labels[cell] >= 0) == (mu <= n), (cell, mu, n)
    assert present[0, 0] == {0: 0, 1: 1, 2: 1, 8: 5}[radius]


def test_clearance_at_its_thresholds(slam, ctx):
    cap = 16
    g, pm = FC.grid_of(slam, ctx, PATTERNS["random_65x63_0.5"])
    fields = np.stack([M.field(pm[0], cap)])
    assert np.array_equal(slam.grid_distance_field_host(g, cap), fields)
    plain = F.mask(pm[0])
    cell = tuple(np.argwhere(plain & (fields[0] >= 2) & (fields[0] < cap))[0])
    v = int(fields[0][cell])
    ctx.timing_enable(True)
    ctx.timing_read()
    FC.check(slam, g, pm, fields=fields, min_clear2=0, cap=cap)
    t = ctx.timing_read()
    assert t["finalize"][1] == 0 and t["grid"][1] == 1                  # no field without a clearance
    for c2 in (1, 4, v, v + 1, cap):
        labels = FC.check(slam, g, pm, fields=fields, min_clear2=c2, cap=cap)[3][0]
        assert (labels[cell] >= 0) == (c2 <= v), (c2, v)
    assert ctx.timing_read()["finalize"][1] == 5
    ctx.timing_enable(False)
    FC.check(slam, g, pm, fields=fields, min_clear2=2, cap=cap, radius=1, min_unknown=2, min_size=2)


# ------------------------------------------------------------------ statistics
def test_crescent_ties_and_min_size(slam, ctx):
    g, pm = FC.grid_of(slam, ctx, PATTERNS["crescent"])
    count, table, sums, labels = FC.check(slam, g, pm, M=4)
    size = int(table[0, 0, 1])
    cx, cy = (2 * sums[0, 0] + size) // (2 * size)
    assert count[0, 0] == 1 and labels[0][cx, cy] == -1                 # the centroid lies outside the crescent
    assert labels[0][table[0, 0, 2], table[0, 0, 3]] == table[0, 0, 0]  # the representative is a member
    g, pm = FC.grid_of(slam, ctx, PATTERNS["ties"])
    table = FC.check(slam, g, pm, M=4)[1]
    assert table[0, :2, :4].tolist() == [[4 * 12 + 5, 4, 4, 5], [9 * 12 + 2, 2, 9, 3]]
    g, pm = FC.grid_of(slam, ctx, PATTERNS["random_65x63_0.6"])
    largest = F.sizes_by_rank(F.label(F.mask(pm[0])))[0]
    for ms, kept in ((1, None), (2, None), (largest, 1), (largest + 1, 0)):
        count, _, _, labels = FC.check(slam, g, pm, min_size=ms, M=32)
        assert kept is None or count[0, 0] == kept
        assert count[0, 1] == (labels >= 0).sum()                        # the labels keep the clusters below min_size


# ------------------------------------------------------------------ real maps
@pytest.mark.parametrize("shape", L.RAGGED, ids=lambda s: "%dx%d" % s)
def test_ragged_maps_have_no_free_cell(slam, ctx, shape):
    want, _ = L.ragged_pmap(*shape)
    g, pm = FC.grid_of(slam, ctx, want)
    count, table, _, labels = FC.check(slam, g, pm, M=8)
    assert count.tolist() == [[0, 0]] and np.all(table == -1) and np.all(labels == -1)


@pytest.mark.parametrize("beams", (120, 360))
def test_room_built_by_update_scans(slam, ctx, syn, beams):
    rep = syn.make_replay(6, beams, seed=4)
    ranges, poses = np.asarray(rep.ranges, dtype=np.float32), np.asarray(rep.poses_true, dtype=np.float64)
    m = slam.Mapping.metric(400, 400, 0.05, context=ctx)
    g = FC.MapGrid(m)
    for lo, hi in ((0, 1), (1, 3), (3, 6)):                             # 1, 3 and 6 scans in the map
        m.update_scans(ranges[lo:hi], R.AMIN, R.AMAX, poses[lo:hi])
        pm = FC.pmaps_of(g)
        assert np.array_equal(pm[0], m.pmap.astype(np.int8))
        plain = FC.check(slam, g, pm, M=256)
        kept = FC.check(slam, g, pm, radius=2, min_unknown=13, min_size=5, M=256)
    assert np.array_equal(pm[0], R.room_pmap(ranges, poses))
    want = {120: ([77, 8672], [23, 500]), 360: ([84, 1342], [1, 38])}[beams]      # the experiment behind the defaults
    assert [plain[0][0].tolist(), kept[0][0].tolist()] == list(want)
    # Mapping.frontiers is the same answer as a dict, next_goal the nearest representative
    fr = m.frontiers()
    K = int(kept[0][0, 0])
    assert fr["count"] == K and fr["n_frontier"] == kept[0][0, 1] and np.array_equal(fr["label"], kept[1][0, :K, 0])
    assert np.array_equal(fr["cell"], kept[1][0, :K, 2:4]) and np.array_equal(fr["bbox"], kept[1][0, :K, 4:8])
    assert np.array_equal(fr["point"], (kept[1][0, :K, 2:4] + 0.5) / 20.0 - 10.0)
    assert np.array_equal(fr["centroid"], (kept[2][0, :K] / kept[1][0, :K, 1:2] + 0.5) / 20.0 - 10.0)
    goal = m.next_goal(poses[-1])
    d = ((fr["point"] - poses[-1][:2]) ** 2).sum(axis=1)
    assert np.array_equal(goal, fr["point"][int(np.argmin(d))])
    with pytest.raises(ValueError):
        m.frontiers(clearance=1.0, cap=64)                               # 20 cells squared is beyond the cap
    assert m.frontiers(clearance=0.1)["count"] <= K


# ------------------------------------------------------------------ batches
def test_batches_routed_alone_reversed_and_entries_without_a_map(slam, ctx):
    names = ["random_130x67_0.3", "u_a", "random_130x67_0.6"]
    g, pm = FC.grid_of(slam, ctx, np.stack([PATTERNS[n] for n in names]))
    maps = np.array([2, 0, 1, 1, -1, 3, 0], dtype=np.int32)              # duplicates, -1 and G among them
    kw = dict(radius=1, min_unknown=2, min_size=2, M=40)
    batch = FC.check(slam, g, pm, maps=maps, **kw)
    assert batch[0][4].tolist() == [-1, -1] == batch[0][5].tolist() and np.all(batch[1][4:6] == -1) and np.all(batch[3][4:6] == -1)
    rev = FC.check(slam, g, pm, maps=maps[::-1].copy(), **kw)
    FC.same(tuple(a[::-1] for a in rev), batch)
    for b, gi in enumerate(maps):
        FC.same(FC.check(slam, g, pm, maps=[gi], **kw), tuple(a[b:b + 1] for a in batch))
    null = FC.check(slam, g, pm, **kw)                                    # NULL routing: B = G, query b reads map b
    FC.same(null, tuple(a[[1, 2, 0]] for a in batch))                     # maps 0, 1, 2 are queries 1, 2, 0 of the batch
    FC.check(slam, g, pm, B=2, **kw)
    with pytest.raises(slam.SlamError, match="B > G"):
        slam.grid_frontiers_host(g, B=4)
    FC.check(slam, g, pm, **kw)
    ctx.check_status()


# ------------------------------------------------------------------ the particle filters
def test_gridslam_frontiers_on_the_best_particles_map(slam, ctx, syn):
    rep = syn.make_replay(3, 120, seed=4)
    s = slam.GridSLAM(200, 200, 0.1, 4, np.random.default_rng(3), context=ctx)
    s.init(rep.poses_true[0])
    for r in np.asarray(rep.ranges, dtype=np.float32)[:2]:
        s.update(r, R.AMIN, R.AMAX)
    pm = s.pmap
    want = F.frontiers(pm, radius=1, min_unknown=3, min_size=2, M=64)
    fr = s.frontiers(radius=1, min_unknown=3, min_size=2, max_clusters=64)
    K = int(want[0][0])
    assert K > 0 and fr["count"] == K and fr["n_frontier"] == want[0][1]
    assert np.array_equal(fr["label"], want[1][:K, 0]) and np.array_equal(fr["cell"], want[1][:K, 2:4])
    goal = s.next_goal(radius=1, min_unknown=3, min_size=2, max_clusters=64)
    d = ((fr["point"] - s.best_pose[:2]) ** 2).sum(axis=1)
    assert np.array_equal(goal, fr["point"][int(np.argmin(d))])


def test_device_gridslam_frontiers_and_a_filter_without_a_particle(slam, ctx):
    import torch
    d = slam.DeviceGridSLAM(2, 2, 65, 63, 0.1, angle_min=R.AMIN, angle_max=R.AMAX, n=8, context=ctx)
    names = ["random_65x63_0.3", "random_65x63_0.5", "random_65x63_0.6", "random_65x63_0.5"]
    pm = FC.write(d.grid, np.stack([PATTERNS[n] for n in names]))
    d.info[:, 0] = torch.tensor([1, -1], dtype=torch.int32, device=d.dev)     # filter 1 has no live particle: no map, not map 1
    torch.cuda.synchronize()
    out = d.frontiers(radius=1, min_unknown=2, min_size=2, max_clusters=32, labels=True)
    ctx.synchronize()
    want = F.frontiers_batch(pm, maps=[1, -1], radius=1, min_unknown=2, min_size=2, M=32)
    FC.same(tuple(t.cpu().numpy() for t in out), want)
    assert want[0][1].tolist() == [-1, -1] and want[0][0, 0] > 0


def test_mapping_has_no_goal_on_an_unknown_and_on_a_free_map(slam, ctx):
    m = slam.Mapping(40, 33, 0.1, context=ctx)
    assert m.next_goal((0.0, 0.0, 0.0)) is None and m.frontiers()["count"] == 0           # nothing is known
    g = FC.MapGrid(m)
    FC.write(g, np.zeros((1, 40, 33), dtype=np.int8))
    fr = m.frontiers(min_unknown=0, min_size=1)
    assert m.next_goal((0.0, 0.0, 0.0), min_unknown=0, min_size=1) is None and fr["count"] == 0 and fr["n_frontier"] == 0
    assert fr["label"].shape == (0,) and fr["point"].shape == (0, 2) and fr["bbox"].shape == (0, 4)
    pm = np.zeros((1, 40, 33), dtype=np.int8)
    pm[0, 30:, :] = 50
    FC.write(g, pm)
    goal = m.next_goal((0.0, 0.0, 0.0), min_unknown=0, min_size=1)
    assert np.array_equal(goal, np.array([(29 + 0.5) / 10.0 - 10.0, (16 + 0.5) / 10.0 - 10.0]))
