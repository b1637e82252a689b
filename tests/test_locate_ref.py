"""Global scan localisation on the CPU: the restatement's search (tests/locate_ref.py) against the definition by brute
force - best, cost and used - over the ring, room and ragged maps, every pyramid depth and regions down to one cell; P_h
against its definition; the launch shape at its edges through slam_plan_query; the entry points in the header and the
binding; and the room recovered from nothing, with its pruning.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import locate_ref as L
import match_ref as M
import raycast_ref as R
from conftest import pkg

LEVELS = (0, 1, 3, 5, 8)


def same(got, want):
    assert tuple(got[0]) == tuple(want[0]) and got[1:3] == want[1:3], (got[:3], want)


def regions_of(xw, yw):
    """The whole map; 1 x 1 in a corner, on an edge and inside; one row, one column; odd sizes that leave partial nodes
    on both far edges; rectangles on every edge."""
    return [(0, 0, xw, yw), (0, 0, 1, 1), (xw - 1, yw - 1, 1, 1), (xw - 1, 3, 1, 1), (5, 7, 1, 1), (4, 0, 1, yw), (0, 9, xw, 1),
            (3, 2, 13, 11), (0, 5, 9, 7), (xw - 9, 4, 9, 5), (6, 0, 7, 10), (2, yw - 11, 19, 11)]


@pytest.mark.parametrize("shape", L.RAGGED)
def test_search_is_brute_force_on_ragged_maps(shape):
    xw, yw = shape
    pm, _ = L.ragged_pmap(xw, yw)
    cap = 50
    fld = M.field(pm, cap)
    ct, st, ranges = L.ragged_scan(23, seed=xw)
    ranges[4], ranges[9], ranges[15] = np.inf, np.nan, 30.0
    _, rot = L.rotations(5)
    pyr = L.pyramid(fld, 8, cap)
    assert (1 << 8) > max(xw, yw)
    for reg in regions_of(xw, yw):
        want = L.brute(fld, 1.0, ranges, ct, st, rot, reg, 20.0, cap)
        assert 0 < want[2] < 20
        for H in LEVELS:
            got = L.search(pyr[:H + 1], 1.0, ranges, ct, st, rot, reg, H, 20.0, cap)
            same(got, want)
            nI, nJ = -(-reg[2] // (1 << H)), -(-reg[3] // (1 << H))
            assert got[3][H] == 5 * nI * nJ and got[3][H + 1] >= got[1] and np.all(got[3][:H] >= 1)
            if H == 0:
                assert got[3][1] == got[1]


def test_search_is_brute_force_on_the_ring_and_in_the_room(syn):
    fld = M.field(R.ring_pmap(), 64)
    ct, st, ranges = L.ragged_scan(40, seed=1, reach=20.0)
    _, rot = L.rotations(7)
    pyr = L.pyramid(fld, 8, 64)
    for reg in ((0, 0, 64, 64), (20, 17, 25, 30), (63, 0, 1, 64)):
        want = L.brute(fld, 1.0, ranges, ct, st, rot, reg, 18.0, 64)
        for H in LEVELS:
            same(L.search(pyr[:H + 1], 1.0, ranges, ct, st, rot, reg, H, 18.0, 64), want)
    # a scan made of the ring itself: beams to the ring of radius 8 from the centre; the centre is found at cost 0
    cells = R.ring(8)
    ct, st = R.tables_to(cells)
    ones = np.ones(len(cells), dtype=np.float32)
    rot1 = np.array([[1.0, 0.0]])
    want = L.brute(fld, 1.0, ones, ct, st, rot1, L.whole(fld), 30.0, 64)
    assert want == ((0, 32, 32), 0, len(cells))
    for H in LEVELS:
        got = L.search(pyr[:H + 1], 1.0, ones, ct, st, rot1, L.whole(fld), H, 30.0, 64)
        same(got, want)
    assert got[3][0] < 64 * 64 // 8                                  # the pyramid prunes: far fewer leaves than cells
    # the room: a rectangle around the true pose and three rotations, by brute force
    case = L.room_case(syn)
    k = int(case["loc_ref"][0][0])
    reg = (case["loc_ref"][0][1] - 20, case["loc_ref"][0][2] - 17, 45, 38)
    rot3 = case["loc_rot"][k - 1:k + 2]
    want = L.brute(case["field"], 20.0, case["scan"], case["cos_t"], case["sin_t"], rot3, reg, **L.ROOM_ARGS)
    assert want[0] == (1,) + tuple(case["loc_ref"][0][1:]) and want[1] == case["loc_ref"][1]
    pyr = L.pyramid(case["field"], 3, 64)
    for H in (0, 1, 3):
        same(L.search(pyr[:H + 1], 20.0, case["scan"], case["cos_t"], case["sin_t"], rot3, reg, H, **L.ROOM_ARGS), want)


def test_an_empty_map_is_the_full_frontier_and_a_dead_scan_is_not_searched():
    xw, yw, cap, K = 70, 33, 9, 3
    fld = M.field(np.full((xw, yw), 50, dtype=np.int8), cap)
    assert np.all(fld == cap)
    ct, st, ranges = L.ragged_scan(17, seed=3)
    _, rot = L.rotations(K)
    for reg in ((0, 0, xw, yw), (7, 5, 21, 13)):
        for H in LEVELS:
            best, cost, used, stats = L.search(L.pyramid(fld, H, cap), 1.0, ranges, ct, st, rot, reg, H, 30.0, cap)
            assert (best, cost, used) == ((0, reg[0], reg[1]), 17 * cap, 17)             # everything ties: flat 0
            assert stats.tolist() == [K * -(-reg[2] // (1 << h)) * -(-reg[3] // (1 << h)) for h in range(H + 1)] + [17 * cap]
            same((best, cost, used), L.brute(fld, 1.0, ranges, ct, st, rot, reg, 30.0, cap))
    pm, _ = L.ragged_pmap(xw, yw)
    fld = M.field(pm, cap)
    for dead in (np.full(17, np.inf, np.float32), np.full(17, np.nan, np.float32), np.full(17, 30.0, np.float32)):
        for H in (0, 3):
            out = L.search(L.pyramid(fld, H, cap), 1.0, dead, ct, st, rot, (7, 5, 21, 13), H, 30.0, cap)
            assert out[:3] == ((0, 7, 5), 0, 0) and not out[3].any()
            assert L.brute(fld, 1.0, dead, ct, st, rot, (7, 5, 21, 13), 30.0, cap) == out[:3]
    # off beams (3 000 km) and NaN rotations add cap to every candidate: the rest of the scan still decides
    far = ranges.copy()
    far[2] = far[11] = 3.0e6
    nanrot = np.array([[np.nan, 0.0], [np.cos(0.3), np.sin(0.3)], [1.0, np.nan]])
    for r, rc in ((far, rot), (ranges, nanrot), (far, nanrot)):
        want = L.brute(fld, 1.0, r, ct, st, rc, (0, 0, xw, yw), 4.0e6, cap)
        assert want[2] == 17
        for H in (0, 3, 8):
            same(L.search(L.pyramid(fld, H, cap), 1.0, r, ct, st, rc, (0, 0, xw, yw), H, 4.0e6, cap), want)
    assert L.offsets(far, ct, st, 1.0, 0.0, 1.0, 4.0e6)[2:] == (2, 17)
    assert L.brute(fld, 1.0, ranges, ct, st, nanrot, (0, 0, xw, yw), 30.0, cap)[0][0] == 1


def test_pyramid_levels_are_their_definition():
    pm, _ = L.ragged_pmap(33, 35)
    cap = 40
    fld = M.field(pm, cap).astype(np.int64)
    E = lambda x, y: int(fld[x, y]) if 0 <= x < 33 and 0 <= y < 35 else cap
    rng = np.random.default_rng(2)
    for h in (0, 1, 2, 3, 6):
        P, s = L.level(fld, h, cap), 1 << h
        assert P.shape == (33 + s - 1, 35 + s - 1)
        pts = [(-(s - 1), -(s - 1)), (32, 34), (-(s - 1), 34), (32, -(s - 1)), (0, 0)]
        pts += [(int(x), int(y)) for x, y in zip(rng.integers(-(s - 1), 33, 40), rng.integers(-(s - 1), 35, 40))]
        for x, y in pts:
            want = min(E(x + a, y + b) for a in range(s) for b in range(s))
            assert P[x + s - 1, y + s - 1] == want == L.level_at(P, h, x, y, cap), (h, x, y)
        assert L.level_at(P, h, -s, 0, cap) == cap and L.level_at(P, h, 0, 35, cap) == cap and L.level_at(P, h, 33, 0, cap) == cap
    # a level is the min of four cells of the level below at offsets 0 and 2^(h-1): what the device builds
    for h in (1, 2, 3, 6):
        lo, s = L.level(fld, h - 1, cap), 1 << (h - 1)
        xs, ys = np.meshgrid(np.arange(-(2 * s - 1), 33), np.arange(-(2 * s - 1), 35), indexing="ij")
        four = np.minimum(np.minimum(L.level_at(lo, h - 1, xs, ys, cap), L.level_at(lo, h - 1, xs + s, ys, cap)),
                          np.minimum(L.level_at(lo, h - 1, xs, ys + s, cap), L.level_at(lo, h - 1, xs + s, ys + s, cap)))
        assert np.array_equal(four, L.level(fld, h, cap))


def query(name, a=0, b=0, c=0, guard=-1):
    abi = pkg("_abi")
    out = C.c_int64()
    abi.check(abi.lib().slam_plan_query(name.encode(), int(a), int(b), int(c), int(guard), C.byref(out)))
    return int(out.value)


def test_launch_shape_at_its_edges():
    threads, rounds, node = query("kLocateThreads"), query("kLocateTileRounds"), query("kLocateNodeBytes")
    assert threads == 256 and threads % query("kWave") == 0 and node == 8 and query("kLocateMaxLevels") == 8
    assert query("kLocateMaxBeams") == 4096
    for ni, nj in ((1, 1), (33, 35), (70, 33), (400, 400), (255, 257), (46340, 46340)):
        for h in range(9):
            assert query("locate_level_nodes", ni, nj, h) == -(-ni // (1 << h)) * -(-nj // (1 << h))
        for H in range(9):
            assert query("locate_pair_bytes", ni, nj, H) == node * sum(-(-ni // (1 << h)) * -(-nj // (1 << h)) for h in range(1, H + 1))
    assert query("locate_pair_bytes", 400, 400, 0) == 0
    assert [query("locate_table_bytes", n) for n in (1, 120, 4096)] == [16, 968, 32776]      # a pair's packed offsets and two counts
    # lanes over nodes: whole waves up to the workgroup; a tile is `rounds` trips of it
    for nodes, want in ((1, 64), (64, 64), (65, 128), (169, 192), (255, 256), (256, 256), (257, 256), (160000, 256)):
        assert query("locate_dense_threads", nodes) == want
    assert query("locate_tile", 400, 400, 5) == 192 * rounds and query("locate_tiles", 400, 400, 5) == 1      # 13 x 13 nodes
    assert query("locate_tile", 400, 400, 0) == threads * rounds and query("locate_tiles", 400, 400, 0) == -(-160000 // (threads * rounds))
    assert query("locate_tiles", 64, 64, 0) == 1 and query("locate_tiles", 64, 65, 0) == 2
    # the offsets of one rotation in LDS, and the guard of the debug build behind them
    for n in (1, 120, 4096):
        assert query("locate_dense_lds", n, guard=0) == 8 * n and query("locate_dense_lds", n, guard=512) == 8 * n + 512
    assert query("locate_dense_lds", 4096, guard=512) <= query("kLdsDefault")
    # chunks: as many pairs as fit the budget; none (0) when one pair does not; H = 0 keeps no list
    pb = query("locate_pair_bytes", 70, 33, 3)
    assert query("locate_chunk_pairs", 64 * 1024, pb, 192) == 192
    assert query("locate_chunk_pairs", 20, pb, 192) == 20 * 1024 // pb == 3
    assert query("locate_chunk_pairs", 6, pb, 192) == 0 and query("locate_chunk_pairs", 7, pb, 192) == 1
    assert query("locate_chunk_pairs", 1, 0, 192) == 192


def test_entry_points_are_declared_bound_and_exported():
    abi, slam = pkg("_abi"), pkg()
    declared = abi.header_symbols()
    for n in ("slam_grid_locate", "slam_grid_locate_dev"):
        assert n in declared and n in abi._SIGS and hasattr(abi.lib(), n), n
    assert abi._SIGS["slam_grid_locate"] == abi._SIGS["slam_grid_locate_dev"] and len(abi._SIGS["slam_grid_locate"][0]) == 19
    for n in ("grid_locate_host", "locate_rotations", "locate_pose"):
        assert n in slam.__all__ and hasattr(slam, n), n
    assert hasattr(slam.DeviceGrid, "locate") and hasattr(slam.Mapping, "locate_scan") and hasattr(slam.MCL, "init_global")
    assert abi.lib().slam_abi_version() == 1 and len(abi.K_NAMES) == 8
    th, rot = slam.locate_rotations(256)
    assert np.array_equal(th, L.rotations(256)[0]) and np.array_equal(rot, L.rotations(256)[1]) and th[0] == -np.pi
    best = np.array([[3, 10, 0], [-1, -1, -1]])
    poses = slam.locate_pose(best, 20.0, 10.0, 10.0, rot)
    assert np.array_equal(poses[0], L.pose_of(best[0], 20.0, 10.0, 10.0, rot)) and np.all(np.isnan(poses[1]))
    assert poses[0, 0] == 10.5 / 20.0 - 10.0 and poses[0, 1] == 0.5 / 20.0 - 10.0


def test_room_recovered_from_nothing(syn):
    """Last scan, K = 256, H = 5, the whole map: within one cell on each axis and one rotation step of the true pose, and
    fewer than 0.01 of the K * ni * nj candidates evaluated."""
    case = L.room_case(syn)
    best, cost, used, stats = case["loc_ref"]
    pose = L.pose_of(best, 20.0, 10.0, 10.0, case["loc_rot"])
    err = pose - case["true"]
    err[2] = (err[2] + np.pi) % (2 * np.pi) - np.pi
    print("room: best", best, "pose", pose, "true", case["true"], "err", err, "cost", cost, "used", used, "stats", stats.tolist())
    assert abs(err[0]) <= 0.05 and abs(err[1]) <= 0.05 and abs(err[2]) <= 2 * np.pi / 256
    assert stats[5] == 256 * 13 * 13 and stats[6] >= cost and used == 120
    share = int(stats[:6].sum()) / (256 * 400 * 400)
    print("room: evaluated", int(stats[:6].sum()), "share", share)
    assert share < 0.01
