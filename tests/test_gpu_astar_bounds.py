"""The A* kernels at their bounds, against the NumPy oracle (tests/astar_ref.py): queries past
the persistent grid's slots, long open lists, truncated paths, the map's edge, non-square maps,
other radii, the trigger walk's ring in global memory, a 2000 x 2000 map, inflation alone on a
new context, a search slot reused after an EDGE stop, and the arguments rejected up front."""
import numpy as np
import pytest

import astar_ref
from conftest import load_golden, pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def slam():
    return pkg()


@pytest.fixture(scope="module")
def course():
    g = load_golden("g12_astar.npz")
    return g["maps"][0, :129, :129], g["inflated"][0, :129, :129].astype(np.int64)


def pairs(imap, n, rng):
    free = np.argwhere(imap == 0)
    return ((free[rng.integers(0, len(free), n)] + 1).astype(np.int32),
            (free[rng.integers(0, len(free), n)] + 1).astype(np.int32))


def agree(o, imap, s, g, cap=None):
    for b in range(len(s)):
        r = astar_ref.plan(imap, s[b], g[b], path_cap=cap)
        assert (o["status"][b], o["expansions"][b], o["path_len"][b]) == (r["status"], r["expansions"], r["length"]), b
        n = r["length"] if cap is None else min(cap, r["length"])
        np.testing.assert_array_equal(o["path"][b, :n], r["path"][:n], err_msg=str(b))


def random_map(rng, H, W, walls=0.02, unknown=0.003, fifty=0.01):
    u = rng.random((H, W))
    m = np.where(u < walls, 100, np.where(u < walls + unknown, -1, np.where(u < walls + unknown + fifty, 50, 0)))
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = 100
    return m.astype(np.int8)


def test_queries_past_the_grid_stride(slam, course):
    m, imap = course
    rng = np.random.default_rng(21)
    s, g = pairs(imap, 40, rng)
    small = slam.astar_host(m, s, g, path_cap=256)
    agree(small, imap, s, g)
    B = (1 << 16) + 40
    rep = B // 40 + 1
    big = slam.astar_host(m, np.tile(s, (rep, 1))[:B], np.tile(g, (rep, 1))[:B], path_cap=256)
    for k in ("status", "path_len", "expansions"):
        np.testing.assert_array_equal(big[k], np.tile(small[k], rep)[:B], err_msg=k)
    written = np.arange(256)[None, :] < np.minimum(big["path_len"], 256)[:, None]     # cells past a path are not written
    np.testing.assert_array_equal(big["path"][written], np.tile(small["path"], (rep, 1, 1))[:B][written])


def test_long_open_lists(slam):
    """A 400 x 400 room with a wall across it: the search floods much of the room, with open
    lists of hundreds of entries."""
    m = np.zeros((400, 400), np.int8)
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = 100
    m[200, 5:395] = 100
    imap = astar_ref.inflate(m, span=400, r=2)
    s = np.array([[300, 200], [390, 10], [250, 380]], np.int32)
    g = np.array([[100, 200], [10, 390], [150, 30]], np.int32)
    o = slam.astar_host(m, s, g, span=400, path_cap=2048)
    agree(o, imap, s, g)
    assert np.all(o["status"] == astar_ref.OK) and np.all(o["expansions"] > 1000)


def test_truncated_path_reports_the_true_length(slam, course):
    m, imap = course
    rng = np.random.default_rng(22)
    s, g = pairs(imap, 64, rng)
    full = slam.astar_host(m, s, g, path_cap=512)
    ok = np.nonzero((full["status"] == astar_ref.OK) & (full["path_len"] > 2))[0][:8]
    assert len(ok) == 8
    for b in ok:
        L = int(full["path_len"][b])
        o = slam.astar_host(m, s[b:b + 1], g[b:b + 1], path_cap=L - 1)
        assert o["status"][0] == astar_ref.TRUNCATED and o["path_len"][0] == L
        np.testing.assert_array_equal(o["path"][0], full["path"][b, :L - 1])
        o = slam.astar_host(m, s[b:b + 1], g[b:b + 1], path_cap=L)
        assert o["status"][0] == astar_ref.OK
    o = slam.astar_host(m, s, g, path_cap=0)                 # no path buffer at all
    np.testing.assert_array_equal(o["path_len"], full["path_len"])
    np.testing.assert_array_equal(o["status"], np.where(full["status"] == astar_ref.OK, astar_ref.TRUNCATED,
                                                        full["status"]))


def test_edge_on_a_map_with_a_free_border(slam):
    m = np.zeros((60, 80), np.int8)
    m[20:40, 30:50] = 100
    imap = astar_ref.inflate(m, span=60, r=2)
    s = np.array([[2, 2], [30, 2], [1, 1], [61, 10], [10, 10], [30, 10]], np.int32)
    g = np.array([[58, 78], [30, 78], [5, 5], [5, 5], [0, 5], [30, 12]], np.int32)
    o = slam.astar_host(m, s, g, span=60, path_cap=256)
    agree(o, imap, s, g)
    assert list(o["status"][2:5]) == [astar_ref.EDGE] * 3      # start on the edge, start / goal outside
    assert o["status"][5] == astar_ref.OK


def test_non_square_map(slam):
    rng = np.random.default_rng(23)
    m = random_map(rng, 100, 170)
    for span in (100, 60):
        imap = astar_ref.inflate(m, span=span, r=2)
        s, g = pairs(imap, 200, rng)
        o = slam.astar_host(m, s, g, span=span, path_cap=1024, want_inflated=True)
        np.testing.assert_array_equal(o["inflated"][0], imap)
        agree(o, imap, s, g)
    # the same map in the pmap layout ([x][y])
    o2 = slam.astar_host(np.ascontiguousarray(m.T), s, g, span=60, wire_layout=False, path_cap=1024, want_inflated=True)
    for k in ("status", "path_len", "expansions", "path", "inflated"):
        np.testing.assert_array_equal(o2[k], o[k], err_msg=k)


@pytest.mark.parametrize("r", [0, 1, 3])
def test_other_radii(slam, r):
    rng = np.random.default_rng(30 + r)
    m = random_map(rng, 150, 150, walls=0.03)
    imap = astar_ref.inflate(m, span=150, r=r)
    s, g = pairs(imap, 150, rng)
    o = slam.astar_host(m, s, g, span=150, r=r, path_cap=1024, want_inflated=True)
    np.testing.assert_array_equal(o["inflated"][0], imap)
    agree(o, imap, s, g)


def test_trigger_ring_in_global_memory(slam):
    """r = 220 over 19 words per row: the ring of dilated rows (33 440 bytes) is past the LDS ring."""
    rng = np.random.default_rng(41)
    m = random_map(rng, 1200, 1200, walls=0.0005, unknown=0.0, fifty=0.0)
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = 0
    np.testing.assert_array_equal(slam.inflate_host(m, span=1200, r=220), astar_ref.inflate(m, span=1200, r=220))


def test_2000_square_map(slam):
    rng = np.random.default_rng(40)
    m = random_map(rng, 2000, 2000, walls=0.004, unknown=0.001)
    imap = astar_ref.inflate(m, span=2000, r=2)
    np.testing.assert_array_equal(slam.inflate_host(m, span=2000, r=2), imap)
    s, g = pairs(imap, 6, rng)
    s[:3] = [[1000, 1000], [100, 100], [1900, 50]]
    g[:3] = [[1100, 1150], [400, 300], [1800, 200]]
    o = slam.astar_host(m, s, g, span=2000, path_cap=4096)
    agree(o, imap, s, g)


def test_bad_map_on_the_device_form(slam, course):
    import torch
    m, imap = course
    da = slam.DeviceAStar(129, 129, G=2)
    maps = torch.from_numpy(np.stack([m, m])).to(da.dev)
    s, g = pairs(imap, 4, np.random.default_rng(50))
    ts, tg = torch.from_numpy(s).to(da.dev), torch.from_numpy(g).to(da.dev)
    q = torch.tensor([0, 1, 2, -1], dtype=torch.int32, device=da.dev)
    torch.cuda.synchronize()
    o = da.run(ts, tg, maps=maps, map_of_query=q)
    da.ctx.synchronize()
    st = o["status"].cpu().numpy()
    assert st[2] == astar_ref.BAD_MAP and st[3] == astar_ref.BAD_MAP
    assert st[0] == astar_ref.plan(imap, s[0], g[0])["status"]
    assert st[1] == astar_ref.plan(imap, s[1], g[1])["status"]


def test_rejected_up_front(slam, course):
    m, _ = course
    s = np.array([[10, 10]], np.int32)
    for kw in (dict(span=130), dict(r=-1), dict(span=-1)):
        with pytest.raises(slam.SlamError):
            slam.astar_host(m, s, s, **kw)
    with pytest.raises(slam.SlamError):                      # H > W
        slam.astar_host(np.zeros((140, 129), np.int8), s, s, span=100)
    with pytest.raises(slam.SlamError):                      # map_of_query outside [0, G)
        slam.astar_host(m, s, s, map_of_query=[1])
    with pytest.raises(slam.SlamError):                      # G neither 1 nor B without map_of_query
        slam.astar_host(np.stack([m, m]), np.tile(s, (3, 1)), np.tile(s, (3, 1)))
    with pytest.raises(IndexError):                          # the drop-in: the reference's 129-cell bound
        slam.find_path(np.zeros((100, 100), np.int8), [5, 5], [9, 9]).start_find()


@pytest.mark.parametrize("n,r", [(2000, 2), (1200, 220)])
def test_inflate_alone_on_a_fresh_context(slam, n, r):
    """The inflation-only path reserves its own workspace: on a new context nothing larger was
    reserved before it."""
    rng = np.random.default_rng(60 + r)
    m = random_map(rng, n, n, walls=0.004 if r == 2 else 0.0005, unknown=0.001 if r == 2 else 0.0)
    ctx = slam.Context(0)
    try:
        got = slam.inflate_host(m, span=n, r=r, ctx=ctx)
    finally:
        ctx.close()
    np.testing.assert_array_equal(got, astar_ref.inflate(m, span=n, r=r))


def test_slot_reused_after_an_edge_stop(slam):
    """A 400 x 400 map with a free border takes 268 search slots, so query b and b + 268 share a
    slot.  The first 400 queries stop with EDGE on the border cell (0, 198) they pop; the next 400
    have that cell as their goal, which they reach by opening it."""
    m = np.zeros((400, 400), np.int8)
    m[100:300, 100:300] = 100
    imap = astar_ref.inflate(m, span=400, r=2)
    edge_s, edge_g = [2, 200], [1, 151]                      # pops (0, 198) first: EDGE
    reach_s, reach_g = [2, 200], [1, 199]                    # its goal is (0, 198): OK, 2 cells
    s = np.array([edge_s] * 400 + [reach_s] * 400, np.int32)
    g = np.array([edge_g] * 400 + [reach_g] * 400, np.int32)
    o = slam.astar_host(m, s, g, span=400, path_cap=64)
    assert astar_ref.plan(imap, edge_s, edge_g)["status"] == astar_ref.EDGE
    assert astar_ref.plan(imap, reach_s, reach_g)["status"] == astar_ref.OK
    for b in (0, 399, 400, 667, 668, 799):
        r = astar_ref.plan(imap, s[b], g[b])
        assert (o["status"][b], o["expansions"][b], o["path_len"][b]) == (r["status"], r["expansions"], r["length"]), b
        np.testing.assert_array_equal(o["path"][b, :r["length"]], r["path"])
    np.testing.assert_array_equal(o["status"], [astar_ref.EDGE] * 400 + [astar_ref.OK] * 400)
    np.testing.assert_array_equal(o["expansions"][400:], o["expansions"][400])
