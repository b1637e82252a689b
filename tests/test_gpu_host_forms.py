"""Every host-pointer entry point against its _dev form on the MI355X: the same seeded inputs go
through the host form (NumPy arrays) and the device form (torch tensors), and every output must
be bit-equal (maps: counters and pmap).  Two sizes per pair: one whose staged inputs fit the
coalesced page-locked copy (at most 64 KB) and one past it (above 128 KB: one copy per piece)."""
import numpy as np
import pytest

import dwa_ref
from conftest import pkg

pytestmark = pytest.mark.gpu

AMIN, AMAX = -3.14159, 3.14159


class Out:
    """An output buffer of both forms (zero-filled, so untouched elements compare too)."""
    def __init__(self, shape, dtype=np.float64):
        self.shape, self.dtype = shape, np.dtype(dtype)


class Ws(Out):
    """A device-only argument of the _dev form (workspace; shape None: a null pointer)."""


class Grid:
    """A map object: each form gets its own, compared afterwards."""
    def __init__(self, G, xw):
        self.G, self.xw = G, xw


def rot(rng, B, spread=0.1):
    a = rng.uniform(-spread, spread, B)
    t = rng.uniform(-spread, spread, (B, 2))
    return a, t


def cloud_pair(rng, B, n, dtype=np.float64):
    """B target / source point sets [B][2][n], the source a small rigid motion of the target plus noise."""
    ang = np.linspace(-3.0, 3.0, n)
    r = rng.uniform(1.0, 6.0, (B, n))
    tar = np.stack([r * np.cos(ang), r * np.sin(ang)], 1)
    a, t = rot(rng, B)
    c, s = np.cos(a)[:, None], np.sin(a)[:, None]
    src = np.stack([c * tar[:, 0] - s * tar[:, 1] + t[:, :1], s * tar[:, 0] + c * tar[:, 1] + t[:, 1:]], 1)
    src += rng.normal(0, 0.01, src.shape)
    return np.ascontiguousarray(tar, dtype), np.ascontiguousarray(src, dtype)


def trig(n):
    return pkg()._abi.trig_tables(AMIN, AMAX, n)


def priors(rng, P):
    a, t = rot(rng, P, 0.05)
    return np.ascontiguousarray(np.stack([np.cos(a), -np.sin(a), t[:, 0], np.sin(a), np.cos(a), t[:, 1]], 1))


def scans(rng, S, n):
    r = rng.uniform(0.5, 8.0, (S, n)).astype(np.float32)
    r[rng.random((S, n)) < 0.02] = np.inf
    return r


def case_scan_to_points(rng, big):
    A = pkg()._abi
    B, n = (128, 360) if big else (2, 360)
    ct, st = trig(n)
    return "slam_scan_to_points", [scans(rng, B, n), ct, st, B, n, 1, A.F32 if big else A.F64,
                                   Out((B, 2, n), np.float32 if big else np.float64)]


def case_nn(rng, big):
    A = pkg()._abi
    B, n = (8, 1200) if big else (2, 300)
    tar, src = cloud_pair(rng, B, n)
    return "slam_nn", [src, tar, B, n, n, A.F64, Out(B * n), Out(B * n, np.int32)]


def case_kabsch2d(rng, big):
    B, n = (16, 800) if big else (4, 100)
    tar, src = cloud_pair(rng, B, n)
    return "slam_kabsch2d", [src, tar, B, n, Out((B, 9))]


def case_icp_batch(rng, big):
    A = pkg()._abi
    B, n = (16, 360) if big else (2, 360)
    tar, src = cloud_pair(rng, B, n)
    return "slam_icp_batch", [tar, src, B, n, n, A.F64, 0, 0, priors(rng, B), 30, 1e-3, Out((B, 9)), Out(B, np.int32), Out(B)]


def case_pose_compose(rng, big):
    L, n = (4, 1000) if big else (2, 50)
    a, t = rot(rng, L * n)
    T = np.zeros((L * n, 9))
    T[:, 0], T[:, 1], T[:, 2] = np.cos(a), -np.sin(a), t[:, 0]
    T[:, 3], T[:, 4], T[:, 5] = np.sin(a), np.cos(a), t[:, 1]
    T[:, 8] = 1.0
    return "slam_pose_compose", [T, rng.normal(0, 1, (L, 3)), L, n, Out((L * n, 3))]


def case_grid_update(rng, big):
    B, n = (32, 360) if big else (2, 360)
    cx, cy = rng.uniform(-1, 1, B), rng.uniform(-1, 1, B)
    ang = np.linspace(AMIN, AMAX, n)
    r = rng.uniform(0.5, 7.0, (B, n))
    ox, oy = cx[:, None] + r * np.cos(ang), cy[:, None] + r * np.sin(ang)
    return "slam_grid_update", [Grid(2, 200), ox, oy, cx, cy, B, n, rng.integers(0, 2, B).astype(np.int32)]


def case_grid_update_scans(rng, big):
    S, n = (100, 360) if big else (4, 360)
    ct, st = trig(n)
    poses = np.column_stack([rng.uniform(-1, 1, (S, 2)), rng.uniform(-3, 3, S)])
    return "slam_grid_update_scans", [Grid(1, 200), scans(rng, S, n), ct, st, poses, poses[:, :2] + 0.05, S, n]


def case_replay(rng, big):
    A = pkg()._abi
    L, n_scan, n = (2, 60, 360) if big else (1, 6, 360)
    rep = pkg().synthetic.make_replay(n_scan, n, seed=int(rng.integers(1 << 30)))
    ranges = np.repeat(rep.ranges[None].astype(np.float32), L, 0)
    ct, st = A.trig_tables(rep.angle_min, rep.angle_max, n)
    pairs = L * (n_scan - 1)
    return "slam_replay", [ranges, ct, st, L, n_scan, n, A.F64, 30, 1e-3, rng.normal(0, 0.1, (L, 3)), Grid(L, 200),
                           np.arange(L, dtype=np.int32)[::-1].copy(), Ws(None), Out((pairs, 3)), Out((pairs, 9)),
                           Out(pairs, np.int32)]


def case_particles(rng, big):
    A = pkg()._abi
    P, n = (3000, 360) if big else (8, 360)
    rep = pkg().synthetic.make_replay(2, n, seed=int(rng.integers(1 << 30)))
    ct, st = A.trig_tables(rep.angle_min, rep.angle_max, n)
    return "slam_particles", [rep.ranges.astype(np.float32), ct, st, n, A.F64, priors(rng, P), rng.normal(0, 0.2, (P, 3)),
                              P, 30, 1e-3, Grid(P, 48 if big else 200), Ws(None), Out((P, 3)), Out((P, 9)), Out(P, np.int32)]


def case_map_obstacles(rng, big):
    W = H = 400 if big else 100
    m = np.zeros(W * H, np.int8)
    m[rng.integers(0, W * H, W * H // 20)] = 100
    m[rng.integers(0, W * H, W * H // 50)] = -1
    cap = W * H // 10
    return "slam_map_obstacles", [m, W, H, 1, 0.05, -5.0, -5.0, Out(cap), Out(cap), cap, Out(1, np.int32)], sort_obstacles


def sort_obstacles(outs):
    """The obstacle list comes in the order of the device's appends: sort it as updateMap does."""
    ox, oy, k = outs[0], outs[1], int(outs[2][0])
    order = np.lexsort((oy[:k], ox[:k]))
    ox[:k], oy[:k] = ox[:k][order], oy[:k][order]


def obstacle_set(rng, K):
    a = rng.uniform(-np.pi, np.pi, K)
    r = rng.uniform(1.0, 6.0, K)
    return np.cos(a) * r, np.sin(a) * r


def case_virtual_scan(rng, big):
    K, B, n = (10000, 8, 360) if big else (500, 4, 360)
    ox, oy = obstacle_set(rng, K)
    poses = rng.normal(0, [0.3, 0.3, 0.5], (B, 3))
    return "slam_virtual_scan", [ox, oy, K, poses, B, AMIN, (AMAX - AMIN) / (n - 1), n, Out((B, n))]


def case_scan_to_points_f64(rng, big):
    B, n = (64, 360) if big else (2, 360)
    ct, st = trig(n)
    return "slam_scan_to_points_f64", [rng.uniform(0.5, 8.0, (B, n)), ct, st, B, n, Out((B, 2, n))]


def case_map_observation(rng, big):
    K, B, n = (10000, 8, 360) if big else (500, 4, 360)
    ox, oy = obstacle_set(rng, K)
    poses = rng.normal(0, [0.1, 0.1, 0.05], (B, 3))
    ct, st = trig(n)
    src = np.stack([ct * 3.0, st * 3.0])
    return "slam_map_observation", [ox, oy, K, poses, src, B, n, 1, ct, st, AMIN, (AMAX - AMIN) / (n - 1), 30, 1e-3,
                                    Ws((B, n)), Ws((B, 2, n)), Out((B, 9)), Out(B, np.int32)]


def dwa_valid_costs(outs):
    """Only the first nv * nw entries of a costs row are the window's: zero the rest (never written)."""
    counts, costs = outs[3], outs[4]
    for b in range(costs.shape[0]):
        costs[b, counts[b, 0] * counts[b, 1]:] = 0.0


def dwa_batch(rng, B):
    cfg = pkg().dwa.config_array(dwa_ref.default_config())
    rows, nvc, nwc = pkg().dwa.shape(dwa_ref.default_config())
    states = np.column_stack([rng.uniform(-1, 1, (B, 2)), rng.uniform(-3, 3, B), rng.uniform(0, 0.5, B),
                              rng.uniform(-0.5, 0.5, B)])
    goals = rng.uniform(-5, 5, (B, 2))
    tail = [Out((B, 2)), Out(B), Out(B, np.int32), Out((B, 2), np.int32), Out((B, nvc * nwc)), nvc * nwc, Out((B, rows, 5))]
    return cfg, states, goals, tail


def case_dwa(rng, big):
    B, M = (64, 200) if big else (4, 50)
    cfg, states, goals, tail = dwa_batch(rng, B)
    ob = rng.uniform(-4, 4, (B, 2, M))
    counts = rng.integers(1, M + 1, B).astype(np.int32)
    return "slam_dwa", [states, goals, ob, counts, M, 0, cfg, B] + tail, dwa_valid_costs


def case_dwa_scans(rng, big):
    B, n = (128, 360) if big else (4, 360)
    cfg, states, goals, tail = dwa_batch(rng, B)
    ct, st = trig(n)
    return "slam_dwa_scans", [states, goals, scans(rng, B, n), n, 0, ct, st, 1.0, cfg, B] + tail, dwa_valid_costs


CASES = [case_scan_to_points, case_nn, case_kabsch2d, case_icp_batch, case_pose_compose, case_grid_update,
         case_grid_update_scans, case_replay, case_particles, case_map_obstacles, case_virtual_scan,
         case_scan_to_points_f64, case_map_observation, case_dwa, case_dwa_scans]


@pytest.mark.parametrize("big", [False, True], ids=["pinned", "per_piece"])
@pytest.mark.parametrize("case", CASES, ids=[c.__name__[5:] for c in CASES])
def test_host_form_equals_device_form(case, big):
    torch = pytest.importorskip("torch")
    slam = pkg()
    A, L = slam._abi, slam._abi.lib()
    ctx = A.Context(0)
    dev = torch.device("cuda", ctx.device)
    name, args, *fix = case(np.random.default_rng(7 + 100 * big + CASES.index(case)), big)
    staged = sum(a.nbytes for a in args if isinstance(a, np.ndarray))
    assert staged <= 64 * 1024 if not big else staged > 128 * 1024, (name, staged)
    host, devargs, houts, douts, grids, keep = [], [], [], [], [], []
    for a in args:
        if isinstance(a, np.ndarray):
            a = np.ascontiguousarray(a)
            t = torch.from_numpy(a).to(dev)
            keep.append(t)
            host.append(a)
            devargs.append(t.data_ptr())
        elif isinstance(a, Ws):
            t = None if a.shape is None else torch.zeros(a.shape, dtype=getattr(torch, a.dtype.name), device=dev)
            keep.append(t)
            devargs.append(None if t is None else t.data_ptr())
        elif isinstance(a, Out):
            h = np.zeros(a.shape, a.dtype)
            t = torch.zeros(a.shape, dtype=getattr(torch, a.dtype.name), device=dev)
            houts.append(h)
            douts.append(t)
            host.append(h)
            devargs.append(t.data_ptr())
        elif isinstance(a, Grid):
            pair = [slam.DeviceGrid(a.G, a.xw, a.xw, 10.0, a.xw / 20.0, a.xw / 20.0, context=ctx) for _ in range(2)]
            grids.append((a.G, pair))
            host.append(pair[0]._h)
            devargs.append(pair[1]._h)
        else:
            host.append(a)
            devargs.append(a)
    fn = getattr(L, name)
    host = [v.ctypes.data_as(t) if isinstance(v, np.ndarray) else v for v, t in zip(host, fn.argtypes[1:])]
    A.check(fn(ctx.handle, *host))
    torch.cuda.synchronize()
    A.check(getattr(L, name + "_dev")(ctx.handle, *devargs))
    ctx.synchronize()
    ctx.check_status()
    douts = [t.cpu().numpy() for t in douts]
    for f in fix:
        f(houts)
        f(douts)
    for k, (h, d) in enumerate(zip(houts, douts)):
        assert np.array_equal(h.view(np.uint8), d.view(np.uint8)), (name, k)
    for G, (gh, gd) in grids:
        for m in range(G):
            a, b = gh.read(m, want=("pmap", "pass", "hit")), gd.read(m, want=("pmap", "pass", "hit"))
            for key in ("pmap", "pass", "hit"):
                assert np.array_equal(a[key], b[key]), (name, m, key)
        for g in (gh, gd):
            g.close()
    ctx.close()
