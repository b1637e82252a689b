"""Scan-to-map observation kernels (k_map_obstacles, k_virtual_scan, k_ranges64_to_points and the
slam_map_observation chain) at the bounds of their launch shapes, against the NumPy oracle
(oracle.oracle_np.map_obstacles / laser_estimation) and the C oracle's ICP.

What the cases are about:
  k_map_obstacles   non-square maps in both layouts, the grid stride (2 048 workgroups of 256 =
                    524 288 cells per pass), cap below / at / above the count, all / no obstacles;
  k_virtual_scan    n up to the 64 KB of LDS that 8 192 bins need, the switch between the
                    one-workgroup path (plain store) and the sliced path (k_fill_u64 + global
                    atomicMin) at slices = min(ceil(2048 / B), ceil(K / 1024)), negative
                    increments, negative q (truncation, not floor; % n with its + n), mostly empty
                    scans, obstacles around distance 100, NaN / inf obstacles;
  slam_map_observation  thousands of beams, and a virtual scan that is mostly the 100.0 ring.

Bars (those of test_gpu_localization.py): obstacle lists bit-equal as sets, the same bins of a
virtual scan hold 100.0, its distances within 1e-12, ICP iteration counts equal and transforms
within 1e-9.

Bin edges.  The bin is int(q), q = (atan2(..) - angle_min - theta) / inc, and the device's atan2
may differ from libm's in the last bits: a few ulp of an angle up to pi, divided by
inc >= 2 pi / 8192, is below 1e-11 in q.  A projection is AMBIGUOUS if
|q - round(q)| <= 1e-9 * max(1, |q|) and round(q) != 0 (zero is no edge under truncation).  Every
randomised case is built without any (offending obstacles - for the fixed golden obstacle set the
offending poses - are drawn again from the case's seed) and asserts so; the screen uses
numpy.arctan2 at twice the tolerance, which covers its own last-bit difference from libm.  The
lattice case is ambiguous by construction and uses a band check instead.

The oracle's laser_estimation is a Python loop, so a case with many rows compares a seeded sample
of at least 32 rows: the first, the last, the rows on both sides of every pass boundary of
k_fill_u64 (1 024 workgroups of 256 = 262 144 values per pass), and random ones."""
import math
import types

import numpy as np
import pytest

from conftest import load_golden, pkg
from oracle import c_oracle as co
from oracle import oracle_np as on

pytestmark = pytest.mark.gpu

AMIN, AMAX = -3.14159, 3.14159
STRIDE = 2048 * 256              # cells per pass of k_map_obstacles
FILL_STRIDE = 1024 * 256         # values per pass of k_fill_u64
AMBIG = 1e-9
CELL_VALUES = np.array([-128, -1, 0, 20, 21, 50, 100, 127], dtype=np.int8)
NONSQUARE = [(3, 7), (7, 3), (1, 513), (513, 1), (200, 320), (640, 48)]
RES, OX0, OY0 = 0.037, -1.25, 2.5
SENTINEL = -777.25


@pytest.fixture(scope="module")
def slam():
    p = pkg()
    p._abi.default_context()
    return p


@pytest.fixture(scope="module")
def g5():
    return load_golden("g5_map_observation.npz")


def grid_msg(data, w, h, res=RES, ox=OX0, oy=OY0):
    return types.SimpleNamespace(data=data, info=types.SimpleNamespace(
        height=h, width=w, resolution=res, origin=types.SimpleNamespace(position=types.SimpleNamespace(x=ox, y=oy))))


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def sorted_set(ob):
    ob = np.asarray(ob, dtype=np.float64).reshape(2, -1)
    return ob[:, np.lexsort((ob[1], ob[0]))]


# ---- k_map_obstacles -------------------------------------------------------------------------

def want_obstacles(data, width, height, wire):
    """The oracle for the raw entry point.  on.map_obstacles reads `data` as rows of its `height`
    argument with tx = the column; wire order data[y*width + x] is that with rows of `width`.
    The [x][y] layout is its transpose: x = c // height, y = c % height."""
    if wire:
        return on.map_obstacles(data, height, width, RES, OX0, OY0)
    c = np.nonzero((data > 20) | (data < -0.5))[0]
    return np.vstack(((c // height) * RES + OX0, (c % height) * RES + OY0)) * 1.0


def obstacles_host(slam, data, width, height, wire, cap, size=None):
    """slam_map_obstacles into sentinel-filled buffers of `size` >= cap -> (count, ox, oy)."""
    import ctypes as C
    A = slam._abi
    size = cap if size is None else size
    ox, oy = np.full(max(size, 1), SENTINEL), np.full(max(size, 1), SENTINEL)
    k = C.c_int(-5)
    A.check(A.lib().slam_map_obstacles(A.default_context().handle, A.ptr(data), width, height, wire, RES, OX0, OY0,
                                       A.ptr(ox), A.ptr(oy), cap, C.byref(k)))
    return k.value, ox[:size], oy[:size]


def obstacles_dev(slam, data, width, height, wire, cap, size=None):
    import torch
    A = slam._abi
    ctx = A.default_context()
    dev = torch.device("cuda", ctx.device)
    size = cap if size is None else size
    m = torch.from_numpy(np.ascontiguousarray(data)).to(dev)
    ox = torch.full((max(size, 1),), SENTINEL, dtype=torch.float64, device=dev)
    oy = torch.full((max(size, 1),), SENTINEL, dtype=torch.float64, device=dev)
    k = torch.full((1,), -5, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    A.check(A.lib().slam_map_obstacles_dev(ctx.handle, m.data_ptr(), width, height, wire, RES, OX0, OY0, ox.data_ptr(),
                                           oy.data_ptr(), cap, k.data_ptr()))
    ctx.synchronize()
    return int(k.cpu()[0]), ox.cpu().numpy()[:size], oy.cpu().numpy()[:size]


def assert_obstacle_set(slam, data, width, height):
    for wire in (1, 0):
        want = want_obstacles(data, width, height, wire)
        for form in (obstacles_host, obstacles_dev):
            k, ox, oy = form(slam, data, width, height, wire, data.size)
            assert k == want.shape[1], (width, height, wire, form.__name__)
            assert bits_equal(sorted_set(np.vstack((ox[:k], oy[:k]))), sorted_set(want)), (width, height, wire, form.__name__)
            assert np.all(ox[k:] == SENTINEL) and np.all(oy[k:] == SENTINEL)


@pytest.mark.parametrize("w,h", NONSQUARE)
def test_map_obstacles_non_square(slam, w, h):
    """1. Both layouts of a non-square map through the raw entry points, and Localization.updateMap,
    whose reading of a non-square message is the reference's reshape((-1, height)).transpose()."""
    rng = np.random.default_rng(1000 + 7 * w + h)
    data = rng.choice(CELL_VALUES, size=w * h)
    assert_obstacle_set(slam, data, w, h)
    # the index rule itself, so that the oracle call above cannot hide a swap of its arguments
    c = np.nonzero((data > 20) | (data < 0))[0]
    assert bits_equal(sorted_set(want_obstacles(data, w, h, 1)), sorted_set(np.vstack(((c % w) * RES + OX0, (c // w) * RES + OY0))))
    loc = slam.Localization()
    loc.updateMap(grid_msg(data, w, h))
    assert bits_equal(loc.obstacle, on.map_obstacles(data, w, h, RES, OX0, OY0))           # values AND np.nonzero order


@pytest.mark.parametrize("w,h,size", [(5, 7, 21), (7, 5, 60), (9, 4, 8), (3, 320, 1600)])
def test_update_map_size_not_width_times_height(slam, w, h, size):
    """1. data.size a multiple of height but not width * height: the reference reshapes to
    (-1, height) without looking at width."""
    assert size % h == 0 and size != w * h
    data = np.random.default_rng(size).choice(CELL_VALUES, size=size)
    loc = slam.Localization()
    loc.updateMap(grid_msg(data, w, h))
    want = on.map_obstacles(data, w, h, RES, OX0, OY0)
    assert want.shape[1] > 0 and bits_equal(loc.obstacle, want)


@pytest.mark.parametrize("w,h", [(1100, 900), (1024, 1024)])
def test_map_obstacles_past_one_stride(slam, w, h):
    """2. More cells than one pass of the grid holds: obstacles in the first and last 256 cells and
    on both sides of cell 524 288, and a sparse scatter everywhere."""
    cells = w * h
    assert cells > STRIDE
    rng = np.random.default_rng(w)
    data = np.zeros(cells, dtype=np.int8)
    for lo, hi in ((0, 256), (cells - 256, cells), (STRIDE - 300, STRIDE), (STRIDE, STRIDE + 300)):
        at = lo + rng.choice(hi - lo, size=40, replace=False)
        data[at] = rng.choice(np.array([-128, -1, 21, 50, 100, 127], dtype=np.int8), size=40)
    data[[0, 255, STRIDE - 1, STRIDE, cells - 256, cells - 1]] = 100
    at = rng.choice(cells, size=3000, replace=False)
    data[at] = rng.choice(CELL_VALUES, size=3000)
    assert np.count_nonzero(data[STRIDE:]) > 1000
    assert_obstacle_set(slam, data, w, h)
    loc = slam.Localization()
    loc.updateMap(grid_msg(data, w, h))
    assert bits_equal(loc.obstacle, on.map_obstacles(data, w, h, RES, OX0, OY0))


def test_map_obstacles_cap(slam):
    """3. cap below, at and above the count K: the count reports K, the first min(cap, K) entries are
    distinct members of the oracle's set, nothing past cap is written."""
    w, h = 40, 25
    data = np.random.default_rng(31).choice(CELL_VALUES, size=w * h)
    for wire in (1, 0):
        want = want_obstacles(data, w, h, wire)
        K = want.shape[1]
        members = set(zip(want[0].tolist(), want[1].tolist()))
        assert 100 < K < w * h and len(members) == K
        for cap in (0, 1, K - 1, K, K + 1):
            for form in (obstacles_host, obstacles_dev):
                k, ox, oy = form(slam, data, w, h, wire, cap, size=K + 8)
                m = min(cap, K)
                got = set(zip(ox[:m].tolist(), oy[:m].tolist()))
                assert k == K, (wire, cap, form.__name__)
                assert len(got) == m and got <= members, (wire, cap, form.__name__)
                assert np.all(ox[m:] == SENTINEL) and np.all(oy[m:] == SENTINEL), (wire, cap, form.__name__)


def test_map_obstacles_all_and_none(slam):
    """4. Every cell an obstacle (K = the cell count), and no cell."""
    w = h = 512
    rng = np.random.default_rng(4)
    full = rng.choice(np.array([-128, -1, 21, 50, 100, 127], dtype=np.int8), size=w * h)
    assert_obstacle_set(slam, full, w, h)
    assert want_obstacles(full, w, h, 1).shape[1] == w * h
    none = rng.choice(np.array([0, 20, 7], dtype=np.int8), size=w * h)
    assert_obstacle_set(slam, none, w, h)
    assert want_obstacles(none, w, h, 0).shape[1] == 0
    loc = slam.Localization()
    loc.updateMap(grid_msg(none, w, h))
    assert loc.obstacle.shape == (2, 0)


# ---- k_virtual_scan --------------------------------------------------------------------------

def slices_of(K, B):
    """launch_virtual_scan's slice rule."""
    return max(1, min((2048 + B - 1) // B, (K + 1023) // 1024))


def scan_host(slam, obs, poses, amin, inc, n):
    A = slam._abi
    obs = np.ascontiguousarray(obs, dtype=np.float64).reshape(2, -1)
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    K = obs.shape[1]
    out = np.full((poses.shape[0], n), SENTINEL)
    x, y = (A.ptr(obs[0]), A.ptr(obs[1])) if K else (None, None)
    A.check(A.lib().slam_virtual_scan(A.default_context().handle, x, y, K, A.ptr(poses), poses.shape[0], float(amin),
                                      float(inc), n, A.ptr(out)))
    return out


def scan_dev(slam, obs, poses, amin, inc, n):
    """slam_virtual_scan_dev into an output buffer pre-filled with garbage (NaN, negative and tiny
    values: everything an unsigned minimum on the bits would keep or lose wrongly)."""
    import torch
    A = slam._abi
    ctx = A.default_context()
    dev = torch.device("cuda", ctx.device)
    obs = np.ascontiguousarray(obs, dtype=np.float64).reshape(2, -1)
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    K, B = obs.shape[1], poses.shape[0]
    junk = np.resize(np.array([np.nan, -1.0, 0.0, 5e-324, 1e300, -np.inf, 0.5, 100.0]), B * n)
    out = torch.from_numpy(junk).to(dev)
    d_obs = torch.from_numpy(obs if K else np.zeros((2, 1))).to(dev)
    d_poses = torch.from_numpy(poses).to(dev)
    torch.cuda.synchronize()
    A.check(A.lib().slam_virtual_scan_dev(ctx.handle, d_obs[0].data_ptr(), d_obs[1].data_ptr(), K, d_poses.data_ptr(), B,
                                          float(amin), float(inc), n, out.data_ptr()))
    ctx.synchronize()
    return out.cpu().numpy().reshape(B, n)


def q_rows(obs, poses, amin, inc, chunk=1 << 22):
    """q of every projection as the oracle forms it (numpy.arctan2 in place of math.atan2), in row
    blocks: yields (first row, q [rows, K])."""
    obs = np.asarray(obs, dtype=np.float64).reshape(2, -1)
    step = max(1, chunk // max(1, obs.shape[1]))
    for r0 in range(0, poses.shape[0], step):
        p = poses[r0:r0 + step]
        yield r0, (np.arctan2(obs[1][None, :] - p[:, 1:2], obs[0][None, :] - p[:, 0:1]) - amin - p[:, 2:3]) / inc


def ambiguous(q, tol=2 * AMBIG):
    r = np.rint(q)
    return (np.abs(q - r) <= tol * np.maximum(1.0, np.abs(q))) & (r != 0)


def count_ambiguous(obs, poses, amin, inc):
    """(ambiguous projections, projections with q < -1, finite projections) over all rows."""
    amb = neg = tot = 0
    with np.errstate(all="ignore"):
        for _, q in q_rows(obs, poses, amin, inc):
            amb += int(np.count_nonzero(ambiguous(q)))
            neg += int(np.count_nonzero(q < -1))
            tot += int(np.count_nonzero(np.isfinite(q)))
    return amb, neg, tot


def settle(rng, obs, poses, amin, inc, draw_obs=None, draw_pose=None, frozen=0):
    """Draw the offending obstacles (columns from `frozen` on) or, with draw_pose, the offending
    poses again until no projection is ambiguous.  Returns copies."""
    obs, poses = np.array(obs, dtype=np.float64).reshape(2, -1), np.array(poses, dtype=np.float64).reshape(-1, 3)
    todo = np.arange(poses.shape[0] if draw_pose is not None else obs.shape[1])      # what was drawn last
    for _ in range(50):
        bad = np.zeros(len(todo), bool)
        with np.errstate(all="ignore"):
            if draw_pose is not None:
                for r0, q in q_rows(obs, poses[todo], amin, inc):
                    bad[r0:r0 + q.shape[0]] = ambiguous(q).any(1)
            else:
                for _, q in q_rows(obs[:, todo], poses, amin, inc):
                    bad |= ambiguous(q).any(0)
        todo = todo[bad & (todo >= frozen)] if draw_pose is None else todo[bad]
        if not len(todo):
            break
        if draw_pose is not None:
            poses[todo] = draw_pose(rng, len(todo))
        else:
            obs[:, todo] = draw_obs(rng, len(todo))
    return obs, poses


def draw_square(rng, k):
    return rng.uniform(-10.0, 10.0, (2, k))


def draw_pose(rng, k):
    return np.column_stack((rng.uniform(-4.0, 4.0, (k, 2)), rng.uniform(-math.pi, math.pi, k)))


def sample_rows(rng, B, n, at_least=32):
    """First, last, both sides of every pass boundary of k_fill_u64, then random rows."""
    if B <= at_least + 8:
        return list(range(B))
    rows = {0, B - 1}
    for e in range(FILL_STRIDE, B * n, FILL_STRIDE):
        rows |= {max(0, e // n - 1), e // n, min(B - 1, e // n + 1)}
    rest = np.setdiff1d(np.arange(B), np.fromiter(rows, int))
    rows |= set(rng.choice(rest, size=max(0, at_least - len(rows)), replace=False).tolist())
    assert len(rows) >= at_least
    return sorted(rows)


def assert_rows(got, obs, poses, rows, amin, inc, n, tag):
    """Sampled rows against the loop oracle: the same bins hold 100.0, distances within 1e-12.
    Returns the oracle's rows."""
    wants = []
    with np.errstate(all="ignore"):
        for r in rows:
            want = on.laser_estimation(obs, poses[r], amin, inc, n)
            assert np.array_equal(got[r] == 100.0, want == 100.0), (tag, r, np.nonzero((got[r] == 100.0) != (want == 100.0))[0][:8])
            assert np.max(np.abs(got[r] - want)) < 1e-12, (tag, r)
            wants.append(want)
    return wants


def check_scan(slam, rng, obs, poses, amin, inc, n, tag, dev=True):
    """No ambiguous projection; host form against the oracle on sampled rows; the device form,
    into a garbage-filled buffer, bit-equal to the host form on every row."""
    amb, neg, tot = count_ambiguous(obs, poses, amin, inc)
    assert amb == 0, (tag, amb)
    got = scan_host(slam, obs, poses, amin, inc, n)
    assert got.shape == (poses.shape[0], n)
    rows = sample_rows(rng, poses.shape[0], n)
    wants = assert_rows(got, obs, poses, rows, amin, inc, n, tag)
    if dev:
        assert bits_equal(scan_dev(slam, obs, poses, amin, inc, n), got), tag
    return got, rows, wants, neg / max(1, tot)


@pytest.mark.parametrize("n,K", [(1, 5000), (2, 5000), (8191, 5000), (8192, 5000), (8192, 1000)])
def test_virtual_scan_bin_counts(slam, n, K):
    """5. n = 1, 2 and the largest two; 8 192 bins are exactly 64 KB of LDS, in the sliced launch
    (K = 5 000: 5 slices) and in the one-workgroup launch (K = 1 000)."""
    rng = np.random.default_rng(50 + n + K)
    inc = 2 * math.pi / n
    obs, poses = settle(rng, draw_square(rng, K), draw_pose(rng, 3), AMIN, inc, draw_obs=draw_square)
    assert slices_of(K, 3) == (5 if K == 5000 else 1)
    got, _, wants, _ = check_scan(slam, rng, obs, poses, AMIN, inc, n, (n, K))
    if n >= 8191:
        assert 0.2 < np.mean(np.array(wants) == 100.0) < 0.95      # both kinds of bin are there


SLICE_CASES = [  # K, B, slices
    (0, 1, 1), (0, 3, 1), (1, 1, 1), (1, 2, 1), (1023, 1, 1), (1023, 2, 1), (1024, 1, 1), (1024, 2048, 1),
    (1025, 1, 2), (1025, 2, 2), (1025, 2047, 2), (1025, 2048, 1), (2047, 1, 2), (2047, 683, 2),
    (2049, 1, 3), (2049, 2, 3), (2049, 683, 3), (2049, 1024, 2), (2049, 2047, 2), (2049, 2049, 1), (2049, 4096, 1),
    (32183, 1, 32), (32183, 2, 32), (32183, 683, 3), (32183, 2048, 1),
]


def test_slice_cases_cover_the_rule():
    """The list above holds what it is meant to: one slice by small K and by large B, two slices, a K
    the slice count does not divide, the largest slice count of these K, and every K and B."""
    for K, B, s in SLICE_CASES:
        assert slices_of(K, B) == s, (K, B)
    assert {K for K, _, _ in SLICE_CASES} == {0, 1, 1023, 1024, 1025, 2047, 2049, 32183}
    assert {B for _, B, _ in SLICE_CASES} == {1, 2, 3, 683, 1024, 2047, 2048, 2049, 4096}
    assert any(s == 1 and K <= 1024 for K, B, s in SLICE_CASES)
    assert any(s == 1 and K > 1024 and B >= 2048 for K, B, s in SLICE_CASES)
    assert any(s == 2 for _, _, s in SLICE_CASES)
    assert any(s > 1 and K % s for K, _, s in SLICE_CASES)
    assert max(s for _, _, s in SLICE_CASES) == (32183 + 1023) // 1024


@pytest.mark.parametrize("K,B,slices", SLICE_CASES)
def test_virtual_scan_slice_rule(slam, g5, K, B, slices):
    """6. Both sides of every switch between the one-workgroup and the sliced path."""
    n = 360
    inc = (AMAX - AMIN) / (n - 1)
    rng = np.random.default_rng(6000 + 13 * K + B)
    poses = draw_pose(rng, B)
    if K == 32183:
        obs, poses = settle(rng, g5["obstacle"], poses, AMIN, inc, draw_pose=draw_pose)
    else:
        obs, poses = settle(rng, draw_square(rng, K), poses, AMIN, inc, draw_obs=draw_square)
    assert obs.shape[1] == K and slices_of(K, B) == slices
    got, rows, wants, _ = check_scan(slam, rng, obs, poses, AMIN, inc, n, (K, B))
    if K == 0:
        assert np.all(got == 100.0)
    elif B > 1:
        assert len({w.tobytes() for w in wants}) == len(rows)      # rows that differ only in the pose differ
        assert len({r.tobytes() for r in got}) == B


@pytest.mark.parametrize("amin", [-3.14159, 0.0, 2.5])
@pytest.mark.parametrize("inc", [2 * math.pi / 360, -(2 * math.pi / 360), (AMAX - AMIN) / 119, -0.05])
def test_virtual_scan_angles(slam, amin, inc):
    """7. Increments of both signs, headings that make q negative for half of the obstacles
    (theta = -angle_min) and for all of them (+-40 rad, several wraps): int() truncates toward zero
    and the wrap needs its + n."""
    n = int(round(2 * math.pi / abs(inc)))
    rng = np.random.default_rng(int(700 + 10 * amin + 1000 * inc))
    poses = draw_pose(rng, 8)
    poses[:, 2] = [-amin, 40.0, -40.0, 7.0, -7.0, 1.0, -amin + 3.0, -amin - 3.0]
    for K in (700, 3000):                                           # one workgroup, three slices
        obs, p = settle(rng, draw_square(rng, K), poses, amin, inc, draw_obs=draw_square)
        assert np.array_equal(p, poses)
        _, _, _, neg = check_scan(slam, rng, obs, p, amin, inc, n, (amin, inc, K))
        assert neg >= 0.25, neg                                     # the truncation rule stays exercised
    _, neg, tot = count_ambiguous(obs, poses[:1], amin, inc)
    assert 0.25 < neg / tot < 0.75                                  # theta = -angle_min: about half


def wedge_set(rng, pose, K=1200):
    """Obstacles in a 30-degree wedge seen from `pose`, then five fixed ones: one exactly on the pose,
    and two each just under and just over distance 100, in directions outside the wedge."""
    def draw(rng, k):
        a, r = rng.uniform(0.2, 0.2 + math.pi / 6, k), rng.uniform(1.0, 8.0, k)
        return np.vstack((pose[0] + r * np.cos(a), pose[1] + r * np.sin(a)))
    fixed = [(pose[0], pose[1])]
    for a, r in ((2.0, 100.0 - 1e-9), (-2.0, 100.0 + 1e-9), (-1.0, 99.5), (3.0, 100.5)):
        fixed.append((pose[0] + r * math.cos(a), pose[1] + r * math.sin(a)))
    return np.hstack((np.array(fixed).T, draw(rng, K))), draw, len(fixed)


WEDGE_POSES = np.array([[0.5, -0.25, 0.0], [0.5, -0.25, 1.3], [0.5, -0.25, -2.9], [0.5, -0.25, 17.0], [-1.0, 2.0, 0.4]])


@pytest.mark.parametrize("n", [360, 1080])
def test_virtual_scan_wedge_and_far(slam, n):
    """8. Most bins stay 100.0; an obstacle just under distance 100 is kept, one just over loses to
    the 100.0 already there; an obstacle on the pose gives distance 0."""
    rng = np.random.default_rng(80 + n)
    inc = (AMAX - AMIN) / (n - 1)
    obs, draw, frozen = wedge_set(rng, WEDGE_POSES[0])
    obs, poses = settle(rng, obs, WEDGE_POSES, AMIN, inc, draw_obs=draw, frozen=frozen)
    got, _, wants, _ = check_scan(slam, rng, obs, poses, AMIN, inc, n, n)
    assert math.hypot(poses[0][0] - obs[0][1], poses[0][1] - obs[1][1]) < 100.0 < math.hypot(poses[0][0] - obs[0][2], poses[0][1] - obs[1][2])
    for r in range(4):                                              # the rows that stand on the fixed obstacles' pose
        w = wants[r]
        assert np.mean(w == 100.0) > 0.85 and w.min() == 0.0 and got[r].min() == 0.0
        far = np.sort(w[(w > 99.0) & (w < 100.0)])
        assert len(far) == 2 and far[0] == pytest.approx(99.5, abs=1e-9) and 100.0 - 2e-9 < far[1] < 100.0
        assert got[r].max() == 100.0


def test_virtual_scan_non_finite_obstacles(slam):
    """9. A NaN obstacle is skipped (the reference raises on it), an infinite one reaches a bin and
    loses to 100.0; a NaN pose gives an empty scan."""
    n = 360
    inc = (AMAX - AMIN) / (n - 1)
    rng = np.random.default_rng(9)
    K = 1500
    obs, poses = settle(rng, draw_square(rng, K), draw_pose(rng, 3), AMIN, inc, draw_obs=draw_square)
    at = rng.choice(K, size=40, replace=False)
    with np.errstate(all="ignore"):
        obs[0, at[0:8]] = np.nan
        obs[1, at[8:16]] = np.nan
        obs[:, at[16:20]] = np.nan
        obs[0, at[20:24]], obs[1, at[24:28]] = np.inf, np.inf
        obs[0, at[28:32]], obs[1, at[32:36]] = -np.inf, -np.inf
        obs[:, at[36:38]] = np.inf
        obs[0, at[38:40]], obs[1, at[38:40]] = -np.inf, np.inf
        obs[0, at[0]], obs[1, at[0]] = np.nan, np.inf                 # hypot(nan, inf) is inf: skipped all the same
        keep = ~np.isnan(obs).any(0)
        assert keep.sum() == K - 20 and np.isinf(obs[:, keep]).any(0).sum() == 20
        assert slices_of(K, 4) == 2 and count_ambiguous(obs[:, keep], poses, AMIN, inc)[0] == 0
        all_poses = np.vstack((poses, [[np.nan, np.nan, np.nan]]))
        for form in (scan_host, scan_dev):
            got = form(slam, obs, all_poses, AMIN, inc, n)
            assert_rows(got, obs[:, keep], all_poses, [0, 1, 2], AMIN, inc, n, form.__name__)
            assert np.all(got[3] == 100.0)
            one = form(slam, obs[:, :700], all_poses[3:], AMIN, inc, n)                     # one-workgroup path
            assert np.all(one == 100.0)


@pytest.mark.parametrize("n", [8, 360])
def test_virtual_scan_lattice_band(slam, n, capsys):
    """Integer-lattice obstacles around a pose on a lattice point, angle_min = -pi, inc = 2 pi / n,
    theta = 0: on the axes and diagonals q is an integer in real arithmetic and the reference's bin
    a rounding accident.  Each bin's value must lie between the minimum over every obstacle that
    could fall into it (an ambiguous one counts for both neighbouring bins) and the minimum over
    the bin's unambiguous obstacles.

    Recorded on the MI355X (an observation, not an assertion): n = 8: 49 ambiguous projections, 49
    placed as libm places them; n = 360: 49 ambiguous, 49 placed as libm places them."""
    R = 6
    amin, inc = -math.pi, 2 * math.pi / n
    pose = np.array([3.0, -2.0, 0.0])
    ij = np.array([(i, j) for i in range(-R, R + 1) for j in range(-R, R + 1)], dtype=np.float64).T
    obs = pose[:2, None] + ij
    lo, hi = np.full(n, 100.0), np.full(n, 100.0)
    amb = []
    for k in range(obs.shape[1]):
        d = math.hypot(pose[0] - obs[0][k], pose[1] - obs[1][k])
        q = (math.atan2(obs[1][k] - pose[1], obs[0][k] - pose[0]) - amin - pose[2]) / inc
        r = round(q)
        if abs(q - r) <= AMBIG * max(1.0, abs(q)) and r != 0:
            amb.append((k, int(q) % n, {(r - 1) % n, r % n}))
            for b in amb[-1][2]:
                lo[b] = min(lo[b], d)
        else:
            lo[int(q) % n] = min(lo[int(q) % n], d)
            hi[int(q) % n] = min(hi[int(q) % n], d)
    assert len(amb) >= 8 * R                                         # the eight rays, at least
    for form in (scan_host, scan_dev):
        got = form(slam, obs, pose[None], amin, inc, n)[0]
        assert np.all(got >= lo - 1e-12) and np.all(got <= hi + 1e-12), (n, form.__name__, got, lo, hi)
    same = 0
    for k, libm_bin, cand in amb:                                    # each ambiguous obstacle alone: where did it go?
        one = scan_host(slam, obs[:, k:k + 1], pose[None], amin, inc, n)[0]
        at = np.nonzero(one != 100.0)[0]
        assert len(at) == 1 and int(at[0]) in cand, (n, k, at, cand)
        same += int(at[0]) == libm_bin
    with capsys.disabled():
        print("\nlattice n=%d: %d ambiguous projections of %d, %d placed as libm places them" % (n, len(amb), obs.shape[1], same))


# ---- slam_map_observation ----------------------------------------------------------------------

def room_obstacles(step=0.02):
    """The wall cells of the 10 m x 8 m room of synthetic.World(5.0, 4.0), `step` apart."""
    xs, ys = np.arange(-5.0, 5.0 + step / 2, step), np.arange(-4.0, 4.0 + step / 2, step)
    return np.hstack((np.vstack((xs, np.full_like(xs, -4.0))), np.vstack((xs, np.full_like(xs, 4.0))),
                      np.vstack((np.full_like(ys, -5.0), ys)), np.vstack((np.full_like(ys, 5.0), ys))))


def check_observation(slam, syn, rng, obs, n, B, centre):
    """slam_map_observation against the oracle's virtual scan -> laserToNumpy -> the C oracle's ICP."""
    inc = (AMAX - AMIN) / (n - 1)
    true_pose = np.array([0.7, -0.4, 0.3])
    ranges = syn.scans_from_poses(syn.World(5.0, 4.0, (), 0.0), true_pose[None], n, 5)[0]
    msg = slam.LaserScan(ranges=tuple(float(v) for v in ranges), angle_min=AMIN, angle_max=AMAX, angle_increment=inc)

    def draw_near(rng, k):
        return centre + rng.normal(0, [0.1, 0.1, 0.03], size=(k, 3))
    obs, poses = settle(rng, obs, draw_near(rng, B), AMIN, inc, draw_pose=draw_near)
    assert count_ambiguous(obs, poses, AMIN, inc)[0] == 0
    loc = slam.Localization()
    loc.obstacle = obs
    loc.src_pc = loc.laserToNumpy(msg)
    src = on.laser_to_numpy(np.asarray(msg.ranges), AMIN, AMAX)
    assert bits_equal(loc.src_pc, src)
    T, it = loc.map_observation_batch(msg, poses)
    vr = [on.laser_estimation(obs, p, AMIN, inc, n) for p in poses]
    tar = np.stack([on.laser_to_numpy(v, AMIN, AMAX)[:2] for v in vr])
    wT, wit, _ = co.icp_batch(tar, np.broadcast_to(src[:2], (B, 2, n)).copy(), 30, 0.001)
    assert np.array_equal(it, wit), (n, B, it, wit)
    assert np.max(np.abs(T - wT)) < 1e-9, (n, B, np.max(np.abs(T - wT)))
    return np.array(vr)


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("n", [1080, 4545, 8192])
def test_map_observation_thousands_of_beams(slam, syn, n, B):
    """10. Virtual scan -> points -> ICP at thousands of beams: the room's walls as obstacles and the
    real scan of that room."""
    rng = np.random.default_rng(100 + n + B)
    vr = check_observation(slam, syn, rng, room_obstacles(), n, B, np.array([0.7, -0.4, 0.3]))
    assert np.any(vr < 100.0)


@pytest.mark.parametrize("B", [1, 5])
def test_map_observation_mostly_empty_scan(slam, syn, B):
    """11. The wedge set of case 8: most target points are the radius-100 ring."""
    n = 1080
    rng = np.random.default_rng(110 + B)
    obs, _, _ = wedge_set(rng, WEDGE_POSES[0])
    vr = check_observation(slam, syn, rng, obs, n, B, WEDGE_POSES[0])
    assert np.mean(vr == 100.0) > 0.85
