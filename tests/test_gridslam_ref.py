"""Grid FastSLAM without a GPU: the restatement of slam_mcl_settle (tests/gridslam_ref.py) and its two consequences, the
launch shape of slam_grid_copy_maps through slam_plan_query, the eight entry points in the header, the binding and the
package, and the SLAM run on the restatement."""
import ctypes as C

import numpy as np
import pytest

import gridslam_ref as G
import match_ref as M
import mcl_ref as X
from conftest import pkg

PS = (1, 2, 63, 64, 65, 1000, 4096)


def resampled(P, seed, zeros=False):
    """Ancestors of a real systematic resample of seeded weights, and the weights."""
    rng = np.random.default_rng(seed)
    w = rng.integers(1, X.W_MAX + 1, P) if seed % 2 else np.rint(X.W_MAX * rng.random(P) ** 8).astype(np.int64) + 1
    if zeros:
        w[rng.permutation(P)[:P // 2]] = 0
    u0 = rng.uniform()
    return (X.resample_ints(w, u0) if P < 4096 else X.resample_u64(w, u0)), w


def check_settled(anc, s):
    anc, s = np.asarray(anc), np.asarray(s)
    P = len(anc)
    cnt = np.bincount(anc, minlength=P)
    assert np.array_equal(np.bincount(s, minlength=P), cnt)                  # the multiset of ancestors is unchanged
    assert np.array_equal(s[cnt > 0], np.flatnonzero(cnt > 0))               # every survivor keeps its slot ...
    src = np.unique(s)
    assert np.array_equal(s[src], src)                                       # ... so every source is a fixed point: (a)
    free = np.flatnonzero(cnt == 0)
    assert np.array_equal(s[free], np.repeat(np.arange(P), np.maximum(cnt - 1, 0)))   # paired in ascending order
    assert not set(free.tolist()) & set(s.tolist())                          # no destination is a source


@pytest.mark.parametrize("P", PS)
def test_settle_on_real_resamples(P):
    for seed in range(6 if P < 1000 else 2):
        for zeros in (False, True):
            if zeros and P < 2:
                continue
            anc, w = resampled(P, 10 * P + seed, zeros)
            s = G.settle(anc)
            check_settled(anc, s)
            heavy = int(np.argmax(w))                                         # (b): w >= S / P spans a whole threshold step
            assert heavy in anc.tolist() and s[heavy] == heavy
            if zeros:
                assert not set(np.flatnonzero(w == 0).tolist()) & set(anc.tolist())


def test_settle_special_inputs():
    assert G.settle(range(7)) == list(range(7))                               # the identity gives the identity
    assert G.settle([3] * 5) == [3, 3, 3, 3, 3]                               # one ancestor for all: it keeps slot 3
    assert G.settle([0]) == [0]
    anc = [4, 0, 4, 2, 0, 0]                                                  # not monotone: cnt = 3, 0, 1, 0, 2, 0
    assert G.settle(anc) == [0, 0, 2, 0, 4, 4]
    check_settled(anc, G.settle(anc))
    rev = list(range(9))[::-1]
    assert G.settle(rev) == list(range(9))
    b = G.settle_batch([[1, 1, 1], [0, 1, 2]], poses_src=np.arange(18.0).reshape(2, 3, 3), map0=3)
    assert b["settled"].tolist() == [[1, 1, 1], [0, 1, 2]] and b["moved"].tolist() == [2, 0]
    assert b["map_src"].tolist() == [[4, 4, 4], [6, 7, 8]] and np.array_equal(b["poses"][0], np.tile([3.0, 4.0, 5.0], (3, 1)))
    assert G.settle_batch([[-5, 9, 1]], clamp=True)["settled"].tolist() == [[0, 1, 2]]


def test_copy_restatement():
    a = np.arange(5 * 4).reshape(5, 4).copy()
    kinds = G.copy_maps([a], [1, -1, 5, 3], first=0)                          # 0 <- 1, kept, kept, self
    assert kinds.tolist() == [-1, 0, 0, 0] and np.array_equal(a, np.arange(20).reshape(5, 4))   # 1 is a destination (src[1] != 1)
    kinds = G.copy_maps([a], [1, 1, 1, 4], first=0)
    assert kinds.tolist() == [1, 0, 1, 1] and a[:, 0].tolist() == [4, 4, 4, 16, 16]


def query(name, a=0, b=0, c=0):
    abi = pkg("_abi")
    out = C.c_int64()
    abi.check(abi.lib().slam_plan_query(name.encode(), int(a), int(b), int(c), -1, C.byref(out)))
    return int(out.value)


def test_copy_launch_shape_at_its_edges():
    chunk, cap, threads = query("kCopyChunkCells"), query("kCopyMaxGroups"), query("kCopyThreads")
    assert chunk % 4 == 0 and chunk >= 4 * threads and cap == 1 << 20 and threads % 64 == 0
    for xw, yw, count in [(1, 1, 1), (33, 35, 5), (chunk, 1, 3), (chunk + 1, 1, 3), (400, 400, 1024), (3, 5, 70000), (3, 5, cap + 7),
                          (200, 200, cap)]:
        chunks = -(-xw * yw // chunk)
        assert query("copy_chunks", xw, yw, count) == chunks
        assert query("copy_groups", xw, yw, count) == chunks * count
        assert query("copy_grid", xw, yw, count) == min(chunks * count, cap)
        assert query("copy_threads", xw, yw, count) == threads
    assert query("copy_grid", 3, 5, 70000) > 65535                            # one launch, past 65 535 groups
    assert query("copy_groups", 0, 5, 3) == 0 and query("copy_grid", 3, 5, 0) == 0


def test_entry_points_are_declared_bound_and_exported():
    abi, slam = pkg("_abi"), pkg()
    names = ["slam_mcl_weigh_maps", "slam_mcl_settle", "slam_grid_copy_maps", "slam_grid_update_particles"]
    names += [n + "_dev" for n in names]
    declared = abi.header_symbols()
    for n in names:
        assert n in declared and n in abi._SIGS and hasattr(abi.lib(), n), n
    assert abi._SIGS["slam_mcl_weigh_maps"] == abi._SIGS["slam_mcl_weigh"]
    for n in ("GridSLAM", "DeviceGridSLAM", "mcl_settle_host", "grid_copy_maps_host", "grid_update_particles_host"):
        assert n in slam.__all__ and hasattr(slam, n), n
    assert hasattr(slam.DeviceGrid, "copy_maps") and hasattr(slam.DeviceGrid, "update_particles")
    assert abi.lib().slam_abi_version() == 1 and len(abi.K_NAMES) == 8


def test_fast_field_is_the_field():
    rng = np.random.default_rng(1)
    for shape, p in (((40, 37), 0.02), ((9, 70), 0.2), ((30, 30), 0.0)):
        pm = np.where(rng.random(shape) < p, 100, rng.choice([0, 50], shape))
        for cap in (1, 64, 100):
            assert np.array_equal(G.fast_field(pm, cap), M.field(pm, cap))


def test_it_maps_better_than_odometry_on_the_restatement(syn):
    """make_replay(16, 120, seed=4), one filter of 64 particles, 400 x 400 cells of 0.05 m.  Motion input: the true steps
    plus the fixed bias (0.015 m, 0, 0.01 rad) per step; noise sigma (0.02, 0.01, 0.01); sigma 2 cells, cap 64, ess_frac
    0.5.  Measured on the restatement: dead reckoning ends 0.2260 m / 0.150 rad from the truth, the best particle
    0.0362 m / 0.0144 rad; every step from the second on resampled, 44 to 61 slots moved."""
    case = G.slam_case(syn)
    dead = X.pose_error(case["dead"][-1], case["true"][-1])
    print("dead reckoning", dead)
    assert dead[0] >= 4 * 0.05
    best, est, info, moved = G.slam_run(case)
    err = X.pose_error(best, case["true"][-1])
    print("best particle", err, "moved", moved.tolist())
    assert err[0] <= G.SLAM_BOUND[0] and err[1] <= G.SLAM_BOUND[1]
    assert err[0] < 0.5 * dead[0]
    assert np.any((info[:, 2] == 1) & (moved > 0))
