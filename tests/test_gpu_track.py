"""slam_track / slam_track_dev on the GPU (include/slam_track.h).

    (A)  every scan of a run is the public calls, bit for bit: the teacher-forced walk of tests/track_cases.py beside a
         shadow grid - L = 3 trajectories, S = 8, n in {65, 120}, a 200 x 200 map at 0.1 m, K = 5, nx = ny = 2, 3
         iterations, gate (0.15, 0.05), biased odometry; host form and device form
    (B)  the batch and chunk rule: S scans in one call = S calls of one = a 3 + 5 split; a trajectory alone = the same
         one in the batch; the batch reversed; map0 > 0 with the maps below it untouched
    (C)  edges, each at the smallest shape that reaches it
    (E)  it tracks better than odometry, on the device and through ScanTracker: the issue's two cases at the defaults,
         the largest error within (0.10 m, 0.03 rad) and the final position error below a tenth of dead reckoning's.
         Device and restatement run free of each other; their difference is printed, not asserted.

A NaN first pose (C): the first-scan rule integrates only a pose the map can take, so such a trajectory is LOST on every
scan, stays unkeyed, and its map is never touched; the context's sticky status stays clean."""
import numpy as np
import pytest

import track_cases as C
import track_ref as T
from conftest import pkg

pytestmark = pytest.mark.gpu
KEYS = ("state", "poses", "info", "trace")


@pytest.fixture(scope="module")
def slam():
    p = pkg()
    p._abi.default_context()   # fails loudly when there is no gfx950 device
    return p


def same_out(a, b, rows=None):
    return all(C.same(a[k] if rows is None else a[k][rows], b[k]) for k in KEYS)


def check_walk(slam, case, device):
    grid, shadow = C.make_grids(slam, case)
    out = C.run(slam, grid, case, device=device)
    end = C.walk(slam, case, out, shadow)
    assert C.same(out["state"], end), (out["state"], end)
    got, want = C.counters(grid), C.counters(shadow)
    assert C.same(got[0], want[0]) and C.same(got[1], want[1])
    return out, got


# ---------------------------------------------------------------- (A)
@pytest.mark.parametrize("n", (65, 120))
@pytest.mark.parametrize("device", (False, True), ids=("host", "dev"))
def test_every_scan_is_the_public_calls(slam, syn, n, device):
    case = C.replay_case(syn, n)
    out, (pass_, _hit) = check_walk(slam, case, device)
    f = out["info"][..., 3]
    assert np.all(f[:, 0] == T.INTEGRATED) and np.all(f[:, 1:] & T.MATCHED)
    later = (f[:, 1:] & T.INTEGRATED) != 0
    assert later.any() and not later.all(), f                  # the gate lets some scans through and holds some back
    assert (f & T.REFINED).any() and pass_.any()


# ---------------------------------------------------------------- (B)
@pytest.fixture(scope="module")
def batch(slam, syn):
    case = C.replay_case(syn, 65)
    grid = C.make_grid(slam, case)
    out = C.run(slam, grid, case, device=True)
    return case, out, C.counters(grid)


def test_chunks_of_scans(slam, batch):
    case, whole, cnt = batch
    S = case["ranges"].shape[1]
    for cuts in ([(k, k + 1) for k in range(S)], [(0, 3), (3, S)]):
        grid, state, parts = C.make_grid(slam, case), case["state"], []
        for a, b in cuts:
            parts.append(C.run(slam, grid, case, device=True, scans=slice(a, b), state=state))
            state = parts[-1]["state"]
        joined = dict(state=state, **{k: np.concatenate([p[k] for p in parts], axis=1) for k in KEYS[1:]})
        assert same_out(whole, joined), cuts
        got = C.counters(grid)
        assert C.same(got[0], cnt[0]) and C.same(got[1], cnt[1])


def test_alone_and_reversed(slam, syn, batch):
    case, whole, cnt = batch
    L = case["ranges"].shape[0]
    alone = dict(case, G=1)
    for l in range(L):
        grid = C.make_grid(slam, alone)
        out = C.run(slam, grid, alone, device=(l == 1), rows=[l])
        assert same_out(whole, out, rows=[l]), l
        got = C.counters(grid)
        assert C.same(got[0][0], cnt[0][l]) and C.same(got[1][0], cnt[1][l])
    grid = C.make_grid(slam, case)
    rev = C.run(slam, grid, case, device=True, rows=list(range(L))[::-1])
    assert same_out(whole, rev, rows=list(range(L))[::-1])
    got = C.counters(grid)
    assert C.same(got[0], cnt[0][::-1]) and C.same(got[1], cnt[1][::-1])


def test_map0(slam, syn, batch):
    case, whole, cnt = batch
    L = case["ranges"].shape[0]
    moved = dict(case, map0=2, G=L + 3)
    grid = C.make_grid(slam, moved)
    assert same_out(whole, C.run(slam, grid, moved, device=True))
    got = C.counters(grid)
    assert C.same(got[0][2:2 + L], cnt[0]) and C.same(got[1][2:2 + L], cnt[1])
    for g in (0, 1, L + 2):
        assert not got[0][g].any() and not got[1][g].any()


# ---------------------------------------------------------------- (C)
def small(syn, **kw):
    kw = dict(dict(n=24, L=1, S=4, K=3, nx=1, ny=1, iters=2), **kw)
    return C.replay_case(syn, kw.pop("n"), **kw)


def test_no_motion(slam, syn):
    case = small(syn, with_motion=False, L=2)
    out, _ = check_walk(slam, case, device=True)
    assert C.same(out["trace"][:, 1:, 0:3], out["poses"][:, :-1])      # pred is the pose before, bit for bit


def test_tracking_in_a_given_map(slam, syn):
    """keyed = 1 on a prebuilt map with both gates +inf: the counters are unchanged and every pose is match + refine of the
    public calls (the walk)."""
    case = small(syn, S=5, gate=(np.inf, np.inf))
    case["pre"] = (case["ranges"][:, 0].copy(), case["state"][:, :3].copy())
    case["state"][:, 3:6], case["state"][:, 6] = case["state"][:, :3], 1.0
    grid = C.make_grid(slam, case)
    before = C.counters(grid)
    out, after = check_walk(slam, case, device=True)
    assert before[0].any() and C.same(before[0], after[0]) and C.same(before[1], after[1])
    assert np.all(out["info"][..., 3] & T.MATCHED) and not (out["info"][..., 3] & T.INTEGRATED).any()


def test_an_empty_scan_mid_stream(slam, syn):
    case = small(syn, S=5, gate=(0.0, 0.0))
    case["ranges"][0, 2] = np.inf
    out, _ = check_walk(slam, case, device=True)
    f = out["info"][0, :, 3]
    assert f[2] == 0 and out["info"][0, 2, 2] == 0 and C.same(out["poses"][0, 2], out["trace"][0, 2, 0:3])
    assert np.all(f[[1, 3, 4]] & T.MATCHED) and np.all(f[[0, 1, 3, 4]] & T.INTEGRATED)


def test_min_used_above_the_scan(slam, syn):
    case = small(syn)
    case["par"]["min_used"] = case["ranges"].shape[2] + 1
    out, _ = check_walk(slam, case, device=False)
    assert out["info"][0, :, 3].tolist() == [T.INTEGRATED, 0, 0, 0] and np.all(out["info"][0, 1:, 2] > 0)
    assert C.same(out["poses"], out["trace"][:, :, 0:3])


@pytest.mark.parametrize("bad", (np.nan, np.inf, 3.0e6))
def test_a_start_the_map_cannot_take(slam, syn, bad):
    good = small(syn, L=3, G=3)
    case = dict(good, state=good["state"].copy())
    case["state"][1, 0] = bad
    want = C.run(slam, C.make_grid(slam, good), good, device=True)
    grid, shadow = C.make_grids(slam, case)
    out = C.run(slam, grid, case, device=True)
    slam._abi.default_context().check_status()                       # nothing raised the sticky status
    C.walk(slam, case, out, shadow)
    assert np.all(out["info"][1, :, 3] == T.LOST) and np.all(out["info"][1, :, :3] == (-1, -1, 0)) and out["state"][1, 6] == 0.0
    pass_, hit = C.counters(grid)
    assert not pass_[1].any() and not hit[1].any()
    assert same_out(want, {k: out[k][[0, 2]] for k in KEYS}, rows=[0, 2])


def test_the_pred_chain(slam, syn):
    """K = 1, nx = ny = 0, iters = 0: the only candidate is the prediction, so the poses are the pred chain and the map is
    slam_grid_update_particles at them."""
    case = small(syn, K=1, nx=0, ny=0, iters=0, gate=(0.0, 0.0), L=2)
    out, (pass_, hit) = check_walk(slam, case, device=True)
    assert C.same(out["poses"], out["trace"][:, :, 0:3]) and np.all(out["info"][:, 1:, 0] == 0)
    chain = slam.DeviceGrid(case["G"], *case["shape"], *case["geom"])
    for s in range(case["ranges"].shape[1]):
        slam.grid_update_particles_host(chain, case["ranges"][:, s], case["ct"], case["st"], out["poses"][:, s][:, None, :])
    want = C.counters(chain)
    assert C.same(pass_, want[0]) and C.same(hit, want[1])


@pytest.mark.parametrize("n", (1, 64))
def test_beam_counts(slam, syn, n):
    check_walk(slam, small(syn, n=n, L=2), device=True)


def test_every_bound(slam, syn):
    case = small(syn, L=2, G=2)
    grid = C.make_grid(slam, case)
    assert C.run(slam, grid, case)["info"][..., 3].any()
    before = C.counters(grid)
    ok = dict(case["par"])
    for name, value in (("nx", -1), ("ny", -1), ("step", 0.0), ("step", np.inf), ("iters", -1), ("iters", 65), ("damping", -1.0),
                        ("damping", np.inf), ("step_cells", 0.0), ("step_rad", 0.0), ("max_range", 0.0), ("cap", 0), ("cap", 32768),
                        ("min_used", 0), ("gate_dist", -1.0), ("gate_dist", np.nan), ("gate_turn", -0.1), ("gate_turn", np.nan),
                        ("nx", 1 << 24)):
        with pytest.raises(slam.SlamError):
            C.run(slam, grid, dict(case, par=dict(ok, **{name: value})))
    for over in (dict(map0=-1), dict(map0=1), dict(rot_off=np.zeros(0), rot_off_cs=np.zeros((0, 2)))):
        with pytest.raises(slam.SlamError):
            C.run(slam, grid, dict(case, **over))
    big = dict(case, ct=np.ones(4097), st=np.zeros(4097), ranges=np.ones((2, 1, 4097), dtype=np.float32), motion=None)
    with pytest.raises(slam.SlamError):
        C.run(slam, grid, big)
    lib, abi = slam._abi.lib(), slam._abi
    r, st = case["ranges"], case["state"].copy()
    off, cs = case["rot_off"], case["rot_off_cs"]
    poses, info = np.empty((2, 4, 3)), np.empty((2, 4, 4), dtype=np.int32)
    p = abi.ptr

    def call(L=2, S=4, ranges=r, state=st, poses_out=poses, info_out=info, rot=off, n=r.shape[2]):
        return lib.slam_track(grid._ctx.handle, grid._h, p(ranges), None, L, S, p(case["ct"]), p(case["st"]), n, p(rot), p(cs), 3, 1, 1,
                              0.1, 2, 0.01, 0.5, 0.02, 30.0, 64, 1, 0.15, 0.05, 0, p(state), p(poses_out), p(info_out), None)
    for kw in (dict(L=0), dict(S=0), dict(L=3), dict(ranges=None), dict(state=None), dict(poses_out=None), dict(info_out=None), dict(rot=None), dict(n=0)):
        assert call(**kw) == abi.ERR_INVALID, kw
    assert lib.slam_track(grid._ctx.handle, grid._h, p(r), None, 1 << 15, 1 << 15, p(case["ct"]), p(case["st"]), 24, p(off), p(cs), 3, 1, 1, 0.1, 2,
                          0.01, 0.5, 0.02, 30.0, 64, 1, 0.15, 0.05, 0, p(st), p(poses), p(info), None) == abi.ERR_INVALID      # L * S * n >= 2^31
    grid._ctx.check_status()
    after = C.counters(grid)
    assert C.same(before[0], after[0]) and C.same(before[1], after[1])
    assert call() == abi.SLAM_OK                                      # the same call with nothing wrong runs


# ---------------------------------------------------------------- (E)
@pytest.mark.parametrize("name", ("dense", "sparse"))
def test_it_tracks_better_than_odometry(slam, syn, name):
    import torch
    c = T.case_inputs(syn, name)
    S, n = c["scans"].shape
    dp, _ = T.errors(c["dead"], c["true"])
    ref, _ = T.run_case(syn, name)
    rp, rh = T.errors(ref, c["true"])
    print("%s restatement: max %.4f m %.4f rad, final %.4f m (dead reckoning %.3f m)" % (name, rp.max(), rh.max(), rp[-1], dp[-1]))
    assert rp.max() <= T.BOUND[0] and rh.max() <= T.BOUND[1] and rp[-1] < 0.1 * dp[-1]
    # the device, batched
    grid = slam.DeviceGrid.metric(1, T.MAP["xw"], T.MAP["yw"], 1.0 / T.MAP["scale"])
    tr = slam.DeviceTracker(grid, 1, c["cos_t"], c["sin_t"])
    tr.set_poses(c["true"][0][None])
    tr.run(torch.from_numpy(c["scans"][None]).to(tr.dev), torch.from_numpy(c["motion"][None]).to(tr.dev))
    dev = tr.results()["poses"][0]
    grid._ctx.check_status()
    # one scan per call through the drop-in class
    m = slam.Mapping.metric(T.MAP["xw"], T.MAP["yw"], 1.0 / T.MAP["scale"])
    st = slam.ScanTracker(m, pose=c["true"][0])
    for s in range(S):
        st.update(c["scans"][s], c["angle_min"], c["angle_max"], u=c["motion"][s])
    one = np.array(st.trajectory)
    for label, poses in (("DeviceTracker", dev), ("ScanTracker", one)):
        ep, eh = T.errors(poses, c["true"])
        print("%s %s: max %.4f m %.4f rad, final %.4f m; largest difference from the restatement %.2e"
              % (name, label, ep.max(), eh.max(), ep[-1], float(np.max(np.abs(poses - ref)))))
        assert ep.max() <= T.BOUND[0] and eh.max() <= T.BOUND[1], (label, ep.max(), eh.max())
        assert ep[-1] < 0.1 * dp[-1], (label, ep[-1], dp[-1])
    assert C.same(dev, one)                                            # the chunk rule, at full size
    assert (m.pmap == 100).any()
