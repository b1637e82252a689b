"""Several contexts ("lanes") on side streams, as bench.py's headline step runs them: each lane a DeviceReplay, a grid, an
int8 pmap and two T buffers of its own, a step = run(reset_grid=True, poses_out=ring[slot], T_out=alternating) followed by
slam_grid_finalize_dev, steps dealt round-robin with no host synchronise between them.  The lanes share the chip and the
library's process-wide tables (the dynamic-LDS allowances, the chip-shape cache of csrc/grid_kernels.hip); bench.py's parity
check looks at the last lane's last step only.  Here EVERY ring slot and every lane's final transforms, iteration counts,
pmap, counters and visit count must equal, bit for bit, that lane's solo result: the same inputs on a context of its own
on the default stream, the same options, a synchronise after every call.  The solo result is held to the C oracle per
trajectory as test_config1_batch_of_8_trajectories_of_1000_scans holds its batch (counters, pmap, visits, iteration counts
exact; poses and transforms within 1e-9).

Options as ReplayWorkload sets them for several lanes: grid_split 0, icp_qpt 3, grid_group 16; "pipeline" 0 and 1.
The ring has a slot per step: the library cannot order a buffer that ANOTHER context reuses, that is the caller's to do.  A
lane that alternates between two pose buffers of its own is the library's to order (the ev_cast wait of slam_replay_dev).
Pose buffers start as NaN, so a slot nobody wrote cannot pass for a result."""
import threading

import numpy as np
import pytest

from conftest import pkg
from oracle import checks

pytestmark = pytest.mark.gpu
FTOL = 1e-9
AMIN, AMAX = -3.14159, 3.14159
L, N_SCANS, N_BEAMS = 2, 40, 360
G, XW, YW, RESO = 2, 200, 200, 0.1
OPTIONS = {"grid_split": 0, "icp_qpt": 3, "grid_group": 16}
STEPS_PER_LANE = 3
MAX_LANES = 4
BIG_SCANS = 80                                  # the replay that makes a lane's workspaces grow mid-run


@pytest.fixture(scope="module")
def slam():
    p = pkg()
    p._abi.default_context()   # fails loudly when there is no gfx950 device
    return p


@pytest.fixture(scope="module")
def streams(slam):
    """Side streams, created once for the module and shared by its tests."""
    import torch
    return [torch.cuda.Stream(device=0) for _ in range(MAX_LANES)]


def lane_ranges(syn, lane, n_scans=N_SCANS):
    """[L, n_scans, 360]: different trajectories, seeds distinct per lane and per trajectory."""
    return np.stack([syn.make_replay(n_scans, N_BEAMS, seed=100 + 10 * lane + l + (50 if n_scans != N_SCANS else 0), stride=5).ranges
                     for l in range(L)])


class Lane:
    """A DeviceReplay of L trajectories into a grid of L maps, a pmap and two T buffers, built under ``stream`` (None: the
    default stream) with the lanes' options."""

    def __init__(self, slam, ranges, pipeline, stream=None):
        import contextlib
        import torch
        self.slam, self.A, self.torch = slam, slam._abi, torch
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            self.dr = slam.DeviceReplay(ranges, AMIN, AMAX, grid_of_traj=np.arange(L))
            self.grid = self.dr.make_grid(G, XW, YW, RESO)
            self.pmap = torch.empty((G, XW, YW), dtype=torch.int8, device=self.dr.dev)
            self.ring_T = torch.empty((2,) + tuple(self.dr.T.shape), dtype=torch.float64, device=self.dr.dev)
            self.own_P = torch.full((2,) + tuple(self.dr.poses.shape), float("nan"), dtype=torch.float64, device=self.dr.dev)
        self.ctx = self.dr.ctx
        for name, value in OPTIONS.items():
            self.ctx.set_option(name, value)
        self.ctx.set_option("pipeline", pipeline)
        self.count = 0
        torch.cuda.synchronize()

    def step(self, poses_out, dr=None, sync=False):
        d = dr or self.dr
        d.run(reset_grid=True, poses_out=poses_out, T_out=self.ring_T[self.count & 1] if dr is None else None)
        self.count += 1
        if sync:
            self.ctx.synchronize()
        self.A.check(self.A.lib().slam_grid_finalize_dev(self.ctx.handle, self.grid._h, self.pmap.data_ptr()))
        if sync:
            self.ctx.synchronize()

    def final(self, dr=None):
        """What the lane holds after its last step (the context synchronised)."""
        poses, T, it = (dr or self.dr).results()
        maps = [self.grid.read(g, want=("pass", "hit")) for g in range(G)]
        return dict(poses=poses, T=T, iters=it, pmap=self.pmap.cpu().numpy(), visits=self.grid.visits(),
                    **{k: np.stack([m[k] for m in maps]) for k in ("pass", "hit")})

    def close(self):
        self.ctx.synchronize()
        self.ctx.set_option("pipeline", 0)
        self.grid.close()
        self.ctx.close()


_SOLO = {}


def solo(slam, syn, lane, pipeline, n_scans=N_SCANS):
    """The lane's step alone: a context of its own on the default stream, a synchronise after every call; checked against the
    oracle per trajectory the first time a lane's inputs are solved."""
    key = (lane, pipeline, n_scans)
    if key not in _SOLO:
        ranges = lane_ranges(syn, lane, n_scans)
        ln = Lane(slam, ranges, pipeline)
        ln.step(None, sync=True)
        ln.ctx.check_status()
        out = ln.final()
        ln.close()
        if (lane, 1 - pipeline, n_scans) in _SOLO:
            same(out, _SOLO[(lane, 1 - pipeline, n_scans)])             # (the option changes no result: held to the oracle once)
        else:
            visits = 0
            for l in range(L):
                og = checks.metric_grid(XW, YW, RESO)
                op, oT, oit, ovis = checks.replay_reference(ranges[l], AMIN, AMAX, og)
                assert np.array_equal(out["iters"][l], oit), (lane, l)
                assert np.max(np.abs(out["poses"][l] - op)) < FTOL and np.max(np.abs(out["T"][l] - oT)) < FTOL, (lane, l)
                assert np.array_equal(out["pass"][l], og.pass_cnt) and np.array_equal(out["hit"][l], og.hit_cnt), (lane, l)
                assert np.array_equal(out["pmap"][l], og.pmap), (lane, l)
                visits += ovis
            assert out["visits"] == visits
        _SOLO[key] = out
    return _SOLO[key]


def same(got, want, what=""):
    for k in ("poses", "T", "iters", "pmap", "pass", "hit"):
        assert got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (what, k, int(np.sum(got[k] != want[k])))
    assert got["visits"] == want["visits"], (what, got["visits"], want["visits"])


def finish(lanes):
    """Synchronise every context, then ask each for its status."""
    for ln in lanes:
        ln.ctx.synchronize()
    for ln in lanes:
        ln.ctx.check_status()
    lanes[0].torch.cuda.synchronize()


# ------------------------------------------------------------------ 3K steps round-robin
@pytest.mark.parametrize("own_buffers", [False, True], ids=["ring", "own_buffers"])
@pytest.mark.parametrize("pipeline", [0, 1])
@pytest.mark.parametrize("K", [2, MAX_LANES])
def test_lanes_round_robin(slam, syn, streams, K, pipeline, own_buffers):
    import torch
    want = [solo(slam, syn, k, pipeline) for k in range(K)]
    assert len({w["poses"].tobytes() for w in want}) == K                  # the lanes really replay different drives
    lanes = [Lane(slam, lane_ranges(syn, k), pipeline, streams[k]) for k in range(K)]
    steps = STEPS_PER_LANE * K
    ring = torch.full((steps,) + tuple(lanes[0].dr.poses.shape), float("nan"), dtype=torch.float64, device=lanes[0].dr.dev)
    torch.cuda.synchronize()
    for s in range(steps):                                                  # no host synchronise in here
        ln = lanes[s % K]
        ln.step(ln.own_P[ln.count & 1] if own_buffers else ring[s])
    finish(lanes)
    for s in range(steps):
        buf = lanes[s % K].own_P[(s // K) & 1] if own_buffers else ring[s]
        assert buf.cpu().numpy().tobytes() == want[s % K]["poses"].tobytes(), ("slot", s)
    for k, ln in enumerate(lanes):
        same(ln.final(), want[k], "lane %d of %d" % (k, K))
        ln.close()


# ------------------------------------------------------------------ a lane whose workspaces grow while the others run
@pytest.mark.parametrize("pipeline", [0, 1])
def test_a_lane_grows_its_workspaces_mid_run(slam, syn, streams, pipeline):
    """Lane 0's third step is a second DeviceReplay of 80 scans on the lane's context: its arenas grow, which frees device
    memory, while the other lanes have work in flight.  Nobody's results change."""
    import torch
    K = MAX_LANES
    want = [solo(slam, syn, k, pipeline) for k in range(K)]
    want_big = solo(slam, syn, 0, pipeline, BIG_SCANS)
    lanes = [Lane(slam, lane_ranges(syn, k), pipeline, streams[k]) for k in range(K)]
    with torch.cuda.stream(streams[0]):
        big = slam.DeviceReplay(lane_ranges(syn, 0, BIG_SCANS), AMIN, AMAX, grid_of_traj=np.arange(L))
    big.ctx.close()
    big.ctx, big.grid = lanes[0].ctx, lanes[0].grid
    steps = STEPS_PER_LANE * K
    ring = torch.full((steps,) + tuple(lanes[0].dr.poses.shape), float("nan"), dtype=torch.float64, device=lanes[0].dr.dev)
    torch.cuda.synchronize()
    grown = (STEPS_PER_LANE - 1) * K                                        # lane 0's third step
    for s in range(steps):
        if s == grown:
            lanes[0].step(None, dr=big)
        else:
            lanes[s % K].step(ring[s])
    finish(lanes)
    for s in range(steps):
        if s != grown:
            assert ring[s].cpu().numpy().tobytes() == want[s % K]["poses"].tobytes(), ("slot", s)
    same(lanes[0].final(big), want_big, "the lane that grew")
    for k in range(1, K):
        same(lanes[k].final(), want[k], "lane %d beside the one that grew" % k)
    for ln in lanes:
        ln.close()


# ------------------------------------------------------------------ a host thread per lane
def test_a_host_thread_per_lane(slam, syn, streams):
    """The contract of _abi.Context is one context per host thread.  Two threads, each with a stream, a context and a replay
    of its own, start together from a barrier and run four steps each: the solo results.  A failure here is a finding about
    the process-wide state of the library (allow_dynamic_lds and the chip-shape cache of csrc/grid_kernels.hip) or its per-thread
    state (the error text, the launch timer, the visit slots): read that code, do not re-run to reproduce it."""
    import torch
    K, steps = 2, 4
    want = [solo(slam, syn, k, 0) for k in range(K)]
    lanes = [Lane(slam, lane_ranges(syn, k), 0, streams[k]) for k in range(K)]
    rings = [torch.full((steps,) + tuple(ln.dr.poses.shape), float("nan"), dtype=torch.float64, device=ln.dr.dev) for ln in lanes]
    torch.cuda.synchronize()
    barrier, errors = threading.Barrier(K, timeout=30), [None] * K

    def work(k):
        try:
            barrier.wait()
            for s in range(steps):
                lanes[k].step(rings[k][s])
            lanes[k].ctx.synchronize()
            lanes[k].ctx.check_status()
        except BaseException as e:              # noqa: B902 - handed to the test's thread
            errors[k] = e
    threads = [threading.Thread(target=work, args=(k,), daemon=True) for k in range(K)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in threads), "a lane's thread did not finish"
    assert errors == [None] * K, errors
    finish(lanes)
    for k, ln in enumerate(lanes):
        for s in range(steps):
            assert rings[k][s].cpu().numpy().tobytes() == want[k]["poses"].tobytes(), (k, s)
        same(ln.final(), want[k], "thread %d" % k)
        ln.close()
