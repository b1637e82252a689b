"""slam_track_dev behind a pipelined replay (context option "pipeline"): a leg in a file of its own, because the table of
tests/pipeline_order_cases.py enumerates the _dev names of include/slam_hip.h only.

    grid    the call tracks in, and integrates into, the map that the piped replay's map stage has just written

Shaped as the legs of tests/test_gpu_refine_order.py: the context is brought to the results of replay A, the decoy, and
synchronised; the tracker is called once on that state (workspaces grow, kernels load) and the state is restored; replay B
is enqueued through the three stages and the tracker is called at once, with no synchronise and no host work between.
The outputs and the map's counters are compared, bit for bit, with the same sequence on a context whose pipeline option
is off and that is synchronised after every call; the serial answer behind B is asserted different from the one behind
A.  Size: 120 scans of 360 beams on a 200 x 200 map at 0.1 m, as there; the tracker follows 3 scans of 24 beams."""
import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu
AMIN, AMAX = -3.14159, 3.14159
N_SCANS, N_BEAMS, NQ = 120, 360, 24
XW, YW, RESO = 200, 200, 0.1
FOLLOW = (60, 62, 64)


@pytest.fixture(scope="module")
def slam():
    p = pkg()
    p._abi.default_context()   # fails loudly when there is no gfx950 device
    return p


class Side:
    def __init__(self, slam, syn, piped):
        import torch
        self.torch, self.piped, self.slam = torch, piped, slam
        self.rep = {k: syn.make_replay(N_SCANS, N_BEAMS, seed=s, stride=5) for k, s in (("A", 3), ("B", 4))}
        self.dr = {k: slam.DeviceReplay(r.ranges, AMIN, AMAX) for k, r in self.rep.items()}
        self.ctx, self.dev = self.dr["A"].ctx, self.dr["A"].dev
        self.dr["B"].ctx = self.ctx
        self.ctx.set_option("pipeline", 1 if piped else 0)
        self.grid = slam.DeviceGrid.metric(1, XW, YW, RESO, context=self.ctx)
        for d in self.dr.values():
            d.grid = self.grid
        self.P = torch.empty_like(self.dr["A"].poses)
        ang = np.linspace(AMIN, AMAX, N_BEAMS)[::N_BEAMS // NQ]
        self.tr = slam.DeviceTracker(self.grid, 1, np.cos(ang), np.sin(ang), n_rot=5, nx=2, ny=2, iters=3, gate_dist=0.0, gate_turn=0.0)
        self.scans = torch.from_numpy(np.ascontiguousarray(self.rep["B"].ranges[list(FOLLOW)][None, :, ::N_BEAMS // NQ])).to(self.dev)
        torch.cuda.synchronize()

    def sync(self):
        self.ctx.synchronize()
        self.torch.cuda.synchronize()

    def replay(self, k):
        self.dr[k].run(reset_grid=True, poses_out=self.P)
        if not self.piped:
            self.sync()

    def track(self, start):
        self.tr.set_poses(start, keyed=True)
        if not self.piped:
            self.sync()
        self.tr.run(self.scans)

    def answer(self):
        out = self.tr.results()
        self.sync()
        self.ctx.check_status()
        got = self.grid.read(0, want=("pass", "hit"))
        return [out["poses"].copy(), out["info"].copy(), out["trace"].copy(), out["state"].copy(), got["pass"], got["hit"]]

    def race(self, start):
        self.replay("A")
        self.sync()
        self.track(start)
        behind_a = self.answer()
        self.replay("A")
        self.sync()
        self.tr.set_poses(start, keyed=True)          # (torch's copies: on torch's stream, before the replay is enqueued)
        self.sync()
        self.replay("B")
        self.tr.run(self.scans)
        return behind_a, self.answer()

    def close(self):
        self.ctx.set_option("pipeline", 0)


@pytest.fixture(scope="module")
def sides(slam, syn):
    s = {piped: Side(slam, syn, piped) for piped in (False, True)}
    yield s
    for v in s.values():
        v.close()


def differs(a, b):
    return any(x.tobytes() != y.tobytes() for x, y in zip(a, b))


def same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_leg_grid(slam, sides):
    got = {}
    for piped, s in sides.items():
        s.replay("B")
        s.sync()
        start = s.P[0, FOLLOW[0] - 1:FOLLOW[0], :].cpu().numpy() + np.array([0.03, -0.02, 0.01])
        got[piped] = s.race(start)
    serial_a, serial_b = got[False]
    assert differs(serial_a, serial_b) and np.all(serial_b[1][..., 3] & 1) and np.all(serial_b[1][..., 3] & 4)
    assert same(got[True][0], serial_a)
    assert same(got[True][1], serial_b)
