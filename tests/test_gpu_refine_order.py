"""slam_grid_refine_dev behind a pipelined replay (context option "pipeline"): the two legs that belong in the table of
tests/pipeline_order_cases.py the next time it may be edited.

    grid    the call rebuilds its field from the counters that the piped replay's map stage has just written
    P-in    ``poses`` is the tail of the piped replay's poses_out (the field is given, so nothing else is read)

Shaped as the legs of tests/test_gpu_pipeline_order.py: the context is brought to the results of replay A, the decoy, and
synchronised; the consumer is called once on that state (workspaces grow, kernels load) and the state is restored; replay
B is enqueued through the three stages and the consumer is called at once, with no synchronise and no host work between.
Each leg is compared, bit for bit, with the same sequence on a context whose pipeline option is off and that is
synchronised after every call; the serial answer behind B is asserted different from the one behind A, so a consumer that
ran early cannot pass by accident.  Size: 120 scans of 360 beams on a 200 x 200 map at 0.1 m, as there."""
import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu
AMIN, AMAX = -3.14159, 3.14159
N_SCANS, N_BEAMS, NQ = 120, 360, 24
XW, YW, RESO, CAP, MAX_RANGE = 200, 200, 0.1, 64, 30.0
TAIL = 4


@pytest.fixture(scope="module")
def slam():
    p = pkg()
    p._abi.default_context()   # fails loudly when there is no gfx950 device
    return p


class Side:
    """Both replays on one context with one grid and one poses buffer P; ``piped`` sets the option, and a side that is not
    piped synchronises after every call."""

    def __init__(self, slam, syn, piped):
        import torch
        self.torch, self.piped = torch, piped
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
        self.ct, self.st = self.up(np.cos(ang)), self.up(np.sin(ang))
        self.scan = self.up(np.ascontiguousarray(self.rep["B"].ranges[60][::N_BEAMS // NQ]))
        self.out = (torch.empty((TAIL, 3), dtype=torch.float64, device=self.dev), torch.empty((TAIL, 2), dtype=torch.float64, device=self.dev),
                    torch.empty(TAIL, dtype=torch.int32, device=self.dev), torch.empty(TAIL, dtype=torch.int32, device=self.dev),
                    torch.empty((TAIL, 9), dtype=torch.float64, device=self.dev))
        torch.cuda.synchronize()

    def up(self, a):
        return self.torch.from_numpy(np.array(a, order="C", copy=True)).to(self.dev)

    def sync(self):
        self.ctx.synchronize()
        self.torch.cuda.synchronize()

    def replay(self, k):
        self.dr[k].run(reset_grid=True, poses_out=self.P)
        if not self.piped:
            self.sync()

    def tail(self):
        return self.P[0, N_SCANS - 1 - TAIL:, :]           # shares P's memory: what the consumer is handed

    def answer(self):
        self.sync()
        self.ctx.check_status()
        return [o.cpu().numpy().copy() for o in self.out]

    def race(self, consumer):
        """(the answer behind A, the answer behind B with nothing between the replay and the consumer)"""
        self.replay("A")
        self.sync()
        consumer()
        behind_a = self.answer()
        self.replay("A")
        self.sync()
        self.replay("B")
        consumer()
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
    """The field is rebuilt by the call from the map the piped map stage has just written; the poses are fixed."""
    got = {}
    for piped, s in sides.items():
        s.replay("B")
        s.sync()
        hyp = s.P[0, [5, 45, 85, 118], :].clone() + s.up(np.array([0.03, -0.02, 0.01]))
        s.sync()
        got[piped] = s.race(lambda s=s, hyp=hyp: s.grid.refine(s.scan, hyp, s.ct, s.st, iters=5, max_range=MAX_RANGE, cap=CAP, out=s.out))
    serial_a, serial_b = got[False]
    assert differs(serial_a, serial_b) and np.all(serial_b[3] == 0) and np.all(serial_b[2] > 0)
    assert same(got[True][0], serial_a)
    assert same(got[True][1], serial_b)


def test_leg_poses_in(slam, sides):
    """``poses`` is the tail of the piped replay's poses_out; the field is B's, made before and handed in."""
    got = {}
    for piped, s in sides.items():
        s.replay("B")
        s.sync()
        field = s.grid.distance_field(cap=CAP)
        s.sync()
        got[piped] = s.race(lambda s=s, field=field: s.grid.refine(s.scan, s.tail(), s.ct, s.st, iters=5, max_range=MAX_RANGE, cap=CAP,
                                                                     field=field, out=s.out))
    serial_a, serial_b = got[False]
    assert differs(serial_a, serial_b) and np.all(serial_b[3] == 0)
    assert same(got[True][0], serial_a)
    assert same(got[True][1], serial_b)
