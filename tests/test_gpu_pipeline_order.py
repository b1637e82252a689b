"""Every later call behind a pipelined replay (context option "pipeline"): include/slam_hip.h promises that poses_out and
pmap_dev of the later stages are visible "to any later call on this context", and the *_dev convention that buffers
may be reused by later calls.  One leg per consumer (tests/pipeline_order_cases.py):

    1. the grid, P (poses) and M (int8 pmap) are brought to the results of replay A, the decoy, and synchronised;
    2. every device argument of the consumer is prepared, the consumer is called once on that state (its workspaces
       grow now, not in the race), and step 1 is repeated;
    3. the pipelined run(reset_grid=True, poses_out=P) of replay B and slam_grid_finalize_dev(M) are enqueued;
    4. the consumer's device form is called at once: no synchronise, no host work but the call itself;
    5. ctx.synchronize(), ctx.check_status();
    6. the answer is compared, bit for bit or at the tolerance of the consumer's own test, with the consumer's plain
       reference (tests/*_ref.py, oracle/) applied to B's expected poses or pmap.

Expected values come from elsewhere: A and B run on serial contexts (pipeline 0, a host synchronise after every call)
and are checked against the C oracle as test_replay_200_scans_vs_oracle does.  Every leg asserts that the reference's
answer on B differs from its answer on A and, for map consumers, from its answer on an all-unknown map: a consumer
that ran early, on the decoy or on a map just reset, cannot pass by accident.

Size: 120 scans of 360 beams (the size of test_pipelined_map_stage_is_bit_identical) on a 200 x 200 map at 0.1 m.  With the
join of slam_grid_raycast_dev taken out of a local build, the raycast leg failed five times out of five at this size
on an MI355X, so the map stage is long enough to lose a race; the replay was not enlarged."""
import numpy as np
import pytest

import astar_ref as AR
import filter_cases as FLT
import frontier_cases as FC
import frontier_ref as F
import gridslam_ref as GS
import locate_cases as LC
import loc_ref
import locate_ref as L
import match_ref as MR
import mcl_checks as MC
import mcl_ref as X
import raycast_ref as R
import travel_cases as TC
import travel_ref as T
import view_ref as V
from conftest import pkg
from oracle import c_oracle as co
from oracle import oracle_np as on
from pipeline_order_cases import LEGS
from test_gpu_match import same_match
from test_gpu_node_replay import assert_matches_host, host_node
from test_gpu_raycast import ref_raycast, same
from test_gpu_view import check as check_view

pytestmark = pytest.mark.gpu
FTOL = 1e-9
AMIN, AMAX = -3.14159, 3.14159
N_SCANS, N_BEAMS = 120, 360
G, XW, YW, RESO = 2, 200, 200, 0.1          # map 0 is the replay's; map 1 stays unknown (copy_maps, update_particles)
GEOM = (10.0, 10.0, 10.0)                   # scale, off_x, off_y of DeviceGrid.metric(.., 200, 200, 0.1)
CAP, MAX_RANGE = 64, 30.0
NQ = 24                                     # beams of a consumer's query: every 15th of the 360


@pytest.fixture(scope="module")
def slam():
    p = pkg()
    p._abi.default_context()   # fails loudly when there is no gfx950 device
    return p


def flat(x):
    if isinstance(x, dict):
        return [v for k in sorted(x) for v in flat(x[k])]
    if isinstance(x, (tuple, list)):
        return [v for y in x for v in flat(y)]
    return [np.ascontiguousarray(x)]


def differs(a, b, by=0.0):
    """Do two answers differ: in a bit (by == 0), or by more than ``by`` somewhere (answers compared at a tolerance)?"""
    fa, fb = flat(a), flat(b)
    assert len(fa) == len(fb)
    if by == 0.0:
        return any(x.shape != y.shape or x.tobytes() != y.tobytes() for x, y in zip(fa, fb))
    return any(x.shape != y.shape or np.nanmax(np.abs(x.astype(np.float64) - y)) > by for x, y in zip(fa, fb))


def serial_replay(slam, ranges, pose0=None, grid=True):
    """One replay on a context of its own, pipeline off, synchronised after every call."""
    dr = slam.DeviceReplay(ranges, AMIN, AMAX, pose0=pose0)
    g = dr.make_grid(G, XW, YW, RESO) if grid else None
    dr.ctx.synchronize()
    dr.run()
    dr.ctx.synchronize()
    poses, Tm, it = dr.results()
    out = dict(poses=poses[0].copy(), T=Tm[0].copy(), iters=it[0].copy())
    if g is not None:
        out.update(g.read(0, want=("pmap", "pass", "hit")), visits=g.visits(), spare=g.read(1, want=("pass", "hit")))
        g.close()
    dr.ctx.close()
    return out


def against_oracle(got, ranges, pose0=(0.0, 0.0, 0.0)):
    """As test_replay_200_scans_vs_oracle; returns the oracle's grid."""
    og = co.Grid(XW, YW, *GEOM) if "pmap" in got else None
    oposes, oT, oit, visits = co.replay(ranges, AMIN, AMAX, og, pose0=pose0, threads=8)
    assert np.array_equal(got["iters"], oit)
    assert np.max(np.abs(got["poses"] - oposes)) < FTOL and np.max(np.abs(got["T"] - oT)) < FTOL
    if og is not None:
        assert np.array_equal(got["pass"], og.pass_cnt) and np.array_equal(got["hit"], og.hit_cnt)
        assert np.array_equal(got["pmap"], og.pmap) and got["visits"] == visits
        assert not got["spare"]["pass"].any() and not got["spare"]["hit"].any()
    return og


class Env:
    """The pipelined context, its grid, P and M, the two replays and what they are expected to leave."""

    def up(self, a):
        return self.torch.from_numpy(np.array(a, order="C", copy=True)).to(self.dev)

    def use(self, grid):
        self.cur = grid
        for d in self.dr.values():
            d.grid = grid

    def finalize(self):
        self.A.check(self.A.lib().slam_grid_finalize_dev(self.ctx.handle, self.cur._h, self.M.data_ptr()))

    def prime(self):
        """Step 1: the decoy's results everywhere."""
        self.dr["A"].run(reset_grid=True, poses_out=self.P)
        self.finalize()
        self.ctx.synchronize()
        self.torch.cuda.synchronize()
        assert self.torch.equal(self.P, self.dev_want["A"][0]) and self.torch.equal(self.M, self.dev_want["A"][1])

    def fire(self):
        """Step 3: replay B through the three stages, then the finalize on the map stream."""
        self.dr["B"].run(reset_grid=True, poses_out=self.P)
        self.finalize()

    def race(self, consumer, keeps_grid=True, keeps_P=True):
        """Steps 1 to 5 around ``consumer``, a function of no arguments whose device arguments exist already."""
        self.prime()
        consumer()                              # workspaces grow, kernels load: not in the race
        self.ctx.synchronize()
        self.prime()
        self.fire()
        out = consumer()
        self.ctx.synchronize()
        self.ctx.check_status()
        self.torch.cuda.synchronize()
        w = self.want["B"]
        if keeps_P:
            assert np.array_equal(self.P.cpu().numpy()[0], w["poses"])
        if keeps_grid:
            assert np.array_equal(self.M.cpu().numpy(), self.pmaps("B"))
            r = self.cur.read(0, want=("pass", "hit"))
            assert np.array_equal(r["pass"], w["pass"]) and np.array_equal(r["hit"], w["hit"])
        return out

    def pmaps(self, k):
        return np.stack([self.pm[k], self.pm["U"]])

    def map_answers(self, ref, of="pm", by=0.0):
        """The reference on B's map (or field); asserted different from its answers on A's and on an unknown map."""
        src = getattr(self, of)
        b, a, u = ref(src["B"]), ref(src["A"]), ref(src["U"])
        assert differs(b, a, by) and differs(b, u, by)
        return b

    def pose_answers(self, ref, by=0.0):
        """The reference on B's poses; asserted different from its answer on A's."""
        b, a = ref(self.want["B"]["poses"]), ref(self.want["A"]["poses"])
        assert differs(b, a, by)
        return b

    def tail(self, k):
        """The last k rows of P as a tensor that shares its memory: what a consumer is handed."""
        return self.P[0, N_SCANS - 1 - k:, :]


@pytest.fixture(scope="module")
def env(slam, syn):
    import torch
    e = Env()
    e.slam, e.A, e.torch = slam, slam._abi, torch
    e.rep = {k: syn.make_replay(N_SCANS, N_BEAMS, seed=s, stride=5) for k, s in (("A", 3), ("B", 4))}
    e.want = {k: serial_replay(slam, r.ranges) for k, r in e.rep.items()}
    e.og = {k: against_oracle(e.want[k], e.rep[k].ranges) for k in e.rep}
    e.keys = {k: k for k in "ABU"}
    e.pm = {"A": e.want["A"]["pmap"], "B": e.want["B"]["pmap"], "U": np.full((XW, YW), 50, dtype=np.int8)}
    assert differs(e.pm["A"], e.pm["B"]) and np.max(np.abs(e.want["A"]["poses"][-1] - e.want["B"]["poses"][-1])) > 1e-2
    e.fields = {k: np.stack([MR.field(pm, CAP), np.full((XW, YW), CAP, dtype=np.int16)]) for k, pm in e.pm.items()}
    # the pipelined context: both replays, one grid, P and M
    e.dr = {k: slam.DeviceReplay(r.ranges, AMIN, AMAX) for k, r in e.rep.items()}
    e.ctx, e.dev = e.dr["A"].ctx, e.dr["A"].dev
    e.dr["B"].ctx = e.ctx
    e.ctx.set_option("pipeline", 1)
    e.grid = slam.DeviceGrid.metric(G, XW, YW, RESO, context=e.ctx)
    e.use(e.grid)
    e.P = torch.empty_like(e.dr["A"].poses)
    e.M = torch.empty((G, XW, YW), dtype=torch.int8, device=e.dev)
    e.dev_want = {k: (e.up(e.want[k]["poses"][None]), e.up(e.pmaps(k))) for k in e.rep}
    # what the consumers ask
    ang = np.linspace(AMIN, AMAX, N_BEAMS)[::N_BEAMS // NQ]
    e.ct, e.st = np.ascontiguousarray(np.cos(ang)), np.ascontiguousarray(np.sin(ang))
    e.scan = np.ascontiguousarray(e.rep["B"].ranges[60][::N_BEAMS // NQ])
    e.hyp = np.ascontiguousarray(e.want["B"]["poses"][[5, 45, 85, 118]] + np.array([0.03, -0.02, 0.01]))
    e.d_ct, e.d_st, e.d_scan, e.d_hyp = e.up(e.ct), e.up(e.st), e.up(e.scan), e.up(e.hyp)
    e.d_gob0 = e.up(np.zeros(1, dtype=np.int32))
    e.ct360, e.st360 = e.A.trig_tables(AMIN, AMAX, N_BEAMS)
    occ = np.argwhere(e.pm["B"] == 100)
    e.obst = np.ascontiguousarray(((occ + 0.5) / GEOM[0] - GEOM[1]).T)           # [2, K]: the middles of B's occupied cells
    torch.cuda.synchronize()
    e.prime()
    e.fire()
    e.ctx.synchronize()
    e.ctx.check_status()
    assert np.array_equal(e.P.cpu().numpy()[0], e.want["B"]["poses"]) and np.array_equal(e.M.cpu().numpy(), e.pmaps("B"))
    yield e
    e.ctx.set_option("pipeline", 0)


@pytest.mark.parametrize("name", sorted(LEGS))
def test_leg(env, name):
    globals()["leg_" + name](env)


# ------------------------------------------------------------------ the grid, read
def leg_raycast(e):
    t = e.torch
    want = e.map_answers(lambda pm: ref_raycast(pm, *GEOM, e.hyp, e.ct, e.st, MAX_RANGE))
    r = t.empty((4, NQ), dtype=t.float32, device=e.dev)
    c = t.empty((4, NQ, 2), dtype=t.int32, device=e.dev)
    e.race(lambda: e.cur.raycast(e.d_hyp, e.d_ct, e.d_st, max_range=MAX_RANGE, ranges_out=r, cells_out=c))
    assert same(c.cpu().numpy(), want[1]) and same(r.cpu().numpy(), want[0])


def leg_scan_score(e):
    t = e.torch
    pc = R.table_points(e.scan, e.ct, e.st)

    def ref(pm):
        out = [R.score(pm, *GEOM, h, pc) for h in e.hyp]
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
    want = e.map_answers(ref)
    counts = t.empty((4, e.A.RAY_CLASSES), dtype=t.int32, device=e.dev)
    cls = t.empty((4, NQ), dtype=t.int8, device=e.dev)
    e.race(lambda: e.cur.score(e.d_scan, e.d_hyp, e.d_ct, e.d_st, counts_out=counts, class_out=cls))
    assert same(counts.cpu().numpy(), want[0]) and same(cls.cpu().numpy(), want[1])


def leg_view_gain(e):
    t = e.torch
    want = e.map_answers(lambda pm: V.views([pm], *GEOM, e.hyp, e.ct, e.st, 5.0))
    counts = t.empty((4, e.A.VIEW_COUNTS), dtype=t.int32, device=e.dev)
    seen = t.empty((4, XW, (YW + 31) // 32), dtype=t.int32, device=e.dev)
    e.race(lambda: e.cur.view_gain(e.d_hyp, e.d_ct, e.d_st, max_range=5.0, counts_out=counts, seen_out=seen))
    check_view((counts.cpu().numpy(), seen.cpu().numpy().view(np.uint32)), want, "behind a pipelined replay")


def leg_distance_field(e):
    t = e.torch
    want = e.map_answers(lambda f: f, of="fields")
    out = t.empty((G, XW, YW), dtype=t.int16, device=e.dev)
    e.race(lambda: e.cur.distance_field(cap=CAP, out=out))
    assert same(out.cpu().numpy(), want)


def leg_match(e):
    t = e.torch
    centres = np.ascontiguousarray(e.hyp[:2, :2])
    rot = np.stack([MR.rotations(h[2], 3, 0.02)[1] for h in e.hyp[:2]])
    want = e.map_answers(lambda f: MR.match_batch(f, *GEOM, e.scan, centres, e.ct, e.st, rot, 2, 2, 0.1, MAX_RANGE, CAP), of="fields")
    d_c, d_r = e.up(centres), e.up(rot)
    new = lambda *shape: t.empty(shape, dtype=t.int32, device=e.dev)       # noqa: E731
    outs = dict(best_out=new(2), cost_out=new(2), used_out=new(2), costs_out=new(2, 3, 5, 5))
    got = e.race(lambda: e.cur.match(e.d_scan, d_c, e.d_ct, e.d_st, d_r, 2, 2, 0.1, max_range=MAX_RANGE, cap=CAP, **outs))
    same_match([g.cpu().numpy() for g in got], want)


def leg_locate(e):
    t = e.torch
    rot = L.rotations(4)[1]
    want = e.map_answers(lambda f: L.locate_batch(f, GEOM[0], e.scan, e.ct, e.st, rot, 3, MAX_RANGE, CAP, maps=[0]), of="fields")
    d_r = e.up(rot)
    new = lambda dt, *shape: t.empty(shape, dtype=dt, device=e.dev)        # noqa: E731
    outs = dict(best_out=new(t.int32, 1, 3), cost_out=new(t.int32, 1), used_out=new(t.int32, 1), stats_out=new(t.int64, 1, 5))
    got = e.race(lambda: e.cur.locate(e.d_scan, e.d_ct, e.d_st, d_r, levels=3, max_range=MAX_RANGE, cap=CAP, grid_of_batch=e.d_gob0,
                                      B=1, **outs))
    LC.same([g.cpu().numpy() for g in got], want)


def leg_frontiers(e):
    t = e.torch
    kw = dict(radius=0, min_unknown=0, min_size=1)            # the plain cell rule: a closed room leaves few frontier cells
    want = e.map_answers(lambda pm: F.frontiers_batch([pm, e.pm["U"]], maps=[0], M=64, **kw))
    assert want[0][0, 0] > 0                    # B's map has frontiers to find
    new = lambda dt, *shape: t.empty(shape, dtype=dt, device=e.dev)        # noqa: E731
    out = (new(t.int32, 1, 2), new(t.int32, 1, 64, 8), new(t.int64, 1, 64, 2), new(t.int32, 1, XW, YW))
    e.race(lambda: e.cur.frontiers(grid_of_batch=e.d_gob0, max_clusters=64, labels=True, out=out, **kw))
    FC.same(tuple(o.cpu().numpy() for o in out), want)


def leg_travel(e):
    t = e.torch
    x, y = e.want["B"]["poses"][-1][:2]
    src = np.array([[[R.to_cell(x, GEOM[0], GEOM[1]), R.to_cell(y, GEOM[0], GEOM[2])]]], dtype=np.int32)
    want = e.map_answers(lambda pm: T.batch(pm[None], src, maps=[0]))
    assert (want["cost"] > 0).sum() > 100        # the robot's cell reaches a good part of B's free space
    d_src = e.up(src)
    out = dict(status=t.empty(1, dtype=t.int32, device=e.dev), cost=t.empty((1, XW, YW), dtype=t.int32, device=e.dev),
               dir=t.empty((1, XW, YW), dtype=t.int8, device=e.dev))
    e.race(lambda: e.cur.travel(d_src, grid_of_batch=e.d_gob0, out=out))
    TC.same({k: v.cpu().numpy() for k, v in out.items()}, want)


def weigh_leg(e, fn, table):
    """slam_mcl_weigh_dev / slam_mcl_weigh_maps_dev: four particles of one filter on map 0, the field rebuilt by the call."""
    t = e.torch
    poses, ranges = e.hyp[None], e.scan[None]
    ref = lambda f: X.weigh(f, *GEOM, poses, ranges, e.ct, e.st, MAX_RANGE, CAP)["cost"]      # noqa: E731
    e.map_answers(ref, of="fields")
    d_p, d_r = e.up(poses), e.up(ranges)
    d_t = None if table is None else e.up(table)
    cost = t.empty((1, 4), dtype=t.int32, device=e.dev)
    used = t.empty(1, dtype=t.int32, device=e.dev)
    call = getattr(e.A.lib(), fn)
    e.race(lambda: e.A.check(call(e.ctx.handle, e.cur._h, d_p.data_ptr(), None, None, d_r.data_ptr(), e.d_ct.data_ptr(),
                                  e.d_st.data_ptr(), e.A.ptr(d_t), 1, 4, NQ, MAX_RANGE, CAP, None, None, cost.data_ptr(),
                                  used.data_ptr())))
    MC.check_weigh(e.slam, e.cur, None, GEOM, poses, ranges, e.ct, e.st, max_range=MAX_RANGE, cap=CAP, fields=e.fields["B"],
                   pmaps=table, got=(d_p.cpu().numpy(), cost.cpu().numpy(), None, used.cpu().numpy()))


def leg_mcl_weigh(e):
    weigh_leg(e, "slam_mcl_weigh_dev", None)


def leg_mcl_weigh_maps(e):
    weigh_leg(e, "slam_mcl_weigh_maps_dev", np.zeros((1, 4), dtype=np.int32))


def counters_of(e, k):
    """[pass, hit] of the G maps behind replay k ("U": behind none)."""
    none = np.zeros((XW, YW), dtype=np.uint32)
    return [np.stack([e.want[k][c] if k in e.want else none, none]) for c in ("pass", "hit")]


def read_counters(grid):
    r = [grid.read(g, want=("pass", "hit")) for g in range(G)]
    return [np.stack([x[c] for x in r]) for c in ("pass", "hit")]


def leg_copy_maps(e):
    t = e.torch
    src = np.array([0], dtype=np.int32)

    def ref(k):
        arrays = counters_of(e, k)
        kinds = GS.copy_maps(arrays, src, first=1)
        return arrays + [kinds]
    want, decoy = ref("B"), ref("A")
    assert differs(want, decoy) and want[0][1].any()          # (an unknown map 0 would leave map 1 empty)
    d_src = e.up(src)
    out = t.empty(1, dtype=t.int32, device=e.dev)
    e.race(lambda: e.cur.copy_maps(d_src, first=1, out=out))
    assert np.array_equal(out.cpu().numpy(), want[2])
    for got, w in zip(read_counters(e.cur), want):
        assert np.array_equal(got, w)


# ------------------------------------------------------------------ the grid, written
def written(e, add):
    """B's counters plus what ``add(pass, hit)`` casts; asserted different from A's plus the same and from the cast alone."""
    outs = []
    for k in ("B", "A", "U"):
        arrays = counters_of(e, k)
        add(*arrays)
        outs.append(arrays)
    assert differs(outs[0], outs[1]) and differs(outs[0], outs[2]) and outs[2][0].any()
    return outs[0]


def check_written(e, want):
    for got, w in zip(read_counters(e.cur), want):
        assert np.array_equal(got, w)
    assert np.array_equal(e.cur.read(0)["pmap"], GS.pmap_of(want[0][0], want[1][0]))


def leg_update(e):
    ox, oy = np.array([[1.0, 2.0, -3.0, 0.5, -1.5]]), np.array([[0.5, -1.0, 2.0, 3.0, -2.5]])
    cx, cy = e.want["B"]["poses"][-1][:1].copy(), e.want["B"]["poses"][-1][1:2].copy()

    def add(pass_, hit):
        m = co.Grid(XW, YW, *GEOM)
        m.update(ox[0], oy[0], cx, cy)
        pass_[0] += m.pass_cnt
        hit[0] += m.hit_cnt
    want = written(e, add)
    d = [e.up(a) for a in (ox, oy, cx, cy)]
    e.race(lambda: e.A.check(e.A.lib().slam_grid_update_dev(e.ctx.handle, e.cur._h, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                                                            d[3].data_ptr(), 1, 5, None)), keeps_grid=False)
    check_written(e, want)


def leg_update_scans(e):
    ranges = np.ascontiguousarray(e.rep["B"].ranges[[30, 90]][:, ::N_BEAMS // NQ])
    poses = np.ascontiguousarray(e.want["B"]["poses"][[29, 89]])

    def add(pass_, hit):
        for s in range(2):
            GS.update_particles(pass_[:1], hit[:1], GEOM, ranges[s:s + 1], e.ct, e.st, poses[s][None, None], make=GS.c_mapping)
    want = written(e, add)
    d_r, d_p = e.up(ranges), e.up(poses)
    e.race(lambda: e.A.check(e.A.lib().slam_grid_update_scans_dev(e.ctx.handle, e.cur._h, d_r.data_ptr(), e.d_ct.data_ptr(),
                                                                  e.d_st.data_ptr(), d_p.data_ptr(), None, 2, NQ)), keeps_grid=False)
    check_written(e, want)


def leg_update_particles(e):
    ranges, poses = e.scan[None], np.ascontiguousarray(e.hyp[None, :2])
    want = written(e, lambda pass_, hit: GS.update_particles(pass_, hit, GEOM, ranges, e.ct, e.st, poses, make=GS.c_mapping))
    d_r, d_p = e.up(ranges), e.up(poses)
    e.race(lambda: e.cur.update_particles(d_r, e.d_ct, e.d_st, d_p), keeps_grid=False)
    check_written(e, want)


# ------------------------------------------------------------------ the grid, handed out or read back
def leg_counters(e):
    want = e.map_answers(lambda k: counters_of(e, k), of="keys")
    def consumer():                             # the header's recipe for a pointer handed out: order the caller's stream, then use it
        views = e.cur.counters_torch()
        e.ctx.stream_order(e.torch.cuda.current_stream(e.dev).cuda_stream, 0)
        return [c.clone() for c in views]
    got = e.race(consumer)
    for g, w in zip(got, want):
        assert np.array_equal(g.cpu().numpy().view(np.uint32), w)


def leg_live_pmap(e):
    t = e.torch
    want = e.map_answers(e.pmaps, of="keys")

    class View:
        def __init__(self, ptr):
            self.__cuda_array_interface__ = {"shape": (G, XW, YW), "typestr": "|i1", "data": (int(ptr), False), "version": 2}
    grid = e.slam.DeviceGrid.metric(G, XW, YW, RESO, context=e.ctx)         # a grid of its own: a live pmap stays for good
    e.use(grid)
    try:
        def consumer():
            view = t.as_tensor(View(grid.live_pmap()), device=e.dev)
            e.ctx.stream_order(t.cuda.current_stream(e.dev).cuda_stream, 0)
            return view.clone()
        got = e.race(consumer)
        assert np.array_equal(got.cpu().numpy(), want)
    finally:
        e.use(e.grid)
        e.ctx.synchronize()
        grid.close()


def leg_occupancy_data(e):
    want = e.map_answers(lambda k: e.og[k].occupancy_grid_data() if k in e.og else on.occupancy_grid_data(e.pm[k]), of="keys")
    assert np.array_equal(want, on.occupancy_grid_data(e.pm["B"]))
    got = e.race(lambda: e.cur.occupancy_grid_data(0))
    assert np.array_equal(got, want)


def leg_visits(e):
    want = e.map_answers(lambda k: np.int64(e.want[k]["visits"] if k in e.want else 0), of="keys")
    assert e.race(e.cur.visits) == want


# ------------------------------------------------------------------ M
def rows_of(pm):
    return AR.to_rows(pm, wire_layout=False).astype(np.int64)


def leg_astar_inflate(e):
    t = e.torch
    want = e.map_answers(lambda pm: AR.inflate(rows_of(pm), span=XW, r=2))
    out = t.empty((1, YW, XW), dtype=t.int8, device=e.dev)
    e.race(lambda: e.A.check(e.A.lib().slam_astar_inflate_dev(e.ctx.handle, e.M.data_ptr(), 1, YW, XW, 0, XW, 2, out.data_ptr())))
    assert np.array_equal(out.cpu().numpy()[0], want)


def leg_astar(e):
    t = e.torch
    free = np.argwhere(AR.inflate(rows_of(e.pm["B"]), span=XW, r=2) == 0)
    pick = np.random.default_rng(5).integers(0, len(free), (2, 4))
    s, g = (free[pick[0]] + 1).astype(np.int32), (free[pick[1]] + 1).astype(np.int32)
    cap = 512

    def ref(pm):
        imap = AR.inflate(rows_of(pm), span=XW, r=2)
        return [AR.plan(imap, s[b], g[b], path_cap=cap) for b in range(4)]
    want = e.map_answers(lambda pm: [[r["status"], r["expansions"], r["length"], r["path"]] for r in ref(pm)])
    assert sum(w[0] == AR.OK for w in want) >= 2
    d_s, d_g = e.up(s), e.up(g)
    new = lambda *shape: t.empty(shape, dtype=t.int32, device=e.dev)       # noqa: E731
    st, ln, path, ex = new(4), new(4), new(4, cap, 2), new(4)
    e.race(lambda: e.A.check(e.A.lib().slam_astar_dev(e.ctx.handle, e.M.data_ptr(), 1, YW, XW, 0, XW, 2, d_s.data_ptr(), d_g.data_ptr(),
                                                      None, 4, cap, st.data_ptr(), ln.data_ptr(), path.data_ptr(), ex.data_ptr(), None)))
    st, ln, path, ex = (a.cpu().numpy() for a in (st, ln, path, ex))
    for b, (status, expansions, length, cells) in enumerate(want):
        assert (st[b], ex[b], ln[b]) == (status, expansions, length), b
        assert np.array_equal(path[b, :min(length, cap)], cells[:cap]), b


def leg_map_obstacles(e):
    t = e.torch
    cells = XW * YW

    def ref(pm):
        o = on.map_obstacles(on.occupancy_grid_data(pm), XW, YW, RESO, -GEOM[1], -GEOM[2])
        return o[:, np.lexsort((o[1], o[0]))]
    want = e.map_answers(ref)
    ox, oy = (t.empty(cells, dtype=t.float64, device=e.dev) for _ in range(2))
    count = t.empty(1, dtype=t.int32, device=e.dev)
    e.race(lambda: e.A.check(e.A.lib().slam_map_obstacles_dev(e.ctx.handle, e.M.data_ptr(), XW, YW, 0, RESO, -GEOM[1], -GEOM[2],
                                                              ox.data_ptr(), oy.data_ptr(), cells, count.data_ptr())))
    k = int(count.cpu().numpy()[0])
    assert k == want.shape[1]
    got = np.stack([ox.cpu().numpy()[:k], oy.cpu().numpy()[:k]])
    assert np.array_equal(got[:, np.lexsort((got[1], got[0]))], want)          # (the device appends in arbitrary order)


# ------------------------------------------------------------------ P, read
def small_transforms(n, seed):
    """[1, n, 9] rigid transforms as test_pose_compose_vs_oracle draws them."""
    rng = np.random.default_rng(seed)
    th = rng.uniform(-0.1, 0.1, size=(1, n))
    Tm = np.zeros((1, n, 9))
    Tm[..., 0], Tm[..., 1], Tm[..., 2] = np.cos(th), -np.sin(th), rng.normal(0, 0.05, (1, n))
    Tm[..., 3], Tm[..., 4], Tm[..., 5] = np.sin(th), np.cos(th), rng.normal(0, 0.05, (1, n))
    Tm[..., 8] = 1
    return Tm


def composed(Tm, pose0):
    out, s = [], np.array(pose0, dtype=np.float64)
    for k in range(Tm.shape[1]):
        s = co.compose_pose(s, Tm[0, k].reshape(3, 3))
        out.append(s)
    return np.stack(out)


def leg_pose_compose_pose0(e):
    t = e.torch
    Tm = small_transforms(5, 3)
    want = e.pose_answers(lambda poses: composed(Tm, poses[-1]), by=1e-3)
    d_T, pose0 = e.up(Tm), e.tail(1)
    out = t.empty((1, 5, 3), dtype=t.float64, device=e.dev)
    e.race(lambda: e.A.check(e.A.lib().slam_pose_compose_dev(e.ctx.handle, d_T.data_ptr(), pose0.data_ptr(), 1, 5, out.data_ptr())))
    assert np.max(np.abs(out.cpu().numpy()[0] - want)) < 1e-10         # the bar of test_pose_compose_vs_oracle


def leg_virtual_scan(e):
    t = e.torch
    inc = (AMAX - AMIN) / (NQ - 1)
    want = e.pose_answers(lambda poses: np.stack([on.laser_estimation(e.obst, p, AMIN, inc, NQ) for p in poses[-4:]]), by=1e-3)
    assert (want < 100.0).sum() > NQ             # B's walls fall into most bins
    d_o, poses = e.up(e.obst), e.tail(4)
    out = t.empty((4, NQ), dtype=t.float64, device=e.dev)
    K = e.obst.shape[1]
    e.race(lambda: e.A.check(e.A.lib().slam_virtual_scan_dev(e.ctx.handle, d_o[0].data_ptr(), d_o[1].data_ptr(), K, poses.data_ptr(), 4,
                                                             AMIN, inc, NQ, out.data_ptr())))
    got = out.cpu().numpy()
    assert np.array_equal(got == 100.0, want == 100.0) and np.max(np.abs(got - want)) < 1e-12     # the bars of test_gpu_localization


def leg_map_observation(e):
    t = e.torch
    n, inc = N_BEAMS, (AMAX - AMIN) / (N_BEAMS - 1)
    src = on.laser_to_numpy(e.rep["B"].ranges[-1].astype(np.float64), AMIN, AMAX)
    want = e.pose_answers(lambda poses: np.stack([on.map_observation(e.obst, p, src, AMIN, AMAX, inc) for p in poses[-2:]]), by=1e-3)
    d_o, d_src, poses = e.up(e.obst), e.up(src[:2]), e.tail(2)
    d_c, d_s = e.up(e.ct360), e.up(e.st360)
    vr, vp = t.empty((2, n), dtype=t.float64, device=e.dev), t.empty((2, 2, n), dtype=t.float64, device=e.dev)
    Tm, it = t.empty((2, 9), dtype=t.float64, device=e.dev), t.empty(2, dtype=t.int32, device=e.dev)
    K = e.obst.shape[1]
    e.race(lambda: e.A.check(e.A.lib().slam_map_observation_dev(
        e.ctx.handle, d_o[0].data_ptr(), d_o[1].data_ptr(), K, poses.data_ptr(), d_src.data_ptr(), 2, n, 1, d_c.data_ptr(),
        d_s.data_ptr(), AMIN, inc, 30, 0.001, vr.data_ptr(), vp.data_ptr(), Tm.data_ptr(), it.data_ptr())))
    assert np.max(np.abs(Tm.cpu().numpy().reshape(2, 3, 3) - want)) < FTOL and it.cpu().numpy().min() >= 1


def ancestors_of(seed):
    return np.random.default_rng(seed).integers(0, N_SCANS - 1, (1, N_SCANS - 1)).astype(np.int32)


def leg_mcl_settle_src(e):
    t = e.torch
    anc = ancestors_of(11)
    want = e.pose_answers(lambda poses: GS.settle_batch(anc, poses_src=poses[None])["poses"])
    d_a = e.up(anc)
    settled = t.empty((1, N_SCANS - 1), dtype=t.int32, device=e.dev)
    out = t.empty_like(e.P)
    e.race(lambda: e.A.check(e.A.lib().slam_mcl_settle_dev(e.ctx.handle, d_a.data_ptr(), e.P.data_ptr(), 1, N_SCANS - 1, 0,
                                                           settled.data_ptr(), out.data_ptr(), None, None)))
    assert np.array_equal(settled.cpu().numpy(), GS.settle_batch(anc)["settled"]) and same(out.cpu().numpy(), want)


def leg_mcl_resample_poses(e):
    t = e.torch
    Pn = N_SCANS - 1
    rng = np.random.default_rng(12)
    acc = rng.integers(0, 4000, (1, Pn)).astype(np.int32)
    table = X.weight_table(2.0)
    u0 = np.array([0.37])
    e.pose_answers(lambda poses: X.resample(poses[None], acc, table, 0, u0, np.inf)["poses"])
    d_tab, d_u, used = e.up(table.view(np.int32)), e.up(u0), []
    out, anc = t.empty_like(e.P), t.empty((1, Pn), dtype=t.int32, device=e.dev)
    est, info = t.empty((1, 4), dtype=t.float64, device=e.dev), t.empty((1, 4), dtype=t.int32, device=e.dev)

    accs = [e.up(acc), e.up(acc)]               # acc is in-out: one copy for the rehearsal, one for the race

    def consumer():
        d_acc = accs.pop()
        used.append(d_acc)
        e.A.check(e.A.lib().slam_mcl_resample_dev(e.ctx.handle, e.P.data_ptr(), d_acc.data_ptr(), d_tab.data_ptr(), len(table), 0,
                                                  d_u.data_ptr(), float("inf"), 1, Pn, out.data_ptr(), anc.data_ptr(), est.data_ptr(),
                                                  info.data_ptr()))
    e.race(consumer)
    MC.check_resample(e.slam, e.ctx, e.want["B"]["poses"][None], acc, table, u0, shift=0, ess_frac=np.inf,
                      got=(out.cpu().numpy(), used[-1].cpu().numpy(), anc.cpu().numpy(), est.cpu().numpy(), info.cpu().numpy()))


def leg_particles_pose_prev(e):
    t = e.torch
    pair = np.ascontiguousarray(e.rep["B"].ranges[-2:])
    tar = np.array(co.laser_to_points(pair[0], AMIN, AMAX))
    src = np.array(co.laser_to_points(pair[1], AMIN, AMAX))
    oT, oit, _ = co.icp_process(tar, src, 30, 0.001)
    want = e.pose_answers(lambda poses: np.stack([co.compose_pose(p, oT) for p in poses[-4:]]), by=1e-3)
    d_r, d_c, d_s, prev = e.up(pair), e.up(e.ct360), e.up(e.st360), e.tail(4)
    out, Tm = t.empty((4, 3), dtype=t.float64, device=e.dev), t.empty((4, 9), dtype=t.float64, device=e.dev)
    it = t.empty(4, dtype=t.int32, device=e.dev)
    e.race(lambda: e.A.check(e.A.lib().slam_particles_dev(e.ctx.handle, d_r.data_ptr(), d_c.data_ptr(), d_s.data_ptr(), N_BEAMS,
                                                          e.A.DTYPES["f64"], None, prev.data_ptr(), 4, 30, 0.001, None, None,
                                                          out.data_ptr(), Tm.data_ptr(), it.data_ptr())))
    assert np.all(it.cpu().numpy() == oit) and np.max(np.abs(Tm.cpu().numpy().reshape(4, 3, 3) - oT)) < FTOL
    assert np.max(np.abs(out.cpu().numpy() - want)) < FTOL


def both_answers(e, ref):
    """The reference on B's map and poses; asserted different from A's map and poses and from an unknown map."""
    b = ref(e.pm["B"], e.want["B"]["poses"][-4:])
    assert differs(b, ref(e.pm["A"], e.want["A"]["poses"][-4:])) and differs(b, ref(e.pm["U"], e.want["B"]["poses"][-4:]))
    assert differs(b, ref(e.pm["B"], e.want["A"]["poses"][-4:]))
    return b


def leg_raycast_poses(e):
    t = e.torch
    want = both_answers(e, lambda pm, poses: ref_raycast(pm, *GEOM, poses, e.ct, e.st, MAX_RANGE))
    r = t.empty((4, NQ), dtype=t.float32, device=e.dev)
    c = t.empty((4, NQ, 2), dtype=t.int32, device=e.dev)
    poses = e.tail(4)
    e.race(lambda: e.cur.raycast(poses, e.d_ct, e.d_st, max_range=MAX_RANGE, ranges_out=r, cells_out=c))
    assert same(c.cpu().numpy(), want[1]) and same(r.cpu().numpy(), want[0])


def leg_view_gain_poses(e):
    t = e.torch
    want = both_answers(e, lambda pm, poses: V.views([pm], *GEOM, poses, e.ct, e.st, 5.0))
    counts = t.empty((4, e.A.VIEW_COUNTS), dtype=t.int32, device=e.dev)
    seen = t.empty((4, XW, (YW + 31) // 32), dtype=t.int32, device=e.dev)
    poses = e.tail(4)
    e.race(lambda: e.cur.view_gain(poses, e.d_ct, e.d_st, max_range=5.0, counts_out=counts, seen_out=seen))
    check_view((counts.cpu().numpy(), seen.cpu().numpy().view(np.uint32)), want, "poses of a pipelined replay")


def chain_leg(e, with_map):
    """Three replays, each starting where the one before ended, without a synchronise: B through the pipeline, then A's
    scans and B's scans again with pose0 = the last row of the poses before.  With a map the followers are pipelined
    themselves; without one they run on the context's stream and read a pose that the pose stream writes."""
    t = e.torch
    scans = [e.rep["A"].ranges, e.rep["B"].ranges]
    want, pose0 = [], e.want["B"]["poses"][-1]
    for r in scans:                             # the serial chain, each link against the oracle from the same start
        w = serial_replay(e.slam, r, pose0=pose0, grid=with_map)
        against_oracle(w, r, pose0=pose0)
        want.append(w)
        pose0 = w["poses"][-1]
    decoy = co.replay(scans[0], AMIN, AMAX, None, pose0=e.want["A"]["poses"][-1])[0]
    assert np.max(np.abs(decoy - want[0]["poses"])) > 1e-3
    drs = [e.slam.DeviceReplay(r, AMIN, AMAX) for r in scans]
    outs = [t.empty_like(e.P) for _ in scans]
    for d, start in zip(drs, (e.P, outs[0])):
        d.ctx = e.ctx
        d.grid = e.cur if with_map else None
        d.pose0 = start[0, N_SCANS - 2:, :]
    t.cuda.synchronize()

    def consumer():
        for d, o in zip(drs, outs):
            d.run(reset_grid=True, poses_out=o)
    e.race(consumer, keeps_grid=not with_map)
    for o, w in zip(outs, want):
        assert np.array_equal(o.cpu().numpy()[0], w["poses"])
    if with_map:
        r = e.cur.read(0, want=("pmap", "pass", "hit"))
        assert all(np.array_equal(r[k], want[1][k]) for k in ("pmap", "pass", "hit")) and e.cur.visits() == want[1]["visits"]


def leg_replay_chain_map(e):
    chain_leg(e, True)


def leg_replay_chain_no_map(e):
    chain_leg(e, False)


# the three nodes that take a start pose: x0 / pose0 is the last row of P
def leg_ekf_lm(e):
    """slam_ekf_lm_dev from x0 = B's last pose: three steps of circle-drive odometry that see one landmark, then a second one
    beside it, then both again (the first trajectory of test_ekf_past_the_group_count)."""
    t = e.torch
    max_lm, steps, N = 2, 3, 7
    u = np.tile(FLT.ODOMETRY, (1, steps, 1))
    rows = [[(3.0, 0.2)], [(3.1, 0.1), (4.0, 2.0)], [(3.0, -0.1), (4.1, 1.8)]]
    z = np.array([r for s in rows for r in s], dtype=np.float64)
    off = np.concatenate([[0], np.cumsum([len(s) for s in rows])]).astype(np.int64)

    def ref(poses):
        r = FLT.host_run(u[0], [np.array(s, dtype=np.float64).reshape(-1, 2) for s in rows], poses[-1], max_lm)
        assert r["status"] == FLT.OK and r["nlm"] == [1, 2, 2]
        return [r["x"], r["P"]]
    want = e.pose_answers(ref, by=1e-3)
    d_u, d_off, d_z, d_n = e.up(u), e.up(off), e.up(z), e.up(np.full(1, steps, dtype=np.int32))
    x0 = e.tail(1)
    x, P = t.empty((1, N), dtype=t.float64, device=e.dev), t.empty((1, N, N), dtype=t.float64, device=e.dev)
    nlm, status = t.empty((1, steps), dtype=t.int32, device=e.dev), t.empty(1, dtype=t.int32, device=e.dev)
    e.race(lambda: e.A.check(e.A.lib().slam_ekf_lm_dev(e.ctx.handle, x0.data_ptr(), d_u.data_ptr(), d_n.data_ptr(), d_off.data_ptr(),
                                                       d_z.data_ptr(), len(z), 1, steps, max_lm, x.data_ptr(), P.data_ptr(),
                                                       nlm.data_ptr(), status.data_ptr())))
    assert status.cpu().numpy().tolist() == [FLT.OK] and nlm.cpu().numpy().tolist() == [[1, 2, 2]]
    dx, dP = np.max(np.abs(x.cpu().numpy()[0] - want[0])), np.max(np.abs(P.cpu().numpy()[0] - want[1]))
    assert dx < 1e-9 and dP < 1e-9, (dx, dP)              # the bar of test_ekf_past_the_group_count (and of check_trajectory)


NODE_SCANS = (48, 49, 53, 56)                   # scans of B that show a landmark (a pillar seen edge-on): the node keeps them all


def leg_node_replay(e):
    """slam_node_replay_dev (no map) from pose0 = B's last pose, over four of B's scans."""
    scans = np.ascontiguousarray(e.rep["B"].ranges[list(NODE_SCANS)])

    def ref(poses):
        class Started:                          # host_node builds its node itself: hand it one that starts at the pose
            LaserScan = e.slam.LaserScan

            @staticmethod
            def SLAM_EKF(**kw):
                node = e.slam.SLAM_EKF(**kw)
                node.xEst = np.array(poses[-1], dtype=np.float64).reshape(3, 1)
                return node
        r = host_node(Started, scans)
        assert r["kept"] == list(range(len(scans))) and not r["raised"] and len(r["nlm"]) == len(scans) - 1
        return r
    want = e.pose_answers(ref, by=1e-3)
    rep = e.slam.DeviceNodeReplay(scans, AMIN, AMAX, max_lm=8)
    rep.ctx.close()
    rep.ctx, rep.pose0 = e.ctx, e.tail(1)
    e.torch.cuda.synchronize()
    e.race(rep.run)
    assert_matches_host(rep.results(), 0, want)           # the bars of tests/test_gpu_node_replay.py: counts exact, states within 1e-9


LOC_SCANS = (119, 118, 117)                     # B's last scans, backwards: the first was taken at B's last pose


def leg_loc_replay(e):
    """slam_loc_replay_dev from pose0 = B's last pose against the occupied cells of B's map, over B's last three scans."""
    ranges = np.ascontiguousarray(e.rep["B"].ranges[list(LOC_SCANS)])
    keys = ("xest", "xodom", "P", "T_obs", "T_odom")

    def ref(poses):
        r = loc_ref.chain(ranges, e.obst, AMIN, AMAX, poses[-1])
        return [r[k] for k in keys] + [r["iters_obs"]]
    want = e.pose_answers(ref, by=1e-3)
    _, worst = loc_ref.stable(ranges, e.obst, AMIN, AMAX, e.want["B"]["poses"][-1])
    assert worst < 1e-10                                  # B's last pose sits away from the chain's discontinuities
    rep = e.slam.DeviceLocalizationReplay(ranges, AMIN, AMAX, e.obst, pose0=np.zeros((1, 3)), context=e.ctx)
    rep.pose0 = e.tail(1)
    e.race(rep.run)
    o = rep.results()
    assert o["status"].tolist() == [0] and o["iters_obs"][0].tolist() == want[-1].tolist()
    for k, w in zip(keys, want):                          # the bars of test_against_oracle_chain
        d = float(np.max(np.abs(o[k][0] - w)))
        assert d < 1e-9, (k, d)


# ------------------------------------------------------------------ P, written while the map stage reads it
def leg_pose_compose_out(e):
    Tm = small_transforms(N_SCANS - 1, 7)
    pose0 = np.array([[0.4, -0.3, 0.2]])
    want = composed(Tm, pose0[0])
    assert np.max(np.abs(want - e.want["B"]["poses"])) > 1e-2 and np.max(np.abs(want - e.want["A"]["poses"])) > 1e-2
    d_T, d_0 = e.up(Tm), e.up(pose0)
    e.race(lambda: e.A.check(e.A.lib().slam_pose_compose_dev(e.ctx.handle, d_T.data_ptr(), d_0.data_ptr(), 1, N_SCANS - 1,
                                                             e.P.data_ptr())), keeps_P=False)       # (race checks B's map)
    assert np.max(np.abs(e.P.cpu().numpy()[0] - want)) < 1e-10


def leg_mcl_settle_out(e):
    t = e.torch
    anc = ancestors_of(13)
    src = np.random.default_rng(14).normal(0.0, 2.0, (1, N_SCANS - 1, 3))
    want = GS.settle_batch(anc, poses_src=src)["poses"]
    assert differs(want[0], e.want["B"]["poses"]) and differs(want[0], e.want["A"]["poses"])
    d_a, d_s = e.up(anc), e.up(src)
    settled = t.empty((1, N_SCANS - 1), dtype=t.int32, device=e.dev)
    e.race(lambda: e.A.check(e.A.lib().slam_mcl_settle_dev(e.ctx.handle, d_a.data_ptr(), d_s.data_ptr(), 1, N_SCANS - 1, 0,
                                                           settled.data_ptr(), e.P.data_ptr(), None, None)), keeps_P=False)
    assert same(e.P.cpu().numpy(), want)


# ------------------------------------------------------------------ the caller's own stream
def leg_stream_order(e):
    t = e.torch
    side = t.cuda.Stream(device=e.dev)
    assert side.cuda_stream != t.cuda.current_stream(e.dev).cuda_stream

    def consumer():
        e.ctx.stream_order(side.cuda_stream, 0)
        with t.cuda.stream(side):
            return e.P.clone(), e.M.clone()
    p, m = e.race(consumer)
    side.synchronize()
    assert np.array_equal(p.cpu().numpy()[0], e.want["B"]["poses"]) and np.array_equal(m.cpu().numpy(), e.pmaps("B"))
