"""The map reset that rides on the scan-matching launch (context option "replay_reset"; icp_clear_on_the_way in
csrc/icp_kernels.hip), driven where it could fail: into a map whose every counter word is dirty, with fewer lanes than
words to clear, with a lane count on either side of the word count, in every launch form of the scan matcher, over a grid
of several maps of which a trajectory writes only some, and through the two routes that use slam_grid_reset instead (a live
pmap, the "pipeline" option).  tests/replay_reset_cases.py has the sizes, tests/test_replay_reset_cases.py holds them to
their edges without a GPU.

Every case runs on one context:
    1. a replay of OTHER scans into the grid, then a non-zero pattern into every word of the grid's state: the pass and hit
       planes of every map, reached through DeviceGrid.counters_torch(), and the visit slots behind them (the state is
       one allocation that starts at the pass counters; slam_plan_query "grid_state_bytes" says where it ends);
    2. ctx.set_option("replay_reset", 1);
    3. slam_replay_dev.
Poses, transforms, iteration counts, pass, hit, pmap and the visit count must then equal, bit for bit, the same replay on a
fresh context into a fresh grid with "replay_reset" 0.  For float64 points that expectation is itself held to the C oracle
(co.replay) at the bar of test_replay_200_scans_vs_oracle - counters, pmap, visits and iteration counts exact, poses and
transforms within 1e-9 - so the device is never its own reference for the counters of those cases.

With the loop of icp_clear_on_the_way cut to its first trip in a local build, every case of fewer lanes than words fails
here (19 of 37: many_trips and below of all five forms, both preferred_trips, several maps, f32 / f16, zero iterations, host
form, on / off / on, two replays) and every case of at least as many lanes passes, as do the two slam_grid_reset routes and
the call without a grid.  The words such a build leaves in the below cases and in the several-map case are visit slots:
they are caught because the pattern goes into the slots too."""
import numpy as np
import pytest

import replay_reset_cases as K
from conftest import pkg
from oracle import c_oracle as co
from oracle import checks

pytestmark = pytest.mark.gpu
FTOL = 1e-9
AMIN, AMAX = -3.14159, 3.14159
PATTERN = 0x5A5A0001                          # below 2^31: the same bits as int32 and as uint32


@pytest.fixture(scope="module")
def slam():
    p = pkg()
    p._abi.default_context()   # fails loudly when there is no gfx950 device
    return p


@pytest.fixture(scope="module")
def scans(syn):
    """One drive for every case of the table (a case takes its first pairs + 1 scans), two more for the several-map case,
    and the few scans that dirty a map first."""
    return {"main": syn.make_replay(K.max_pairs() + 1, K.BEAMS, seed=21, stride=5).ranges,
            "two": np.stack([syn.make_replay(K.MANY["n_scan"], K.BEAMS, seed=s, stride=5).ranges for s in (31, 32)]),
            "other": syn.make_replay(4, K.BEAMS, seed=9, stride=5).ranges}


# ------------------------------------------------------------------ one replay, its results, its expectation
class Run:
    """A DeviceReplay on a context of its own with the case's options, and a grid (or none)."""

    def __init__(self, slam, ranges, options=None, grid=(1, K.XW, K.YW, K.RESO), live=False, **kw):
        self.slam, self.A = slam, slam._abi
        self.dr = slam.DeviceReplay(ranges, AMIN, AMAX, **kw)
        self.ctx = self.dr.ctx
        for name, value in (options or {}).items():
            self.ctx.set_option(name, value)
        self.grid = self.dr.make_grid(*grid) if grid else None
        if live:
            assert self.grid.live_pmap() != 0

    def replay_dev(self, dr=None, grid=True):
        """slam_replay_dev itself: DeviceReplay.run() would choose "replay_reset" for the caller."""
        d = dr or self.dr
        g = self.grid if grid else None
        self.A.check(self.A.lib().slam_replay_dev(
            self.ctx.handle, d.ranges.data_ptr(), d.cos_t.data_ptr(), d.sin_t.data_ptr(), d.L, d.n_scan, d.n, d.code, d.max_iter,
            d.tol, d.pose0.data_ptr(), g._h if g is not None else None, d.got.data_ptr() if d.got is not None and g is not None else None,
            None, d.poses.data_ptr(), d.T.data_ptr(), d.iters.data_ptr()))

    def state_words(self):
        """The grid object's whole state as one int32 tensor: slam_grid_create's single allocation [pass | hit | visit
        slots] of K.grid_state_bytes(...) bytes, which starts where the pass counters do."""
        import torch
        g = self.grid
        p, h = g.counters_torch()
        nbytes = K.grid_state_bytes(g.G, g.xw, g.yw)
        plane = h.data_ptr() - p.data_ptr()
        assert plane >= g.G * g.xw * g.yw * 4 and plane % 256 == 0 and nbytes - 2 * plane == K.grid_state_bytes(1, 1, 1) - 2 * 256

        class View:
            __cuda_array_interface__ = {"shape": (nbytes // 4,), "typestr": "<i4", "data": (p.data_ptr(), False), "version": 2}
        return torch.as_tensor(View(), device=self.dr.dev)

    def dirty(self, other):
        """Step 1: a replay of other scans, then the pattern into every word of the state - the counters of every map,
        the padding behind them and the visit slots, those the other replay's few workgroups did not use included."""
        import torch
        o = self.slam.DeviceReplay(other, AMIN, AMAX)
        o.ctx.close()
        o.ctx = self.ctx
        self.ctx.set_option("replay_reset", 0)
        self.replay_dev(o)
        assert self.grid.visits() > 0
        self.state_words().fill_(PATTERN)
        torch.cuda.synchronize()
        for plane in self.grid.counters_torch():
            assert bool((plane == PATTERN).all())
        assert self.grid.visits() != 0

    def collect(self, dr=None):
        poses, T, it = (dr or self.dr).results()
        out = dict(poses=poses, T=T, iters=it)
        if self.grid is not None:
            maps = [self.grid.read(g, want=("pmap", "pass", "hit")) for g in range(self.grid.G)]
            out.update({k: np.stack([m[k] for m in maps]) for k in ("pmap", "pass", "hit")}, visits=self.grid.visits())
        return out

    def close(self):
        self.ctx.synchronize()
        self.ctx.check_status()
        if self.grid is not None:
            self.grid.close()
        self.ctx.close()


def fresh(slam, ranges, options=None, **kw):
    """The expectation: the replay on a fresh context into a fresh grid, "replay_reset" 0."""
    r = Run(slam, ranges, options, **kw)
    r.ctx.set_option("replay_reset", 0)
    r.replay_dev()
    out = r.collect()
    r.close()
    return out


def reset_run(slam, ranges, other, options=None, **kw):
    """Steps 1 to 3 on one context."""
    r = Run(slam, ranges, options, **kw)
    r.dirty(other)
    r.ctx.set_option("replay_reset", 1)
    r.replay_dev()
    out = r.collect()
    r.close()
    return out


RESULTS = ("poses", "T", "iters")
MAPS = ("pass", "hit", "pmap")


def same(got, want, keys=RESULTS + MAPS):
    """Bit for bit; with the maps, the visit count as well."""
    for k in keys:
        assert got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (k, int(np.sum(got[k] != want[k])))
    if "pass" in keys:
        assert got["visits"] == want["visits"], (got["visits"], want["visits"])


_ORACLE = {}


def against_oracle(want, ranges, key, xw=K.XW, yw=K.YW, reso=K.RESO, max_iter=30, g=0, l=0):
    """The expectation of trajectory l into map g against the C oracle, as test_replay_200_scans_vs_oracle; the oracle's
    answer is kept by ``key`` (the five forms share their drives).  Returns the oracle's visit count."""
    if key not in _ORACLE:
        og = checks.metric_grid(xw, yw, reso)
        _ORACLE[key] = (og,) + tuple(co.replay(ranges, AMIN, AMAX, og, max_iter=max_iter, threads=8))
    og, oposes, oT, oit, visits = _ORACLE[key]
    assert np.array_equal(want["iters"][l], oit)
    assert np.max(np.abs(want["poses"][l] - oposes)) < FTOL and np.max(np.abs(want["T"][l] - oT)) < FTOL
    assert np.array_equal(want["pass"][g], og.pass_cnt) and np.array_equal(want["hit"][g], og.hit_cnt)
    assert np.array_equal(want["pmap"][g], og.pmap)
    return visits


# ------------------------------------------------------------------ the table: every form at the edges of the loop
@pytest.mark.parametrize("case", K.cases() + K.preferred_cases(), ids=K.case_id)
def test_reset_at_the_edges_of_the_clearing_loop(slam, scans, case):
    ranges = scans["main"][:case.pairs + 1]
    side = K.XW if case.kind != "preferred_trips" else K.PREFERRED_MAP
    grid = (1, side, side, K.RESO)
    want = fresh(slam, ranges, case.options, grid=grid)
    assert want["visits"] == against_oracle(want, ranges, (case.pairs, side), side, side)
    assert want["visits"] > 0 and np.any(want["pass"] == 0)            # (cells the replay does not touch: where a residue would stay)
    same(reset_run(slam, ranges, scans["other"], case.options, grid=grid), want)


# ------------------------------------------------------------------ several maps, of which the trajectories write two
def test_a_map_no_trajectory_writes_comes_back_zero(slam, scans):
    m = K.MANY
    grid, got = (m["G"], m["xw"], m["yw"], m["reso"]), list(m["grid_of_traj"])
    want = fresh(slam, scans["two"], grid=grid, grid_of_traj=got)
    visits = sum(against_oracle(want, scans["two"][l], ("two", l), m["xw"], m["yw"], m["reso"], g=g, l=l) for l, g in enumerate(got))
    assert want["visits"] == visits
    out = reset_run(slam, scans["two"], scans["other"], grid=grid, grid_of_traj=got)
    same(out, want)
    assert not out["pass"][1].any() and not out["hit"][1].any() and np.all(out["pmap"][1] == 50)     # as slam_grid_reset leaves it
    assert out["pass"][0].any() and out["pass"][2].any()


# ------------------------------------------------------------------ storage types, zero iterations
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_reset_with_reduced_point_storage(slam, scans, dtype):
    ranges = scans["main"][:6]
    want = fresh(slam, ranges, dtype=dtype)
    assert want["visits"] > 0
    same(reset_run(slam, ranges, scans["other"], dtype=dtype), want)


def test_reset_with_zero_iterations(slam, scans):
    """max_iter = 0: the scan matcher's lanes have nothing to solve and still clear."""
    ranges = scans["main"][:6]
    want = fresh(slam, ranges, max_iter=0)
    assert want["visits"] == against_oracle(want, ranges, "max_iter 0", max_iter=0) and not want["iters"].any()
    same(reset_run(slam, ranges, scans["other"], max_iter=0), want)


# ------------------------------------------------------------------ the two routes through slam_grid_reset
def test_reset_of_a_grid_with_a_live_pmap(slam, scans):
    import torch
    ranges = scans["main"][:6]
    want = fresh(slam, ranges)
    r = Run(slam, ranges, live=True)
    r.dirty(scans["other"])
    r.ctx.set_option("replay_reset", 1)
    r.replay_dev()
    out = r.collect()                                        # (reading the pmap brings the live one up to date)
    same(out, want)

    class View:
        def __init__(self, ptr):
            self.__cuda_array_interface__ = {"shape": (1, K.XW, K.YW), "typestr": "|i1", "data": (int(ptr), False), "version": 2}
    live = torch.as_tensor(View(r.grid.live_pmap()), device=r.dr.dev).cpu().numpy()
    assert np.array_equal(live, want["pmap"]) and np.all(live[(want["pass"] + want["hit"]) == 0] == 50)
    r.close()


def test_reset_on_the_map_stream_behind_a_main_stream_update(slam, scans):
    """ "pipeline" = 1: the reset is slam_grid_reset on the map stream.  The map is dirtied once more by a main-stream
    slam_grid_update_dev immediately before the replay, with no synchronise in between: the reset has to wait for it."""
    import torch
    ranges = scans["main"][:6]
    want = fresh(slam, ranges)
    r = Run(slam, ranges, {"pipeline": 1})
    r.dirty(scans["other"])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(r.dr.dev)        # noqa: E731
    ox, oy = up(np.linspace(-4.0, 4.0, 64)[None]), up(np.linspace(3.0, -3.0, 64)[None])
    cx, cy = up(np.array([0.5])), up(np.array([-0.5]))
    torch.cuda.synchronize()
    r.ctx.set_option("replay_reset", 1)
    r.A.check(r.A.lib().slam_grid_update_dev(r.ctx.handle, r.grid._h, ox.data_ptr(), oy.data_ptr(), cx.data_ptr(), cy.data_ptr(), 1, 64, None))
    r.replay_dev()
    r.ctx.synchronize()
    same(r.collect(), want)
    r.ctx.set_option("pipeline", 0)
    r.close()


# ------------------------------------------------------------------ host form, no grid
def test_reset_through_the_host_form(slam, scans):
    ranges = scans["main"][:6]
    want = fresh(slam, ranges)
    r = Run(slam, ranges)
    r.dirty(scans["other"])
    r.ctx.set_option("replay_reset", 1)
    poses, T, it = slam.replay_host(ranges, AMIN, AMAX, grid=r.grid, context=r.ctx)
    out = r.collect()
    out.update(poses=poses[None], T=T[None], iters=it[None])
    same(out, want)
    r.close()


def test_option_without_a_grid_touches_no_map(slam, scans):
    ranges = scans["main"][:6]
    want = fresh(slam, ranges, grid=None)
    r = Run(slam, ranges)                                    # a grid of this context that the call is NOT given
    r.dirty(scans["other"])
    r.ctx.set_option("replay_reset", 1)
    r.replay_dev(grid=False)
    out = r.collect()
    same(out, want, keys=RESULTS)
    assert np.all(out["pass"] == PATTERN) and np.all(out["hit"] == PATTERN)
    r.close()


# ------------------------------------------------------------------ on, off, on
def test_reset_on_off_on(slam, scans):
    ranges = scans["main"][:6]
    want = fresh(slam, ranges)
    r = Run(slam, ranges)
    r.dirty(scans["other"])
    for reset, times in ((1, 1), (0, 2), (1, 1)):
        r.ctx.set_option("replay_reset", reset)
        r.replay_dev()
        out = r.collect()
        same(out, want, keys=RESULTS)
        assert np.array_equal(out["pass"], times * want["pass"]) and np.array_equal(out["hit"], times * want["hit"]), (reset, times)
        assert out["visits"] == times * want["visits"], (reset, times)
    r.close()


def test_two_replays_on_one_context_each_get_the_reset_they_ask_for(slam, scans):
    """DeviceReplay.run(reset_grid=...) with two replays on ONE context (as test_pipelined_map_stage_is_bit_identical and
    tests/test_gpu_pipeline_order.py use them): the option is the context's, so what one replay set last says nothing to
    the other.  A clears, B accumulates on A, A clears again; then the owner sets the option behind both.
    (Red before DeviceReplay looked the option up on its context: B, which had never set it, left the context on A's 1
    and cleared the map it was asked to accumulate into.)"""
    ra, rb = scans["main"][:6], scans["main"][6:12]
    wa, wb = fresh(slam, ra), fresh(slam, rb)
    assert wa["pass"].tobytes() != wb["pass"].tobytes()
    r = Run(slam, ra)
    b = slam.DeviceReplay(rb, AMIN, AMAX)
    b.ctx.close()
    b.ctx, b.grid = r.ctx, r.grid
    r.dirty(scans["other"])
    r.dr.run(reset_grid=True)
    same(r.collect(), wa)
    b.run(reset_grid=False)
    out = r.collect(b)
    same(out, wb, keys=RESULTS)
    assert np.array_equal(out["pass"], wa["pass"] + wb["pass"]) and np.array_equal(out["hit"], wa["hit"] + wb["hit"])
    assert out["visits"] == wa["visits"] + wb["visits"]
    r.dr.run(reset_grid=True)
    same(r.collect(), wa)
    r.ctx.set_option("replay_reset", 1)                      # the context's owner, directly
    b.run(reset_grid=False)
    out = r.collect(b)
    assert np.array_equal(out["pass"], wa["pass"] + wb["pass"]) and out["visits"] == wa["visits"] + wb["visits"]
    r.ctx.set_option("replay_reset", 0)
    r.dr.run(reset_grid=True)
    same(r.collect(), wa)
    r.close()
