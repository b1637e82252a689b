"""slam_track's restatement (tests/track_ref.py) and its seeded cases (tests/track_cases.py) on the host, no GPU: the
binding's third header; ``match_fast`` pinned to ``match_ref.match``; the two "tracks better than odometry" cases of the
issue on the restatement; why the gate exists; the restatement's gate against a literal loop; and which edges the default
seeds reach."""
import math

import numpy as np

import match_ref as M
import track_cases as C
import track_ref as T
from conftest import pkg


def test_third_header_is_bound():
    abi = pkg("_abi")
    assert sorted(abi._SIGS_TRACK) == ["slam_track", "slam_track_dev"]
    assert not set(abi._SIGS_TRACK) & (set(abi._SIGS) | set(abi._SIGS_REFINE))
    assert abi._SIGS_TRACK["slam_track"] == abi._SIGS_TRACK["slam_track_dev"] and len(abi._SIGS_TRACK["slam_track"][0]) == 29
    assert (abi.TRACK_MATCHED, abi.TRACK_REFINED, abi.TRACK_INTEGRATED, abi.TRACK_LOST) == (T.MATCHED, T.REFINED, T.INTEGRATED, T.LOST)
    p = pkg()
    defaults = dict(p.tracker.DEFAULTS)
    assert defaults.pop("step") is None                       # one cell of the grid it is given
    assert defaults == T.DEFAULTS


def test_match_fast_is_match_ref():
    rng = np.random.default_rng(5)
    for shape, rule, n, K, nx, ny in (((33, 17), (10.0, 2.0, 3.0), 37, 3, 2, 1), ((8, 8), (1.0, 0.0, 0.0), 65, 1, 0, 0), ((40, 65), (10.0, 2.0, 3.0), 9, 5, 1, 3)):
        pm = np.full(shape, 50, dtype=np.int8)
        pm[rng.random(shape) < 0.1] = 100
        fld = M.field(pm, 64)
        th = np.linspace(-3.0, 3.0, n)
        r = rng.uniform(0.5 / rule[0], 20.0 / rule[0], n).astype(np.float32)
        r[1], r[2], r[3] = np.inf, np.nan, 1.0e6
        rot = T.rot_table(math.cos(0.3), math.sin(0.3), T.rotations(K, 0.05)[1])
        for centre in ((shape[0] / 2 / rule[0] - rule[1], shape[1] / 3 / rule[0] - rule[2]), (-1.0e3, 0.0), (np.nan, 0.0), (4.0e6, 0.0)):
            want = M.match(fld, *rule, r, centre, np.cos(th), np.sin(th), rot, nx, ny, 1.0 / rule[0], 15.0 / rule[0], 64)
            got = T.match_fast(fld, *rule, r, centre, np.cos(th), np.sin(th), rot, nx, ny, 1.0 / rule[0], 15.0 / rule[0], 64)
            assert got == want[:3], (shape, centre, got, want[:3])


def report(syn, name, gate=None):
    c = T.case_inputs(syn, name)
    poses, info = T.run_case(syn, name, gate)
    ep, eh = T.errors(poses, c["true"])
    dp, dh = T.errors(c["dead"], c["true"])
    print("%s gate %s: tracker max %.4f m %.4f rad, final %.4f m; dead reckoning final %.3f m %.3f rad; %d scans integrated"
          % (name, gate, ep.max(), eh.max(), ep[-1], dp[-1], dh[-1], int(((info[:, 3] & T.INTEGRATED) != 0).sum())))
    return ep, eh, dp, dh


def test_restatement_tracks_better_than_odometry(syn):
    """The issue's two cases at the defaults: the largest error over the run within (0.10 m, 0.03 rad), the final position
    error below a tenth of dead reckoning's (0.59 m and 0.63 m)."""
    for name in ("dense", "sparse"):
        ep, eh, dp, _dh = report(syn, name)
        assert abs(dp[-1] - T.CASES[name]["dead_end"]) < 0.005
        assert ep.max() <= T.BOUND[0] and eh.max() <= T.BOUND[1], (name, ep.max(), eh.max())
        assert ep[-1] < 0.1 * dp[-1], (name, ep[-1], dp[-1])


def test_why_the_gate_exists(syn):
    """120 beams with every scan integrated ends worse than behind the (0.2 m, 0.1 rad) gate: a map that takes every
    refined scan follows the tracker's own error."""
    gated, _, _, _ = report(syn, "sparse")
    every, _, _, _ = report(syn, "sparse", gate=(0.0, 0.0))
    assert every[-1] > gated[-1] and every.max() > T.BOUND[0] >= gated.max(), (every[-1], gated[-1], every.max(), gated.max())


def test_gate_flags_equal_a_literal_loop(syn):
    for name in ("dense", "sparse"):
        poses, info = T.run_case(syn, name)
        key, want = None, []
        for s in range(len(poses)):
            if key is None:
                go = True
            else:
                dx, dy, dth = poses[s] - key
                go = dx * dx + dy * dy >= 0.2 * 0.2 or abs(dth) >= 0.1
            if go:
                key = poses[s]
            want.append(go)
        assert [bool(f & T.INTEGRATED) for f in info[:, 3]] == want
        assert all(f & T.MATCHED for f in info[1:, 3]) and info[0, 3] == T.INTEGRATED
    assert not T.gate((np.nan, 0, np.nan), (0, 0, 0), 0.0, 0.0) and not T.gate((9, 9, 9), (0, 0, 0), np.inf, np.inf)
    assert T.gate((0, 0, 0), (0, 0, 0), 0.0, 0.0)


def test_default_seeds_reach_every_edge():
    reached = {}
    for seed in range(30):
        case = C.case_of(seed)
        out, _pass, _hit = C.ref_run(case)
        for e in C.edges_of(case, out):
            reached.setdefault(e, []).append(seed)
    for e in C.EDGES:
        print("%-50s %s" % (e, reached.get(e, [])))
    assert set(reached) == set(C.EDGES), set(C.EDGES) - set(reached)
    assert {C.case_of(s)["geom"] for s in range(30)} == set(C.RC.RULES)
    assert {C.case_of(s)["shape"] for s in range(30)} == set(C.RC.SHAPES)
    assert max(C.case_of(s)["ranges"].shape[0] for s in range(30)) == 3 and max(C.case_of(s)["ranges"].shape[1] for s in range(30)) <= 6


def test_plan_track_names():
    """The launch shapes of the tracker's own steps, through slam_plan_query (csrc/launch_shapes.h, plan_track)."""
    import ctypes
    lib = pkg("_abi").lib()

    def plan(name, a=0):
        out = ctypes.c_int64(0)
        assert lib.slam_plan_query(name.encode(), int(a), 0, 0, -1, ctypes.byref(out)) == 0, name
        return out.value
    cap, lanes = plan("kTrackMaxBlocks"), plan("kTrackThreads")
    assert plan("kTrackRowThreads") == plan("kWave") and lanes == 256
    for L in (1, 3, 255, 256, 257, cap - 1, cap, cap + 1, cap * lanes + 1, 2 ** 31 - 1):
        assert plan("track_rows", L) == min(L, cap)
        assert plan("track_lanes", L) == min((L + lanes - 1) // lanes, cap)
    assert plan("track_rows", 0) == 0 and plan("track_lanes", 0) == 0
