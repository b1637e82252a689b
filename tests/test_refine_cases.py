"""The two restatements of slam_grid_refine against each other, and the NumPy one on the synthetic room (no GPU).

The 50-digit run is the truth; the NumPy run's deviation from it over the sure default cases is E, the unit of the
device's allowance (tests/refine_cases.py).  This file holds the conditions under which the cases are accepted: at most
2 % of the seeds unsure, E within the constants, every edge of the list reached."""
import numpy as np

import match_ref as MR
import refine_cases as RC
import refine_ref as R


def test_numpy_against_50_digits_and_the_constants():
    E, unsure = [0.0, 0.0, 0.0], []
    for seed in RC.seeds():
        case, want = RC.case_of("refine", seed), RC.answer_mp(seed)
        got = RC.answer(case, R.refine)
        if not RC.sure(want):
            unsure.append((seed, float(want["margin"].min())))
            continue
        E = [max(a, b) for a, b in zip(E, RC.deviation(got, want))]
    print("E pose %.3g cost %.3g normal %.3g; unsure %s" % (E[0], E[1], E[2], unsure))
    assert len(unsure) <= 0.02 * len(RC.seeds())
    assert E[0] <= RC.E_POSE and E[1] <= RC.E_COST and E[2] <= RC.E_NORMAL
    assert RC.ALLOW_POSE <= 1e-9 and RC.ALLOW_POSE == 16 * RC.E_POSE        # the allowance is 16 E, not the project's cap


def test_default_seeds_reach_every_edge():
    reached, iters, beams = {}, set(), set()
    for seed in RC.seeds():
        case = RC.case_of("refine", seed)
        iters.add(case["iters"])
        beams.add(len(case["ct"]))
        for e in RC.edges_of(case, RC.answer_mp(seed)):
            reached.setdefault(e, []).append(seed)
    print({e: len(s) for e, s in reached.items()})
    if len(RC.seeds()) >= 60:
        assert set(reached) == set(RC.EDGES)
        assert iters == set(RC.ITERS) and beams == set(RC.BEAMS)
        assert {RC.case_of("refine", s)["pmaps"].shape[1:] for s in RC.seeds()} == set(RC.SHAPES)


def test_unanswered_rows_and_nothing_occupied():
    """What the contract says of the rows without an answer, and of a map where the field is flat: g = 0, H = 0 and the pose
    stays where it was, bit for bit."""
    seen = 0
    for seed in RC.seeds():
        case, ans = RC.case_of("refine", seed), RC.answer(RC.case_of("refine", seed), R.refine)
        for b in range(len(case["poses"])):
            g = case["maps"][b]
            if not 0 <= g < len(case["pmaps"]):
                assert ans["status"][b] == R.NO_MAP
            elif not np.isfinite(case["poses"][b]).all():
                assert ans["status"][b] == R.BAD_POSE
            else:
                assert ans["status"][b] == R.OK
            if ans["status"][b] != R.OK:
                assert np.array_equal(ans["pose"][b], case["poses"][b], equal_nan=True) and np.all(ans["cost"][b] == -1.0)
                assert not ans["normal"][b].any() and ans["used"][b] == 0
            elif not (case["pmaps"][g] == 100).any() or ans["used"][b] == 0:
                seen += 1
                assert not ans["normal"][b].any() and ans["pose"][b].tobytes() == case["poses"][b].tobytes()
                assert ans["cost"][b][0] == ans["cost"][b][1] and (ans["used"][b] > 0 or ans["cost"][b][0] == 0.0)
                assert abs(ans["cost"][b][0] - ans["used"][b] * float(case["cap"])) <= 1e-12 * max(1, ans["used"][b]) * case["cap"]
    assert seen > 0 or len(RC.seeds()) < 60


ROOM = dict(xw=240, scale=20.0, off=6.0, scans=40, beams=360, cap=64)
_room = {}


def room(syn):
    """The issue's prototype setting: 40 scans of 360 beams in the synthetic room, a 240 x 240 map at 0.05 m whose occupied
    cells are the cells of the ideal end points, starts off by up to a cell in x and y and 0.01 rad in heading."""
    if not _room:
        rep = syn.make_replay(ROOM["scans"], ROOM["beams"], seed=4)
        ranges, poses = np.asarray(rep.ranges, dtype=np.float32), np.asarray(rep.poses_true, dtype=np.float64)
        ang = np.linspace(rep.angle_min, rep.angle_max, ROOM["beams"])
        ct, st = np.cos(ang), np.sin(ang)
        pm = np.full((ROOM["xw"], ROOM["xw"]), 50, dtype=np.int8)
        for r, p in zip(ranges, poses):
            rr = r[np.isfinite(r)].astype(np.float64)
            lx, ly = ct[np.isfinite(r)] * rr, st[np.isfinite(r)] * rr
            x, y = np.cos(p[2]) * lx - np.sin(p[2]) * ly + p[0], np.sin(p[2]) * lx + np.cos(p[2]) * ly + p[1]
            i, j = (ROOM["scale"] * (x + ROOM["off"])).astype(int), (ROOM["scale"] * (y + ROOM["off"])).astype(int)
            assert i.min() >= 0 and j.min() >= 0 and i.max() < ROOM["xw"] and j.max() < ROOM["xw"]
            pm[i, j] = 100
        rng = np.random.default_rng(7)
        cell = 1.0 / ROOM["scale"]
        off = np.stack([rng.uniform(-cell, cell, len(poses)), rng.uniform(-cell, cell, len(poses)), rng.uniform(-0.01, 0.01, len(poses))], axis=1)
        _room.update(ranges=ranges, poses=poses, ct=ct, st=st, pmap=pm, field=MR.field(pm, ROOM["cap"]), starts=poses + off, amin=rep.angle_min,
                     amax=rep.angle_max)
    return _room


def test_room_cost_never_rises_and_heading_improves(syn):
    """Ten iterations of the restatement on the prototype's setting.  The prototype (issue): never above the start's cost,
    mean heading error 6e-3 -> 2e-4.  This restatement on these starts: 0 of 40 above, 5.0e-3 -> 8.2e-4 (0.16 of the
    start's); the mark is a quarter.  x and y are not compared with the truth: they keep the map's own bias."""
    rm = room(syn)
    res = [R.refine(rm["field"], ROOM["scale"], ROOM["off"], ROOM["off"], rm["ranges"][k], rm["starts"][k], rm["ct"], rm["st"], 10, 1e-3,
                    0.5, 0.02, 30.0, ROOM["cap"]) for k in range(ROOM["scans"])]
    cost = np.array([r["cost"] for r in res])
    e0 = np.abs(rm["starts"][:, 2] - rm["poses"][:, 2])
    e1 = np.abs(np.array([r["pose"][2] for r in res]) - rm["poses"][:, 2])
    print("above the start: %d; mean heading error %.3g -> %.3g" % (int((cost[:, 1] > cost[:, 0]).sum()), e0.mean(), e1.mean()))
    assert np.all(cost[:, 1] <= cost[:, 0])
    assert e1.mean() < 0.25 * e0.mean()
