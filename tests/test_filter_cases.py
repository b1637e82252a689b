"""The seeded cases of tests/filter_cases.py without a device: every case builds and the host class answers it in time, the
host class agrees with the 50-digit restatement of tests/ekf_ref.py on every trajectory the sweep calls sure, few
trajectories are unsure, and the sweep reaches the decisions it was written for.

The GPU file (tests/test_gpu_filter_properties.py) compares the device with the host class at 1e-9 on exactly these cases;
here the host class's x and P lie within REF_BOUND = 1e-11 of the true result of its own formulas, one hundredth of that, so
a device within 1e-9 of the host class is within 1.01e-9 of the truth.  What is asserted about the
default 60 seeds - observations with two landmarks under the gate that the lower index loses, distances next to the gate on
both sides, raises and early returns at step 0 and later, a yaw left outside [-pi, pi) that the next step starts from, stops
at max_lm 1 and 32, innovations that wrap - is what that file can be trusted to have exercised.  The thresholds are named
constants, set from what the host class reports here, never from a device.  The node's cases are answered by a host class
whose scan matcher and map are library calls, so only what the extraction decides (the lm_cap stops) is counted here; the
GPU file counts the node's max_lm stops and raises.  Every message carries (kind, seed)."""
import functools
import math
import time

import numpy as np
import pytest

import ekf_ref as E
import filter_cases as F
from test_map_cases import same_case
from test_plan_cases import same_value

DEFAULT = 60                                # the seeds over which the edge reach is asserted, whatever SLAM_HYP_EXAMPLES says
N = len(F.seeds())
ANSWER_SECONDS = 1.0                        # answer(case) of the host class, per seed on average
REF_SECONDS = 3.0                           # the 50-digit restatement, per seed on average
REF_BOUND = 1e-11                           # host class to 50-digit answer, on x and P of every sure trajectory
MARGIN_BOUND = 1e-9                         # the float64 margin to the 50-digit margin
UNSURE = 0.02                               # at most this share of the trajectories may be unsure
NEAR_GATE = 0.10                            # "next to the gate": within this share of 0.6 (a gate row aimed at 0.9 or 1.1
NEAR_SLACK = 1e-6                           # times the gate lands within its bisection's last step of the edge: the slack)
NEVER_UNSURE = ("gate", "burst", "cap")

# reach over the default seeds: about half of what the host class counted when this file was written
MIN_TWO_UNDER_GATE = 25                     # observations with >= 2 landmarks under the gate
MIN_LOWER_INDEX_LOSES = 12                  # ... of which the winner is not the lowest index under the gate
MIN_NEAR_GATE_EACH_SIDE = 8
MIN_GATE_ROWS = 12                          # gate trajectories whose bisected row was kept
MIN_EARLY_LATER, MIN_RAISE_LATER = 50, 3    # at a step after 0
MIN_YAW_LEFT_OUTSIDE = 4
MIN_YAW_LEFT_AT_THE_END = 3                 # ... on the last step of a trajectory, where it is an output
MIN_WRAPS = 5000
MIN_NODE_OBS_STOPS = 4


@functools.lru_cache(maxsize=None)
def solved(n):
    """(cases, answers, seconds the host class took) of the ekf seeds 0 .. n - 1, worked out once."""
    cases = [F.case_of("ekf", s) for s in range(n)]
    t = time.perf_counter()
    answers = [F.answer(c) for c in cases]
    return cases, answers, time.perf_counter() - t


def default():
    cases, answers, _ = solved(max(N, DEFAULT))
    return list(zip(cases[:DEFAULT], answers[:DEFAULT]))


def sweep(n=None):
    cases, answers, _ = solved(max(N, DEFAULT))
    return list(zip(cases[:n or N], answers[:n or N]))


def trajectories(pairs):
    """(case, b, trajectory, its answer) over the trajectories of (case, answers) pairs."""
    return [(c, b, t, r) for c, a in pairs for b, (t, r) in enumerate(zip(c["trajs"], a))]


def tag(c, b=None):
    return (c["kind"], c["seed"]) if b is None else (c["kind"], c["seed"], "trajectory %d" % b, c["trajs"][b]["style"])


def show(name, value):
    print("reach %-34s %s" % (name, value))
    return value


# ------------------------------------------------------------------ the cases build, and in time
def test_cases_build_and_the_host_class_answers_in_time():
    cases, answers, seconds = solved(max(N, DEFAULT))
    print("ekf: %d host answers in %.2f s" % (len(cases), seconds))
    assert seconds < ANSWER_SECONDS * len(cases), seconds
    t = time.perf_counter()
    nodes = [F.case_of("node", s) for s in range(max(N, DEFAULT))]
    print("node: %d cases in %.2f s" % (len(nodes), time.perf_counter() - t))
    assert time.perf_counter() - t < ANSWER_SECONDS * len(nodes)


@pytest.mark.parametrize("kind", F.KINDS)
def test_a_case_is_a_pure_function_of_kind_and_seed(kind):
    for seed in (0, 7, 19, 20, 41, 57):
        a, b = F.case_of(kind, seed), F.case_of(kind, seed)
        assert all(same_value(a[k], b[k]) for k in a), (kind, seed)
    one, two = F.case_of(kind, 1), F.case_of(kind, 2)
    assert not all(same_value(one[k], two[k]) for k in one if k != "kind")
    assert same_case(F.packed(F.case_of("ekf", 7))["z"], F.packed(F.case_of("ekf", 7))["z"])


def test_kind_ids_are_apart_from_the_first_sweeps():
    import map_cases
    import plan_cases
    taken = set(map_cases.KIND_ID.values()) | set(plan_cases.KIND_ID.values())
    assert not set(F.KIND_ID.values()) & taken and min(F.KIND_ID.values()) == 201 and len(set(F.KIND_ID.values())) == len(F.KINDS)


def test_cases_stay_inside_their_bounds():
    styles = set()
    for c, a in sweep():
        p = F.packed(c)
        assert 1 <= c["B"] <= 5 and c["max_lm"] in F.MAX_LMS and len(c["trajs"]) == len(c["run"]) == c["B"], tag(c)
        assert p["u"].shape == (c["B"], p["steps"], 3) and p["z_off"].shape == (c["B"] * p["steps"] + 1,) and p["z_off"][-1] == len(p["z"]), tag(c)
        assert np.all(np.diff(p["z_off"]) >= 0) and np.all(np.isfinite(p["u"])) and np.all(np.isfinite(p["x0"])), tag(c)
        assert np.all(np.abs(p["x0"][:, 2]) <= math.pi), tag(c)
        for b, t in enumerate(c["trajs"]):
            assert 0 <= c["run"][b] <= len(t["u"]) == len(t["z"]) <= 64 and (t["style"] == "empty") == (len(t["u"]) == 0), tag(c, b)
            assert t["noise"][0] in F.RANGE_NOISE and (t["noise"][1] in F.BEARING_NOISE or t["style"] == "wrap"), tag(c, b)
            finite = all(np.all(np.isfinite(zs)) for zs in t["z"])
            assert finite or (b == c["spoiled"] and c["seed"] % 10 == 7), tag(c, b)
            styles.add(t["style"])
        assert (c["spoiled"] is not None) == (c["seed"] % 10 == 7), tag(c)
    assert styles >= set(F.STYLES) | {"empty"}
    yaws = np.array([c["trajs"][0]["x0"][2] for c, _ in default()])
    assert yaws.min() < -2.5 and yaws.max() > 2.5 and np.sum(yaws > 0) > 15 and np.sum(yaws < 0) > 15       # the full circle
    ragged = sum(1 for c, _ in default() if len({len(t["u"]) for t in c["trajs"]}) > 1)
    short = sum(1 for c, _ in default() for b, t in enumerate(c["trajs"]) if c["run"][b] < len(t["u"]))
    empty = sum(1 for c, _ in default() for t in c["trajs"] if t["style"] == "empty")
    assert show("calls of ragged length", ragged) >= 20 and show("step counts below the rows", short) >= 10 and show("empty", empty) >= 8
    for s in range(max(N, DEFAULT)):
        c = F.case_of("node", s)
        assert 1 <= c["L"] <= 3 and 6 <= c["n_scan"] <= 14 and c["n"] in F.NODE_BEAMS and c["side"] in F.NODE_MAPS, tag(c)
        assert c["ranges"].shape == (c["L"], c["n_scan"], c["n"]) and c["ranges"].dtype == np.float32 and not np.any(np.isnan(c["ranges"])), tag(c)
        for w in c["worlds"]:
            assert w["pair_gap"] < 1.0 and 2 <= w["enter"] < c["n_scan"], tag(c)


# ------------------------------------------------------------------ the host class against 50 digits
@functools.lru_cache(maxsize=None)
def restated(n):
    """{(seed, b): ekf_ref.run of the steps that run} for the sure trajectories of seeds 0 .. n - 1, and the seconds."""
    t = time.perf_counter()
    out = {}
    for c, b, tr, r in trajectories(sweep(n)):
        if r["sure"]:
            run = c["run"][b]
            out[c["seed"], b] = E.run(tr["u"][:run], tr["z"][:run], tr["x0"], c["max_lm"])
    return out, time.perf_counter() - t


def far_from(x, P, e):
    """The largest distance of the float64 x and P from the 50-digit entry ``e``."""
    n = len(x)
    dx = max(abs(E.mpf(float(x[i])) - e["x"][i]) for i in range(n))
    dP = max(abs(E.mpf(float(P[i, j])) - e["P"][i][j]) for i in range(n) for j in range(n))
    return float(max(dx, dP))


def test_the_host_class_agrees_with_50_digits_on_every_sure_trajectory():
    n = max(N, DEFAULT)
    refs, seconds = restated(n)
    worst, worst_margin, where, compared = 0.0, 0.0, None, 0
    for c, b, tr, r in trajectories(sweep(n)):
        if not r["sure"]:
            continue
        ref = refs[c["seed"], b]
        assert len(ref) == len(r["steps"]), tag(c, b) + ("steps",)
        margin = E.mpf("inf")
        for k, ((x, P, log), e) in enumerate(zip(r["steps"], ref)):
            stopped = k == len(r["steps"]) - 1 and r["status"] != F.OK
            rows = e["rows"]
            assert [(i, w) for _, i, w in log] == [(i, w) for _, i, w in rows], tag(c, b) + ("step %d" % k, "branch or index")
            margin = min(margin, E.margin(rows))
            for (d, _, _), (dr, _, _) in zip(log, rows):
                assert len(d) == len(dr), tag(c, b) + ("step %d" % k,)
            if stopped:
                assert e["status"] == r["status"] and rows[-1][2] == ("raises" if r["status"] == F.RAISES else "appended"), tag(c, b)
            else:
                assert e["status"] == 0 and e["nlm"] == r["nlm"][k], tag(c, b) + ("step %d" % k, "count or status")
                d = far_from(x, P, e)
                if d > worst:
                    worst, where = d, tag(c, b) + ("step %d" % k,)
                assert d < REF_BOUND, tag(c, b) + ("step %d" % k, d)
        compared += 1
        if math.isfinite(r["margin"]):
            worst_margin = max(worst_margin, abs(float(E.mpf(r["margin"]) - margin)))
            assert abs(E.mpf(r["margin"]) - margin) < MARGIN_BOUND, tag(c, b) + (r["margin"], float(margin))
        else:
            assert margin == E.mpf("inf"), tag(c, b)
    print("host class to 50 digits over %d sure trajectories of %d seeds: worst %.3g at %s; margins agree to %.3g; %.1f s"
          % (compared, n, worst, where, worst_margin, seconds))
    assert compared > 2 * n and seconds < REF_SECONDS * n, (compared, seconds)


# ------------------------------------------------------------------ few are unsure
def unsure_share(pairs):
    finite = [(c, b, t, r) for c, b, t, r in trajectories(pairs) if r["finite"]]
    unsure = [(c, b, t, r) for c, b, t, r in finite if not r["sure"]]
    return len(unsure) / max(len(finite), 1), unsure, len(finite)


def test_few_trajectories_are_unsure_and_none_of_the_aimed_ones():
    for name, pairs in (("default", default()), ("sweep", sweep())):
        share, unsure, total = unsure_share(pairs)
        print("unsure share, %s: %d of %d trajectories = %.2f %%  %s" % (name, len(unsure), total, 100 * share,
              [tag(c, b) + (r["margin"], r["moved"]) for c, b, t, r in unsure]))
        assert share <= UNSURE, (name, share)
        for c, b, t, r in unsure:
            assert t["style"] not in NEVER_UNSURE, tag(c, b) + (r["margin"], r["moved"])
    spoiled = [(c, b, t, r) for c, b, t, r in trajectories(default()) if not r["finite"]]
    assert {t["spoiled"][1] for c, b, t, r in spoiled} == set(F.NONFINITE)
    for c, b, t, r in spoiled:                                          # only the trajectory that was given such a row
        assert b == c["spoiled"], tag(c, b)
    for c, a in default():                                               # ... and the one that was given it shows it, or stopped before
        if c["spoiled"] is not None:
            t, r = c["trajs"][c["spoiled"]], a[c["spoiled"]]
            assert not r["finite"] or t["spoiled"][1] == "zero", tag(c, c["spoiled"])      # (a zero range may match a landmark)


# ------------------------------------------------------------------ the edges the sweep reaches
def decisions(pairs):
    """(case, b, step, dists, chosen, branch, trajectory's answer) over every decision of the finite, sure trajectories."""
    return [(c, b, k, d, i, w, r) for c, b, t, r in trajectories(pairs) if r["sure"]
            for k, (_, _, log) in enumerate(r["steps"]) for d, i, w in log]


def test_several_landmarks_under_the_gate_and_the_first_minimum():
    two = [(d, i) for _, _, _, d, i, _, _ in decisions(default()) if sum(v < F.GATE for v in d[:-1]) >= 2]
    loses = [(d, i) for d, i in two if i != min(j for j, v in enumerate(d[:-1]) if v < F.GATE)]
    assert show("two or more under the gate", len(two)) >= MIN_TWO_UNDER_GATE
    assert show("... the lowest index loses", len(loses)) >= MIN_LOWER_INDEX_LOSES
    for d, i in two:
        assert d[i] == min(d) and d.index(min(d)) == i


def test_distances_next_to_the_gate_on_both_sides():
    lo = hi = 0
    for _, _, _, d, _, _, _ in decisions(default()):
        lo += sum(1 for v in d[:-1] if v < F.GATE and 1.0 - v / F.GATE <= NEAR_GATE + NEAR_SLACK)
        hi += sum(1 for v in d[:-1] if v > F.GATE and v / F.GATE - 1.0 <= NEAR_GATE + NEAR_SLACK)
    assert show("distances just under the gate", lo) >= MIN_NEAR_GATE_EACH_SIDE
    assert show("distances just over the gate", hi) >= MIN_NEAR_GATE_EACH_SIDE
    kept = [(c, b, t, r) for c, b, t, r in trajectories(default()) if t["style"] == "gate" and t["factor"] is not None]
    assert show("gate rows kept", len(kept)) >= MIN_GATE_ROWS and {t["factor"] for _, _, t, _ in kept} == set(F.GATE_FACTORS)
    for c, b, t, r in kept:                                             # the row does what it was aimed to do
        if c["run"][b] == len(t["u"]) and len(r["steps"]) == len(t["u"]):
            d, i, w = r["steps"][-1][2][0]
            assert abs(d[t["gate_lm"]] / F.GATE - t["factor"]) < NEAR_SLACK, tag(c, b) + (d, t["factor"])
            assert (i == t["gate_lm"]) == (t["factor"] < 1.0), tag(c, b)


def test_raises_and_early_returns_at_step_0_and_later():
    seen = {(w, k > 0): 0 for w in ("early", "raises") for k in (0, 1)}
    for _, _, k, _, _, w, _ in decisions(default()):
        if w in ("early", "raises"):
            seen[w, k > 0] += 1
    show("early / raises at step 0, later", seen)
    assert seen["early", False] >= 3 and seen["raises", False] >= 1
    assert seen["early", True] >= MIN_EARLY_LATER and seen["raises", True] >= MIN_RAISE_LATER


def test_an_early_return_leaves_the_yaw_outside_and_the_next_step_starts_from_it():
    """... and trajectories end on such a step: only there is that yaw an output of the call (a later step wraps it, and
    everything else is periodic in it)."""
    left = last = 0
    for c, b, t, r in trajectories(default()):
        if not r["sure"]:
            continue
        done = len(r["nlm"])
        for k, (x, _, log) in enumerate(r["steps"][:done]):
            if log and log[-1][2] == "early":
                outside = abs(x[2]) > math.pi
                left += outside and k + 1 < len(r["steps"])
                last += outside and k + 1 == len(r["steps"])
            else:
                assert -math.pi <= x[2] < math.pi, tag(c, b)
    assert show("yaw left outside, a step follows", left) >= MIN_YAW_LEFT_OUTSIDE
    assert show("yaw left outside, the last step", last) >= MIN_YAW_LEFT_AT_THE_END


def test_stops_at_max_lm_1_and_32_and_innovations_that_wrap():
    stops = {m: 0 for m in F.MAX_LMS}
    exact = {m: 0 for m in F.MAX_LMS}
    for c, b, t, r in trajectories(default()):
        if r["sure"]:
            stops[c["max_lm"]] += r["status"] == F.LM_CAP
            exact[c["max_lm"]] += r["status"] == F.OK and bool(r["nlm"]) and r["nlm"][-1] == c["max_lm"]
            if r["status"] == F.LM_CAP:
                assert len(r["steps"]) < len(t["u"]) or t["style"] != "cap", tag(c, b)      # further steps behind the stop
    show("stops at max_lm, by max_lm", stops)
    show("reach max_lm exactly, by max_lm", exact)
    assert stops[1] >= 2 and stops[32] >= 1 and exact[1] >= 1 and exact[32] >= 1
    wraps = sum(r["wraps"] for _, _, _, r in trajectories(default()) if r["sure"])
    assert show("innovation bearings that wrap", wraps) >= MIN_WRAPS


def test_node_cases_that_stop_on_lm_cap():
    """What the extraction alone decides.  The stops on max_lm and the reference's raise need the node's scan matcher: the
    GPU file counts them over the same seeds."""
    stops = 0
    for s in range(DEFAULT):
        c = F.case_of("node", s)
        stops += sum(F.obs_stop(c, counts) is not None for counts in F.node_counts(c))
    assert show("node trajectories that stop on lm_cap", stops) >= MIN_NODE_OBS_STOPS
