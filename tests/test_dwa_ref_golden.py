"""The NumPy DWA oracle (tests/dwa_ref.py) reproduces the reference's own dwa.py exactly on
the recorded cases of tests/golden/g11_dwa.npz (tools/gen_dwa_golden.py): controls,
trajectories, sample counts and every sample's cost, inf and NaN included."""
import numpy as np
import pytest

import dwa_ref
from conftest import load_golden


@pytest.fixture(scope="module")
def g11():
    return load_golden("g11_dwa.npz")


def config_of(g, k):
    return dict(zip(dwa_ref.FIELDS, (float(v) for v in g["configs"][k])))


def test_golden_has_the_cases_the_spec_names(g11):
    names = [str(n) for n in g11["names"]]
    assert len(names) >= 40
    for want in ("edge_own_cell", "edge_sentinel_only", "edge_nan_goal", "edge_empty_window", "pt1.0_rt0", "pt0.3_rt1",
                 "dt0.05_rt1", "obgain0_rt0"):
        assert want in names, want
    rt = g11["configs"][:, dwa_ref.FIELDS.index("robot_type")]
    assert set(rt.tolist()) == {0.0, 1.0}
    k = names.index("edge_own_cell")
    assert g11["index"][k] == g11["nv"][k] * g11["nw"][k] - 1 and np.isinf(g11["cost"][k])
    for e in ("edge_nan_goal", "edge_empty_window", "edge_obgain0_all_hit"):
        k = names.index(e)
        assert g11["index"][k] == -1 and g11["traj_rows"][k] == 1 and np.array_equal(g11["u"][k], [0.0, 0.0])
    # non-edge cases leave a margin between the best and the second-best sample
    edge = np.array([n.startswith("edge") for n in names])
    assert np.all(g11["gap"][~edge] > 1e-9)


def test_oracle_reproduces_the_reference_exactly(g11):
    for k, name in enumerate(g11["names"]):
        c = config_of(g11, k)
        ob = g11["ob"][k, :g11["ob_count"][k]]
        r = dwa_ref.plan(g11["states"][k], c, g11["goals"][k], ob)
        assert (r["nv"], r["nw"]) == (g11["nv"][k], g11["nw"][k]), name
        S = r["nv"] * r["nw"]
        np.testing.assert_array_equal(r["costs"], g11["costs"][k, :S], err_msg=str(name))
        assert r["index"] == g11["index"][k], name
        assert np.array_equal(r["u"], g11["u"][k]), name
        rows = g11["traj_rows"][k]
        assert r["traj"].shape == (rows, 5), name
        np.testing.assert_array_equal(r["traj"], g11["traj"][k, :rows], err_msg=str(name))


def test_scan_preprocessing_gives_the_recorded_obstacles(g11):
    for k, name in enumerate(g11["names"]):
        if not g11["has_scan"][k]:
            continue
        c = config_of(g11, k)
        ob = dwa_ref.scan_obstacles(g11["scans"][k], float(g11["angle_min"]), float(g11["angle_increment"]),
                                    c["max_speed"] * c["predict_time"])
        np.testing.assert_array_equal(ob, g11["ob"][k, :g11["ob_count"][k]], err_msg=str(name))


def test_arange_rule_matches_numpy():
    rng = np.random.default_rng(3)
    for _ in range(2000):
        a = float(rng.uniform(-2, 2))
        b = a + float(rng.uniform(-0.05, 0.4))
        step = float(rng.choice([0.01, 100.0 * np.pi / 180.0 * 0.1 / 10.0]))
        np.testing.assert_array_equal(dwa_ref.arange(a, b, step), np.arange(a, b, step))
