"""The conditions test_gpu_landmark_sizes.py puts on its inputs, checked without a GPU: the host class reaches 32
landmarks on the committed drive and holds 1e-10 under a nudge of 1e-12, the three beam counts sit on the 64 KiB
boundary of the extraction's LDS, and the empty scans straddle the 64-scan chunks of the kept-scan rule."""
import numpy as np
import pytest

import landmark_cases as lc
from conftest import load_golden, pkg

AMIN, AMAX = -3.14159, 3.14159


def test_drive_reaches_32_landmarks_and_is_stable():
    drive = lc.grid_drive(1)
    assert len(drive["u"]) == lc.GRID_STEPS >= 32
    states, worst = lc.nudge_stability(pkg("ekf_lm").EKF(), drive)
    assert worst < 1e-10, worst
    x, P, nlm, status = states[-1]
    assert status == 0 and nlm[-1] == lc.MAX_LM and len(x) == 67 and len(states) == lc.GRID_STEPS + 1
    assert nlm[:32] == list(range(1, 33))                                  # one new landmark a step, none lost
    assert [lc.first_step_with(states, c) for c in (15, 16, 31, 32)] == [15, 16, 31, 32]
    assert max(len(zs) for zs in drive["z"]) == 22 and np.linalg.cond(P) < 1e3
    yaw = np.cumsum([u[2] for u in drive["u"]])
    assert yaw[-1] > 2 * np.pi


def test_lds_bytes_around_64_kib():
    assert [lc.landmark_lds_bytes(n) for n in (2047, 2048, 4096)] == [65520, 65552, 131088]
    assert lc.landmark_lds_bytes(2047) <= 65536 < lc.landmark_lds_bytes(2048)
    for n in (2047, 2048, 4096):
        assert lc.row_of_length(n).shape == (n,)


@pytest.mark.parametrize("k,tail,closed", [(255, (9.0, 9.01), 510), (257, (9.0, 9.01), 514), (512, (9.0, 9.01), 1024),
                                           (128, (), 255), (128, (9.0, 9.01), 256), (128, (9.0, 5.0, 5.01), 257)])
def test_pole_rows_have_the_clusters_they_are_named_for(k, tail, closed):
    row = lc.pole_row(k, tail=tail).astype(np.float64)
    labels, found = pkg("extraction").Extraction().labels(np.vstack([row, np.zeros_like(row)]))
    gaps = np.abs(np.diff(row))
    assert len(found) == k and int((gaps >= 1.0).sum()) == closed


def test_empty_scans_straddle_the_chunks(syn):
    a, b, c = (set(p) for p in lc.EMPTY_AT)
    assert {62, 63, 64, 65, 127, 128} == a and b == set(range(1, 64)) and c == {lc.N_SCAN - 1} and lc.N_SCAN > 128
    world = syn.World(5.0, 4.0, ((1.5, 1.0), (-1.8, -0.9), (0.5, -2.0), (-2.5, 1.5)), 0.08)
    empty = np.full(360, np.inf, dtype=np.float32)
    ex = pkg("extraction").Extraction()
    for l, places in enumerate(lc.EMPTY_AT):
        real = lc.N_SCAN - len(places)
        scans = lc.with_empties_at(syn.scans_from_poses(world, syn.trajectory(world, real * 5, 5 + l)[::5], 360, 5 + l), places, empty)
        counts = lc.host_counts(ex, scans, AMIN, AMAX)
        assert len(counts) == lc.N_SCAN
        assert lc.kept_rule(counts) == [k for k in range(lc.N_SCAN) if k not in places]


def test_crowded_scan_overflows_and_node_counts():
    scans = np.array(load_golden("g7_w12_node.npz")["node_ranges"][4::5], dtype=np.float32)
    ex = pkg("extraction").Extraction()
    assert lc.host_counts(ex, scans, AMIN, AMAX) == [4, 4, 4, 4, 3, 4, 3, 4, 3, 4, 5, 4, 4]
    assert lc.host_counts(ex, lc.crowded_scan(scans[0])[None], AMIN, AMAX)[0] > 5
