"""The inputs of test_gpu_raycast_bounds.py (tests/raycast_cases.py) reach what they are there for - checked on the
reference alone, without a GPU, so that no GPU test passes for want of a beam of the right kind."""
import numpy as np
import pytest

import raycast_cases as K
import raycast_ref as R
from oracle import oracle_np as O

A_CASES = [g + (h,) for g in K.A_GEOMS for h in K.HIT_INCS]
A_IDS = ["%dx%d-s%g-hit%d" % (c[0], c[1], c[2], c[5]) for c in A_CASES]


def class_counts(cls):
    return np.bincount(np.asarray(cls).reshape(-1), minlength=7)


def check_mix(cls, ranges, flagged, what):
    """at least 8 beams in each of the six classes a finite pose can give; at least a third of the finite ray-cast
    answers on flagged lines and a third on unflagged"""
    counts = class_counts(cls)
    print(what, "classes (empty hit blocked free unknown out bad):", counts)
    for k in K.CLASSES6:
        assert counts[k] >= 8, (what, k, counts)
    fin = np.isfinite(ranges)
    on = int((fin & flagged).sum())
    print(what, "finite answers:", int(fin.sum()), "on flagged lines:", on)
    assert 3 * on >= fin.sum() > 0 and 3 * (fin.sum() - on) >= fin.sum(), (what, on, fin.sum())


def test_the_rules_and_the_pmap():
    assert K.table(20) == [1001] and K.table(4) == [1001, 601, 201]
    p = np.array([0, 0, 1, 1000, 1001, 600, 601, 200, 201, 0, 5])
    h = np.array([0, 1, 0, 0, 0, 1, 1, 2, 2, 3, 0])
    assert list(K.pmap_of(p, h, 4)) == [50, 0, 0, 0, 100, 0, 100, 0, 100, 100, 0]
    assert list(K.pmap_of(p, h, 20)) == [50, 100, 0, 0, 100, 100, 100, 100, 100, 100, 0]
    # the same rule as the oracle's own Mapping applies to its counters
    m = O.Mapping(1, len(p), 1.0, hit_inc=4.0)
    m.pass_cnt[0], m.hit_cnt[0] = p, h
    assert np.array_equal(m.pmap_from_counts()[0], K.pmap_of(p, h, 4))


@pytest.mark.parametrize("case", A_CASES, ids=A_IDS)
def test_a_maps_and_beams(case):
    xw, yw, scale, ox, oy, hit_inc = case
    c = K.case_a(*case)
    t = K.table(hit_inc)
    pass_, hit, thresh_cells = c["maps"][0]
    pm = c["pmaps"][0]
    assert pm.shape == (xw, yw) and c["poses"].shape == (8, 3) and len(c["ct"]) == 37
    assert len(c["maps"]) == (3 if (xw, yw) in K.A_MULTI and scale == 1.0 else 1)
    touched = (pass_ | hit) != 0
    assert set(np.unique(hit)) == set(range(len(t) + 1))
    # the forced cells
    for cell in [(0, 0), (0, yw - 1), (xw - 1, 0), (xw - 1, yw - 1)] + [(xw - 1, ly) for ly in (31, 32, 63, 64, 255, 256, yw - 1) if ly < yw]:
        assert pm[cell] == 100, cell
    if xw > 1:
        assert np.all(pm[0] == 100)
        assert 0.05 < (touched[1:].mean()) < 0.25
    assert np.any(pm == 0) and np.any(pm == 50)
    # the poses: inside and up to three cells outside, headings on both sides of zero
    cx, cy = scale * (c["poses"][:, 0] + ox), scale * (c["poses"][:, 1] + oy)
    inside = (cx >= 0) & (cx < xw) & (cy >= 0) & (cy < yw)
    assert 2 <= inside.sum() <= 6
    assert np.all((np.trunc(cx) >= -3) & (np.trunc(cx) <= xw + 2) & (np.trunc(cy) >= -3) & (np.trunc(cy) <= yw + 2))     # cells, as int() gives them
    assert c["poses"][:, 2].min() < -1.0 and c["poses"][:, 2].max() > 1.0
    # the aimed beams end on the cells they were aimed at
    at = 37
    for b, cell, mine in zip(K.AIM_POSES, K.aim_cells(xw, yw), c["aimed"]):
        start, ends = K.beam_cells(c["poses"][b], c["sct"], c["sst"], c["scan"], *c["geom"])
        assert start == cell and ends[at:at + len(mine)] == mine and c["poses"][b, 2] == 0.0
        assert {pm[e] for e in mine} == {100, 0, 50}
        at += len(mine)
    assert at == len(c["sct"]) == len(c["scan"])
    # the reference's answers
    r, cells, counts, cls = K.ref_a(*case)
    check_mix(cls, r, K.flagged_of(c["poses"], c["ct"], c["st"], c["max_range"], c["geom"]), A_IDS[A_CASES.index(case)])
    found = cells[cells[:, :, 0] >= 0]
    assert np.any(found[:, 0] == xw - 1)
    assert np.any(found[:, 1] // 32 == (yw - 1) // 32) and yw % 32 != 0          # in the last, partial mask word
    if yw > 256:
        assert np.any(found[:, 1] >= 256)
    # every threshold of the rule, one below and one above, on a cell that a cast line crosses
    for h in range(len(t)):
        for d in (-1, 0, 1):
            cell = thresh_cells[(h, d)]
            assert cell in c["crossed"] and hit[cell] == h and pass_[cell] == t[h] + d
            assert pm[cell] == (0 if d < 0 else 100)
    assert len(set(thresh_cells.values())) == 3 * len(t)


@pytest.mark.parametrize("shape", K.A_MULTI)
def test_a_three_maps_differ(shape):
    for hit_inc in K.HIT_INCS:
        c = K.case_a(shape[0], shape[1], 1.0, 0.0, 0.0, hit_inc)
        pm = c["pmaps"]
        assert not np.array_equal(pm[0], pm[1]) and not np.array_equal(pm[1], pm[2]) and not np.array_equal(pm[0], pm[2])
        one, three = K.ref_a(shape[0], shape[1], 1.0, 0.0, 0.0, hit_inc), K.ref_a(shape[0], shape[1], 1.0, 0.0, 0.0, hit_inc, True)
        for b, g in enumerate(K.A_GOB):
            if g == 0:
                assert np.array_equal(one[1][b], three[1][b]) and np.array_equal(one[3][b], three[3][b]), b
        assert sum(not np.array_equal(one[1][b], three[1][b]) for b in range(8)) >= 3      # routing changes the answers
    assert sorted(set(K.A_GOB)) == [0, 1, 2] and np.any(np.diff(K.A_GOB) < 0) and np.any(np.diff(K.A_GOB) > 0)


def test_b_rows_past_one_pass():
    rows = K.B_G * K.B_XW
    assert rows > 2 ** 20 and 1024 * K.B_XW == 2 ** 20                 # map 1024 begins at global row 2^20
    c = K.case_b()
    assert sorted({lx for lx, _, _, _ in c["cells"][1024]}) == [0, 1, 1023]
    assert set(c["gob"]) == set(K.B_MAPS) and not c["cells"][512]
    r, cells, counts, cls = K.ref_b()
    in_last = cells[c["gob"] == 1024]
    assert np.any(in_last[:, :, 0] == 0) and np.any(in_last[:, :, 0] == 1023)
    for g in (0, 1023):
        assert np.any(cells[c["gob"] == g][:, :, 0] >= 0)
    assert np.all(cells[c["gob"] == 512] == -1) and np.all(np.isinf(r[c["gob"] == 512]))
    print("B classes:", class_counts(cls))
    assert len(np.unique(cls)) >= 4


@pytest.mark.parametrize("B", K.C_BS)
def test_c_blocks(B):
    hpb = K.hyps_per_block(B)
    assert hpb == {2048: 1, 2049: 2, 4097: 3}[B]
    gob = K.c_gob(B)
    pats = K.run_patterns(gob, hpb)
    if hpb == 1:
        assert pats == {(1, (0,))}
    if hpb == 2:
        assert {(2, (0,)), (2, (0, 1)), (1, (0,))} <= pats             # one map twice, two maps, and the last block of one
    if hpb == 3:
        # one map thrice, two maps, three maps, A-B-A, and a partial last block
        assert {(3, (0,)), (3, (0, 1)), (3, (0, 1, 2)), (3, (0, 1, 0))} <= pats and any(k < 3 for k, _ in pats)
    assert (B + hpb - 1) // hpb <= K.STAGED_BLOCKS
    # the invalid entries: between two runs of one map, first and last of a block, two different ones side by side
    bad = K.c_invalid(B)
    inv = (bad < 0) | (bad >= 3)
    assert 8 <= inv.sum() <= 10 and inv[B - 1]
    assert not inv[0] and inv[1] and not inv[2] and bad[0] == bad[2]
    assert inv[12] and not inv[13] and inv[14]
    assert inv[24] and inv[25] and bad[24] != bad[25] and inv[38] and inv[39] and bad[38] != bad[39]
    assert {3, -1} <= set(bad[inv])
    assert np.array_equal(bad[~inv], gob[~inv])


@pytest.mark.parametrize("n", K.C_NS)
def test_c_beams(n):
    c = K.case_c(n)
    assert c["rows"].shape == (4, n) and c["poses"].shape == (6, 3) and len(c["pmaps"]) == 3
    assert K.mask_bytes(*K.C_SHAPE) // 4 > 256                         # staging a map takes a lane more than one word
    assert np.gcd(K.C_ROW_PERIOD, K.C_POSES) == 1 and K.C_PERIOD % 12 == 0 and K.C_PERIOD % K.C_ROW_PERIOD == 0 and K.C_PERIOD % K.C_POSES == 0
    for B in K.C_BS:
        poses, ranges, gob = K.c_batch(n, B)
        r, cells, counts, cls = K.c_expected(n, B)
        assert r.shape == (B, n) and cells.shape == (B, n, 2) and counts.shape == (B, 7) and cls.shape == (B, n)
        assert np.all(counts.sum(axis=1) == n)
        flagged = K.flagged_of(c["poses"][np.arange(12) % 6], c["ct"], c["st"], c["max_range"], c["geom"])[np.arange(B) % 12]
        check_mix(cls, r, flagged, "C n=%d B=%d" % (n, B))
        if n == 1:
            print("classes of the first wave:", class_counts(cls[:64]))
            assert len(np.unique(cls[:64, 0])) >= 5                    # the 64 hypotheses of the direct engine's first wave
    # a spot check of the tiling against the reference applied row by row
    poses, ranges, gob = K.c_batch(n, 200)
    r, cells, counts, cls = K.c_expected(n, 200)
    for b in (0, 83, 84, 131, 199):
        rr, rc = R.raycast(c["pmaps"][gob[b]], 1.0, 0.0, 0.0, poses[b], c["ct"], c["st"], c["max_range"])
        n1, k1 = R.score(c["pmaps"][gob[b]], 1.0, 0.0, 0.0, poses[b], R.table_points(ranges[b], c["ct"], c["st"]))
        assert np.array_equal(rr, r[b], equal_nan=True) and np.array_equal(rc, cells[b]) and np.array_equal(n1, counts[b]) and np.array_equal(k1, cls[b])
    # rows that name no map
    bad = K.c_invalid(2049)
    r, cells, counts, cls = K.c_expected(n, 2049, bad)
    assert np.all(np.isnan(r[1])) and np.all(cells[12] == -1) and np.all(cls[2048] == R.BAD) and counts[25, R.BAD] == n


def test_d_the_sixth_pose():
    assert K.D_B * K.D_N == 2 ** 28 + 4096 and (K.D_B - 1) * K.D_N == 2 ** 28      # 2^20 blocks of 256 lanes: one pass is 2^28 rays
    assert K.hyps_per_block(K.D_B) == 33
    d = K.case_d()
    assert d["scan"].max() <= 3.0 and d["ranges"].shape == (6, K.D_N) and d["counts"].shape == (6, 7)
    for k in range(5):
        assert not np.array_equal(d["ranges"][5], d["ranges"][k], equal_nan=True), k
        assert not np.array_equal(d["counts"][5], d["counts"][k]), k
    assert np.isfinite(d["ranges"][5]).sum() > 100 and np.isinf(d["ranges"][5]).sum() > 100
    idx = K.d_index()
    assert idx[-1] == 5 and np.all(idx[:-1] < 5) and len(idx) == K.D_B
    print("D counts of the six poses:\n", d["counts"])


def test_e_the_fit_boundary():
    assert K.mask_bytes(*K.E_SHAPES[0]) == K.LDS_BYTES and K.mask_bytes(*K.E_SHAPES[1]) == K.LDS_BYTES + 128
    for shape in K.E_SHAPES:
        c = K.case_e(*shape)
        r, cells, counts, cls = K.ref_e(*shape)
        found = cells[cells[:, :, 0] >= 0]
        assert len(found) > 50 and np.any(found[:, 0] == shape[0] - 1)            # a cell of the map's last row is found
        print("E", shape, "classes:", class_counts(cls), "finite:", len(found))
        assert len(np.unique(cls)) >= 4


def test_f_skip_at_the_ends():
    pm = R.ring_pmap()
    want_flag = [False, True, False, True]
    for k, (s, e, kind) in enumerate(K.F_BEAMS):
        pose, ct, st, scan, Lp = K.f_case(k)
        start, ends = K.beam_cells(pose[0], ct, st, scan, 1.0, 0.0, 0.0)
        assert start == s and ends == [e] and Lp == max(abs(e[0] - s[0]), abs(e[1] - s[1])) + 1
        seq = [K.f_expected(k, skip)[0] for skip in (Lp - 2, Lp - 1, Lp, Lp + 1)]
        if kind == "occupied":
            assert pm[e] == 100 and R.is_flagged(s, e) == want_flag[k]
            assert seq[0] in (R.BLOCKED, R.HIT) and seq[1:] == [R.HIT, R.FREE, R.FREE], (k, seq)
            assert K.f_expected(k, Lp - 1)[2][0].tolist() == list(e) and K.f_expected(k, Lp)[2][0].tolist() == [-1, -1]
        elif kind == "untouched":
            assert pm[e] == 50 and seq == [R.UNKNOWN] * 4, (k, seq)
        else:
            assert not (0 <= e[0] < 64 and 0 <= e[1] < 64) and seq == [R.OUT] * 4, (k, seq)
    assert {K.f_expected(k, K.f_case(k)[4] - 2)[0] for k in range(4)} == {R.BLOCKED, R.HIT}    # both ways into the last cell
    assert len({R.is_flagged(s, e) for s, e, kind in K.F_BEAMS if kind == "untouched"}) == 2
