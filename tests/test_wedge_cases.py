"""The inputs of test_gpu_wedge_forms.py (tests/wedge_cases.py) reach the branches of the wedge cast they are there for
- checked on the model and on the oracle's own Bresenham cells, without a GPU, so that no GPU test passes for want of
a ray of the right kind.  Every test prints the counts it asserts on."""
import numpy as np
import pytest

import wedge_cases as K
from oracle import c_oracle as co


def paths(case, pick=None):
    """[(b, i, pass cells [k, 2])] of the case's rays (pick: boolean [B, n]); the path's last cell is the hit."""
    out = []
    orgs, ends = case["orgs"], case["ends"]
    for b in range(ends.shape[0]):
        for i in range(ends.shape[1]):
            if (pick is None or pick[b, i]) and tuple(orgs[b]) != tuple(ends[b, i]):
                p = co.bresenham(orgs[b], ends[b, i])
                assert tuple(p[-1]) == tuple(ends[b, i]) and tuple(p[0]) == tuple(orgs[b])
                out.append((b, i, p[:-1]))
    return out


def unit_bands(case):
    """{unit: band_model(...)} from the true pass cells of every unit (all units here are one part)."""
    c = K.classify(case)
    out = {}
    for u in np.unique(c["unit"][c["unit"] >= 0]):
        assert int((c["unit"] == u).sum()) <= K.PART_RAYS
        steep, M = (u % K.CLASSES) // K.SLOPES >= 2, int(K.wedge_shear(u % K.CLASSES))
        cells = np.concatenate([p for _, _, p in paths(case, c["unit"] == u)])
        a, y = K.walk_coords(cells, steep)
        out[int(u)] = K.band_model(a, y - M * a)
    return out


def check_round_trip(case):
    """The cell centres index back to their cells, and every cell lies in the map."""
    xw, yw, scale, off_x, off_y = case["dims"]
    OX, OY, CX, CY = K.world(case)
    assert np.array_equal(K.to_cell(OX, scale, off_x), case["ends"][..., 0]) and np.array_equal(K.to_cell(OY, scale, off_y), case["ends"][..., 1])
    assert np.array_equal(K.to_cell(CX, scale, off_x), case["orgs"][:, 0]) and np.array_equal(K.to_cell(CY, scale, off_y), case["orgs"][:, 1])
    for cells, hi in ((case["ends"][..., 0], xw), (case["ends"][..., 1], yw), (case["orgs"][:, 0], xw), (case["orgs"][:, 1], yw)):
        assert cells.min() >= 0 and cells.max() < hi


def test_model_of_the_classes():
    """The four quarters of [-1, 1], the min() at +1, the shear of each quarter and the direction bits."""
    f, t = np.array(False), np.array(True)
    q = [int(K.wedge_class(f, f, np.array(8), np.array(m))) for m in (-8, -5, -4, -1, 0, 3, 4, 7, 8)]
    assert q == [0, 0, 1, 1, 2, 2, 3, 3, 3]
    assert int(K.wedge_class(f, t, np.array(-8), np.array(4))) == 4 + 1      # towards -x: the slope as the walk sees it is -1/2
    assert int(K.wedge_class(t, f, np.array(4), np.array(8))) == 8 + 3
    assert list(K.wedge_shear(np.arange(16))) == [-1, 0, 0, 1] * 4
    r = K.ray_setup(5, 5, 2, 9)
    assert bool(r["steep"]) and not bool(r["flag"]) and (int(r["x0"]), int(r["y0"]), int(r["dx"]), int(r["ystep"])) == (5, 5, 4, -1)
    assert not bool(K.ray_setup(3, 4, 3, 4)["valid"]) and not bool(K.ray_setup(0, 0, 4, 4)["steep"])
    assert K.group_size(0, 128, 16) == 16 and K.group_size(64, 8192, 9) == 7 and K.group_size(64, 65, 64) == 64


def test_a_class_boundaries():
    case = K.case_a()
    check_round_trip(case)
    assert K.plan_cast(900, 900, 1, case["ends"].shape[1]) == "wedges"
    c = K.classify(case)
    cls0 = c["cls"][0]
    counts = np.bincount(cls0[cls0 >= 0], minlength=K.CLASSES)
    print("A rays per class:", counts.tolist(), "no ray:", int((cls0 < 0).sum()))
    assert counts.min() >= 8 and int((cls0 < 0).sum()) == 16
    dd = case["ends"][0] - case["orgs"][0]
    maj = np.where(c["steep"][0], dd[:, 1], dd[:, 0])
    mnr = np.where(c["steep"][0], dd[:, 0], dd[:, 1])
    seen = {}
    for k, q in K.A_RATIOS:
        for steep in (False, True):
            if steep and abs(k) == q:
                continue                                             # adx == ady is never steep
            for flag in (False, True):
                m = (c["steep"][0] == steep) & (c["flag"][0] == flag) & (maj != 0) & (mnr * np.sign(maj) * q == k * np.abs(maj))
                seen[(k, steep, flag)] = sorted(set(np.abs(maj[m]).tolist()))
                assert len(seen[(k, steep, flag)]) >= (4 if k % 2 == 0 else 3), (k, steep, flag, seen[(k, steep, flag)])
    print("A exact slopes k/4 (k, steep, towards origin) -> major lengths:", seen)
    diag = (np.abs(dd[:, 0]) == np.abs(dd[:, 1])) & (dd[:, 0] != 0)
    assert diag.sum() >= 4 * len(K.A_LENGTHS) and not c["steep"][0][diag].any()
    ties = sum(K.float_walk_ties(int(c["dx"][0][i]), int(c["dy"][0][i])) > 0 for i in range(len(cls0)) if cls0[i] >= 0)
    print("A rays whose walk meets error == 0.5:", ties)
    assert ties >= 8
    assert (c["dx"][1] == 1).all() and set(c["cls"][1].tolist()) == {0, 2, 3, 4, 6, 7, 10, 14}   # length 1: slopes -1, 0, 1 only
    print("A length-1 scan classes:", sorted(set(c["cls"][1].tolist())))


@pytest.mark.parametrize("turned", [False, True])
def test_b1_bands_of_full_height(turned):
    case = K.transposed(K.case_b1()) if turned else K.case_b1()
    check_round_trip(case)
    c = K.classify(case)
    assert set(np.unique(c["cls"])) == {10 if turned else 2} and sorted(set(c["dx"][0].tolist())) == [520, 1030, 1540]
    (unit, bands), = unit_bands(case).items()
    print("b1", "steep" if turned else "flat", "unit", unit, "bands (a_lo, rows, Hw >=, direct):", bands)
    assert len(bands) >= 4 and bands[0][1] == K.BAND_ROWS and not any(b[3] for b in bands)
    ends = sorted(set((int(c["x0"][0][i]) + int(c["dx"][0][i]) - 1 - bands[0][0]) // K.BAND_ROWS + 1 for i in range(c["dx"].shape[1])))
    assert ends == [2, 3, 4]                                          # bands a ray passes cells in: 2, 3 and 4


def test_b2_bands_cut_to_the_window():
    case = K.case_b2()
    check_round_trip(case)
    assert K.plan_cast(700, 500, 1, case["ends"].shape[1]) == "wedges"
    c = K.classify(case)
    assert c["G"] == 16 and set(np.unique(c["cls"])) == {2}
    (unit, bands), = unit_bands(case).items()
    print("b2 unit", unit, "bands (a_lo, rows, Hw >=, direct):", bands)
    fits = [(K.WIN_CELLS // b[2]) & ~1 for b in bands]
    assert len(bands) >= 5 and max(fits) < K.BAND_ROWS and min(b[2] for b in bands[:-1]) >= 300 and not any(b[3] for b in bands)


def test_b3_direct_bands_before_bands_that_fit():
    case = K.case_b3()
    check_round_trip(case)
    c = K.classify(case)
    assert c["G"] == 3 and set(np.unique(c["cls"])) == {2}
    (unit, bands), = unit_bands(case).items()
    print("b3 unit", unit, "bands (a_lo, rows, Hw >=, direct):", bands)
    near, far = [b for b in bands if b[0] < 516], [b for b in bands if b[0] >= 516]
    assert near and far and all(b[3] and b[2] > K.WIN_CELLS // 2 for b in near)
    # the kernel's width is the true one plus at most one cell of prediction either side and the rounding to even cells
    assert all(0 < b[2] and (b[2] + 4) * 2 <= K.WIN_CELLS for b in far)
    cells2 = np.concatenate([p for _, _, p in paths(case, np.arange(3)[:, None] == np.full((1, case["ends"].shape[1]), 2))])
    assert cells2[:, 0].min() >= 516                                  # scan 2 alone has cells in the far bands


@pytest.mark.parametrize("name", list(K.C_CASES))
def test_c_parts(name):
    scans, n, group = K.C_CASES[name]
    case = K.case_c(scans, n, group)
    check_round_trip(case)
    assert K.plan_cast(600, 600, 1, n) == "wedges"
    c = K.classify(case)
    assert set(np.unique(c["cls"])) == {2}
    rays = K.unit_rays(case)
    print("C", name, "G =", c["G"], "rays per unit:", rays, "parts:", {u: K.parts_of(r) for u, r in rays.items()})
    assert [rays[u] for u in sorted(rays)] == K.C_UNIT_RAYS[name]
    if name == "one_part":
        assert [K.parts_of(r) for r in rays.values()] == [[2048]]
    if name == "two_parts":
        assert [K.parts_of(r) for r in rays.values()] == [[2048, 16]]
    if name == "three_parts":
        assert [K.parts_of(r) for r in rays.values()] == [[2048, 2048, 64]]
    if name == "ragged_groups":
        assert c["G"] == 7 and sorted(rays) == [2, 16 + 2]


@pytest.mark.parametrize("xw,yw", K.D_MAPS)
def test_d_rows_of_both_parities(xw, yw):
    """A flushed row starts at cell gbase = mx * yw + my0 of its map; my0 is even for a steep class (the band's first row)
    and v_lo + M * mx with an even v_lo otherwise.  Pass cells per flush kind and parity of gbase."""
    case = K.case_d(xw, yw)
    check_round_trip(case)
    assert K.plan_cast(xw, yw, 1, case["ends"].shape[1]) == "wedges"
    c = K.classify(case)
    assert case["orgs"][0, 0] % 2 == 0 and case["orgs"][1, 0] % 2 == 1
    ends = {tuple(e) for e in case["ends"][0]}
    assert {(0, 0), (xw - 1, yw - 1)} <= ends and case["orgs"][2, 0] == xw - 1 and case["orgs"][3, 1] == yw - 1
    count = {}
    for b, i, p in paths(case):
        cls = int(c["cls"][b, i])
        steep, M = cls // K.SLOPES >= 2, int(K.wedge_shear(cls))
        par = (p[:, 0] * yw + (0 if steep else M * p[:, 0])) & 1
        key = ("steep" if steep else "flat", "sheared" if M else "straight")
        count.setdefault(key, np.zeros(2, dtype=np.int64))
        count[key] += np.bincount(par, minlength=2)
    print("D %d x %d pass cells on rows of even / odd gbase:" % (xw, yw), {k: v.tolist() for k, v in count.items()})
    assert np.bincount(c["cls"][c["cls"] >= 0], minlength=K.CLASSES).min() >= 8
    if yw % 2:
        assert count[("steep", "straight")].min() >= 100 and count[("steep", "sheared")].min() >= 100
        assert count[("flat", "straight")].min() >= 100
    else:
        assert count[("flat", "sheared")].min() >= 100 and count[("steep", "straight")][1] == 0
    # the last pair of the map's last row: pass cells in row xw - 1 at y >= yw - 2
    last = sum(int(((p[:, 0] == xw - 1) & (p[:, 1] >= yw - 2)).sum()) for _, _, p in paths(case))
    print("D pass cells in the last pair of the last row:", last)
    assert last >= 2


def test_e_sides():
    a, b = K.case_e(65535), K.case_e(65536)
    check_round_trip(a)
    check_round_trip(b)
    n = a["ends"].shape[1]
    assert np.array_equal(a["ends"], b["ends"]) and a["ends"][..., 0].min() >= 65535 - 300 and a["ends"][..., 0].max() == 65534
    assert [K.plan_cast(65535, 8, m, n) for m in (1, 2, 4)] == ["wedges", "tiles", "wedges"]
    assert [K.plan_cast(65536, 8, m, n) for m in (1, 2, 4)] == ["tiles", "tiles", "tiles"]
    assert K.plan_cast(65536, 8, 4, n, maps=True) == "window"          # a map per trajectory never reaches the tiles
    c = K.classify(a)
    print("E rays per class:", np.bincount(c["cls"][c["cls"] >= 0], minlength=K.CLASSES).tolist())
    assert (c["cls"] >= 0).sum() > 1500


def test_f_odd_map_offsets(syn):
    """Map 1 of the 601 x 601 maps starts at byte 4 mod 8.  Steep rays cast into it have pass cells on rows mx whose first
    cell is even in the map (mx * yw even) and odd in the allocation: a flush that pairs by the parity in the map alone
    sends those rows as 64-bit adds to addresses of 4 mod 8."""
    from oracle import checks
    cells = K.F_SIDE * K.F_SIDE
    assert (1 * cells * 4) % 8 == 4 and (2 * cells * 4) % 8 == 0
    assert K.plan_cast(K.F_SIDE, K.F_SIDE, 1, K.F_BEAMS, maps=True) == "wedges" and K.plan_cast(K.F_SIDE, K.F_SIDE, 4, K.F_BEAMS, maps=True) == "wedges"
    ranges = K.case_f(syn)
    assert ranges.shape == (K.F_MAPS, K.F_SCANS, K.F_BEAMS)
    scale, off = 1.0 / K.F_RESO, K.F_SIDE / (2.0 / K.F_RESO)
    for route in K.F_ROUTES:
        assert 1 in route
        rows = 0
        for l in [l for l in range(K.F_MAPS) if route[l] == 1]:
            poses, _, _, _ = checks.replay_reference(ranges[l], K.F_AMIN, K.F_AMAX, None, pose0=tuple(K.F_POSE0[l]), threads=1)
            for k in range(len(poses)):
                px, py = co.laser_to_points(ranges[l][k + 1], K.F_AMIN, K.F_AMAX)
                wx, wy = co.world_points(poses[k], np.array(px), np.array(py))
                org = np.array([[int(K.to_cell(poses[k][0], scale, off)), int(K.to_cell(poses[k][1], scale, off))]])
                ends = np.stack([K.to_cell(wx, scale, off), K.to_cell(wy, scale, off)], axis=1)[None]
                inside = (ends.min() >= 0) and (ends.max() < K.F_SIDE)
                case = K.make(K.dims_of(K.F_SIDE, K.F_SIDE), org, ends)
                c = K.classify(case)
                if inside:
                    for b, i, p in paths(case, c["steep"] & c["valid"]):
                        rows += int(((p[:, 0] * K.F_SIDE) % 2 == 0).sum())
        print("F route", route, "steep pass cells of map 1 on rows that are even in the map, odd in the allocation:", rows)
        assert rows >= 100
