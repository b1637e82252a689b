"""Rays traced through a map on the GPU at the edges of their launch shapes (tests/raycast_cases.py; what those
inputs reach is checked without a GPU in test_raycast_bound_cases.py): non-square, ragged maps under both occupied
rules, more rows than the pack kernel has blocks, staged blocks that hold several hypotheses of several maps, more
rays than the direct engine has lanes, masks at the LDS fit boundary, `skip` at the ends of a scored line.

The maps are written as (pass, hit) counters straight into the device arrays.  The reference reads the pmap that
NumPy computes from those counters, and that pmap is asserted equal to the one the device finalizes - so the mask,
the finalize kernel and NumPy agree on every cell.  Cells, classes and counts are compared bit-equal, ranges equal
as float32 bits; with the mask words from global memory ("raycast_lds" 0) and from LDS (1)."""
import numpy as np
import pytest

import raycast_cases as K
import raycast_ref as R
from conftest import pkg
from test_gpu_raycast import ring_grid, same

pytestmark = pytest.mark.gpu

A_CASES = [g + (h,) for g in K.A_GEOMS for h in K.HIT_INCS]
A_IDS = ["%dx%d-s%g-hit%d" % (c[0], c[1], c[2], c[5]) for c in A_CASES]


@pytest.fixture(scope="module")
def slam():
    p = pkg()
    p._abi.default_context()   # fails loudly when there is no gfx950 device
    return p


@pytest.fixture(scope="module", params=[0, 1], ids=["direct", "staged"])
def ctx(request, slam):
    c = slam.Context(0)
    c.set_option("raycast_lds", request.param)
    yield c
    c.close()


def up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def grid_of(slam, ctx, c, maps=None):
    """A DeviceGrid of case c with the counters of `maps` (indices into c["maps"]) written into it, and its pmaps
    checked against NumPy's."""
    import torch
    maps = list(range(len(c["maps"]))) if maps is None else maps
    g = slam.DeviceGrid(len(maps), c["xw"], c["yw"], c["geom"][0], c["geom"][1], c["geom"][2], hit_inc=float(c["hit_inc"]), context=ctx)
    ctx.synchronize()                                                  # the new grid's reset is on the context's stream, the copies on torch's
    p, h = g.counters_torch()
    p.copy_(up(np.stack([c["maps"][k][0] for k in maps])))
    h.copy_(up(np.stack([c["maps"][k][1] for k in maps])))
    torch.cuda.synchronize()
    for i, k in enumerate(maps):
        assert same(g.read(i)["pmap"], c["pmaps"][k]), k
    return g


def check(got, want, what):
    for name, a, b in zip(("ranges", "cells", "counts", "classes"), got, want):
        if not same(a, b):
            a, b = np.asarray(a), np.asarray(b)
            where = np.argwhere(a.view(np.int32 if a.dtype == np.float32 else a.dtype) != b.view(np.int32 if b.dtype == np.float32 else b.dtype))
            raise AssertionError("%s: %s differ in %d places, first at %s: %s against %s"
                                 % (what, name, len(where), tuple(where[0]), a[tuple(where[0])], b[tuple(where[0])]))


# ------------------------------------------------------------------ A. non-square, ragged maps, both rules
@pytest.mark.parametrize("case", A_CASES, ids=A_IDS)
def test_ragged_maps(slam, ctx, case):
    c = K.case_a(*case)
    g = grid_of(slam, ctx, c, [0])
    r, cells = slam.grid_raycast_host(g, c["poses"], c["ct"], c["st"], max_range=c["max_range"], return_cells=True)
    counts, cls = slam.grid_score_host(g, c["scan"], c["poses"], c["sct"], c["sst"], return_classes=True)
    check((r, cells, counts, cls), K.ref_a(*case), "one map")
    if len(c["maps"]) == 3:
        g3 = grid_of(slam, ctx, c)
        r, cells = slam.grid_raycast_host(g3, c["poses"], c["ct"], c["st"], max_range=c["max_range"], grid_of_batch=K.A_GOB, return_cells=True)
        counts, cls = slam.grid_score_host(g3, c["scan"], c["poses"], c["sct"], c["sst"], grid_of_batch=K.A_GOB, return_classes=True)
        check((r, cells, counts, cls), K.ref_a(*case, True), "three maps")
    ctx.check_status()


# ------------------------------------------------------------------ B. pack past one pass of rows
def test_more_rows_than_pack_blocks(slam, ctx):
    import torch
    c = K.case_b()
    g = slam.DeviceGrid(K.B_G, K.B_XW, K.B_YW, 1.0, 0.0, 0.0, context=ctx)
    ctx.synchronize()
    p, h = g.counters_torch()
    hp, hh = np.zeros((K.B_G, K.B_XW, K.B_YW), dtype=np.int32), np.zeros((K.B_G, K.B_XW, K.B_YW), dtype=np.int32)
    for m, cs in c["cells"].items():
        for lx, ly, pv, hv in cs:
            hp[m, lx, ly], hh[m, lx, ly] = pv, hv
    p.copy_(up(hp))
    h.copy_(up(hh))
    torch.cuda.synchronize()
    for m in K.B_MAPS:
        assert same(g.read(m)["pmap"], c["pmaps"][m]), m
    r, cells = slam.grid_raycast_host(g, c["poses"], c["ct"], c["st"], max_range=c["max_range"], grid_of_batch=c["gob"], return_cells=True)
    counts, cls = slam.grid_score_host(g, c["scan"], c["poses"], c["ct"], c["st"], grid_of_batch=c["gob"], return_classes=True)
    check((r, cells, counts, cls), K.ref_b(), "G = 1025")
    ctx.check_status()


# ------------------------------------------------------------------ C. staged blocks of several hypotheses and maps
@pytest.fixture(scope="module")
def c_grid(slam, ctx):
    return grid_of(slam, ctx, K.case_c(37))                            # (the maps are those of every n)


@pytest.mark.parametrize("n", K.C_NS)
@pytest.mark.parametrize("B", K.C_BS)
def test_blocks_of_several_maps(slam, ctx, c_grid, B, n):
    import torch
    c = K.case_c(n)
    poses, ranges, gob = K.c_batch(n, B)
    r, cells = slam.grid_raycast_host(c_grid, poses, c["ct"], c["st"], max_range=c["max_range"], grid_of_batch=gob, return_cells=True)
    counts, cls = slam.grid_score_host(c_grid, ranges, poses, c["ct"], c["st"], grid_of_batch=gob, return_classes=True)
    check((r, cells, counts, cls), K.c_expected(n, B), "valid maps")
    # entries that name no map, on the _dev forms: those rows BAD / NaN / (-1, -1), every other row as before
    bad = K.c_invalid(B)
    torch.cuda.synchronize()
    d = dict(poses=up(poses), cos_t=up(c["ct"]), sin_t=up(c["st"]), grid_of_batch=up(bad))
    d_ranges = up(ranges)
    torch.cuda.synchronize()
    counts_d, cls_d = c_grid.score(d_ranges, return_classes=True, **d)
    r_d, cells_d = c_grid.raycast(max_range=c["max_range"], return_cells=True, **d)
    ctx.synchronize()
    want = K.c_expected(n, B, bad)
    check((r_d.cpu().numpy(), cells_d.cpu().numpy(), counts_d.cpu().numpy(), cls_d.cpu().numpy()), want, "invalid entries")
    inv = (bad < 0) | (bad >= 3)
    assert same(want[0][~inv], r[~inv]) and same(want[3][~inv], cls[~inv]) and np.all(want[3][inv] == R.BAD)
    ctx.check_status()


# ------------------------------------------------------------------ D. the direct engine past 2^28 rays
def test_more_rays_than_one_pass(slam, ctx):
    import torch
    d = K.case_d()
    g = ring_grid(slam, ctx)
    assert same(g.read()["pmap"], R.ring_pmap())
    idx = K.d_index()
    poses = d["six"][idx]
    counts = slam.grid_score_host(g, d["scan"], poses, d["ct"], d["st"])
    assert same(counts, d["counts"][idx])
    d_poses, d_ct, d_st = up(poses), up(d["ct"]), up(d["st"])
    torch.cuda.synchronize()
    r = g.raycast(d_poses, d_ct, d_st, max_range=K.D_MAX_RANGE)
    ctx.synchronize()
    bits = r.view(torch.int32)
    want = up(d["ranges"].view(np.int32))
    for k in range(5):
        assert bool((bits[k:K.D_B - 1:5] == want[k]).all()), k
    assert bool((bits[K.D_B - 1] == want[5]).all())                    # the one hypothesis of the second pass
    del r, bits
    ctx.check_status()


# ------------------------------------------------------------------ E. the LDS fit boundary
@pytest.mark.parametrize("shape", K.E_SHAPES, ids=["fits", "one-row-more"])
def test_lds_fit_boundary(slam, ctx, shape):
    c = K.case_e(*shape)
    g = grid_of(slam, ctx, c)
    r, cells = slam.grid_raycast_host(g, c["poses"], c["ct"], c["st"], max_range=c["max_range"], return_cells=True)
    counts, cls = slam.grid_score_host(g, c["scan"], c["poses"], c["ct"], c["st"], return_classes=True)
    check((r, cells, counts, cls), K.ref_e(*shape), str(shape))
    ctx.check_status()


# ------------------------------------------------------------------ F. skip at the ends of a scored line
def test_skip_at_the_ends(slam, ctx):
    g = ring_grid(slam, ctx)
    assert same(g.read()["pmap"], R.ring_pmap())
    for k, (s, e, kind) in enumerate(K.F_BEAMS):
        pose, ct, st, scan, Lp = K.f_case(k)
        seq = []
        for skip in (Lp - 2, Lp - 1, Lp, Lp + 1):
            counts, cls = slam.grid_score_host(g, scan, pose, ct, st, skip=skip, return_classes=True)
            r, cells = slam.grid_raycast_host(g, pose, ct, st, max_range=1.0, skip=skip, return_cells=True)
            want_cls, want_r, want_cells = K.f_expected(k, skip)
            assert cls[0, 0] == want_cls and counts[0, want_cls] == 1 and counts.sum() == 1, (k, skip)
            assert same(r[0], want_r) and same(cells[0], want_cells), (k, skip)
            seq.append(int(cls[0, 0]))
        if kind == "occupied":
            assert seq[0] in (R.BLOCKED, R.HIT) and seq[1:] == [R.HIT, R.FREE, R.FREE], (k, seq)
        else:
            assert seq == [R.UNKNOWN if kind == "untouched" else R.OUT] * 4, (k, seq)
