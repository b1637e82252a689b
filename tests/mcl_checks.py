"""What the GPU test files of the particle filter share (test infrastructure only): one slam_mcl_weigh /
slam_mcl_weigh_maps and one slam_mcl_resample compared with the restatement (tests/mcl_ref.py).

Integer outputs compare with array_equal, poses and estimates at 1e-9, ESS exactly.  The device's cosine and sine may
differ from NumPy's in the last place: a particle whose cost differs from the restatement's must be one whose restated
cost changes when the cosine or the sine is moved one ulp either way, and at most 2 % of a case's particles may be such."""
import numpy as np

import match_ref as M
import mcl_ref as X


def fields_of(pm, cap):
    pm = pm if pm.ndim == 3 else pm[None]
    return np.stack([M.field(p, cap) for p in pm])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def weigh_maps(fields, geom, poses, ranges, ct, st, max_range, cap, pmaps, motion=None, noise=None, acc=None, ulp=False, moved=None):
    """slam_mcl_weigh_maps restated as gridslam_ref.weigh_maps does - every particle weighed on its table entry's map by
    mcl_ref.weigh - but with the particles of a filter that share a map taken together, so the cost loop runs once per
    (filter, map) instead of once per particle.  The dict of mcl_ref.weigh with [F, P] shapes, ``unsure`` included."""
    poses = np.asarray(poses, dtype=np.float64)
    F, P, _ = poses.shape
    pmaps = np.asarray(pmaps).reshape(F, P)
    ranges = np.asarray(ranges, dtype=np.float32).reshape(F, -1)
    out = dict(poses=X.move(poses, motion, noise), cost=np.full((F, P), -1, dtype=np.int32), used=np.zeros(F, dtype=np.int32),
               acc=None if acc is None else np.array(acc, dtype=np.int32).reshape(F, P), unsure=np.zeros((F, P), dtype=bool))
    for f in range(F):
        for gi in np.unique(pmaps[f]):
            idx = np.flatnonzero(pmaps[f] == gi)
            sub = lambda a: None if a is None else np.asarray(a)[f:f + 1, idx]
            w = X.weigh(fields, *geom, poses[f:f + 1, idx], ranges[f:f + 1], ct, st, max_range, cap,
                        motion=None if motion is None else np.asarray(motion)[f:f + 1], noise=sub(noise), maps=[int(gi)], acc=sub(acc),
                        ulp=ulp, moved=sub(moved))
            out["cost"][f, idx], out["unsure"][f, idx], out["used"][f] = w["cost"][0], w["unsure"][0], w["used"][0]
            if acc is not None:
                out["acc"][f, idx] = w["acc"][0]
    return out


def check_weigh(slam, g, pm, geom, poses, ranges, ct, st, max_range=19.0, cap=64, motion=None, noise=None, maps=None, acc=None,
                field=None, pmaps=None, fields=None, got=None, tag=None):
    """One slam_mcl_weigh against the restatement; returns (poses, cost, acc, used) of the device.  ``pmaps`` int32 [F, P]:
    slam_mcl_weigh_maps with that particle-to-map table instead.  ``fields``: the restatement's fields when the caller has
    them already; ``got``: the device's outputs when the caller made the call itself (the device form)."""
    fields = fields_of(pm, cap) if fields is None else fields
    poses = np.ascontiguousarray(poses, dtype=np.float64)
    if got is None:
        got = slam.mcl_weigh_host(g, poses, ranges, ct, st, motion=motion, noise=noise, max_range=max_range, cap=cap,
                                  grid_of_filter=maps, field=field, acc=acc, grid_of_particle=pmaps)
    gp, gc, ga, gu = got
    assert gc.dtype == np.int32 and gu.dtype == np.int32 and (ga is None) == (acc is None), tag
    if motion is None:
        assert same_bits(gp, poses), tag
    else:
        assert np.allclose(gp, X.move(poses, motion, noise), rtol=0.0, atol=1e-9, equal_nan=True), tag
    if pmaps is None:
        ref = X.weigh(fields, *geom, gp, ranges, ct, st, max_range, cap, maps=maps, acc=acc)  # the cost of the device's own moved poses
    else:
        ref = weigh_maps(fields, geom, gp, ranges, ct, st, max_range, cap, pmaps, acc=acc)
    assert np.array_equal(gu, ref["used"]), tag
    diff = gc != ref["cost"]
    F, P = gc.shape
    for f, p in np.argwhere(diff):
        gi = int(pmaps[f][p]) if pmaps is not None else 0 if maps is None else int(maps[f])
        beams = X.used_beams(np.asarray(ranges, dtype=np.float32).reshape(F, -1)[f], ct, st, max_range)
        assert gc[f, p] >= 0 and ref["cost"][f, p] >= 0 and X.is_unsure(fields[gi], *geom, beams, gp[f, p], cap), (tag, f, p)
    assert diff.sum() <= 0.02 * F * P, tag
    if acc is not None:
        assert ga.dtype == np.int32 and np.array_equal(ga[~diff], ref["acc"][~diff]), tag
        tot = np.minimum(np.asarray(acc, dtype=np.int64).reshape(F, P) + gc, X.ACC_MAX)
        assert np.array_equal(ga[diff], tot[diff]), tag
    return gp, gc, ga, gu


def check_resample(slam, ctx, poses, acc, table, u0, shift=0, ess_frac=np.inf, got=None, tag=None):
    """One slam_mcl_resample against the restatement; ``got``: the device's outputs when the caller made the call itself."""
    if got is None:
        got = slam.mcl_resample_host(ctx, poses, acc, table, u0, shift=shift, ess_frac=ess_frac)
    ref = X.resample(poses, acc, table, shift, u0, ess_frac)
    assert same_bits(got[0], ref["poses"]), tag
    for a, k in zip(got[1:3], ("acc", "ancestors")):
        assert a.dtype == np.int32 and np.array_equal(a, ref[k]), (tag, k)
    assert np.allclose(got[3], ref["est"], rtol=0.0, atol=1e-9, equal_nan=True), tag
    assert got[4].dtype == np.int32 and np.array_equal(got[4], ref["info"]), tag
    assert np.array_equal(got[3][:, 3], ref["est"][:, 3]), tag         # ESS: one multiply and one divide on exact integers
    return got
