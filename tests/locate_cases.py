"""What the two GPU test files of slam_grid_locate share (test infrastructure only): maps written straight into the
counters, the read-back fields, and the comparison of every output with the restatement (tests/locate_ref.py)."""
import numpy as np

import locate_ref as L
import match_ref as M


def occupy(g, cells):
    """Occupied cells written straight into the hit counters (one hit occupies): cells[gi] = [(x, y), ...].  Returns the
    pmaps read back."""
    import torch
    g._ctx.synchronize()       # a reset before this has run: torch copies on a stream of its own
    _, h = g.counters_torch()
    hit = np.zeros((g.G, g.xw, g.yw), dtype=np.int32)
    for gi, cs in enumerate(cells):
        for x, y in cs:
            hit[gi, x, y] = 1
    h.copy_(torch.from_numpy(hit).to(h.device))
    torch.cuda.synchronize()
    pm = np.stack([g.read(gi)["pmap"] for gi in range(g.G)])
    assert np.array_equal(pm == 100, hit == 1)
    return pm


def fields_of(slam, g, cap):
    """The restatement's fields of the pmaps read back from the device; the device's own field must be the same."""
    pm = np.stack([g.read(gi)["pmap"] for gi in range(g.G)])
    f = np.stack([M.field(p, cap) for p in pm])
    assert np.array_equal(slam.grid_distance_field_host(g, cap), f)
    return f


def ragged_grid(slam, ctx, xw, yw):
    g = slam.DeviceGrid(1, xw, yw, 1.0, 0.0, 0.0, context=ctx)
    pm, cells = L.ragged_pmap(xw, yw)
    assert np.array_equal(occupy(g, [cells])[0], pm)
    return g


def same(got, want):
    for a, b, dt in zip(got, want, (np.int32, np.int32, np.int32, np.int64)):
        assert a.dtype == dt and a.shape == b.shape and np.array_equal(a, b), (a, b)


def check(slam, g, fields, scale, ranges, ct, st, rot, H, max_range, cap, maps=None, regions=None, B=None):
    want = L.locate_batch(fields, scale, ranges, ct, st, rot, H, max_range, cap, maps=maps, regions=regions, B=B)
    got = slam.grid_locate_host(g, ranges, ct, st, rot, levels=H, region=regions, max_range=max_range, cap=cap, grid_of_batch=maps,
                                B=B, return_stats=True)
    same(got, want)
    return got
