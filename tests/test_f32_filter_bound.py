"""The float32 pre-filter of the one-wave scan matcher's beam windows (csrc/icp_kernels.hip: F32Image, F32Best::settled),
restated in NumPy float32 and checked against float64 on the CPU.  The kernel scans a query's candidates in float32 - the
square of each, its two lowest mantissa bits replaced by the candidate's place in its trip of four - keeps the smallest
key km and the runner-up kr, and takes the winner without a float64 scan only when

    b b 1.000002 + 1e-30 < min(kr 0.999998, 1e30),   b = sqrt(km) 1.000002 + 2 Ef,
    Ef = 2^-23 1.00001 (|fs.x| + |fs.y| + tmax),     tmax >= |t.x| + |t.y| for every target of the pair

("settled").  The set of candidates float64 has to look at is then the winner alone; otherwise it is every candidate (the
wave runs the float64 scan).  Asserted here: every target within a factor 1 + 2^-49 of the true minimum - the class of
equal distances the float64 tie bookkeeping watches - is in that set, i.e. a settled query has exactly one such target and
it is the float32 winner.  The issue that asked for the filter words the bound as err(d) = 2 sqrt(2 d) E + 2 E^2 + 4 2^-24 d
with E = 2^-23 (|s.x| + |s.y| + |t.x| + |t.y|), confirming every candidate whose d - err(d) does not exceed the smallest
d + err(d); that rule is checked the same way.  A square root one unit in the last place off, as the hardware's may be, is
tried too."""
import numpy as np
import pytest

f32, f64 = np.float32, np.float64
CLASS = 1 + 2.0 ** -49


def squares32(qx, qy, tx, ty):
    """[query, target] float32 squares as the kernel forms them: fl(fma(dy, dy, fl(dx dx))) from the float32 roundings."""
    fsx, fsy, ftx, fty = qx.astype(f32), qy.astype(f32), tx.astype(f32), ty.astype(f32)
    with np.errstate(over="ignore", invalid="ignore"):
        dx, dy = fsx[:, None] - ftx[None, :], fsy[:, None] - fty[None, :]
        d = (dy.astype(f64) ** 2 + (dx * dx).astype(f64)).astype(f32)          # (dy^2 is exact in float64: one rounding, as the fma's)
    return fsx, fsy, ftx, fty, d


def keys_of(d):
    """The low two bits replaced by the place in the trip; trips start at index 0 here."""
    place = (np.arange(d.shape[1]) & 3).astype(np.uint32)
    return (d.view(np.uint32) & np.uint32(0xFFFFFFFC)) | place[None, :]


def shipped(qx, qy, tx, ty, sqrt_err=0.0):
    """-> settled [query], winner [query]: F32Best over all targets of the pair."""
    fsx, fsy, ftx, fty, d = squares32(qx, qy, tx, ty)
    k = keys_of(d)
    order = np.argsort(k, axis=1, kind="stable")
    win = order[:, 0]
    rows = np.arange(len(qx))
    km = k[rows, win].view(f32)
    kr = (k[rows, order[:, 1]] if k.shape[1] > 1 else np.full(len(qx), 0x7F800000, dtype=np.uint32)).view(f32)
    fin = np.isfinite(ftx) & np.isfinite(fty)
    with np.errstate(over="ignore", invalid="ignore"):
        tmax = f32(np.max(np.abs(ftx[fin]) + np.abs(fty[fin]), initial=f32(0)) * f32(1.000001)) if fin.all() else f32(np.inf)
        a = np.sqrt(km) * f32(1 - sqrt_err) * f32(1.000002)
        ef = (np.abs(fsx) + np.abs(fsy) + tmax) * f32(f32(2.0 ** -23) * f32(1.00001))
        b = a + f32(2) * ef
        settled = b * b * f32(1.000002) + f32(1e-30) < np.minimum(kr * f32(0.999998), f32(1e30))
    return settled, win


def issue_rule(qx, qy, tx, ty):
    """-> confirmed [query, target]: the confirmation set of the bound as the issue words it."""
    fsx, fsy, ftx, fty, d = squares32(qx, qy, tx, ty)
    d = d.astype(f64)
    E = 2.0 ** -23 * (np.abs(qx)[:, None] + np.abs(qy)[:, None] + np.abs(tx)[None, :] + np.abs(ty)[None, :])
    err = 2 * np.sqrt(2 * d) * E + 2 * E * E + 4 * 2.0 ** -24 * d
    return d - err <= np.min(d + err, axis=1)[:, None]


def check(qx, qy, tx, ty, expect_settled=None):
    """Both rules on one pair; -> number of settled queries."""
    dx, dy = qx[:, None] - tx[None, :], qy[:, None] - ty[None, :]
    D = dy * dy + dx * dx                                            # float64, as the kernel's scan to its last place
    near = D <= np.min(D, axis=1)[:, None] * CLASS                   # the true minimum's tie class
    assert np.all(near <= issue_rule(qx, qy, tx, ty))
    total = 0
    for sqrt_err in (0.0, 1.2e-7):
        settled, win = shipped(qx, qy, tx, ty, sqrt_err)
        only = np.zeros_like(near)
        only[np.arange(len(qx)), win] = True
        confirmed = np.where(settled[:, None], only, True)           # not settled: the float64 scan sees every candidate
        bad = near & ~confirmed
        assert not bad.any(), np.argwhere(bad)[:5]
        assert np.all(near[settled].sum(axis=1) == 1)
        total += int(settled.sum())
    if expect_settled is not None:
        assert (total > 0) == expect_settled, total
    return total // 2


def scan_pair(rng, n, span, kind, scale=1.0):
    ang = np.linspace(-span / 2, span / 2, n)
    ct, st = np.cos(ang), np.sin(ang)
    if kind == "noise":
        r = rng.uniform(0.1, 20, n)
    elif kind == "steps":
        r = np.round(rng.uniform(0.5, 8) + np.cumsum(rng.integers(-1, 2, n)) * 0.25, 2).clip(0.25, 30)
    else:
        r = 5 + np.sin(ang * 3 + rng.uniform(0, 6)) * 2 + rng.normal(0, 0.01, n)
    r = r.astype(f32).astype(f64) * scale
    tx, ty = ct * r, st * r
    th, tr = rng.normal(0, 0.02), rng.normal(0, 0.03, 2) * scale
    r2 = r * (1 + rng.normal(0, 0.005, n))
    qx = np.cos(th) * ct * r2 - np.sin(th) * st * r2 + tr[0]
    qy = np.sin(th) * ct * r2 + np.cos(th) * st * r2 + tr[1]
    return tx, ty, qx, qy


@pytest.mark.parametrize("n,span", [(360, 6.28318), (360, 4.712), (90, 3.0), (22, 4.0)])
@pytest.mark.parametrize("kind", ["noise", "steps", "smooth"])
def test_random_and_stepped_scans(n, span, kind):
    rng = np.random.default_rng(n * 11 + len(kind))
    settled = sum(check(*scan_pair(rng, n, span, kind)) for _ in range(12))
    assert settled > 0.9 * 12 * n                                    # (the bound is of use: nearly every query is settled)


@pytest.mark.parametrize("scale", [0.01, 1.0, 50.0])
def test_coordinates_from_centimetres_to_a_kilometre(scale):
    """Ranges of 0.05 ... 0.3 m, of metres, and of up to 1 000 m."""
    rng = np.random.default_rng(int(scale * 100))
    for kind in ("noise", "steps", "smooth"):
        for _ in range(6):
            check(*scan_pair(rng, 360, 4.712, kind, scale), expect_settled=True)


def test_offsets_a_million_times_the_spread():
    """float32 separates nothing: no query may be settled, every one goes to the float64 scan."""
    rng = np.random.default_rng(5)
    for off in ((1.0e6, -4.0e6), (3.0e7, 2.0e6)):
        for kind in ("noise", "steps", "smooth"):
            tx, ty, qx, qy = scan_pair(rng, 120, 4.712, kind, 0.25)
            check(tx + off[0], ty + off[1], qx + off[0], qy + off[1], expect_settled=False)


def test_exact_ties():
    """Two targets mirrored about the query's axis - the same square to the last bit - and coinciding targets: never
    settled; a lone nearest target next to them is."""
    rng = np.random.default_rng(6)
    qx, qy = rng.uniform(1, 10, 64), np.zeros(64)
    a, h = rng.uniform(-0.5, 0.5, 64), rng.uniform(0.01, 0.5, 64)
    for q in range(64):
        tx = np.array([qx[q] + a[q], qx[q] + a[q], qx[q] + 3.0, qx[q] - 4.0])
        ty = np.array([h[q], -h[q], 0.5, 0.25])
        settled, _ = shipped(qx[q:q + 1], qy[q:q + 1], tx, ty)
        assert not settled[0]
        check(qx[q:q + 1], qy[q:q + 1], tx, ty)
        tx2, ty2 = np.array([tx[0], tx[0], tx[2], tx[3]]), np.array([ty[0], ty[0], ty[2], ty[3]])    # coinciding targets
        assert not shipped(qx[q:q + 1], qy[q:q + 1], tx2, ty2)[0][0]
        check(qx[q:q + 1], qy[q:q + 1], tx2, ty2)
        check(qx[q:q + 1], qy[q:q + 1], tx[1:], ty[1:], expect_settled=True)
    circle = np.linspace(-3.14159, 3.14159, 360)                     # every beam equally far from a query at the centre
    settled, _ = shipped(np.zeros(1), np.zeros(1), 4.0 * np.cos(circle), 4.0 * np.sin(circle))
    assert not settled[0]
    check(np.zeros(1), np.zeros(1), 4.0 * np.cos(circle), 4.0 * np.sin(circle))


def test_near_ties_in_the_last_places_of_float64():
    """tests/golden/g10_sqrt_ties.npz's kind: two targets whose float64 squares differ by a few last places (one
    coordinate moved by some units in the last place) - a tie class of two.  Never settled."""
    rng = np.random.default_rng(10)
    checked = 0
    for _ in range(300):
        qx, qy = rng.uniform(-5, 5, 1), rng.uniform(-5, 5, 1)
        dx, dy = rng.uniform(0.05, 2.0), rng.uniform(0.05, 2.0)
        x1 = qx[0] + dx
        for _ in range(int(rng.integers(1, 4))):
            x1 = np.nextafter(x1, np.inf)
        tx = np.array([qx[0] + dx, x1, qx[0] + 5.0])
        ty = np.array([qy[0] + dy, qy[0] - dy, qy[0] + 1.0])
        D = (qx[0] - tx) ** 2 + (qy[0] - ty) ** 2
        if not (D[1] != D[0] and max(D[0], D[1]) <= min(D[0], D[1]) * CLASS):
            continue
        assert not shipped(qx, qy, tx, ty)[0][0]
        check(qx, qy, tx, ty)
        checked += 1
    assert checked > 100


def test_invalid_targets_and_queries():
    """NaN targets are +inf in the image and never win; a pair with a target that float32 cannot hold, an infinite or NaN
    query, or no finite target at all is never settled."""
    rng = np.random.default_rng(12)
    tx, ty, qx, qy = scan_pair(rng, 90, 3.0, "smooth")

    def image(t):                                                    # what the kernel writes for a NaN coordinate
        return np.where(np.isnan(t), np.inf, t)
    holes = tx.copy()
    holes[[0, 17, 18, 19, 89]] = np.nan
    D = (qx[:, None] - holes[None, :]) ** 2 + (qy[:, None] - ty[None, :]) ** 2
    settled, win = shipped(qx, qy, image(holes), ty)
    assert not settled.any()                                         # (tmax is infinite: the kernel skips NaN targets for tmax instead,
    keep = ~np.isnan(holes)                                          #  which is the pair without them)
    settled, win = shipped(qx, qy, holes[keep], ty[keep])
    assert settled.sum() > 60
    assert np.array_equal(np.flatnonzero(keep)[win[settled]], np.nanargmin(D, axis=1)[settled])
    for bad in (np.inf, -np.inf, np.nan, 1e39):
        q = qx.copy()
        q[3] = bad
        with np.errstate(invalid="ignore", over="ignore"):
            assert not shipped(q, qy, tx, ty)[0][3]
        t = tx.copy()
        t[40] = 1e39 if np.isnan(bad) else bad
        with np.errstate(invalid="ignore", over="ignore"):
            assert not shipped(qx, qy, t, ty)[0].any()
    assert not shipped(qx, qy, np.full(4, np.inf), np.full(4, np.inf))[0].any()
