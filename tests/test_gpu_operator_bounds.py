"""The stand-alone operators behind the drop-in classes (k_scan_to_points, k_ranges64_to_points,
k_pose_compose, k_pose_step, k_kabsch, k_nn, k_grid_finalize, k_grid_datamap, k_grid_transpose) at
the sizes and edges of their launch shapes, through the C ABI, against the oracles
(oracle.c_oracle, oracle.oracle_np) or plain NumPy of the same operation.

What the cases are about:
  points from ranges  the float16 store rounds ONCE (inputs on float16 midpoints, moved off them by
                      2^-40 through the caller's trig table: a float32 step in between rounds them to
                      even), float16 subnormals, 65504 / 65520, both signs; the float32 store of a
                      float64 product; inf, -inf, NaN, +-0 and denormal ranges with clip_inf 0 / 1 in
                      every storage type; n = 1 and one element more than one trip of the grid-stride
                      loop (4 096 x 256 lanes; 2 048 x 256 for the float64 entry point);
  dead reckoning      every trajectory length around the 64-step chunks and the nc + 4 stages of the
                      four-wave pipeline (fewer than 4 chunks: fill and drain overlap), full-circle
                      rotations, the prefix property bit for bit, headings past 2 pi, atan2 at quarter
                      and half turns and on signed zeros, and the n == 1 routing between
                      k_pose_compose (L <= 64) and k_pose_step (L > 64);
  rigid fit           n past one pass of the 256-lane stride loop and off the wave size, three
                      different pairs per call, a set collapsed on ONE side only, NaN, exact quarter
                      and half turns, reflected clouds;
  nearest neighbour   the launch that raises the dynamic-LDS limit (nn_lds_bytes > 64 KiB) on both
                      sides of it, n_tar = 8 191 / 8 192, every storage type, exact ties of quantised
                      coordinates and near-ties decided by the reference's sqrt rule;
  map read-back       cell counts that are no multiple of 4 with G = 3 (maps 1, 2 start off a 16-byte
                      boundary: the uint4 loads and the scalar tail of k_grid_finalize), transpose
                      tiles cut on both sides, guard bytes behind every output.

Bars: integers, int8 maps and stored roundings bit-exact; poses and transforms 1e-9;
datamap 1e-9; NN distances 1e-14 (test_find_nearest_ties_nan_and_sizes).  Where bit patterns are
compared a NaN matches any NaN: sign and payload of an invalid operation's result (0 * inf) are the
processor's choice."""
import ctypes as C
import math

import numpy as np
import pytest

import icp_shapes
from conftest import pkg
from oracle import c_oracle as co
from oracle import oracle_np as on

gpu = pytest.mark.gpu
FTOL = 1e-9
EPS = 2.0 ** -40
POINT_LANES = 4096 * 256         # lanes of one trip of k_scan_to_points
POINT64_LANES = 2048 * 256       # ... of k_ranges64_to_points


@pytest.fixture(scope="module")
def slam():
    p = pkg()
    p._abi.default_context()
    return p


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_bits(got, want, tag=None):
    """Equal bit patterns (so -0 and inf count); a NaN matches any NaN."""
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape)
    bad = (bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), (tag, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])


# ---- 1. points from ranges -----------------------------------------------------------------------

HALF_EXPONENTS = (-14, -8, -3, 0, 4, 15)


def half_rounding_inputs():
    """Beams whose float64 product lies 2^-40 (relative) off a float16 midpoint -> (ranges float32 [n],
    cos_t [n], sin_t [n]).  The midpoints (m + 0.5) 2^(e-10), m = 1024 .. 2047, and the subnormal ones
    (k + 0.5) 2^-24, k = 0 .. 1023, are exact float32 values; x = (1 +- 2^-40) r and
    y = -(1 -+ 2^-40) r put every midpoint above and below, in both signs.  Then the overflow edge:
    65520 (1 - 2^-40) -> 65504, 65520 and 65520 (1 + 2^-40) -> inf.

    Asserted here, on the CPU: the construction is exact, and one rounding differs from two
    (float64 -> float32 -> float16) on HALF of the normal values (6 144 of 12 288 per coordinate) and
    of the subnormal ones (512 of 1 024 per table sign) - the midpoint goes to even in the second
    step, which is wrong whenever the true side is the odd neighbour; the issue asks for a third."""
    m = np.arange(1024, 2048, dtype=np.float64)
    normal = np.concatenate([(m + 0.5) * 2.0 ** (e - 10) for e in HALF_EXPONENTS])
    sub = (np.arange(1024, dtype=np.float64) + 0.5) * 2.0 ** -24
    mid = np.concatenate((normal, sub))
    r = np.concatenate((mid, mid, [65520.0, 65520.0, 65520.0]))
    up = np.concatenate((np.ones(mid.size), -np.ones(mid.size), [-1.0, 0.0, 1.0]))
    r32 = r.astype(np.float32)
    ct, st = 1.0 + up * EPS, -(1.0 - up * EPS)
    assert np.array_equal(r32.astype(np.float64), r) and np.array_equal(ct - 1.0, up * EPS) and np.array_equal(st + 1.0, up * EPS)
    with np.errstate(over="ignore"):
        for v in (ct * r, st * r):
            once, twice = v.astype(np.float16), v.astype(np.float32).astype(np.float16)
            differ = bits(once) != bits(twice)
            both = np.concatenate((differ[:normal.size], differ[mid.size:mid.size + normal.size]))
            assert both.sum() * 3 >= both.size and both.sum() * 2 == both.size == 12288, (both.sum(), both.size)
            for lo in (normal.size, mid.size + normal.size):            # the subnormals of each table sign
                assert differ[lo:lo + 1024].sum() == 512, differ[lo:lo + 1024].sum()
            edge_once, edge_twice = np.abs(once[-3:].astype(np.float64)), np.abs(twice[-3:].astype(np.float64))
            low = 0 if v[-1] > 0 else 2                                     # the entry with |table| = 1 - 2^-40
            assert edge_once[low] == 65504.0 and np.isinf(edge_twice[low])
            assert np.isinf(edge_once[1]) and np.isinf(edge_once[2 - low])
    return r32, np.ascontiguousarray(ct), np.ascontiguousarray(st)


def float_rounding_inputs():
    """The same for the float32 store: r = M 2^(e-23) with M odd in [2^23, 2^25 / 3), so that 1.5 r
    is a float32 midpoint (3 M / 2 is a half-integer below 2^24); the table holds 1.5 +- 2^-40.  No
    float32 arithmetic reaches the right neighbour: the float32 product of the rounded table entry
    (1.5) is the tie, which goes to even - asserted to differ from the one rounding of the float64
    product on about half of the values."""
    rng = np.random.default_rng(5)
    k = 6000
    M = 2 ** 23 + 2 * rng.integers(0, (2 ** 25 // 3 - 2 ** 23) // 2 - 1, size=k) + 1
    assert np.all(M % 2 == 1) and np.all(3 * M < 2 ** 25) and np.all(M >= 2 ** 23)
    r = M.astype(np.float64) * 2.0 ** (rng.integers(-40, 40, size=k) - 23)
    r32 = r.astype(np.float32)
    up = np.where(rng.random(k) < 0.5, 1.0, -1.0)
    ct, st = 1.5 + up * EPS, -(1.5 - up * EPS)
    assert np.array_equal(r32.astype(np.float64), r)
    for t in (ct, st):
        once, in_float = (t * r).astype(np.float32), t.astype(np.float32) * r32
        share = np.mean(bits(once) != bits(in_float))
        assert 1 / 3 <= share <= 2 / 3, share
    return r32, np.ascontiguousarray(ct), np.ascontiguousarray(st)


def test_rounding_inputs_tell_one_rounding_from_two():
    """The CPU-side condition of the two rounding tests, on its own: passes without a GPU."""
    half_rounding_inputs()
    float_rounding_inputs()


def to_points(slam, ranges, ct, st, clip, dtype):
    """slam_scan_to_points (dtype f64 / f32 / f16) or slam_scan_to_points_f64 (dtype r64: float64
    ranges) -> [B][2][n]."""
    A = slam._abi
    n = len(ct)
    h = A.default_context().handle
    if dtype == "r64":
        r = np.ascontiguousarray(ranges, dtype=np.float64).reshape(-1, n)
        out = np.empty((r.shape[0], 2, n))
        A.check(A.lib().slam_scan_to_points_f64(h, A.ptr(r), A.ptr(ct), A.ptr(st), r.shape[0], n, A.ptr(out)))
        return out
    r = np.ascontiguousarray(ranges, dtype=np.float32).reshape(-1, n)
    out = np.empty((r.shape[0], 2, n), dtype=A.NP_DTYPES[A.DTYPES[dtype]])
    A.check(A.lib().slam_scan_to_points(h, A.ptr(r), A.ptr(ct), A.ptr(st), r.shape[0], n, int(clip), A.DTYPES[dtype], A.ptr(out)))
    return out


NPDT = {"f64": np.float64, "f32": np.float32, "f16": np.float16, "r64": np.float64}


def want_points(ranges, ct, st, clip, dtype):
    """NumPy's: the float64 product of the table entry and the range, then ONE rounding to the
    storage type; with clip_inf only +inf becomes 30 m (slam_ekf.py:119)."""
    r = np.asarray(ranges).astype(np.float64).reshape(-1, len(ct))
    if clip:
        r = np.where(r == np.inf, 30.0, r)
    with np.errstate(all="ignore"):
        return np.stack((ct[None] * r, st[None] * r), axis=1).astype(NPDT[dtype])


@gpu
@pytest.mark.parametrize("dtype", ["f16", "f32", "f64"])
def test_points_round_once(slam, dtype):
    """float16: 7 168 midpoints of both signs from either side, the smallest subnormal
    ((0.5 2^-24) (1 + 2^-40) -> 2^-24, not 0), 65504 / inf; float32: 6 000 midpoints of a float64
    product.  Every input set goes through every storage type; bit patterns, no NaN among them."""
    for build in (half_rounding_inputs, float_rounding_inputs):
        r, ct, st = build()
        want = want_points(r, ct, st, 0, dtype)
        assert not np.isnan(want).any()
        got = to_points(slam, r, ct, st, 0, dtype)
        assert np.array_equal(bits(got), bits(want)), (dtype, build.__name__, int((bits(got) != bits(want)).sum()),
                                                        np.argwhere(bits(got) != bits(want))[:4].tolist())
    if dtype == "f16":
        r, ct, st = half_rounding_inputs()
        k = len(HALF_EXPONENTS) * 1024                                      # subnormal k = 0 under the + table
        assert r[k] == 2.0 ** -25 and to_points(slam, r, ct, st, 0, "f16")[0, 0, k] == np.float16(2.0 ** -24)


SPECIAL_RANGES = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, -5.9e-39, 6e-8, 2.98e-8, 30.0, -30.0,
                           65504.0, 65520.0, 3.4028235e38, -3.4028235e38, 1.0], dtype=np.float32)
SPECIAL_TABLE = [(1.0, 0.0), (0.0, 1.0), (-1.0, -0.0), (math.cos(0.3), math.sin(0.3)), (math.cos(2.5), math.sin(-2.5)),
                 (2.0 ** -10, -(2.0 ** -30)), (1.0 - EPS, -(1.0 + EPS))]


@gpu
@pytest.mark.parametrize("dtype,clip", [(d, c) for d in ("f16", "f32", "f64") for c in (0, 1)] + [("r64", 0)])
def test_points_special_ranges(slam, dtype, clip):
    """inf, -inf, NaN, +-0, float32 denormals, the float16 and float32 ends of range, against every
    kind of table entry (0 x inf = NaN, a negative zero, entries that push a product into the
    subnormals of the storage type).  Only +inf is clipped, and only by the float32 entry point
    with clip_inf (the float64 one has no such rule, localization.py:168-174)."""
    assert np.all(np.abs(SPECIAL_RANGES[5:9].astype(np.float64)) < 2.0 ** -126)      # denormal float32 they are
    ns, nt = len(SPECIAL_RANGES), len(SPECIAL_TABLE)
    ct = np.ascontiguousarray(np.repeat([t[0] for t in SPECIAL_TABLE], ns))
    st = np.ascontiguousarray(np.repeat([t[1] for t in SPECIAL_TABLE], ns))
    r = np.stack((np.tile(SPECIAL_RANGES, nt), np.tile(SPECIAL_RANGES[::-1], nt)))
    if dtype == "r64":
        r = r.astype(np.float64)
        r[0, :4] = [5e-324, -2.2e-308, 1.7976931348623157e308, -1e308]
    want = want_points(r, ct, st, clip, dtype)
    got = to_points(slam, r, ct, st, clip, dtype)
    assert_bits(got, want, (dtype, clip))
    if dtype != "r64":
        x_of_inf = want[0, 0, 0].astype(np.float64)                         # table (1, 0), range +inf
        assert (x_of_inf == 30.0) if clip else np.isinf(x_of_inf)
        assert np.isinf(want[0, 0, 1]) and np.isnan(want[0, 1, 0]) == (not clip)    # -inf stays; 0 x inf


@gpu
@pytest.mark.parametrize("B,n", [(1, 1), (2913, 361), (2048, 512)])
@pytest.mark.parametrize("dtype", ["f16", "f32", "f64", "r64"])
def test_points_sizes(slam, dtype, B, n):
    """n = 1; B n = 1 051 593 (neither factor a power of two: every lane of the 4 096 x 256 launch
    takes a second trip, and the float64 entry point's 2 048 x 256 a third); B n = 2^20 exactly.
    Every row: a row of a later trip must use the trig entry of ITS beam."""
    rng = np.random.default_rng(1000 * B + n)
    lanes = POINT64_LANES if dtype == "r64" else POINT_LANES
    assert B * n == 1 or B * n >= lanes
    if (B, n) == (2913, 361):
        assert POINT_LANES < B * n < POINT_LANES + 4096 and 2 * POINT64_LANES < B * n and B & (B - 1) and n & (n - 1)
    ct, st = slam._abi.trig_tables(-3.14159, 3.14159, n) if n > 1 else (np.array([math.cos(0.7)]), np.array([math.sin(0.7)]))
    r = rng.uniform(0.05, 60.0, size=(B, n)).astype(np.float32)
    at = rng.integers(0, B * n, size=min(64, B * n))
    r.reshape(-1)[at[::2]] = np.inf
    r.reshape(-1)[at[1::2]] = np.nan
    if dtype == "r64":
        r = r.astype(np.float64) * 1.0000001
    want = want_points(r, ct, st, 1 if dtype != "r64" else 0, dtype)
    got = to_points(slam, r, ct, st, 1, dtype)
    assert_bits(got, want, (dtype, B, n))
    if n > 1:
        assert len(np.unique(np.abs(ct))) > n // 4                          # the table does tell the beams apart


# ---- 2. dead reckoning ---------------------------------------------------------------------------

CHUNK_EDGES = [1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 321]


def compose(slam, T, p0):
    """slam_pose_compose: T [L][n][9], p0 [L][3] -> [L][n][3]."""
    A = slam._abi
    T, p0 = np.ascontiguousarray(T, dtype=np.float64), np.ascontiguousarray(p0, dtype=np.float64)
    L, n = T.shape[:2]
    out = np.full((L, n, 3), -777.25)
    A.check(A.lib().slam_pose_compose(A.default_context().handle, A.ptr(T), A.ptr(p0), L, n, A.ptr(out)))
    return out


def oracle_walk(T, p0):
    """co.compose_pose step by step."""
    L, n = T.shape[:2]
    out = np.empty((L, n, 3))
    for l in range(L):
        s = np.array(p0[l], dtype=np.float64)
        for k in range(n):
            s = co.compose_pose(s, T[l, k])
            out[l, k] = s
    return out


def motions(rng, shape, spread=1.0):
    """Rigid motions [..., 9]: rotations uniform over the circle, translations of order `spread`."""
    th = rng.uniform(-math.pi, math.pi, size=shape)
    T = np.zeros(tuple(shape) + (9,))
    T[..., 0], T[..., 1], T[..., 2] = np.cos(th), -np.sin(th), rng.normal(0, spread, shape)
    T[..., 3], T[..., 4], T[..., 5] = np.sin(th), np.cos(th), rng.normal(0, spread, shape)
    T[..., 8] = 1.0
    return T


def start_poses(rng, L):
    """Positions of order 3, headings of several turns."""
    return np.column_stack((rng.normal(0, 3.0, (L, 2)), rng.uniform(-20.0, 20.0, L)))


@pytest.fixture(scope="module")
def walk():
    """Three 321-step trajectories with data of their own, and the oracle's poses."""
    rng = np.random.default_rng(21)
    T, p0 = motions(rng, (3, 321)), start_poses(rng, 3)
    want = oracle_walk(T, p0)
    assert np.abs(p0[:, 2]).max() > 2 * math.pi and not np.array_equal(T[0], T[1])
    assert np.ptp(np.diff(want[0, :, 2])) > 6.0                             # the steps do turn by radians, both ways
    return T, p0, want


@pytest.fixture(scope="module")
def walk_full(slam, walk):
    return compose(slam, walk[0], walk[1])


@gpu
@pytest.mark.parametrize("n", CHUNK_EDGES)
def test_pose_compose_chunk_and_pipeline_edges(slam, walk, walk_full, n):
    """Every n from one step to five chunks and a step: below four chunks the fill and the drain of
    the pipeline overlap, at 64 k + 1 the last chunk holds one step.  With full-circle rotations a
    value taken from a neighbouring chunk or buffer is off by radians.  The n-step call equals the
    first n poses of the 321-step call bit for bit: no stage past the end leaks into the result."""
    T, p0, want = walk
    got = compose(slam, T[:, :n], p0)
    assert np.max(np.abs(got - want[:, :n])) < FTOL, (n, np.argwhere(np.abs(got - want[:, :n]) >= FTOL)[:4].tolist())
    assert np.array_equal(bits(got), bits(walk_full[:, :n])), (n, np.argwhere(bits(got) != bits(walk_full[:, :n]))[:4].tolist())


@gpu
def test_pose_compose_heading_is_not_wrapped(slam):
    """400 steps of +0.1 rad from 0.5: the heading passes 2 pi six times and goes on (icp.py:190)."""
    T = np.zeros((1, 400, 9))
    T[..., 0], T[..., 1], T[..., 2] = math.cos(0.1), -math.sin(0.1), 0.05
    T[..., 3], T[..., 4], T[..., 5] = math.sin(0.1), math.cos(0.1), -0.01
    T[..., 8] = 1.0
    p0 = np.array([[1.0, -2.0, 0.5]])
    want = oracle_walk(T, p0)
    got = compose(slam, T, p0)
    assert np.max(np.abs(got - want)) < FTOL
    assert got[0, -1, 2] == pytest.approx(40.5, abs=1e-9) and got[0, -1, 2] > 6 * 2 * math.pi
    assert np.all(np.diff(got[0, :, 2]) > 0.09)


def atan2_rows():
    """(T00, T10) of the edge cases: quarter and half turns, +-pi by the sign of a zero T10, both
    zero in all four sign combinations, rotation blocks scaled by 3 (the kernel takes atan2 of the
    entries, not a normalised angle), tiny and huge entries."""
    rows = [(0.0, 1.0), (0.0, -1.0), (-0.0, 1.0), (-0.0, -1.0), (-1.0, 0.0), (-1.0, -0.0), (1.0, 0.0), (1.0, -0.0),
            (0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0), (1e-310, 1e-310), (-1e300, 1e300), (5e-324, -5e-324)]
    rows += [(3.0 * math.cos(a), 3.0 * math.sin(a)) for a in (0.3, 1.9, -2.8, math.pi / 2, math.pi, -math.pi / 2)]
    rows += [(-3.0, 0.0), (-3.0, -0.0), (0.0, 3.0)]
    return rows


@gpu
def test_pose_compose_atan2_edges(slam):
    """delta_yaw = atan2(T10, T00) as math.atan2 gives it, signed zeros included (atan2(+0, -1) = pi,
    atan2(-0, -1) = -pi, atan2(+-0, -0) = +-pi, atan2(0, 0) = 0), through the three ways a step
    reaches a kernel: one step each of K trajectories (k_pose_compose), the K steps of one
    trajectory (the chain), and K trajectories tiled past 64 (k_pose_step)."""
    rows = atan2_rows()
    K = len(rows)
    assert K <= 64
    T = np.zeros((K, 9))
    for k, (t00, t10) in enumerate(rows):
        T[k] = [t00, -t10, 1.0 + 0.1 * k, t10, t00, -2.0 + 0.05 * k, 0, 0, 1]
    p0 = np.tile([0.5, -1.5, 0.25], (K, 1))
    want = oracle_walk(T[:, None], p0)
    for k, (t00, t10) in enumerate(rows):
        assert want[k, 0, 2] == 0.25 + math.atan2(t10, t00)
    assert want[4, 0, 2] - want[5, 0, 2] == pytest.approx(2 * math.pi) and want[8, 0, 2] == 0.25
    assert want[9, 0, 2] > 3.0 and want[10, 0, 2] == 0.25 and want[11, 0, 2] < -2.8       # atan2(+0, -0), (-0, +0), (-0, -0)
    got = compose(slam, T[:, None], p0)
    assert np.max(np.abs(got - want)) < FTOL, np.argwhere(np.abs(got - want) >= FTOL).tolist()
    rep = 5
    got = compose(slam, np.tile(T, (rep, 1))[:, None], np.tile(p0, (rep, 1)))
    assert K * rep > 64 and np.max(np.abs(got - np.tile(want, (rep, 1, 1)))) < FTOL
    chain = oracle_walk(T[None], p0[:1])
    got = compose(slam, T[None], p0[:1])
    assert np.max(np.abs(got - chain)) < FTOL, np.argwhere(np.abs(got - chain) >= FTOL).tolist()


@gpu
def test_pose_compose_route_boundary(slam):
    """n = 1: L <= 64 runs k_pose_compose (one workgroup per trajectory), L > 64 k_pose_step (one
    lane each) - documented as the same arithmetic, so the shared rows agree bit for bit; and
    L = 1, 64, 65, 257 against the oracle."""
    rng = np.random.default_rng(22)
    T, p0 = motions(rng, (257, 1)), start_poses(rng, 257)
    want = oracle_walk(T, p0)
    got = {L: compose(slam, T[:L], p0[:L]) for L in (1, 64, 65, 257)}
    for L, g in got.items():
        assert np.max(np.abs(g - want[:L])) < FTOL, L
    assert np.array_equal(bits(got[65][:64]), bits(got[64])), np.argwhere(bits(got[65][:64]) != bits(got[64]))[:4].tolist()
    assert np.array_equal(bits(got[257][:65]), bits(got[65])) and np.array_equal(bits(got[64][:1]), bits(got[1]))


# ---- 3. rigid fit --------------------------------------------------------------------------------

def kabsch(slam, src, tar):
    """slam_kabsch2d: paired rows src, tar [B][n][2] -> T [B][3][3]."""
    A = slam._abi
    s = np.ascontiguousarray(np.asarray(src, dtype=np.float64).transpose(0, 2, 1))
    t = np.ascontiguousarray(np.asarray(tar, dtype=np.float64).transpose(0, 2, 1))
    B, _, n = s.shape
    T = np.full((B, 9), -777.25)
    A.check(A.lib().slam_kabsch2d(A.default_context().handle, A.ptr(s), A.ptr(t), B, n, A.ptr(T)))
    return T.reshape(B, 3, 3)


def rot(a):
    return np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]])


def cloud(rng, n):
    """An anisotropic cloud away from the origin."""
    return rng.normal(0, [3.0, 1.0], size=(n, 2)) + rng.uniform(-5, 5, 2)


def assert_fit(got, src, tar, tag, numpy_too=True):
    for b in range(len(src)):
        want = co.get_transform(src[b], tar[b])
        assert np.max(np.abs(got[b] - want)) < FTOL, (tag, b, got[b], want)
        if numpy_too:
            assert np.max(np.abs(got[b] - on.get_transform(src[b], tar[b]))) < FTOL, (tag, b)


@gpu
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1000, 5000])
def test_kabsch_sizes_three_pairs(slam, n):
    """n below, at and above a wave and one pass of the 256-lane loop, up to 20 passes; three pairs
    with rotations and offsets of their own in one call."""
    rng = np.random.default_rng(300 + n)
    src = np.stack([cloud(rng, n) for _ in range(3)])
    angles = rng.uniform(-math.pi, math.pi, 3)
    tar = np.stack([src[b].dot(rot(angles[b]).T) + rng.uniform(-4, 4, 2) + rng.normal(0, 0.01, (n, 2)) for b in range(3)])
    got = kabsch(slam, src, tar)
    assert_fit(got, src, tar, n)
    if n >= 63:
        for b in range(3):
            d = math.atan2(got[b, 1, 0], got[b, 0, 0]) - angles[b]
            assert abs((d + math.pi) % (2 * math.pi) - math.pi) < 0.01       # three different answers
    assert np.all(got[:, 2] == [0.0, 0.0, 1.0])


POINTS = np.array([[0.1, 0.7], [1.0 / 3.0, -2.7], [1000.3, 7.77]])


@gpu
@pytest.mark.parametrize("n", [65, 300, 1000])
def test_kabsch_collapsed_on_one_side(slam, n):
    """Every source row one point and the target spread, then the converse: the canonical R = I,
    t = centroid_tar - centroid_src in both, for three points whose n-fold sums do
    not all divide back exactly.  All rows equal but the LAST: an ordinary fit."""
    rng = np.random.default_rng(310 + n)
    spread = np.stack([cloud(rng, n) for _ in range(3)])
    one = np.repeat(POINTS[:, None, :], n, axis=1)
    for src, tar, tag in ((one, spread, "source"), (spread, one, "target")):
        got = kabsch(slam, src, tar)
        assert_fit(got, src, tar, (tag, n))
        assert np.all(got[:, :2, :2] == np.eye(2)), (tag, got)
        assert np.max(np.abs(got[:, :2, 2] - (tar.mean(1) - src.mean(1)))) < FTOL
    almost = one.copy()
    almost[:, -1] += [0.5, -0.25]
    for src, tar, tag in ((almost, spread, "source"), (spread, almost, "target")):
        assert all(abs(co.get_transform(src[b], tar[b])[1, 0]) > 1e-3 for b in range(3))   # not the canonical answer
        got = kabsch(slam, src, tar)
        assert_fit(got, src, tar, (tag, "last row differs", n))
    got = kabsch(slam, one, one[::-1].copy())                              # both sides collapsed
    assert np.all(got[:, :2, :2] == np.eye(2)) and np.max(np.abs(got[:, :2, 2] - (POINTS[::-1] - POINTS))) < FTOL


@gpu
def test_kabsch_single_point_and_nan(slam):
    """n = 1 is collapsed on both sides.  A NaN in the FIRST row makes no row equal to it: not
    collapsed, and the NaN propagates as the C oracle's does - also when the other side is collapsed."""
    rng = np.random.default_rng(33)
    src, tar = rng.normal(size=(3, 1, 2)), rng.normal(size=(3, 1, 2))
    got = kabsch(slam, src, tar)
    assert_fit(got, src, tar, "n = 1")
    assert np.all(got[:, :2, :2] == np.eye(2)) and np.max(np.abs(got[:, :2, 2] - (tar - src)[:, 0])) < 1e-15
    n = 300
    src, tar = np.stack([cloud(rng, n) for _ in range(3)]), np.stack([cloud(rng, n) for _ in range(3)])
    src[0, 0, 0] = np.nan                                                  # x of the first source row
    tar[1, 0, 1] = np.nan                                                  # y of the first target row
    src[2] = src[2, 5]
    src[2, 0] = np.nan                                                     # NaN first, every other row one point
    got = kabsch(slam, src, tar)
    for b in range(3):
        want = co.get_transform(src[b], tar[b])
        assert np.array_equal(np.isnan(got[b]), np.isnan(want)), (b, got[b], want)
        assert np.isnan(want[:2]).all() and np.all(got[b, 2] == [0.0, 0.0, 1.0])
    one = np.repeat(POINTS[:, None, :], n, axis=1)                          # a NaN source against a collapsed target
    got = kabsch(slam, src[:1], one[:1])
    want = co.get_transform(src[0], one[0])
    assert np.array_equal(np.isnan(got[0]), np.isnan(want)) and np.all(got[0][~np.isnan(want)] == want[~np.isnan(want)])


@gpu
def test_kabsch_exact_rotations_and_reflections(slam):
    """target = source turned by exactly 90, 180 and by 179.999 degrees, and mirrored clouds (the
    reflection fix of icp.py:164-169), n = 300.  Matrices are compared, not angles: at 180 degrees
    the angle's sign is a rounding accident, the matrix is not."""
    rng = np.random.default_rng(34)
    n = 300
    src = np.stack([cloud(rng, n) for _ in range(3)])
    quarter, half = np.array([[0.0, -1.0], [1.0, 0.0]]), np.array([[-1.0, 0.0], [0.0, -1.0]])
    R = [quarter, half, rot(math.radians(179.999))]
    tar = np.stack([src[b].dot(R[b].T) + [0.5 * b, -1.0] for b in range(3)])
    got = kabsch(slam, src, tar)
    assert_fit(got, src, tar, "rotations")
    for b in range(3):
        assert np.max(np.abs(got[b, :2, :2] - R[b])) < FTOL, (b, got[b])
    mirror = [np.diag([1.0, -1.0]), np.diag([-1.0, 1.0]).dot(rot(0.7)), rot(-2.0).dot(np.diag([1.0, -1.0]))]
    tar = np.stack([src[b].dot(mirror[b].T) + [0.5 * b, -1.0] for b in range(3)])
    got = kabsch(slam, src, tar)
    assert_fit(got, src, tar, "reflections")
    assert np.max(np.abs(np.linalg.det(got[:, :2, :2]) - 1.0)) < FTOL        # a rotation all the same


# ---- 4. nearest neighbour, the operator ------------------------------------------------------------

NN_SMALL, NN_RAISED = 3344, 3345


def test_nn_lds_threshold_arithmetic():
    """launch_nn_t raises the kernel's dynamic-LDS limit when nn_lds_bytes(n_tar) > 64 KiB = 65 536.
    Per block 272 bytes of points; per 4 blocks 5 boxes = 160 bytes.
      n_tar = 3 344: 209 blocks -> 209 * 272 = 56 848, boxes padded to 212 -> (212 + 53) * 32 = 8 480: 65 328 <= 65 536;
      n_tar = 3 345: 210 blocks -> 210 * 272 = 57 120, boxes 212 -> 8 480: 65 600 > 65 536;
      n_tar = 8 192: 512 blocks -> 139 264 + (512 + 128) * 32 = 159 744 <= 160 KiB, the kernel's bound.
    Passes without a GPU; the sizes are the library's own (slam_plan_query)."""
    nn_lds_bytes = icp_shapes.nn_lds_bytes
    assert nn_lds_bytes(NN_SMALL) == 56848 + 8480 == 65328 <= 64 * 1024
    assert nn_lds_bytes(NN_RAISED) == 57120 + 8480 == 65600 > 64 * 1024
    assert all(nn_lds_bytes(n) <= 64 * 1024 for n in range(1, NN_SMALL + 1))
    assert all(nn_lds_bytes(n) > 64 * 1024 for n in range(NN_RAISED, 8193))
    assert nn_lds_bytes(8191) == nn_lds_bytes(8192) == 159744 <= 160 * 1024
    assert icp_shapes.LDS_DEFAULT == 64 * 1024 and icp_shapes.LDS_LIMIT == 160 * 1024      # launch_nn_t's two limits


def nn_clouds(rng, n_src, n_tar):
    """One pair -> (src [n_src][2], tar [n_tar][2]), float64, three kinds of points in each:
      staircase  the first third of the targets is a polar scan with ranges in steps of 0.25; every
                 staircase query sits on a beam whose two neighbours hold the query's range, mirror
                 images of each other about the query's beam: tied in real arithmetic, their squares
                 round apart, and where they share a square root the reference's rule (lowest
                 index) differs from the order of the squares;
      lattice    targets on multiples of 1/4 (many sites taken twice: exact ties, the lower index
                 wins), queries on multiples of 1/8 (equidistant from 2 or 4 sites);
      free       uniform in the square, one NaN among the targets and one among the queries."""
    kt, ks = n_tar // 3, n_src // 3
    ang = np.linspace(-math.pi, math.pi, kt, endpoint=False)
    rt = np.clip(3.0 + 0.25 * np.cumsum(rng.integers(-1, 2, size=kt)), 0.5, 6.0)
    beams = 1 + 3 * rng.choice((kt - 2) // 3, size=ks, replace=False)
    rq = rt[beams]
    rt[beams - 1] = rt[beams + 1] = rq
    rt[beams] = rq + 0.25
    tar = [np.column_stack((np.cos(ang) * rt, np.sin(ang) * rt)),
           rng.integers(-24, 25, size=(kt, 2)) * 0.25, rng.uniform(-6.0, 6.0, size=(n_tar - 2 * kt, 2))]
    src = [np.column_stack((np.cos(ang[beams]) * rq, np.sin(ang[beams]) * rq)),
           rng.integers(-48, 49, size=(ks, 2)) * 0.125, rng.uniform(-6.0, 6.0, size=(n_src - 2 * ks, 2))]
    tar[2][3, 0] = np.nan
    src[2][1, 1] = np.nan
    return np.vstack(src), np.vstack(tar)


def nn_pairs(n_src, n_tar):
    """Three pairs of nn_clouds, drawn again from the case's seed until the C oracle counts, in
    float64, at least one query that ordering by the square would answer differently (about one
    mirrored pair in a hundred shares a square root with squares that differ)."""
    rng = np.random.default_rng(4000 + n_tar + 7 * n_src)
    for _ in range(64):
        pairs = [nn_clouds(rng, n_src, n_tar) for _ in range(3)]
        co.nn_rule_splits()
        for s, t in pairs:
            co.find_nearest(s, t)
        if co.nn_rule_splits() > 0:
            return pairs
    raise AssertionError("no draw exercises the tie rule")


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32", "f16"])
@pytest.mark.parametrize("n_src", [255, 256, 257])
@pytest.mark.parametrize("n_tar", [NN_SMALL, NN_RAISED, 8191, 8192])
def test_nn_operator_sizes_and_storage(slam, n_tar, n_src, dtype):
    """slam_nn on three different pairs per call: the last n_tar under the 64 KiB of dynamic LDS and
    the first that needs the limit raised, and the largest two; n_src around one workgroup of
    queries.  The oracle is fed the points as the storage type rounds them.  Indices exact,
    distances to 1e-14.  In float64 the oracle counts queries on which ordering by the square would
    pick another target than the reference's rule: the exact pass ran."""
    A = slam._abi
    npdt = NPDT[dtype]
    pairs = nn_pairs(n_src, n_tar)
    src = np.ascontiguousarray(np.stack([p[0].T for p in pairs]).astype(npdt))     # [B][2][n_src]
    tar = np.ascontiguousarray(np.stack([p[1].T for p in pairs]).astype(npdt))
    dist, idx = np.full((3, n_src), -1.0), np.full((3, n_src), -1, dtype=np.int32)
    A.check(A.lib().slam_nn(A.default_context().handle, A.ptr(src), A.ptr(tar), 3, n_src, n_tar, A.DTYPES[dtype],
                            A.ptr(dist), A.ptr(idx)))
    co.nn_rule_splits()
    ties = 0
    for b in range(3):
        s64, t64 = src[b].astype(np.float64).T, tar[b].astype(np.float64).T
        wd, wi = co.find_nearest(s64, t64)
        assert np.array_equal(idx[b], wi), (b, np.nonzero(idx[b] != wi)[0][:8], idx[b][idx[b] != wi][:8], wi[idx[b] != wi][:8])
        assert np.max(np.abs(dist[b] - wd)) < 1e-14, b
        d2 = ((s64[n_src // 3:2 * (n_src // 3), None, :] - t64[None, :, :]) ** 2).sum(-1)     # the lattice queries: exact squares
        ties += int(np.sum(np.sum(d2 == np.nanmin(d2, axis=1, keepdims=True), axis=1) > 1))
        assert wi[2 * (n_src // 3) + 1] == 0 and wd[2 * (n_src // 3) + 1] == 0.0               # the NaN query: (0, index 0)
    splits = co.nn_rule_splits()
    assert ties >= 20, ties                                                 # exact ties are there at this size
    if dtype == "f64":
        assert splits > 0, splits


# ---- 5. map read-back ----------------------------------------------------------------------------

GRIDS = [(37, 203), (5, 3), (33, 31), (64, 32), (1, 1)]
GUARD = 0x5A                     # 90: no value a pmap holds


def at(c):
    """A world coordinate whose cell is c under scale 1, offset 0 (int() truncates toward zero)."""
    return c + 0.5 if c >= 0 else c - 0.5


def border(xw, yw):
    cells = [(x, 0) for x in range(xw)] + [(xw - 1, y) for y in range(1, yw)]
    cells += [(x, yw - 1) for x in range(xw - 2, -1, -1)] + [(0, y) for y in range(yw - 2, 0, -1)]
    return list(dict.fromkeys(cells))


def fan_scans(xw, yw):
    """Per map two scans of equal length -> [(ox, oy, cx, cy, map)]: from the centre cell to every
    border cell (hits) and to cells two past every third one (rays that leave the map); from an
    origin outside the map to every other border cell.  Each map its own subsets."""
    ring = border(xw, yw)
    out = []
    for gi in range(3):
        ends = list(ring)
        for x, y in ring[gi::3]:
            ends.append((x + 2 * ((x == xw - 1) - (x == 0)), y + 2 * ((y == yw - 1) - (y == 0))))
        out.append((ends, (xw // 2, yw // 2), gi))
        out.append(([c for k, c in enumerate(ring) if k % 2 == gi % 2] or [(-2, yw // 2 + gi)], (-2, yw // 2 + gi), gi))
    n = max(len(e) for e, _, _ in out)
    scans = []
    for ends, org, gi in out:
        ends = ends + [org] * (n - len(ends))                               # an end in the origin's cell: an empty path
        scans.append((np.array([at(x) for x, _ in ends]), np.array([at(y) for _, y in ends]), at(org[0]), at(org[1]), gi))
    return scans


def line_scans(xw, yw):
    """1 000 + gi rays from cell (0, 0) to a cell outside the far corner, into map gi: the cells of the
    line hold 1 000, 1 001 and 1 002 passes - below, at and above the pass threshold (1 001)."""
    n = 1002
    scans = []
    for gi in range(3):
        ox, oy = np.full(n, at(0)), np.full(n, at(0))                       # padding: empty paths ...
        ox[:1000 + gi], oy[:1000 + gi] = at(xw + 1), at(yw)
        if gi == 0:
            ox[-1] = np.inf                                                 # ... and a beam mapping.py:30 skips
        scans.append((ox, oy, at(0), at(0), gi))
    return scans


def cast(grid, oracles, scans):
    grid.update_host(np.stack([s[0] for s in scans]), np.stack([s[1] for s in scans]), [s[2] for s in scans],
                     [s[3] for s in scans], grid_of_batch=[s[4] for s in scans])
    for ox, oy, cx, cy, gi in scans:
        oracles[gi].update(ox, oy, cx, cy)


def canonical_pmap(og, hit_inc):
    """The integer rule on the oracle's counters (hits first) and the cells on which the
    reference's own answer depends on the order of arrival (none for hit_inc > thresh)."""
    table = on.occupied_rule(0.01, hit_inc, 10.0)
    p, h = og.pass_cnt.astype(np.int64), og.hit_cnt.astype(np.int64)
    occ = h >= len(table)
    sens = np.zeros(p.shape, dtype=bool)
    for k, t in enumerate(table):
        occ |= (h == k) & (p >= t)
        if k >= 1:
            sens |= (h == k) & ((p == t) | (p == t - 1))
    return np.where(p + h > 0, np.where(occ, 100, 0), 50).astype(np.int8), sens


def read_guarded(slam, grid, gi):
    """slam_grid_read and slam_grid_occupancy_data of map gi into host buffers one guard line longer."""
    A = slam._abi
    per, line = grid.xw * grid.yw, grid.yw
    fills = {"pmap": (np.int8, GUARD), "datamap": (np.float64, -777.25), "pass": (np.uint32, 0xA5A5A5A5),
             "hit": (np.uint32, 0xA5A5A5A5), "data": (np.int8, GUARD)}
    bufs = {k: np.full(per + line, v, dtype=dt) for k, (dt, v) in fills.items()}
    h = grid._ctx.handle
    A.check(A.lib().slam_grid_read(h, grid._h, gi, A.ptr(bufs["pmap"]), A.ptr(bufs["datamap"]), A.ptr(bufs["pass"]), A.ptr(bufs["hit"])))
    A.check(A.lib().slam_grid_occupancy_data(h, grid._h, gi, A.ptr(bufs["data"])))
    out = {}
    for k, b in bufs.items():
        assert np.all(b[per:] == fills[k][1]), (k, gi)
        out[k] = b[:per].reshape(grid.xw, grid.yw) if k != "data" else b[:per]
    return out


def finalize_guarded(slam, grid, front):
    """slam_grid_finalize_dev of all maps into a caller's buffer that starts `front` bytes (a multiple
    of 16) into a pattern-filled allocation and ends a guard line before its end."""
    import torch
    A = slam._abi
    ctx = grid._ctx
    per, line = grid.xw * grid.yw, max(grid.yw, 16)
    buf = torch.full((front + grid.G * per + line,), GUARD, dtype=torch.int8, device=torch.device("cuda", ctx.device))
    torch.cuda.synchronize()
    A.check(A.lib().slam_grid_finalize_dev(ctx.handle, grid._h, buf.data_ptr() + front))
    ctx.synchronize()
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    assert np.all(b[:front] == GUARD) and np.all(b[front + grid.G * per:] == GUARD), front
    return b[front:front + grid.G * per].reshape(grid.G, grid.xw, grid.yw)


@gpu
@pytest.mark.parametrize("live", [False, True])
@pytest.mark.parametrize("hit_inc", [20.0, 4.0])
@pytest.mark.parametrize("xw,yw", GRIDS)
def test_map_read_back(slam, xw, yw, hit_inc, live):
    """Three maps of xw x yw cells (7 511 = 3 mod 4; 15; 1 023; 2 048; 1), index rule int(x): a line
    of cells driven to 1 000 / 1 001 / 1 002 passes, fans that hit every border cell and leave the
    map, scans through slam_grid_update_scans (they go to map 0).  Then every read-back of every
    map against the C oracle's grid: counters, pmap and OccupancyGrid data exact, datamap to 1e-9,
    data[y xw + x] == pmap[x][y], guard bytes untouched - with and without a live pmap."""
    A = slam._abi
    ctx = slam.Context(0)
    grid = slam.DeviceGrid(3, xw, yw, 1.0, 0.0, 0.0, hit_inc=hit_inc, context=ctx)
    if live:
        grid.live_pmap()
    oracles = [co.Grid(xw, yw, 1.0, 0.0, 0.0, 0.01, hit_inc, 10.0) for _ in range(3)]
    cast(grid, oracles, line_scans(xw, yw))
    for gi in range(3):                                                     # the threshold itself, before anything else arrives
        r = grid.read(gi, want=("pmap", "pass"))
        assert r["pass"][0, 0] == 1000 + gi and r["pmap"][0, 0] == (100 if gi >= 1 else 0), (gi, r["pass"][0, 0], r["pmap"][0, 0])
        assert np.array_equal(r["pmap"], oracles[gi].pmap), gi
    fans = fan_scans(xw, yw)
    cast(grid, oracles, fans)
    cast(grid, oracles, fans[::2])                                          # hits twice: 8 > thresh is false for + 4, 12 > thresh true
    rng = np.random.default_rng(50 + xw)
    S, n = 4, 48
    ct, st = A.trig_tables(-3.14159, 3.14159, n)
    ranges = rng.uniform(0.3, 0.8 * max(xw, yw) + 2.0, size=(S, n)).astype(np.float32)
    ranges[1, 5] = np.inf                                                   # clipped to 30 m (slam_ekf.py:119)
    poses = np.column_stack((rng.uniform(0.2, xw - 0.2, S), rng.uniform(0.2, yw - 0.2, S), rng.uniform(-3.0, 3.0, S)))
    A.check(A.lib().slam_grid_update_scans(ctx.handle, grid._h, A.ptr(ranges), A.ptr(ct), A.ptr(st), A.ptr(poses), None, S, n))
    for k in range(S):
        obs = on.world_points(poses[k], on.laser_to_numpy(ranges[k], -3.14159, 3.14159, clip_inf=True))
        oracles[0].update(obs[0], obs[1], poses[k, 0], poses[k, 1])
    ctx.check_status()
    want = [canonical_pmap(og, hit_inc) for og in oracles]
    reads = []
    for gi, og in enumerate(oracles):
        r = read_guarded(slam, grid, gi)
        assert np.array_equal(r["pass"], og.pass_cnt) and np.array_equal(r["hit"], og.hit_cnt), gi
        assert np.array_equal(r["pmap"], want[gi][0]), (gi, np.argwhere(r["pmap"] != want[gi][0])[:6].tolist())
        keep = ~want[gi][1]
        assert np.array_equal(r["pmap"][keep], og.pmap[keep]), gi            # the oracle's own float sums
        assert hit_inc == 4.0 or keep.all()
        assert np.max(np.abs(r["datamap"] - og.datamap)) < FTOL, gi
        assert np.array_equal(r["data"], r["pmap"].T.reshape(-1)), gi        # data[y xw + x] == pmap[x][y]
        if keep.all():
            assert np.array_equal(r["data"], og.occupancy_grid_data()), gi
        reads.append(r)
    if xw * yw > 1:
        ring = border(xw, yw)
        for gi in range(3):
            assert all(reads[gi]["hit"][c] + reads[gi]["pass"][c] > 0 for c in ring), gi      # the border was reached
        assert not np.array_equal(reads[1]["pass"], reads[2]["pass"])
    pm = finalize_guarded(slam, grid, 64)
    for gi in range(3):
        assert np.array_equal(pm[gi], reads[gi]["pmap"]), gi
    grid.close()
    ctx.close()
