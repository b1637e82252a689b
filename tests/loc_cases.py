"""Inputs of test_gpu_loc_replay_bounds.py (and the helpers test_gpu_loc_replay.py shares with it), built on the CPU:
seeded streams through the g5 room, the route tables, the padded allocations of the refused routes, the streams that
stop, the shapes on both sides of the 64-lane launch of ``k_loc_step``, the start poses that drive the scan matcher to
its iteration cap, and the hypothesis sets of the batch-invariance cases.  Nothing here touches the library;
test_loc_cases.py asserts, without a GPU, that every case has the property its GPU test relies on - above all that
each run compared with ``loc_ref.chain`` is stable under a nudge of ``xEst`` (the seeds are in the tables below)."""
import numpy as np

import loc_ref

AMIN, AMAX = -3.14159, 3.14159
KEYS = ("xest", "xodom", "P", "status", "T_obs", "iters_obs", "T_odom")
GUARD = 0x5A                     # the fill of the bounds tests (test_gpu_operator_bounds.py)
SPREAD = np.array([0.3, 0.3, 0.1])   # half-widths of a cloud of start-pose hypotheses


def make_stream(syn, seed, n, steps=8):
    """A seeded drive through the empty 10 m x 8 m room whose walls ``obs_wall`` lists -> (ranges [steps, n], pose0)."""
    rng = np.random.default_rng(seed)
    p = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.5, 0.5)])
    v, w = rng.uniform(0.02, 0.06), rng.uniform(-0.02, 0.02)
    poses = [p]
    for _ in range(steps - 1):
        p = poses[-1]
        poses.append(np.array([p[0] + v * np.cos(p[2]), p[1] + v * np.sin(p[2]), p[2] + w]))
    return syn.scans_from_poses(syn.World(5.0, 4.0, (), 0.0), np.array(poses), n, seed), poses[0]


def same_bits(a, b, keys=KEYS):
    return all(a[k].tobytes() == b[k].tobytes() for k in keys)


def pick(o, idx, keys=KEYS):
    return {k: np.ascontiguousarray(o[k][idx]) for k in keys}


def wall_subset(wall, K):
    """K obstacles taken evenly from the wall list (K = 0: the empty 2 x 0 list)."""
    if K == 0:
        return np.zeros((2, 0))
    return np.ascontiguousarray(wall[:, np.round(np.linspace(0, wall.shape[1] - 1, K)).astype(int)])


def hypotheses(pose, L, seed, spread=SPREAD):
    """L start poses around ``pose``; hypothesis 0 is ``pose`` itself."""
    p = np.asarray(pose, dtype=np.float64) + np.random.default_rng(seed).uniform(-1, 1, size=(L, 3)) * spread
    p[0] = pose
    return p


def raise_step(ranges, obstacle, pose0, **kw):
    """The step at which the CPU chain raises LinAlgError: the chain over the first k scans runs for k <= that step and
    raises for every longer prefix.  None when the whole stream runs."""
    first = None
    for k in range(1, len(ranges) + 1):
        try:
            loc_ref.chain(ranges[:k], obstacle, AMIN, AMAX, pose0, **kw)
            assert first is None, "the chain ran %d scans after raising at step %d" % (k, first)
        except np.linalg.LinAlgError:
            first = k - 1 if first is None else first
    return first


# ---- 1. random routing: 3 streams, 4 maps, 11 trajectories ---------------------------------------------------------

ROUTE_STREAM_SEEDS = (2, 4, 7)
ROUTE_DRAW_SEED = 1              # the generator of both route tables and of the start poses (0 leaves map 0 unused)
ROUTE_CHAIN = (0, 2, 8)          # the trajectories also compared with loc_ref.chain (stable: test_loc_cases.py)


def route_maps(wall):
    return [wall, np.ascontiguousarray(wall[:, ::2]), np.zeros((2, 0)), np.ascontiguousarray(wall[:, ::3])]


def routing_case(syn, wall, draw_seed=None):
    n, steps, L = 64, 4, 11
    streams = [make_stream(syn, s, n, steps) for s in ROUTE_STREAM_SEEDS]
    rng = np.random.default_rng(ROUTE_DRAW_SEED if draw_seed is None else draw_seed)
    sot = rng.integers(0, len(streams), size=L).astype(np.int32)
    mot = rng.integers(0, 4, size=L).astype(np.int32)
    pose0 = np.stack([streams[s][1] for s in sot]) + rng.uniform(-1, 1, size=(L, 3)) * np.array([0.05, 0.05, 0.02])
    return {"n": n, "ranges": np.stack([s[0] for s in streams]), "maps": route_maps(wall), "sot": sot, "mot": mot, "pose0": pose0}


def routing_properties(c):
    """What test 1 needs of the tables: neither monotone, every stream and map used, a shared (stream, map) pair."""
    sot, mot = c["sot"], c["mot"]
    mono = lambda a: bool(np.all(np.diff(a) >= 0) or np.all(np.diff(a) <= 0))
    pairs = {}
    for l, key in enumerate(zip(sot.tolist(), mot.tolist())):
        pairs.setdefault(key, []).append(l)
    shared = [v for v in pairs.values() if len(v) >= 2 and not np.array_equal(c["pose0"][v[0]], c["pose0"][v[1]])]
    return {"sot_not_monotone": not mono(sot), "mot_not_monotone": not mono(mot),
            "every_stream": set(sot.tolist()) == set(range(c["ranges"].shape[0])),
            "every_map": set(mot.tolist()) == set(range(len(c["maps"]))), "shared_pair": bool(shared),
            "route_differs_from_index": bool(np.any(sot != np.arange(len(sot)) % c["ranges"].shape[0]))}


# ---- 2. routes the kernel refuses, and an obs_off outside [0, K] ----------------------------------------------------

BAD_STREAM_SEEDS = (2, 4)
BAD_PAD_SEEDS = (7, 9)           # the streams that lie before and behind the real ones in the allocation
PAD_OBS = 64


def ring(centre, radius, count):
    a = np.arange(count) * (2 * np.pi / count)
    return np.vstack([centre[0] + radius * np.cos(a), centre[1] + radius * np.sin(a)])


def bad_route_case(syn, wall):
    """L = 6 over S = 2 streams and M = 2 maps; trajectories 1-4 each have one route entry out of range.  Every array a
    route indexes is the middle of a larger one whose padding is finite and would change the result: a stream before
    and behind ``ranges``, 64 obstacles 0.7 m around the start poses before and behind ``ox`` / ``oy``, two entries
    around ``obs_off`` - a guard that fails shows as a wrong status or wrong bits, never as a read outside an allocation."""
    n, steps, S, M = 64, 3, 2, 2
    streams = [make_stream(syn, s, n, steps) for s in BAD_STREAM_SEEDS]
    pads = [make_stream(syn, s, n, steps)[0] for s in BAD_PAD_SEEDS]
    maps = [wall, np.ascontiguousarray(wall[:, ::2])]
    sot = np.array([0, -1, S, 1, 0, 1], dtype=np.int32)
    mot = np.array([0, 0, 0, -1, M, 1], dtype=np.int32)
    rng = np.random.default_rng(3)
    pose0 = np.stack([streams[int(np.clip(s, 0, S - 1))][1] for s in sot])
    pose0 = pose0 + rng.uniform(-1, 1, size=(6, 3)) * np.array([0.05, 0.05, 0.02])
    K = sum(m.shape[1] for m in maps)
    centre = np.mean([s[1][:2] for s in streams], axis=0)
    pad_xy = ring(centre, 0.7, PAD_OBS)
    cat = np.concatenate(maps, axis=1)
    k1 = maps[0].shape[1]
    return {"n": n, "S": S, "M": M, "K": K, "k1": k1, "maps": maps, "sot": sot, "mot": mot, "pose0": pose0,
            "ranges": np.stack([s[0] for s in streams]),
            "ranges_padded": np.ascontiguousarray(np.stack([pads[0]] + [s[0] for s in streams] + [pads[1]]), dtype=np.float32),
            "ox_padded": np.concatenate([pad_xy[0], cat[0], pad_xy[0]]),
            "oy_padded": np.concatenate([pad_xy[1], cat[1], pad_xy[1]]),
            "off": np.array([0, k1, K], dtype=np.int64),
            "off_padded": np.array([0, 0, 0, k1, K, K + PAD_OBS, K + PAD_OBS], dtype=np.int64),
            # the second call: first entry negative, last past K; the kernel must clamp both to `off`
            "off_wild_padded": np.array([0, 0, -5, k1, K + 7, K + PAD_OBS, K + PAD_OBS], dtype=np.int64),
            "pad_xy": pad_xy, "good": (0, 5), "bad": (1, 2, 3, 4)}


# ---- 4. stops -------------------------------------------------------------------------------------------------------

STOP_STREAM_SEEDS = (2, 4, 7)
STOP_VALUES = [(np.inf, np.nan), (-np.inf, np.inf), (np.nan, -np.inf)]     # (stream A at step 0, stream B at step 3)
STOP_BEAMS = (17, 40)


def stop_case(syn, value_a, value_b):
    """S = 3 streams of 4 scans, two trajectories each (interleaved): one bad beam in scan 0 of stream A and in scan 3
    (the last) of stream B; stream C is clean."""
    n, steps = 64, 4
    streams = [make_stream(syn, s, n, steps) for s in STOP_STREAM_SEEDS]
    r = np.stack([s[0] for s in streams]).astype(np.float32)
    r[0, 0, STOP_BEAMS[0]] = value_a
    r[1, 3, STOP_BEAMS[1]] = value_b
    sot = np.array([0, 1, 2, 0, 1, 2], dtype=np.int32)
    pose0 = np.stack([streams[s][1] for s in sot])
    pose0[3:] += np.random.default_rng(8).uniform(-1, 1, size=(3, 3)) * np.array([0.05, 0.05, 0.02])
    return {"n": n, "ranges": r, "sot": sot, "pose0": pose0, "A": (0, 3), "B": (1, 4), "C": (2, 5)}


# ---- 5. both sides of the 64-lane launch of k_loc_step (n <= 64 and K <= 64) --------------------------------------

# (n, K, seed, eps of the stability probe).  With no obstacle every bin is 100.0 wherever the pose is, so the chain has no
# discontinuity in xEst at all, but the room matched against a circle of 100 m gives a transform whose translation is
# about 100 m, and z = compose(xEst, t) passes a nudge of the heading on with that gain (measured: 1.9e-9 at eps = 1e-11,
# linear in eps).  That case is probed with eps = 1e-13 against the same 1e-10.
LANE_CASES = [(63, 64, 0, 1e-11), (64, 64, 1, 1e-11), (65, 64, 2, 1e-11), (63, 65, 3, 1e-11), (64, 65, 4, 1e-11),
              (65, 65, 5, 1e-11), (8, 1, 6, 1e-11), (64, 0, 7, 1e-13)]


def lane_case(syn, wall, n, K, seed):
    r, p0 = make_stream(syn, seed, n, steps=3)
    return {"n": n, "ranges": r, "obstacle": wall_subset(wall, K), "pose0": p0}


def loc_step_threads(n, K):
    """launch_loc_step's rule, restated: the cases above must sit on both sides of it."""
    return 64 if n <= 64 and K <= 64 else 256


# ---- 6. iteration limits --------------------------------------------------------------------------------------------

ITER_STREAM_SEED = 2
ITER_OFFSETS = [(0.3, 0.3, 0.1), (1.5, -1.0, 0.6), (0.0, 0.0, 2.0)]
ITER_LIMITS = (0, 1, 5, 30)


def iter_case(syn, offset):
    r, p0 = make_stream(syn, ITER_STREAM_SEED, 120, steps=3)
    return {"n": 120, "ranges": r, "pose0": p0 + np.asarray(offset, dtype=np.float64)}


# ---- 7. the caller's increment ----------------------------------------------------------------------------------------

INC_SEED = 2
INC_N = 360
INC = 2 * np.pi / 360            # not (AMAX - AMIN) / 359


def increment_case(syn):
    r, p0 = make_stream(syn, INC_SEED, INC_N, steps=3)
    return {"n": INC_N, "ranges": r, "pose0": p0, "angle_increment": INC}


# ---- 8. scan-matcher launch shapes -----------------------------------------------------------------------------------

def icp_waves_at_two(B, n):
    """launch_icp's measure of a batch, restated: waves at two queries per lane."""
    return B * ((n + 127) // 128)


def hypotheses_case(syn, seed, n, steps, L, draw):
    """L start-pose hypotheses of one stream -> (ranges [steps, n], pose0 [L, 3], stream_of_traj zeros)."""
    r, p = make_stream(syn, seed, n, steps=steps)
    return r, hypotheses(p, L, draw), np.zeros(L, dtype=np.int32)


SHAPE_A = dict(seed=2, n=361, steps=2, L=2600, draw=21)       # 7 800 waves at two queries per lane in the per-step launch
SHAPE_C = dict(seed=4, n=200, steps=1, L=16500, draw=22)      # past 4 x kWaveRound pairs of more than 192 points
SHAPE_B_SEEDS, SHAPE_B_S, SHAPE_B_N = (2, 4, 7, 9), 2600, 200
SHAPE_B_ROUTES = (0, 1301, 2598, 2599)


def many_streams_case(syn):
    """S = 2 600 streams (four distinct ones in turn), n_scan = 2: 7 800 pairs in the stream-only launch; L = 4."""
    four = [make_stream(syn, seed, SHAPE_B_N, steps=2) for seed in SHAPE_B_SEEDS]
    r = np.stack([four[s % 4][0] for s in range(SHAPE_B_S)])
    sot = np.array(SHAPE_B_ROUTES, dtype=np.int32)
    return {"ranges": r, "sot": sot, "pose0": np.stack([four[s % 4][1] for s in sot]), "alone": [four[s % 4][0] for s in sot]}


OPTION_CASES = [("icp_qpt", 1), ("icp_qpt", 3), ("icp_one_wave", 1), ("icp_team", 1)]
OPTION_SEED = 2                  # streams of 120 and 361 beams, 3 steps


# ---- 9. bounds ----------------------------------------------------------------------------------------------------------

MAX_L = 65535
SMALL_SPREAD = np.array([0.05, 0.05, 0.02])


def max_hypotheses_case(syn, wall):
    """L = 65 535 over one stream of 8 beams and 16 obstacles; pose0 cycles through 5 distinct poses."""
    r, p = make_stream(syn, 6, 8, steps=2)
    five = hypotheses(p, 5, 24, spread=SMALL_SPREAD)
    return {"ranges": r, "five": five, "pose0": five[np.arange(MAX_L) % 5], "obstacle": wall_subset(wall, 16),
            "sot": np.zeros(MAX_L, dtype=np.int32)}


MANY_S, MANY_ROUTES = 65537, (0, 32768, 65536)


def stream_index_case(syn):
    """S = 65 537 streams of 16 beams, n_scan = 2: 196 611 stream-only pairs.  Streams 0, 32 768 and 65 536 are seeds
    2, 4, 7; every other stream is seed 9, so a pair index cut to 16 bits reads another stream's scans."""
    filler, a, b, c = [make_stream(syn, seed, 16, steps=2) for seed in (9, 2, 4, 7)]
    r = np.empty((MANY_S, 2, 16), dtype=np.float32)
    r[:] = filler[0]
    sot = np.array(MANY_ROUTES, dtype=np.int32)
    for s, stream in zip(sot, (a, b, c)):
        r[s] = stream[0]
    return {"ranges": r, "sot": sot, "pose0": np.stack([a[1], b[1], c[1]]), "alone": [a[0], b[0], c[0]], "filler": filler[0]}


# ---- 10. workspace ------------------------------------------------------------------------------------------------------

def loc_workspace_bytes(S, n_scan, n, L):
    """slam_loc_replay_dev's arena request, restated without its alignment: pair points and transforms, the step's pair,
    its transform and count, the 16-double state."""
    pairs = S * (2 * n_scan - 1)
    return pairs * 4 * n * 8 + pairs * 72 + 2 * L * 2 * n * 8 + L * 72 + L * 4 + L * 128


def workspace_case(syn):
    small = hypotheses_case(syn, 2, 64, 3, 2, 25)
    small = (small[0], hypotheses(small[1][0], 2, 25, spread=SMALL_SPREAD), small[2])
    return {"small": small, "large": hypotheses_case(syn, 4, 361, 2, 600, 26)}


# ---- 11. a long recurrence ---------------------------------------------------------------------------------------------

LONG_SEED, LONG_STEPS, LONG_EPS = 2, 64, 1e-12
