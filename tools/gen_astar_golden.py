#!/usr/bin/env python3
"""Generate tests/golden/g12_astar.npz by running the REFERENCE's own A* global planner.

TEST INFRASTRUCTURE ONLY; runs where the reference checkout lies, never on the GPU box.
NAV/global_planner.py (NAV = "W12_LiDAR SLAM/w12-mapping/course_agv_nav/scripts") is loaded
from where it lies, its tabs expanded and its Python-2 prints rewritten IN MEMORY by lib2to3's
fix_print, and exec'd with stub modules for rospy, tf and the message packages (the recipe of
oracle/gen_golden.py O4 / O5).  Only inputs and outputs are written:

  maps / inflated   every map as OccupancyGrid data [H][W] and as start_find leaves it (:148-155)
  queries           (map, start, goal) as find_path receives them ([row, col] before its -1)
  status            OK, INVALID_START / INVALID_GOAL (`return "None"`), NO_PATH (IndexError)
  paths             start_find's list reversed (start -> goal), [row, col]
  expansions        len(close_list) when start_find returned or raised
  planner_*         two successive plans of one GlobalPlanner (map_callback, init_pose_callback,
                    two goal_pose_callbacks): its map after each plan, start_map_point after
                    each plan (find_path shifts it in place) and the accumulated current_path

The course map is map.png through map_server's trinary rule (map.yaml: negate 1, occupied
0.65, free 0.196).  The serpentine case drives every open f past 100 000 before a room where
find_min_cost_f's index-0 fallback picks an entry whose f is not the smallest; the run checks
that this happened.  Every recorded case is also checked against tests/astar_ref.py.

Usage:  python tools/gen_astar_golden.py --reference <reference checkout> [--out tests/golden]
"""
from __future__ import annotations

import argparse
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import astar_ref  # noqa: E402

NAV = os.path.join("W12_LiDAR SLAM", "w12-mapping", "course_agv_nav", "scripts")
GAZEBO = os.path.join("W12_LiDAR SLAM", "w12-mapping", "course_agv_gazebo")
SPAN, R = 129, 2


class _Anything:
    def __init__(self, *a, **k):
        pass

    def __getattr__(self, name):
        return _Anything()

    def __call__(self, *a, **k):
        return _Anything()


class _Publisher:
    def __init__(self, *a, **k):
        self.sent = []

    def publish(self, msg):
        self.sent.append(msg)


def _ns(**k):
    return types.SimpleNamespace(**k)


class _Path:
    def __init__(self):
        self.header = _ns(stamp=None, frame_id="")
        self.poses = []


class _PoseStamped:
    def __init__(self):
        self.pose = _ns(position=_ns(x=0.0, y=0.0, z=0.0), orientation=_ns(x=0.0, y=0.0, z=0.0, w=1.0))


class Int8:
    """std_msgs Int8 is a message class: np.array(data, dtype=Int8) is an object array (:69)."""


def install_stubs():
    def mod(name, **attrs):
        m = sys.modules.get(name) or types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    mod("rospy", Publisher=_Publisher, Subscriber=_Anything, sleep=lambda *a: None, spin=lambda: None,
        Rate=_Anything, init_node=lambda *a, **k: None, get_rostime=lambda: 0.0)
    mod("tf")
    for pkg, names in (("nav_msgs.msg", dict(Path=_Path, OccupancyGrid=_Anything)),
                       ("nav_msgs.srv", dict(GetMap=_Anything)),
                       ("geometry_msgs.msg", dict(PoseStamped=_PoseStamped, Pose=_Anything)),
                       ("course_agv_nav.srv", dict(Plan=_Anything, PlanResponse=_Anything)),
                       ("gazebo_msgs.msg", dict(ModelStates=_Anything)),
                       ("std_msgs.msg", dict(Int8=Int8))):
        mod(pkg.split(".")[0])
        mod(pkg, **names)


def load_reference(root):
    from lib2to3.refactor import RefactoringTool
    install_stubs()
    path = os.path.join(root, NAV, "global_planner.py")
    text = open(path).read().expandtabs(8)
    tree = RefactoringTool(["lib2to3.fixes.fix_print"]).refactor_string(text + "\n", path)
    m = types.ModuleType("ref_global_planner")
    m.__file__ = path
    exec(compile(str(tree), path, "exec"), m.__dict__)
    return m


def course_map(root):
    from PIL import Image
    rgb = np.array(Image.open(os.path.join(root, GAZEBO, "models", "ground_plane_for_agv", "map", "map.png")))
    return astar_ref.map_from_png(rgb, negate=True, occupied_thresh=0.65, free_thresh=0.196)


def random_map(rng, H=129, W=129):
    m = np.zeros((H, W), np.int8)
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = 100
    for _ in range(14):                                   # wall segments
        r, c = int(rng.integers(5, H - 5)), int(rng.integers(5, W - 5))
        L = int(rng.integers(5, 40))
        if rng.random() < 0.5:
            m[r, c:c + L] = 100
        else:
            m[r:r + L, c] = 100
    for v, k in ((-1, 10), (50, 12)):                     # unknown blobs, SLAM's 50-valued unknowns
        for _ in range(k):
            r, c = int(rng.integers(3, H - 6)), int(rng.integers(3, W - 6))
            h, w = int(rng.integers(1, 5)), int(rng.integers(1, 5))
            m[r:r + h, c:c + w] = v
    return m


def serpentine_map():
    """200 x 200: a one-cell corridor of 60 rows joined at alternate ends (walls of 50, which
    neither inflate nor count as free), then a room below.  The goal lies in the room, close
    to the start in Manhattan terms, so g passes 100 000 long before the room."""
    H = W = 200
    m = np.full((H, W), 50, np.int8)
    rows = [3 + 2 * k for k in range(60)]
    for k, r in enumerate(rows):
        m[r, 3:W - 3] = 0
        if k + 1 < len(rows):
            m[r + 1, W - 4 if k % 2 == 0 else 3] = 0
    last = rows[-1]
    m[last + 1:last + 3, W - 4 if (len(rows) - 1) % 2 == 0 else 3] = 0
    m[last + 3:last + 15, 3:W - 3] = 0                    # the room
    return m, [rows[0] + 1, 5 + 1], [last + 12 + 1, 40 + 1]


def free_cells(imap, rng, k):
    rr, cc = np.nonzero(imap == 0)
    sel = rng.choice(len(rr), size=k, replace=False)
    return [[int(rr[i]) + 1, int(cc[i]) + 1] for i in sel]       # as find_path receives them


def obj_map(m):
    return np.array(list(np.asarray(m).reshape(-1)), dtype=Int8).reshape(m.shape)


def run_find_path(ref, m, start, goal, watch=None):
    """(status, path start -> goal, expansions, inflated map) of find_path(map, start, goal).start_find()."""
    om = obj_map(m)
    fp = ref.find_path(om, list(start), list(goal))
    if watch is not None:
        watch(fp)
    try:
        out = fp.start_find()
    except IndexError:
        return astar_ref.NO_PATH, np.zeros((0, 2), np.int32), len(fp.close_list), om.astype(np.int64)
    if isinstance(out, str):
        assert out == "None"
        st = astar_ref.INVALID_START if om[fp.start[0]][fp.start[1]] != 0 else astar_ref.INVALID_GOAL
        return st, np.zeros((0, 2), np.int32), 0, om.astype(np.int64)
    return astar_ref.OK, np.array(out[::-1], dtype=np.int32).reshape(-1, 2), len(fp.close_list), om.astype(np.int64)


def fallback_watch(flag):
    """Wraps find_min_cost_f: sets flag[0] when it returns index 0 while some other open entry has
    a smaller f (every f >= 100 000), i.e. when the clamp of the (min(f, 100000), seq) key decides."""
    def watch(fp):
        orig = fp.find_min_cost_f

        def wrapped():
            mc, idx = orig()
            if fp.open_list and mc == 100000 and idx == 0:
                if min(n.cost_f for n in fp.open_list) < fp.open_list[0].cost_f:
                    flag[0] = True
            return mc, idx
        fp.find_min_cost_f = wrapped
    return watch


def planner_case(ref, m, res, origin, start_xy, goals_xy):
    """Two successive plans of one GlobalPlanner: the first inflates its map in place,
    start_map_point is shifted by -1 on every plan (find_path mutates it) and current_path
    accumulates."""
    gp = ref.GlobalPlanner.__new__(ref.GlobalPlanner)
    gp.path_pub = _Publisher()
    gp.current_path = _Path()
    gp.start_map_point, gp.goal_map_point, gp.path_map, gp.path_world = [], [], [], []
    gp.if_start_find_path = False
    H, W = m.shape
    msg = _ns(info=_ns(origin=_ns(position=_ns(x=origin[0], y=origin[1])), resolution=res, width=W, height=H),
              data=[int(v) for v in m.reshape(-1)])
    gp.map_callback(msg)
    gp.init_pose_callback(_ns(pose=[None, _ns(position=_ns(x=start_xy[0], y=start_xy[1]))]))
    maps, counts, smp = [], [], []
    for gx, gy in goals_xy:
        gp.goal_pose_callback(_ns(pose=_ns(position=_ns(x=gx, y=gy))))
        maps.append(np.array(gp.map, dtype=np.int64))
        counts.append(len(gp.current_path.poses))
        smp.append(list(gp.start_map_point))
    xy = np.array([[p.pose.position.x, p.pose.position.y] for p in gp.current_path.poses], dtype=np.float64)
    return maps, np.array(counts, np.int32), xy, np.array(smp, np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    ref = load_reference(a.reference)
    rng = np.random.default_rng(12)

    maps, names, queries = [], [], []          # queries: (map, start, goal, name)
    course = course_map(a.reference)
    maps.append(course)
    names.append("course")
    ic = astar_ref.inflate(course, SPAN, R)
    for k, (s, g) in enumerate(zip(free_cells(ic, rng, 20), free_cells(ic, rng, 20))):
        queries.append((0, s, g, "course_%d" % k))
    occ = np.argwhere(ic[1:-1, 1:-1] == 99)[0] + 2
    fr = free_cells(ic, rng, 2)
    queries.append((0, [int(occ[0]), int(occ[1])], fr[0], "invalid_start"))
    queries.append((0, fr[1], [int(occ[0]), int(occ[1])], "invalid_goal"))
    queries.append((0, fr[0], list(fr[0]), "start_is_goal"))
    for t in range(3):
        m = random_map(rng)
        if t == 2:                                            # an enclosed free pocket: unreachable goal
            m[60:75, 60:75] = 100
            m[64:71, 64:71] = 0
        maps.append(m)
        names.append("random%d" % t)
        im = astar_ref.inflate(m, SPAN, R)
        cells = free_cells(im, rng, 16)
        for k in range(8):
            queries.append((len(maps) - 1, cells[2 * k], cells[2 * k + 1], "random%d_%d" % (t, k)))
        if t == 2:
            assert im[67, 67] == 0
            queries.append((len(maps) - 1, cells[0], [68, 68], "unreachable"))
    serp, s0, g0 = serpentine_map()
    maps.append(serp)
    names.append("serpentine")
    queries.append((len(maps) - 1, s0, g0, "serpentine"))

    res = []
    fallback = [False]
    for mi, s, g, name in queries:
        t0 = time.time()
        watch = fallback_watch(fallback) if name == "serpentine" else None
        st, path, exp, infl = run_find_path(ref, maps[mi], s, g, watch)
        o = astar_ref.plan(astar_ref.inflate(maps[mi], SPAN, R), s, g)
        assert o["status"] == st and o["expansions"] == exp and np.array_equal(o["path"], path), name
        res.append((mi, s, g, name, st, path, exp))
        print("%-16s %-13s len %5d exp %6d  %.2f s" % (name, astar_ref.STATUS_NAMES[st], len(path), exp,
                                                        time.time() - t0), flush=True)
    if not fallback[0]:
        raise SystemExit("the serpentine case never reached find_min_cost_f's index-0 fallback")
    inflated = []
    for m in maps:                       # a start on a non-free cell: start_find inflates, then returns "None"
        nz = np.argwhere(m != 0)[0] + 1
        st, _, _, im = run_find_path(ref, m, [int(nz[0]), int(nz[1])], [int(nz[0]), int(nz[1])])
        assert st == astar_ref.INVALID_START and np.array_equal(astar_ref.inflate(m, SPAN, R), im)
        inflated.append(im)

    # two successive plans of one GlobalPlanner on the course map (map.yaml: 0.155 m, origin -10, -10).
    # The start is chosen so that the second plan's start, shifted once more, is free too.
    pres, porg = 0.155, (-10.0, -10.0)
    ok = [c for c in free_cells(ic, rng, 400) if ic[c[0] - 2, c[1] - 2] == 0]
    cells = [ok[0], ok[1], ok[2]]
    to_xy = lambda rc: (porg[0] + (rc[1] + 0.5) * pres, porg[1] + (rc[0] + 0.5) * pres)   # noqa: E731
    start_xy = to_xy(cells[0])
    goals_xy = [to_xy(cells[1]), to_xy(cells[2])]
    pmaps, pcounts, pxy, psmp = planner_case(ref, course, pres, porg, start_xy, goals_xy)
    assert np.array_equal(pmaps[0], pmaps[1]) and np.array_equal(pmaps[0], inflated[0])
    print("planner: poses after each plan %s, start_map_point %s" % (pcounts.tolist(), psmp.tolist()))

    H = max(m.shape[0] for m in maps)
    W = max(m.shape[1] for m in maps)
    Q = len(res)
    Lmax = max(len(q[5]) for q in res)
    d = dict(
        map_names=np.array(names), map_h=np.array([m.shape[0] for m in maps], np.int32),
        map_w=np.array([m.shape[1] for m in maps], np.int32),
        maps=np.zeros((len(maps), H, W), np.int8), inflated=np.zeros((len(maps), H, W), np.int8),
        span=np.int32(SPAN), r=np.int32(R),
        names=np.array([q[3] for q in res]), map_of_query=np.array([q[0] for q in res], np.int32),
        starts=np.array([q[1] for q in res], np.int32), goals=np.array([q[2] for q in res], np.int32),
        status=np.array([q[4] for q in res], np.int32), path_len=np.array([len(q[5]) for q in res], np.int32),
        paths=np.full((Q, Lmax, 2), -1, np.int32), expansions=np.array([q[6] for q in res], np.int32),
        planner_resolution=np.float64(pres), planner_origin=np.array(porg, np.float64),
        planner_start_xy=np.array(start_xy, np.float64), planner_goals_xy=np.array(goals_xy, np.float64),
        planner_counts=pcounts, planner_path_xy=pxy, planner_start_map_point=psmp,
    )
    for k, (m, im) in enumerate(zip(maps, inflated)):
        d["maps"][k, :m.shape[0], :m.shape[1]] = m
        d["inflated"][k, :m.shape[0], :m.shape[1]] = im
    for k, q in enumerate(res):
        d["paths"][k, :len(q[5])] = q[5]
    path = os.path.join(a.out, "g12_astar.npz")
    np.savez_compressed(path, **d)
    print("wrote %s: %d maps, %d queries, %d bytes" % (path, len(maps), Q, os.path.getsize(path)))


if __name__ == "__main__":
    main()
