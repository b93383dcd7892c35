"""CPU restatement of fuelmi_map_goal_paths: the geometric part of FastExplorationManager::planExploreMotion
(exploration_manager/src/fast_exploration_manager.cpp:234-276) with shortenPath (:295-325).

The raw path is the lattice path of tests/path_cost_ref.py (Lattice.dijkstra / csgraph_dist + Lattice.search, WITHOUT
straight_line_safe: the manager calls Astar::search directly); shortenPath, the length, the branch and the truncation
are the reference's sequential loops, line by line; the ray is path_cost_ref.ray_voxels with the predicate of :311-312
(no box test; a voxel outside the map reads -1 twice and passes).  first_push_shorten() is the form the device kernel
uses; it is here only so that the CPU tests can state that both forms agree.  The scenes the GPU tests run are built
here too, so that the CPU tests can check that they are what they claim."""
import math

import numpy as np

import path_cost_ref as pr

CLOSE, MID, FAR, NO_PATH = 0, 1, 2, 3
RAW_OVER = -1  # the raw path has more than max_path_points points (FUELMI_ELIMIT)
WINDOW = 64    # k_goal_shorten's window (GS_WIN in fuel_amd/csrc/goal_path.hip)
DEFAULTS = dict(res=0.2, edge_step=0.1, shorten_dist=3.0, end_eps=1e-3, radius_close=1.5, radius_far=5.0)


def dist(a, b):
    return pr.norm3(a[0] - b[0], a[1] - b[1], a[2] - b[2])


def ray_blocked(pm, om, a, b):
    """:308-316: some voxel of RayCaster::input(a, b) / nextId has getInflateOccupancy == 1 or getOccupancy == UNKNOWN"""
    for v in pr.ray_voxels(om, a, b):
        if all(0 <= v[k] < pm.nvox[k] for k in range(3)) and pm.bad[v[0], v[1], v[2]]:
            return True
    return False


def shorten_loop(pm, om, path, shorten_dist=3.0, log=None):
    """shortenPath's loop (:302-318), literally.  log collects ("dist" | "ray", i) per push."""
    short = [path[0]]
    for i in range(1, len(path) - 1):                           # :303
        if dist(path[i], short[-1]) > shorten_dist:             # :304
            short.append(path[i])
            if log is not None:
                log.append(("dist", i))
        elif ray_blocked(pm, om, short[-1], path[i + 1]):        # :308-316
            short.append(path[i])
            if log is not None:
                log.append(("ray", i))
    return short


def shorten(pm, om, path, shorten_dist=3.0, end_eps=1e-3, log=None):
    """shortenPath (:295-325)"""
    short = shorten_loop(pm, om, path, shorten_dist, log)
    if dist(path[-1], short[-1]) > end_eps:                     # :319
        short.append(path[-1])
    if len(short) == 2:                                         # :322-323
        short.insert(1, np.array([0.5 * (short[0][k] + short[1][k]) for k in range(3)]))
    return short


def first_push_shorten(pm, om, path, shorten_dist=3.0, end_eps=1e-3, runs=None):
    """the same result as the first candidate behind each anchor for which push(i) holds, every candidate judged
    against the anchor alone.  runs collects, per anchor, how many candidates behind it did not push."""
    short = [path[0]]
    i0, n = 1, len(path)
    while i0 <= n - 2:
        a = short[-1]
        hit = None
        for i in range(i0, n - 1):
            if dist(path[i], a) > shorten_dist or ray_blocked(pm, om, a, path[i + 1]):
                hit = i
                break
        if runs is not None:
            runs.append((hit if hit is not None else n - 1) - i0)
        if hit is None:
            break
        short.append(path[hit])
        i0 = hit + 1
    if dist(path[-1], short[-1]) > end_eps:
        short.append(path[-1])
    if len(short) == 2:
        short.insert(1, np.array([0.5 * (short[0][k] + short[1][k]) for k in range(3)]))
    return short


def branch(short, goal, radius_close=1.5, radius_far=5.0):
    """:242-276: (status, length, way-points, next_goal, points the truncation dropped)"""
    length = pr.path_length(short)                               # :244
    if length < radius_close:                                    # :245
        return CLOSE, length, short, goal, 0
    if length > radius_far:                                      # :251
        len2 = 0.0
        trunc = [short[0]]
        i = 1
        while i < len(short) and len2 < radius_far:              # :257
            len2 += dist(short[i], trunc[-1])
            trunc.append(short[i])
            i += 1
        return FAR, length, trunc, trunc[-1], len(short) - len(trunc)
    return MID, length, short, goal, 0


class Source:
    """one start's lattice with its distances (shared by every problem from that start)"""

    def __init__(self, pm, start, res=0.2, edge_step=0.1, csgraph=False):
        self.lat = pr.Lattice(pm, start, res, edge_step)
        self.lat.d = self.lat.csgraph_dist() if csgraph else self.lat.dijkstra()

    def raw(self, goal):
        """Astar::search(start, goal) -> getPath (:234-239) as the lattice path; None: no goal reachable"""
        kind, _, path = self.lat.search(goal, self.lat.d)
        return None if kind == 2 else path


def solve(pm, om, src, goal, shorten_dist=3.0, end_eps=1e-3, radius_close=1.5, radius_far=5.0, max_path_points=None,
          log=None, **_):
    """one problem: dict(status, length, way, next_goal, raw, dropped)"""
    goal = np.asarray(goal, dtype=np.float64)
    raw = src.raw(goal)
    if raw is None:                                              # :235-238
        return dict(status=NO_PATH, length=0.0, way=[], next_goal=goal, raw=[], raw_len=0, dropped=0)
    if max_path_points is not None and len(raw) > max_path_points:
        return dict(status=RAW_OVER, length=0.0, way=[], next_goal=goal, raw=[], raw_len=len(raw), dropped=0)
    short = shorten(pm, om, raw, shorten_dist, end_eps, log)
    status, length, way, nxt, dropped = branch(short, goal, radius_close, radius_far)
    return dict(status=status, length=length, way=way, next_goal=np.asarray(nxt), raw=raw, raw_len=len(raw),
                short=short, dropped=dropped)


def solve_case(pm, om, case, sources=None, csgraph=False):
    """every problem of a case (dict: starts, goals, cfg) -> list of solve() results; sources caches by start"""
    cfg = dict(DEFAULTS, **case.get("cfg", {}))
    sources = {} if sources is None else sources
    out = []
    for s, g in zip(case["starts"], case["goals"]):
        key = (np.asarray(s, dtype=np.float64).tobytes(), cfg["res"], cfg["edge_step"])
        if key not in sources:
            sources[key] = Source(pm, s, cfg["res"], cfg["edge_step"], csgraph)
        out.append(solve(pm, om, sources[key], g, **cfg))
    return out


# ---- scenes ---------------------------------------------------------------------------------------------------------
def door_scene(n_goals=43, seed=5):
    """the wall-and-door map of path_cost_ref.chunk_map at lattice 0.2: two starts west of the wall x n_goals random
    goals each, plus start = goal (a single point comes out) and a goal 0.5 m from the start (two points: the mid-point)"""
    om, pm = pr.chunk_map()
    rng = np.random.default_rng(seed)
    s = [np.array([-3.0, -2.5, 1.0]), np.array([-1.2, 2.9, 2.2])]
    starts, goals = [], []
    for a in s:
        for _ in range(n_goals):
            starts.append(a)
            goals.append(np.array([-3.7, -3.7, 0.2]) + np.array([7.4, 7.4, 2.5]) * rng.random(3))
    starts += [s[0], s[0]]
    goals += [s[0].copy(), s[0] + np.array([0.5, 0.03, 0.02])]
    return om, pm, pr.CHUNK_SIZE, pr.CHUNK_BOX, dict(starts=np.array(starts), goals=np.array(goals), cfg={})


CORRIDOR_SIZE = (8.0, 8.0, 4.0)
CORRIDOR_BOX = ((-3.9, -0.15, 0.85), (3.9, 0.15, 1.15))
CORRIDOR_RES = 0.04
CORRIDOR_START = np.array([-3.72, 0.003, 1.002])


def corridor_map():
    """open space; the box leaves a corridor of a few lattice nodes across, so that Python's Dijkstra is cheap at 0.04"""
    from oracle import fuel_oracle as fo
    om = fo.OracleMap(CORRIDOR_SIZE, CORRIDOR_BOX[0], CORRIDOR_BOX[1])
    om.occ[:] = om.l_min
    nv = om.nvox
    om.set_local_bound((0, 0, 0), (nv[0] - 1, nv[1] - 1, nv[2] - 1))
    om.inflate_local()
    return om, pr.PathMap.from_oracle(om)


def goal_for_points(src, n_points, start, res):
    """a goal along +x whose raw path has exactly n_points points (a sweep: the goal node is the cheapest of the goal's
    neighbourhood, which the restatement decides)"""
    for t in np.arange(0.0, (n_points + 3) * res, res / 8):
        g = start + np.array([t, 0.011, 0.007])
        p = src.raw(g)
        if p is not None and len(p) == n_points:
            return g
    raise AssertionError("no goal with a raw path of %d points" % n_points)


def window_cases(pm):
    """open space at lattice 0.04.  (1) runs: in open space only the distance pushes, so with shorten_dist = (r + 0.5)
    lattice steps the r candidates behind an anchor do not push and the next one does: r = W - 1, W, W + 1, 2 W + 1.
    (2) raw paths of 2, 3, 64, 65, 66 points."""
    res, W = CORRIDOR_RES, WINDOW
    src = Source(pm, CORRIDOR_START, res)
    far_goal = np.array([3.7, 0.02, 1.01])
    cases = []
    for r in (W - 1, W, W + 1, 2 * W + 1):
        cases.append(dict(starts=np.array([CORRIDOR_START]), goals=np.array([far_goal]),
                          cfg=dict(res=res, shorten_dist=(r + 0.5) * res), run=r))
    goals = [goal_for_points(src, n, CORRIDOR_START, res) for n in (2, 3, 64, 65, 66)]
    cases.append(dict(starts=np.repeat([CORRIDOR_START], len(goals), axis=0), goals=np.array(goals),
                      cfg=dict(res=res, shorten_dist=0.9), points=(2, 3, 64, 65, 66)))
    return cases, src


FACE_SIZE = (8.0, 8.0, 4.0)
FACE_BOX = ((-4.0, -4.0, -1.0), (4.0, 4.0, 3.0))  # the map itself
FACE_UNKNOWN = (20, 60, 25)                       # one unknown voxel: centre (-1.95, 2.05, 1.55)


def face_map():
    from oracle import fuel_oracle as fo
    om = fo.OracleMap(FACE_SIZE, FACE_BOX[0], FACE_BOX[1])
    occ = np.full(om.nvox, om.l_min)
    occ[FACE_UNKNOWN] = om.l_min - 0.01
    om.occ[:] = occ.reshape(-1)
    nv = om.nvox
    om.set_local_bound((0, 0, 0), (nv[0] - 1, nv[1] - 1, nv[2] - 1))
    om.inflate_local()
    return om, pr.PathMap.from_oracle(om)


def face_case():
    """problem 0: a start beside the +x face and a goal 0.15 m beyond it (the search never tests the goal point): the
    rays to the goal walk through voxels outside the map, which pass.  Problem 1: a goal inside the unknown voxel: the
    walk stops before the end voxel."""
    starts = np.array([[3.43, 0.52, 1.03], [-3.0, 1.0, 1.0]])
    goals = np.array([[4.15, 0.93, 1.21], [-1.95, 2.05, 1.55]])
    return dict(starts=starts, goals=goals, cfg={})


def threshold_cases(pm, om, start, goal, cfg=None):
    """For one problem: each threshold set to the restatement's own value of the quantity it is compared with, and to
    that value's two neighbours.  Returns [(name, value, [case below, case at, case above])]."""
    cfg = dict(DEFAULTS, **(cfg or {}))
    src = Source(pm, start, cfg["res"], cfg["edge_step"])
    base = solve(pm, om, src, goal, **cfg)
    raw = base["raw"]
    out = []
    # shorten_dist against |path[i] - path[0]| of a candidate behind the first anchor
    i = min(len(raw) - 2, 9)
    out.append(("shorten_dist", dist(raw[i], raw[0])))
    out.append(("radius_close", base["length"]))
    out.append(("radius_far", base["length"]))
    # end_eps against the tail distance |path.back() - short.back()| before the tail push
    out.append(("end_eps", dist(raw[-1], shorten_loop(pm, om, raw, cfg["shorten_dist"])[-1])))
    cases = []
    for name, v in out:
        three = [dict(starts=np.array([start]), goals=np.array([goal]), cfg=dict(cfg, **{name: x}))
                 for x in (np.nextafter(v, -math.inf), v, np.nextafter(v, math.inf))]
        cases.append((name, v, three))
    return cases, src
