"""CPU restatement of fuelmi_map_refine_tours: FastExplorationManager::refineLocalTour
(exploration_manager/src/fast_exploration_manager.cpp:429-503) and its single-destination branch (:185-220),
GraphSearch::DijkstraSearch (active_perception/include/active_perception/graph_search.h), ViewNode::computeCost
(active_perception/src/graph_node.cpp:63-88) and FrontierFinder::getViewpointsInfo
(active_perception/src/frontier_finder.cpp:452-484).

The searchPath lengths are inputs (from SDFMap.path_costs or hand-worked); everything else is restated here in f64 with
the operation order of the facade's FrontierFinder::hostCost: left-to-right sums, as the Eigen stand-in computes them."""
import heapq
import math

import numpy as np

G_INIT = 1000000.0      # BaseNode::g_value_ (graph_node.h:31)
ARGMIN_INIT = 100000.0  # min_cost of the single-destination branch (fast_exploration_manager.cpp:199)


def norm3(a, b, c):
    a, b, c = float(a), float(b), float(c)
    return math.sqrt(a * a + b * b + c * c)


def compute_cost(length, p1, p2, y1, y2, v1, vm, yd, w_dir):
    """ViewNode::computeCost with searchPath's length given.  normalized() as real Eigen (3.3 and later): a zero vector
    is returned unchanged, so a zero-length edge adds w_dir * acos(0) = w_dir * pi / 2."""
    pos_cost = float(length) / vm
    if norm3(*v1) > 1e-3:
        d = [float(p2[k]) - float(p1[k]) for k in range(3)]
        z = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        if z > 0.0:
            nz = math.sqrt(z)
            d = [d[k] / nz for k in range(3)]
        nv = norm3(*v1)
        vd = [float(v1[k]) / nv for k in range(3)]
        dot = vd[0] * d[0] + vd[1] * d[1] + vd[2] * d[2]
        diff = math.acos(dot) if -1.0 <= dot <= 1.0 else math.nan  # C's acos: NaN outside [-1, 1]
        pos_cost += w_dir * diff
    diff = abs(float(y2) - float(y1))
    other = 2 * math.pi - diff
    diff = other if other < diff else diff  # std::min
    yaw_cost = diff / yd
    return yaw_cost if pos_cost < yaw_cost else pos_cost  # std::max: NaN pos_cost stays NaN


class Graph:
    """A refinement problem as the reference builds it: node 0 = the start, then the layers; the last layer keeps
    only its first node (:459-462) unless last_argmin.  edges[(u, v)] = cost, from a length function len_fn(u, v)
    over global node ids."""

    def __init__(self, pos, vel, yaw, layers, last_argmin=False):
        self.pts = [np.asarray(pos, dtype=np.float64)]
        self.yaws = [float(yaw)]
        self.vel = np.asarray(vel, dtype=np.float64)
        self.layer_ids = []
        for i, layer in enumerate(layers):
            layer = np.asarray(layer, dtype=np.float64).reshape(-1, 4)
            if i == len(layers) - 1 and not last_argmin:
                layer = layer[:1]
            ids = []
            for row in layer:
                ids.append(len(self.pts))
                self.pts.append(row[:3].copy())
                self.yaws.append(float(row[3]))
            self.layer_ids.append(ids)
        self.last_argmin = last_argmin

    def edge_pairs(self):
        """every edge (u, v) in the device's order: layer blocks, slot u * nv + v"""
        out, prev = [], [0]
        for ids in self.layer_ids:
            out += [(u, v) for u in prev for v in ids]
            prev = ids
        return out

    def costs(self, lengths, vm, yd, w_dir):
        """lengths: {(u, v): searchPath length}; only the start has a velocity"""
        zero = np.zeros(3)
        return {(u, v): compute_cost(lengths[(u, v)], self.pts[u], self.pts[v], self.yaws[u], self.yaws[v],
                                     self.vel if u == 0 else zero, vm, yd, w_dir)
                for (u, v) in self.edge_pairs()}


def dijkstra(g, cost):
    """GraphSearch::DijkstraSearch literally: a binary heap on g, g = 1e6 initially, closed_ set on pop, strict <,
    early exit at the goal (the last layer's node 0).  The heap breaks exactly equal g by node id, where libstdc++'s
    priority_queue may order differently.  Returns (choices per layer or None, goal g or inf)."""
    n = len(g.pts)
    nbr = [[] for _ in range(n)]
    for (u, v) in g.edge_pairs():
        nbr[u].append(v)
    gv = [G_INIT] * n
    parent = [None] * n
    closed = [False] * n
    goal = g.layer_ids[-1][0]
    gv[0] = 0.0
    heap = [(0.0, 0)]
    while heap:
        _, vc = heapq.heappop(heap)
        closed[vc] = True
        if vc == goal:
            chain = []
            while vc is not None:
                chain.append(vc)
                vc = parent[vc]
            chain.reverse()
            return [g.layer_ids[i].index(chain[i + 1]) for i in range(len(g.layer_ids))], gv[goal]
        for vb in nbr[vc]:
            if closed[vb]:
                continue
            t = gv[vc] + cost[(vc, vb)]
            if t < gv[vb]:
                gv[vb] = t
                parent[vb] = vc
                heapq.heappush(heap, (t, vb))
    return None, math.inf


def layer_dp(g, cost):
    """the layer-by-layer min-plus pass of k_refine: g(v) = min over u of fl(g(u) + c(u, v)) among candidates < 1e6,
    key (total, g(u), u); goal: the last layer's node 0, or with last_argmin its first cheapest node below 1e5.
    Returns (choices per layer or None, goal g or inf)."""
    gv = {0: 0.0}
    par = {}
    prev = [0]
    for ids in g.layer_ids:
        for v in ids:
            best = None
            for ui, u in enumerate(prev):
                gu = gv[u]
                t = gu + cost[(u, v)]
                if not t < G_INIT:
                    continue
                key = (t, gu, ui)
                if best is None or key < best:
                    best = key
            gv[v] = G_INIT if best is None else best[0]
            par[v] = None if best is None else prev[best[2]]
        prev = ids
    last = g.layer_ids[-1]
    goal = None
    if g.last_argmin:
        m = ARGMIN_INIT
        for v in last:
            if gv[v] < m:
                m, goal = gv[v], v
    elif gv[last[0]] < G_INIT:
        goal = last[0]
    if goal is None:
        return None, math.inf
    chain, v = [], goal
    for _ in g.layer_ids:
        chain.append(v)
        v = par[v]
    chain.reverse()
    return [g.layer_ids[i].index(chain[i]) for i in range(len(g.layer_ids))], gv[goal]


def single_destination(pos, vel, yaw, points, yaws, lengths, vm, yd, w_dir):
    """fast_exploration_manager.cpp:197-208: argmin over computeCost(pos -> point i), strict < from 100000"""
    min_cost, min_id = ARGMIN_INIT, -1
    for i in range(len(points)):
        c = compute_cost(lengths[i], pos, points[i], yaw, yaws[i], vel, vm, yd, w_dir)
        if c < min_cost:
            min_cost, min_id = c, i
    return min_id, min_cost


def polyline(cur_pos, refined_pts, legs):
    """:486-497: [cur_pos], then per refined point the whole searchPath(back(), pt) path when its cost is non-zero,
    else the point.  legs[i] = (length, path [k, 3]) of the leg ending at refined_pts[i]."""
    out = [np.asarray(cur_pos, dtype=np.float64)]
    for pt, (length, path) in zip(refined_pts, legs):
        if length != 0.0:
            out += [np.asarray(q) for q in path]
        else:
            out.append(np.asarray(pt, dtype=np.float64))
    return np.array(out)


def viewpoints_info(cur_pos, frontiers, ids, view_num, max_decay, min_candidate_dist):
    """FrontierFinder::getViewpointsInfo (:452-484).  frontiers[id] = list of (pos [3], yaw, visib_num), best
    coverage first.  Returns (points, yaws): per id a list."""
    points, yaws = [], []
    for fid in ids:
        views = frontiers[fid]
        if not views:
            continue
        visib_thresh = int(views[0][2] * max_decay)
        pts, ys = [], []
        for pos, yaw, vis in views:
            if len(pts) >= view_num or vis <= visib_thresh:
                break
            if norm3(*(np.asarray(pos) - np.asarray(cur_pos))) < min_candidate_dist:
                continue
            pts.append(np.asarray(pos, dtype=np.float64))
            ys.append(float(yaw))
        if not pts:  # all viewpoints are very close: take them regardless of the distance
            for pos, yaw, vis in views:
                if len(pts) >= view_num or vis <= visib_thresh:
                    break
                pts.append(np.asarray(pos, dtype=np.float64))
                ys.append(float(yaw))
        points.append(pts)
        yaws.append(ys)
    return points, yaws
