"""A literal Python restatement of TopologyPRM::findTopoPaths (path_searching/src/topo_prm.cpp:43-98) over a given sample
stream, with RayCaster::setInput / step (plan_env/src/raycast.cpp:228-321) and SDFMap::getDistWithGrad
(plan_env/src/sdf_map.cpp:497-536): plain Python floats, every sum in the reference's order.  It takes the distance field
as an array and a decision mode:
  f64   dist <= thresh on the array's values (the reference's comparison; the array is res * sqrt(k))
  cut   the device rule of fuelmi_map_topo_paths: the array's values rounded to f32 against an f32 cut between the device's
        values for kmax and kmax + 1, kmax the largest k with res * sqrt(k) <= thresh in f64
Returns what fuelmi_map_topo_paths returns (status, counts, events, the pruned graph, the three path sets, pathLength of
the select paths) plus, per path point, whether a gradient push produced it.  The kernel's own caps are restated too
(status -1 without path outputs); max_nodes / max_path_points are the caller's business (the lists here are complete).

A witness trace (TopoPRM(..., trace={}), off by default; it changes no result) records what the kernel's lane windows, rounds
and caps would see of a problem, so that a test can assert that a scene reaches the edge it was made for:
  trace["shortcut"]   per pass of shortcutPath: nd, the windows of the kernel's loop as (first point, live lanes, lane of the
                      first blocked point or None), the blocked points committed, whether the pass was rolled back
  trace["same_topo"]  per sameTopoPath call: pt_num, the index of the first pair that is not visible (or None)
  trace["graph"]      per createGraph: the graph before pruneGraph as (id, kind, neighbour ids), its nodes and guards, the
                      largest neighbour count, the largest place in the guard list of a visible guard, the rounds of the
                      kernel's synchronous prune (prune_rounds), the surviving nodes
  trace["search"]     per searchPaths: the deepest stack of the depth-first search, the raw paths found, and per raw length
                      (nodes, paths of that length, those the filter kept)
prune_restart / prune_rounds are pruneGraph on plain (id, neighbour ids) lists: the reference's restart after every erase,
and the kernel's rounds."""
import math

import numpy as np

OK, NO_PATH, UNDEFINED = 0, 1, 2
GUARD, CONNECTOR = 1, 2
MAX_PATH_POINTS, MAX_DIS_POINTS, MAX_NEIGHBORS, RAW_NODES = 256, 4096, 64, 100
EVENTS = ("rejected", "guards", "connectors", "moved", "three", "rollbacks")
DEFAULTS = dict(sample_inflate=(1.0, 3.5, 1.0), clearance=0.2, ratio_to_short=5.5, max_sample_num=300, max_raw_path=300,
                max_raw_path2=25, reserve_num=6, max_path_points=64, max_nodes=128)
NO_SOURCE = 1.7976931348623157e308  # fillESDF's sentinel: a field without a source is res * sqrt(DBL_MAX)


class Undefined(Exception):
    pass


class OverCap(Exception):
    pass


def kmax(res, thresh):
    """the largest integer k >= 0 with res * sqrt(k) <= thresh in f64 (thresh >= 0)"""
    k = max(int(math.floor((thresh / res) * (thresh / res))), 0)
    while res * math.sqrt(k + 1) <= thresh:
        k += 1
    while k > 0 and not res * math.sqrt(k) <= thresh:
        k -= 1
    return k


def cut_of(res, thresh):
    return np.float32(float(np.float32(res)) * math.sqrt(kmax(res, thresh) + 0.5))


class Field:
    """origin, resolution, voxel counts and the distance array [nx, ny, nz] (f64; the values are used as they are by the
    gradient, and by the decisions as the mode says)"""

    def __init__(self, origin, res, dist, mode="f64"):
        self.origin = [float(v) for v in origin]
        self.res = float(res)
        self.res_inv = 1.0 / self.res
        self.dist = np.ascontiguousarray(dist, dtype=np.float64)
        self.nvox = self.dist.shape
        self.minb = list(self.origin)
        self.maxb = [self.origin[k] + self.nvox[k] * self.res for k in range(3)]
        self.mode = mode
        self.offset = [0.5 - self.origin[k] / self.res for k in range(3)]
        if mode == "cut":
            with np.errstate(over="ignore"):
                self.d32 = self.dist.astype(np.float32)
            self.cuts = {}
        self.flat = self.dist.reshape(-1).tolist()
        self.flat32 = self.d32.reshape(-1).tolist() if mode == "cut" else None
        self.at_thresh = {}  # f64 mode: decisions taken on a value equal to its threshold, per threshold

    def value(self, x, y, z):  # SDFMap::getDistance(id)
        nx, ny, nz = self.nvox
        if x < 0 or y < 0 or z < 0 or x > nx - 1 or y > ny - 1 or z > nz - 1:
            return -1.0
        return self.flat[(x * ny + y) * nz + z]

    def blocked(self, x, y, z, thresh):  # getDistance(id) <= thresh
        nx, ny, nz = self.nvox
        if x < 0 or y < 0 or z < 0 or x > nx - 1 or y > ny - 1 or z > nz - 1:
            return True
        if self.mode == "f64":
            d = self.flat[(x * ny + y) * nz + z]
            if d == thresh:
                self.at_thresh[thresh] = self.at_thresh.get(thresh, 0) + 1
            return d <= thresh
        if thresh not in self.cuts:
            self.cuts[thresh] = float(cut_of(self.res, thresh))
        return self.flat32[(x * ny + y) * nz + z] <= self.cuts[thresh]

    def pos_to_index(self, p):
        return [int(math.floor((p[k] - self.origin[k]) * self.res_inv)) for k in range(3)]

    def grad(self, pos):  # getDistWithGrad's gradient
        for k in range(3):
            if pos[k] < self.minb[k] + 1e-4:
                return [0.0, 0.0, 0.0]
        for k in range(3):
            if pos[k] > self.maxb[k] - 1e-4:
                return [0.0, 0.0, 0.0]
        res, ri = self.res, self.res_inv
        idx = [int(math.floor(((pos[k] - 0.5 * res * 1.0) - self.origin[k]) * ri)) for k in range(3)]
        d = [(pos[k] - ((idx[k] + 0.5) * res + self.origin[k])) * ri for k in range(3)]
        v = [[[self.value(idx[0] + x, idx[1] + y, idx[2] + z) for z in range(2)] for y in range(2)] for x in range(2)]
        v00 = (1 - d[0]) * v[0][0][0] + d[0] * v[1][0][0]
        v01 = (1 - d[0]) * v[0][0][1] + d[0] * v[1][0][1]
        v10 = (1 - d[0]) * v[0][1][0] + d[0] * v[1][1][0]
        v11 = (1 - d[0]) * v[0][1][1] + d[0] * v[1][1][1]
        v0 = (1 - d[1]) * v00 + d[1] * v10
        v1 = (1 - d[1]) * v01 + d[1] * v11
        g2 = (v1 - v0) * ri
        g1 = ((1 - d[2]) * (v10 - v00) + d[2] * (v11 - v01)) * ri
        g0 = (1 - d[2]) * (1 - d[1]) * (v[1][0][0] - v[0][0][0])
        g0 += (1 - d[2]) * d[1] * (v[1][1][0] - v[0][1][0])
        g0 += d[2] * (1 - d[1]) * (v[1][0][1] - v[0][0][1])
        g0 += d[2] * d[1] * (v[1][1][1] - v[0][1][1])
        return [g0 * ri, g1, g2]


def _mod(value, modulus):
    return math.fmod(math.fmod(value, modulus) + modulus, modulus)


def _intbound(s, ds):
    if ds < 0:
        return _intbound(-s, -ds)
    s = _mod(s, 1)
    if ds == 0:
        return math.inf  # (1 - s) / 0.0
    return (1 - s) / ds


def _norm(v):
    return math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def _sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def _finite(p):
    return all(math.isfinite(c) for c in p)


def _div(v, s):
    if s == 0.0:  # x / 0.0 of the reference: NaN or an infinity, not finite either way
        return [math.nan, math.nan, math.nan]
    return [v[0] / s, v[1] / s, v[2] / s]


def path_length(path):
    length = 0.0
    for i in range(len(path) - 1):
        length += _norm(_sub(path[i + 1], path[i]))
    return length


LANES = 64  # the kernel's lanes: the width of a window of shortcutPath, a stride of sameTopoPath and pruneGraph


def windows_of(blocked):
    """the windows k_topo_path's shortcut loop walks over the verdicts of dis[1:] (blocked[i - 1]: point i is not visible
    from the back it was tested against): (first point, live lanes, lane of the first blocked point or None)"""
    nd, out, i = len(blocked) + 1, [], 1
    while i < nd:
        live = min(LANES, nd - i)
        first = next((t for t in range(live) if blocked[i + t - 1]), None)
        out.append((i, live, first))
        i += LANES if first is None else first + 1
    return out


def prune_restart(nodes):
    """pruneGraph (:272-299) on [(id, [neighbour ids])]: the reference's scan, restarted after every erase"""
    graph = [(i, list(nb)) for i, nb in nodes]
    if len(graph) > 2:
        i = 0
        while i < len(graph) and len(graph) > 2:
            ident, nb = graph[i]
            if ident <= 1:
                i += 1
                continue
            if len(nb) <= 1:
                for _, onb in graph:
                    if ident in onb:
                        onb.remove(ident)
                del graph[i]
                i = 0
            i += 1
    return graph


def prune_rounds(nodes):
    """pruneGraph the way k_topo_path does it: in a round every live node past the first two with at most one neighbour
    is marked, then every live node's neighbour list is compacted in place, front to back, over the marked ones, then
    the marked ones are erased; until a round marks nothing.  -> (the graph, the rounds that marked something)"""
    ids = [i for i, _ in nodes]
    at = {ident: k for k, ident in enumerate(ids)}
    nb = [list(v) for _, v in nodes]
    alive = [1] * len(ids)
    rounds = 0
    while True:
        marked = False
        for n in range(len(ids)):
            if ids[n] > 1 and alive[n] == 1 and len(nb[n]) <= 1:
                alive[n], marked = 2, True
        if not marked:
            break
        rounds += 1
        for n in range(len(ids)):
            if alive[n] != 1:
                continue
            kept = 0
            for i in range(len(nb[n])):
                o = nb[n][i]
                if alive[at[o]] == 2:
                    continue
                nb[n][kept] = o
                kept += 1
            del nb[n][kept:]
        for n in range(len(ids)):
            if alive[n] == 2:
                alive[n] = 0
    return [(ids[n], nb[n]) for n in range(len(ids)) if alive[n]], rounds


class Node:
    def __init__(self, pos, kind, ident):
        self.pos, self.kind, self.id, self.nb = list(pos), kind, ident, []


class TopoPRM:
    def __init__(self, field, cfg, trace=None):
        self.f, self.cfg = field, dict(DEFAULTS, **cfg)
        self.trace = trace
        if trace is not None:
            for key in ("shortcut", "same_topo", "graph", "search"):
                trace.setdefault(key, [])
        self.res = field.res
        self.ev = dict.fromkeys(EVENTS, 0)
        self.far_visible = 0  # visible guards found at place 64 or later of the guard list (not an output of the library)

    # lineVisib (:252-270)
    def line_visib(self, p1, p2, thresh):
        res, f = self.res, self.f
        s = [p1[k] / res for k in range(3)]
        e = [p2[k] / res for k in range(3)]
        x = [int(math.floor(c)) for c in s]
        end = [int(math.floor(c)) for c in e]
        d = [float(end[k] - x[k]) for k in range(3)]
        step = [0 if c == 0 else (-1 if c < 0 else 1) for c in d]
        tmax = [_intbound(s[k], d[k]) for k in range(3)]
        tdel = [(step[k] / d[k]) if d[k] != 0 else math.nan for k in range(3)]
        while True:
            if x == end:
                return True, None
            idx = [int(float(x[k]) + f.offset[k]) for k in range(3)]
            if f.blocked(idx[0], idx[1], idx[2], thresh):
                return False, [(idx[k] + 0.5) * res + f.origin[k] for k in range(3)]
            if tmax[0] < tmax[1]:
                a = 0 if tmax[0] < tmax[2] else 2
            else:
                a = 1 if tmax[1] < tmax[2] else 2
            x[a] += step[a]
            tmax[a] += tdel[a]

    # discretizePath(path, pt_num) (:427-461)
    def discretize_n(self, path, pt_num):
        if len(path) < 2:
            raise Undefined("no segment")
        len_list = [0.0]
        for i in range(len(path) - 1):
            len_list.append(_norm(_sub(path[i + 1], path[i])) + len_list[i])
        dl = len_list[-1] / float(pt_num - 1)
        out = []
        for i in range(pt_num):
            cur_l = float(i) * dl
            idx = -1
            for j in range(len(len_list) - 1):
                if cur_l >= len_list[j] - 1e-4 and cur_l <= len_list[j + 1] + 1e-4:
                    idx = j
                    break
            if idx < 0:
                raise Undefined("no segment")
            den = len_list[idx + 1] - len_list[idx]
            if den == 0.0:
                raise Undefined("0 / 0")
            lam = (cur_l - len_list[idx]) / den
            pt = [(1 - lam) * path[idx][k] + lam * path[idx + 1][k] for k in range(3)]
            if not _finite(pt):
                raise Undefined("not finite")
            out.append(pt)
        return out

    # sameTopoPath (:379-402)
    def same_topo(self, path1, path2, thresh):
        if len(path1) < 2 or len(path2) < 2:
            raise Undefined("a path without a segment")
        if len(path1) > MAX_PATH_POINTS or len(path2) > MAX_PATH_POINTS:
            raise OverCap()
        max_len = max(path_length(path1), path_length(path2))
        pt_num = int(math.ceil(max_len / self.res))
        if pt_num < 2:
            raise Undefined("pt_num < 2")
        pts1, pts2 = self.discretize_n(path1, pt_num), self.discretize_n(path2, pt_num)
        rec = None
        if self.trace is not None:
            rec = dict(pt_num=pt_num, first_invisible=None)
            self.trace["same_topo"].append(rec)
        for i in range(pt_num):
            if not self.line_visib(pts1[i], pts2[i], thresh)[0]:
                if rec:
                    rec["first_invisible"] = i
                return False
        return True

    # discretizePath(path) (:549-566) over discretizeLine (:533-547)
    def discretize(self, path):
        dis = []
        if len(path) < 2:
            return dis
        for i in range(len(path) - 1):
            p1, p2 = path[i], path[i + 1]
            d = _sub(p2, p1)
            seg_num = int(math.ceil(_norm(d) / self.res))
            if seg_num <= 0:
                continue
            dis.extend([p1[k] + d[k] * float(j) / float(seg_num) for k in range(3)] for j in range(seg_num + 1))
            if i != len(path) - 2:
                dis.pop()
            if len(dis) > MAX_DIS_POINTS:
                if self.trace is not None:  # the pass ends here, before its first window
                    self.trace["shortcut"].append(dict(nd=len(dis), blocked=[], committed=0, rolled_back=False))
                raise OverCap()
        return dis

    # dis_path.back() is p1 + (p2 - p1) * 1 of the last segment discretizeLine walks: a pushed p1 (or p2) reaches into it
    def _tail_pushed(self, path, flags):
        for i in range(len(path) - 2, -1, -1):
            if int(math.ceil(_norm(_sub(path[i + 1], path[i])) / self.res)) > 0:
                return flags[i] or flags[i + 1]
        return False

    # shortcutPath (:468-514); returns the path and, per point, whether a gradient push made it (pushed: the same for
    # the path that comes in, whose points a roll-back hands back as they are)
    def shortcut(self, path, iter_num, pushed=None):
        if len(path) > MAX_PATH_POINTS:
            raise OverCap()
        short, flags = [list(p) for p in path], list(pushed) if pushed is not None else [False] * len(path)
        res = self.res
        for _ in range(iter_num):
            last, last_flags = short, flags
            dis = self.discretize(short)
            if len(dis) < 2:
                return dis, [False] * len(dis)
            short, flags = [dis[0]], [False]
            verdicts = []
            rec = dict(nd=len(dis), blocked=verdicts, committed=0, rolled_back=False)
            if self.trace is not None:  # (filled as the pass goes: a pass that ends at a cap keeps what it saw)
                self.trace["shortcut"].append(rec)
            for i in range(1, len(dis)):
                vis, colli = self.line_visib(short[-1], dis[i], res)
                verdicts.append(not vis)
                if vis:
                    continue
                if len(short) + 2 > MAX_PATH_POINTS:
                    raise OverCap()
                grad = self.f.grad(colli)
                pushed = False
                gn = _norm(grad)
                if gn > 1e-3:
                    grad = _div(grad, gn)
                    dr = _sub(dis[i], short[-1])
                    dr = _div(dr, _norm(dr))
                    dot = grad[0] * dr[0] + grad[1] * dr[1] + grad[2] * dr[2]
                    push = [grad[k] - dot * dr[k] for k in range(3)]
                    push = _div(push, _norm(push))
                    colli = [colli[k] + res * push[k] for k in range(3)]
                    pushed = True
                if not _finite(colli):
                    raise Undefined("a pushed point that is not finite")
                short.append(colli)
                flags.append(pushed)
                rec["committed"] += 1
            if len(short) + 1 > MAX_PATH_POINTS:
                raise OverCap()
            short.append(dis[-1])
            flags.append(self._tail_pushed(last, last_flags))
            if path_length(short) > path_length(last):
                self.ev["rollbacks"] += 1
                rec["rolled_back"] = True
                short, flags = last, last_flags
                break
        return short, flags

    # pruneEquivalent (:301-337): the kept indices
    def prune_equivalent(self, paths):
        if len(paths) < 1:
            return []
        exist = [0]
        for i in range(1, len(paths)):
            new_path = True
            for j in exist:
                if self.same_topo(paths[i], paths[j], 0.0):
                    new_path = False
                    break
            if new_path:
                exist.append(i)
        return exist

    # createGraph (:100-188)
    def create_graph(self, start, end, samples):
        cfg, f = self.cfg, self.f
        graph = [Node(start, GUARD, 0), Node(end, GUARD, 1)]
        diff = _sub(end, start)
        infl = cfg["sample_inflate"]
        r = [0.5 * _norm(diff) + infl[0], infl[1], infl[2]]
        tr = [0.5 * (start[k] + end[k]) for k in range(3)]
        xtf = _sub(end, tr)
        xtf = _div(xtf, _norm(xtf))
        ytf = [xtf[1] * -1.0 - xtf[2] * 0.0, xtf[2] * 0.0 - xtf[0] * -1.0, xtf[0] * 0.0 - xtf[1] * 0.0]
        ytf = _div(ytf, _norm(ytf))
        ztf = [xtf[1] * ytf[2] - xtf[2] * ytf[1], xtf[2] * ytf[0] - xtf[0] * ytf[2], xtf[0] * ytf[1] - xtf[1] * ytf[0]]
        if not (_finite(xtf) and _finite(ytf) and _finite(ztf)):
            raise Undefined("a vertical start -> end")
        node_id = 1
        far_place = -1
        for s in range(cfg["max_sample_num"]):
            loc = [float(samples[s][k]) * r[k] for k in range(3)]
            pt = [((xtf[k] * loc[0] + ytf[k] * loc[1]) + ztf[k] * loc[2]) + tr[k] for k in range(3)]
            idx = f.pos_to_index(pt)
            if f.blocked(idx[0], idx[1], idx[2], cfg["clearance"]):
                self.ev["rejected"] += 1
                continue
            visib = []  # findVisibGuard (:190-208)
            place = -1
            for n in graph:
                if n.kind == CONNECTOR:
                    continue
                place += 1
                if self.line_visib(pt, n.pos, self.res)[0]:
                    visib.append(n)
                    self.far_visible += place >= 64
                    far_place = max(far_place, place)
                    if len(visib) > 2:
                        break
            if len(visib) == 0:
                node_id += 1
                graph.append(Node(pt, GUARD, node_id))
                self.ev["guards"] += 1
            elif len(visib) == 2:
                if not self.need_connection(visib[0], visib[1], pt):
                    continue
                if len(visib[0].nb) >= MAX_NEIGHBORS or len(visib[1].nb) >= MAX_NEIGHBORS:
                    raise OverCap()
                node_id += 1
                c = Node(pt, CONNECTOR, node_id)
                graph.append(c)
                visib[0].nb.append(c)
                visib[1].nb.append(c)
                c.nb.extend(visib)
                self.ev["connectors"] += 1
            elif len(visib) == 3:
                self.ev["three"] += 1
        if self.trace is not None:
            before = [(n.id, n.kind, [q.id for q in n.nb]) for n in graph]
            pruned, rounds = prune_rounds([(i, nb) for i, _, nb in before])
            self.trace["graph"].append(dict(before=before, nodes=len(before), guards=sum(k == GUARD for _, k, _ in before),
                                            max_nb=max(len(nb) for _, _, nb in before), far_place=far_place,
                                            rounds=rounds, survivors=len(pruned)))
        # pruneGraph (:272-299), with its restart
        if len(graph) > 2:
            i = 0
            while i < len(graph) and len(graph) > 2:
                n = graph[i]
                if n.id <= 1:
                    i += 1
                    continue
                if len(n.nb) <= 1:
                    for o in graph:
                        for k, q in enumerate(o.nb):
                            if q.id == n.id:
                                del o.nb[k]
                                break
                    del graph[i]
                    i = 0
                i += 1
        return graph

    # needConnection (:210-238)
    def need_connection(self, g1, g2, pt):
        path1 = [g1.pos, pt, g2.pos]
        for a in g1.nb:
            for b in g2.nb:
                if a.id == b.id:
                    path2 = [g1.pos, a.pos, g2.pos]
                    if self.same_topo(path1, path2, 0.0):
                        if path_length(path1) < path_length(path2):
                            a.pos = list(pt)
                            self.ev["moved"] += 1
                        return False
        return True

    # searchPaths / depthFirstSearch (:606-684): (raw paths found, the kept ones)
    def search_paths(self, graph):
        cfg = self.cfg
        raw = []
        deepest = [0]

        def dfs(vis):
            deepest[0] = max(deepest[0], len(vis))
            cur = vis[-1]
            for n in cur.nb:
                if n.id == 1:
                    raw.append([list(v.pos) for v in vis] + [list(n.pos)])
                    if len(raw) >= cfg["max_raw_path"]:
                        return
                    break
            for n in cur.nb:
                if n.id == 1:
                    continue
                if any(n.id == v.id for v in vis):
                    continue
                vis.append(n)
                dfs(vis)
                if len(raw) >= cfg["max_raw_path"]:
                    return
                vis.pop()

        import sys
        sys.setrecursionlimit(max(sys.getrecursionlimit(), 20000))
        dfs([graph[0]])
        if any(len(p) >= RAW_NODES for p in raw):
            raise Undefined("a raw path past path_list(100)")
        min_n, max_n = 100000, 1
        for p in raw:
            max_n, min_n = max(max_n, len(p)), min(min_n, len(p))
        kept = []
        reach_max = False
        for i in range(min_n, max_n + 1):
            for p in raw:
                if len(p) != i:
                    continue
                kept.append(p)
                if len(kept) >= cfg["max_raw_path2"]:
                    reach_max = True
                    break
            if reach_max:
                break
        if self.trace is not None:
            sizes = sorted(set(len(p) for p in raw))
            self.trace["search"].append(dict(depth=deepest[0], found=len(raw), buckets=[
                (n, sum(len(p) == n for p in raw), sum(len(p) == n for p in kept)) for n in sizes]))
        return len(raw), kept

    # findTopoPaths (:43-98) with selectShortPaths (:339-377)
    def find(self, start, end, start_pts, end_pts, samples):
        cfg = self.cfg
        out = dict(status=OK, counts=[0, 0, 0, 0], nodes=[], raw=[], filt=[], sel=[], sel_length=[], filt_pushed=[],
                   sel_pushed=[])
        start, end = [float(v) for v in start], [float(v) for v in end]
        try:
            graph = self.create_graph(start, end, samples)
            out["nodes"] = [(n.id, n.kind, tuple(n.pos), [q.id for q in n.nb]) for n in graph]
            found, raw = self.search_paths(graph)
            out["counts"][0] = found
            shorts = [self.shortcut(p, 1) for p in raw]
            keep = self.prune_equivalent([s[0] for s in shorts])
            filt = [shorts[i] for i in keep]
            paths = list(filt)
            sel = []
            min_len = 0.0
            for i in range(cfg["reserve_num"]):
                if not paths:
                    break
                short_id, best = -1, 100000000
                for a, p in enumerate(paths):
                    ln = path_length(p[0])
                    if ln < best:
                        short_id, best = a, ln
                if short_id < 0:
                    raise Undefined("paths[-1]")
                if i == 0:
                    min_len = best
                elif not best / min_len < cfg["ratio_to_short"]:
                    break
                sel.append(paths.pop(short_id))
            merged = []
            for p, fl in sel:
                m = [[float(c) for c in q] for q in start_pts] + p + [[float(c) for c in q] for q in end_pts]
                if len(m) > MAX_PATH_POINTS:
                    raise OverCap()
                merged.append((m, [False] * len(start_pts) + fl + [False] * len(end_pts)))
            sel = [self.shortcut(m, 5, fl) for m, fl in merged]
            keep2 = self.prune_equivalent([s[0] for s in sel])
            sel = [sel[i] for i in keep2]
            # (the filtered set the caller gets back is what selectShortPaths left of it: it erases what it takes)
            out.update(counts=[found, len(raw), len(filt), len(sel)], raw=raw, filt=[s[0] for s in paths],
                       filt_pushed=[s[1] for s in paths], sel=[s[0] for s in sel], sel_pushed=[s[1] for s in sel],
                       sel_length=[path_length(s[0]) for s in sel])
            out["status"] = NO_PATH if not sel else OK
        except Undefined:
            out["status"] = UNDEFINED
            out["counts"][1:] = [0, 0, 0]
        except OverCap:
            out["status"] = -1
            out["counts"][1:] = [0, 0, 0]
        out["events"] = [self.ev[k] for k in EVENTS]
        out["far_visible"] = self.far_visible
        return out


def find_topo_paths(field, cfg, start, end, samples, start_pts=(), end_pts=(), trace=None):
    out = TopoPRM(field, cfg, trace).find(start, end, list(start_pts), list(end_pts), samples)
    if trace is not None:
        for rec in trace["shortcut"]:
            rec["windows"] = windows_of(rec["blocked"])
    return out
