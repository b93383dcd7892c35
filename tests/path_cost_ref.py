"""CPU restatement of fuelmi_map_path_costs (ViewNode::searchPath, active_perception/src/graph_node.cpp:32-61, with
the deterministic lattice search of DESIGN.md section 10).

The map state is plain arrays (from the oracle map or from fuelmi_map_sync_host); the straight line is p1's voxel
followed by OracleMap.raycast_cells, the walk RayCaster::nextId makes (plan_env/src/raycast.cpp:374-407).  The lattice
part: numpy for node / edge masks, heapq Dijkstra with the predecessor rule for paths, scipy.sparse.csgraph for
distances alone on large lattices.  Every quantity is f64; Python floats and numpy element-wise operations round like
the device."""
import heapq
import math

import numpy as np

# step j = (dx, dy, dz) with dx = j // 9 - 1, dy = j // 3 % 3 - 1, dz = j % 3 - 1: the reference's loop order
STEPS = [(j // 9 - 1, j // 3 % 3 - 1, j % 3 - 1) for j in range(27)]


class PathMap:
    """What searchPath reads of SDFMap: geometry, the exploration box, the inflated and unknown voxels."""

    def __init__(self, origin, res, nvox, box_mind, box_maxd, box_min, box_max, infl, unknown):
        self.origin = np.asarray(origin, dtype=np.float64)
        self.res = float(res)
        self.res_inv = 1.0 / self.res
        self.nvox = tuple(int(v) for v in nvox)
        self.box_mind = np.asarray(box_mind, dtype=np.float64)
        self.box_maxd = np.asarray(box_maxd, dtype=np.float64)
        self.box_min = tuple(int(v) for v in box_min)
        self.box_max = tuple(int(v) for v in box_max)
        self.bad = (np.asarray(infl).reshape(self.nvox) == 1) | np.asarray(unknown, dtype=bool).reshape(self.nvox)

    @classmethod
    def from_oracle(cls, om):
        c = om.cfg
        bmin, bmax = om.box_index()
        return cls(om.origin, om.res, om.nvox, list(c.box_min), list(c.box_max), bmin, bmax, om.infl,
                   om.occ < om.l_min - 1e-3)

    @classmethod
    def from_device(cls, gm):
        h = gm.syncHost(occupancy=True, inflate=True)
        clamp_min = gm.info.clamp_min_log
        bmin, bmax = gm.getBoxIndex()
        return cls(gm.origin, gm.res, gm.nvox, list(gm.cfg.box_min), list(gm.cfg.box_max), bmin, bmax, h["inflate"],
                   h["occupancy"] < clamp_min - 1e-3)

    def blocked(self, pos):
        """getInflateOccupancy(pos) == 1 || getOccupancy(pos) == UNKNOWN, element-wise over [..., 3]; outside the map
        both read -1 and the position passes."""
        pos = np.asarray(pos, dtype=np.float64)
        idx = np.floor((pos - self.origin) * self.res_inv).astype(np.int64)
        inside = np.all((idx >= 0) & (idx < np.array(self.nvox)), axis=-1)
        out = np.zeros(pos.shape[:-1], dtype=bool)
        i = idx[inside]
        out[inside] = self.bad[i[:, 0], i[:, 1], i[:, 2]]
        return out

    def in_box_d(self, pos):
        pos = np.asarray(pos, dtype=np.float64)
        return np.all((pos > self.box_mind) & (pos < self.box_maxd), axis=-1)

    def voxel_bad_or_out(self, idx):
        if any(idx[k] < self.box_min[k] or idx[k] >= self.box_max[k] for k in range(3)):
            return True
        if all(0 <= idx[k] < self.nvox[k] for k in range(3)):
            return bool(self.bad[idx[0], idx[1], idx[2]])
        return False


def norm3(a, b, c):
    a, b, c = float(a), float(b), float(c)
    return math.sqrt(a * a + b * b + c * c)


def ray_voxels(om, p1, p2):
    """RayCaster::input(p1, p2) + nextId: p1's voxel, then the oracle's cells; empty when both share a voxel"""
    res, org = om.res, om.origin
    c = [math.floor(p1[k] / res) for k in range(3)]
    e = [math.floor(p2[k] / res) for k in range(3)]
    if c == e:
        return []
    first = tuple(int(c[k] + (0.5 - org[k] / res)) for k in range(3))
    return [first] + [tuple(v) for v in om.raycast_cells(p1, p2)]


def straight_line_safe(pm, om, p1, p2):
    return not any(pm.voxel_bad_or_out(v) for v in ray_voxels(om, p1, p2))


def weights(res):
    return [norm3(d[0] * res, d[1] * res, d[2] * res) for d in STEPS]


class Lattice:
    """The 26-connected lattice of one source p1: node n at p1 + n * res, domain isInBox(pos) plus the start."""

    def __init__(self, pm, p1, res=0.4, edge_step=0.1):
        self.pm, self.res, self.edge_step = pm, float(res), float(edge_step)
        self.p1 = np.asarray(p1, dtype=np.float64)
        lo, hi = [], []
        for k in range(3):
            base = (pm.box_mind[k] - self.p1[k]) / res
            top = (pm.box_maxd[k] - self.p1[k]) / res
            ns = [n for n in range(int(math.floor(base)) - 2, int(math.ceil(top)) + 3)
                  if pm.box_mind[k] < self.p1[k] + n * res < pm.box_maxd[k]]
            lo.append(min(ns + [0]))
            hi.append(max(ns + [0]))
        self.nlo = np.array(lo)
        self.E = tuple(int(h - l + 1) for l, h in zip(lo, hi))
        ax = [np.arange(lo[k], hi[k] + 1) for k in range(3)]
        self.n = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1)  # [E0, E1, E2, 3]
        self.pos = self.p1 + self.n * self.res  # per component p1[k] + n[k] * res
        self.start = tuple(-self.nlo)
        self.domain = pm.in_box_d(self.pos)
        self.domain[self.start] = True
        self.w = weights(self.res)
        self.in_edge = self._edges()

    def _edges(self):
        """in_edge[j][v]: the edge v - s_j -> v is usable (astar2.cpp:86-113)"""
        pm, E = self.pm, self.E
        target_ok = self.domain & ~self.pm.blocked(self.pos)
        target_ok[self.start] = False  # the start is never entered again (d = 0)
        out = []
        for j, s in enumerate(STEPS):
            m = np.zeros(E, dtype=bool)
            if j == 13:
                out.append(m)
                continue
            # v ranges over the nodes whose u = v - s lies in the extent
            vs = tuple(slice(max(s[k], 0), E[k] + min(s[k], 0)) for k in range(3))
            us = tuple(slice(max(-s[k], 0), E[k] + min(-s[k], 0)) for k in range(3))
            ok = target_ok[vs] & self.domain[us]
            pu = self.pos[us]
            w = self.w[j]
            d = np.array([s[k] * self.res for k in range(3)]) / w
            l = self.edge_step
            while l < w:
                ok &= ~pm.blocked(pu + l * d)
                l += self.edge_step
            m[vs] = ok
            out.append(m)
        return out

    def flat(self, idx):
        return (idx[0] * self.E[1] + idx[1]) * self.E[2] + idx[2]

    def dijkstra(self):
        """least fixed point of d(v) = min_u fl(d(u) + w), heapq"""
        E = self.E
        d = np.full(E, np.inf)
        d[self.start] = 0.0
        heap = [(0.0, self.start)]
        done = np.zeros(E, dtype=bool)
        while heap:
            du, u = heapq.heappop(heap)
            if done[u]:
                continue
            done[u] = True
            for j, s in enumerate(STEPS):
                if j == 13:
                    continue
                v = (u[0] + s[0], u[1] + s[1], u[2] + s[2])
                if not all(0 <= v[k] < E[k] for k in range(3)) or not self.in_edge[j][v]:
                    continue
                c = du + self.w[j]
                if c < d[v]:
                    d[v] = c
                    heapq.heappush(heap, (c, v))
        return d

    def csgraph_dist(self):
        """the same distances through scipy.sparse.csgraph (large lattices)"""
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import dijkstra
        N = self.E[0] * self.E[1] * self.E[2]
        ids = np.arange(N).reshape(self.E)
        rows, cols, vals = [], [], []
        for j, s in enumerate(STEPS):
            if j == 13:
                continue
            vi = np.argwhere(self.in_edge[j])
            if len(vi) == 0:
                continue
            ui = vi - np.array(s)
            rows.append(ids[ui[:, 0], ui[:, 1], ui[:, 2]])
            cols.append(ids[vi[:, 0], vi[:, 1], vi[:, 2]])
            vals.append(np.full(len(vi), self.w[j]))
        g = coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N, N)).tocsr()
        return dijkstra(g, directed=True, indices=int(ids[self.start])).reshape(self.E)

    def search(self, p2, d):
        """goal choice + backtrack: (kind, length, path)"""
        p2 = np.asarray(p2, dtype=np.float64)
        pm = self.pm
        res, inv = self.res, 1.0 / self.res
        gi = [math.floor((p2[k] - pm.origin[k]) * inv) for k in range(3)]
        cand = []
        for k in range(3):
            c = math.floor((p2[k] - self.p1[k]) / res + 0.5)
            cand.append([n for n in range(c - 5, c + 6)
                         if abs(math.floor((self.p1[k] + n * res - pm.origin[k]) * inv) - gi[k]) <= 1
                         and self.nlo[k] <= n < self.nlo[k] + self.E[k]])
        best, bv = math.inf, None
        for a in cand[0]:
            for b in cand[1]:
                for c in cand[2]:
                    li = (a - self.nlo[0], b - self.nlo[1], c - self.nlo[2])
                    if not self.domain[li] or not d[li] < math.inf:
                        continue
                    q = self.pos[li]
                    f = d[li] + norm3(p2[0] - q[0], p2[1] - q[1], p2[2] - q[2])
                    if f < best:
                        best, bv = f, li
        if bv is None:
            return 2, None, [self.p1.copy(), p2.copy()]
        nodes = [bv]
        v = bv
        while v != self.start:
            for j, s in enumerate(STEPS):
                if j == 13 or not self.in_edge[j][v]:
                    continue
                u = (v[0] - s[0], v[1] - s[1], v[2] - s[2])
                if d[u] + self.w[j] == d[v]:
                    v = u
                    break
            else:
                raise AssertionError("no predecessor")
            nodes.append(v)
        nodes.reverse()
        path = [self.p1.copy()] + [self.pos[v].copy() for v in nodes[1:]] + [p2.copy()]
        return 1, path_length(path), path


def path_length(path):
    """Astar::pathLength (astar2.cpp:186-192): sequential sum of segment norms"""
    L = 0.0
    for a, b in zip(path[:-1], path[1:]):
        L += norm3(b[0] - a[0], b[1] - a[1], b[2] - a[2])
    return L


def search_path(pm, om, p1, p2, res=0.4, edge_step=0.1, no_path_cost=1000.0, lattice=None):
    """one pair: (kind, length, path as [k, 3])"""
    p1 = np.asarray(p1, dtype=np.float64)
    p2 = np.asarray(p2, dtype=np.float64)
    if straight_line_safe(pm, om, p1, p2):
        return 0, norm3(p1[0] - p2[0], p1[1] - p2[1], p1[2] - p2[2]), np.array([p1, p2])
    if lattice is None:
        lattice = Lattice(pm, p1, res, edge_step)
        lattice.d = lattice.dijkstra()
    kind, length, path = lattice.search(p2, lattice.d)
    if kind == 2:
        return 2, float(no_path_cost), np.array(path)
    return kind, length, np.array(path)


def edge_ok(pm, a, b, res=0.4, edge_step=0.1):
    """the edge-safety rule for consecutive lattice points a -> b (a 26-neighbour step of b - a)"""
    s = np.rint((np.asarray(b) - np.asarray(a)) / res).astype(int)
    assert np.abs(s).max() <= 1 and np.abs(s).max() > 0, "not a 26-neighbour step"
    step = s * res
    w = norm3(step[0], step[1], step[2])
    d = step / w
    if pm.blocked(np.asarray(b)) or not pm.in_box_d(np.asarray(b)):
        return False
    l = edge_step
    while l < w:
        if pm.blocked(np.asarray(a) + l * d):
            return False
        l += edge_step
    return True


# ---- a serpentine map: one lattice layer, a shortest path of more than 8192 lattice edges ---------------------------
SERP_SIZE = (24.0, 24.0, 3.0)
SERP_BOX = ((-11.9, -11.9, 0.97), (11.9, 11.9, 1.03))  # z: one lattice layer for sources at z = 1
SERP_RES = 0.05                                        # lattice resolution (voxels are 0.1)
SERP_P1 = (-11.437, 10.013, 1.0)                       # corridor 0, below the gap at the top of wall 0; off the
                                                       # voxel faces, so lattice nodes sit inside cells


def serpentine_occupancy(om):
    """walls of one voxel across the whole z range at x voxel 10, 18, .., 226, each open for 15 voxels at alternating
    ends (top for even walls); after the 0.199 m inflation the corridors keep 3 free voxels"""
    occ = np.full(om.nvox, om.l_min)
    for k, ix in enumerate(range(10, 230, 8)):
        if k % 2 == 0:
            occ[ix, :225, :] = om.l_max
        else:
            occ[ix, 15:, :] = om.l_max
    return occ


def serpentine_map():
    """(OracleMap, PathMap) of the serpentine, inflated by the oracle"""
    from oracle import fuel_oracle as fo
    om = fo.OracleMap(SERP_SIZE, SERP_BOX[0], SERP_BOX[1])
    om.occ[:] = serpentine_occupancy(om).reshape(-1)
    nv = om.nvox
    om.set_local_bound((0, 0, 0), (nv[0] - 1, nv[1] - 1, nv[2] - 1))
    om.inflate_local()
    return om, PathMap.from_oracle(om)


def goals_at_hops(pm, om, p1, hops, res):
    """goal points p2 whose restated path from p1 runs through exactly H lattice edges, one per H in hops.  Node H of the
    chain to the farthest reachable node is the goal when it is the earliest chain node in p2's neighbourhood (+-1
    lattice cell): p2 is placed a cell or two ahead of it along the chain and nudged sideways, so that among the chain
    nodes ahead the earliest one is strictly cheapest; the first placement whose restated search gives H edges is kept.
    Returns ({H: p2}, lattice with .d)."""
    lat = Lattice(pm, p1, res)
    lat.d = lat.csgraph_dist()
    d = np.where(np.isfinite(lat.d), lat.d, -1.0)
    far = np.unravel_index(int(np.argmax(d)), lat.E)
    _, _, path = lat.search(lat.pos[far], lat.d)
    p1 = np.asarray(p1, dtype=np.float64)
    out = {}
    for H in hops:
        assert H + 2 < len(path), (H, len(path))
        a, b = np.array(path[H]), np.array(path[H + 1])
        ahead = (b - a) / norm3(*(b - a))
        side = np.array([-ahead[1], ahead[0], 0.0])
        found = None
        for along in (1.5, 1.2, 1.8, 1.0, 2.0, 0.6, 1.1, 1.3, 1.4, 1.6, 1.7, 1.9):
            for nudge in (0.2, -0.2, 0.35, -0.35):
                p2 = a + (along * ahead + nudge * side) * res
                kind, _, p = lat.search(p2, lat.d)
                if kind == 1 and len(p) == H + 2 and not straight_line_safe(pm, om, p1, p2):
                    found = p2
                    break
            if found is not None:
                break
        assert found is not None, H
        out[H] = found
    return out, lat


# ---- many ~0.8 M-node lattices: more than one source chunk (48 M nodes) ----------------------------------------------
CHUNK_SIZE = (8.0, 8.0, 4.0)
CHUNK_BOX = ((-3.9, -3.9, 0.05), (3.9, 3.9, 2.9))
CHUNK_RES = 0.06
CHUNK_NODE_BUDGET = 48 << 20  # path_cost.hip


def chunk_map():
    """(OracleMap, PathMap): a wall at x ~ -0.2 with a door, a second wall open at low y (the small map of
    tests/test_path_cost_gpu.py), inflated by the oracle"""
    from oracle import fuel_oracle as fo
    om = fo.OracleMap(CHUNK_SIZE, CHUNK_BOX[0], CHUNK_BOX[1])
    occ = np.full(om.nvox, om.l_min)
    occ[38:40, :, :] = om.l_max
    occ[38:40, 52:60, 10:26] = om.l_min
    occ[50:52, 20:70, 10:40] = om.l_max
    om.occ[:] = occ.reshape(-1)
    nv = om.nvox
    om.set_local_bound((0, 0, 0), (nv[0] - 1, nv[1] - 1, nv[2] - 1))
    om.inflate_local()
    return om, PathMap.from_oracle(om)


def lattice_nodes(pm, p1, res):
    """the node count of p1's lattice (Lattice's extent, without its edges)"""
    E = 1
    for k in range(3):
        base = (pm.box_mind[k] - p1[k]) / res
        top = (pm.box_maxd[k] - p1[k]) / res
        ns = [n for n in range(int(math.floor(base)) - 2, int(math.ceil(top)) + 3)
              if pm.box_mind[k] < p1[k] + n * res < pm.box_maxd[k]]
        E *= max(ns + [0]) - min(ns + [0]) + 1
    return E


def chunk_case(pm, om, n_src=72, seed=21):
    """n_src distinct sources west of the wall, each with one goal east of it (the straight line blocked), and the
    chunk of every source as path_cost_enqueue forms them (sources in first-seen order while the nodes fit)"""
    rng = np.random.default_rng(seed)
    p1, p2 = [], []
    while len(p1) < n_src:
        a = np.array([-3.5, -3.5, 0.3]) + np.array([2.8, 7.0, 2.3]) * rng.random(3)
        b = np.array([0.6, -3.5, 0.3]) + np.array([2.9, 7.0, 2.3]) * rng.random(3)
        near = b + 0.1 * np.array(STEPS, dtype=np.float64)  # the goal clear of the walls: some goal node is reached
        if pm.blocked(a[None])[0] or pm.blocked(near).any() or straight_line_safe(pm, om, a, b):
            continue
        p1.append(a)
        p2.append(b)
    chunk, nodes, c = [], 0, 0
    for a in p1:
        nn = lattice_nodes(pm, a, CHUNK_RES)
        if nodes and nodes + nn > CHUNK_NODE_BUDGET:
            c, nodes = c + 1, 0
        nodes += nn
        chunk.append(c)
    return np.array(p1), np.array(p2), chunk
