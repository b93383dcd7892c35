"""CPU restatement of fuelmi_tsp_solve (include/fuelmi.h "Global tour") and of the reference's file route around LKH
(exploration_manager/src/fast_exploration_manager.cpp:327-420).

  held_karp(c)                 the exact method: suffix DP, the lexicographically smallest optimal order
  ils(c, restarts, kicks, seed) the heuristic: nearest neighbour, best-improvement 2-opt + Or-opt, double bridge
  local_optimum_violations(c, order)  improving moves left in either neighbourhood (none for a local optimum)
  tour_cost(c, order)          the closed-tour cost in exact integers
  ref_int_matrix / write_tsp / read_tour  the reference's int(cost * 100), its single.tsp text and its parse
Everything is integer arithmetic: results must equal the device's bit for bit."""
import itertools
import math

import numpy as np

M64 = (1 << 64) - 1


def tour_cost(c, order):
    c = np.asarray(c)
    d = len(order)
    return sum(int(c[order[k], order[(k + 1) % d]]) for k in range(d))


def solve(c, restarts, kicks, exact_max, seed):
    """(order, cost, method) as fuelmi_tsp_solve answers one problem"""
    d = len(c)
    if d - 1 <= exact_max:
        o, v = held_karp(c)
        return o, v, 0
    o, v = ils(c, restarts, kicks, seed)
    return o, v, 1


# ---- exact --------------------------------------------------------------------------------------------------------------
def held_karp(c):
    c = np.asarray(c, dtype=np.int64)
    d = len(c)
    if d == 1:
        return [0], 0
    n = d - 1
    full = (1 << n) - 1
    masks = np.arange(full + 1, dtype=np.int64)
    pop = np.array([bin(m).count("1") for m in range(full + 1)])
    g = np.full((full + 1, n), 1 << 62, dtype=np.int64)  # g[S, j-1]; entries with j outside S are never read
    g[full, :] = c[1:, 0]
    for p in range(n - 1, 0, -1):
        layer = masks[pop == p]
        for k in range(n):
            sel = layer[(layer >> k & 1) == 0]
            val = c[1:, k + 1][None, :] + g[sel | 1 << k, k][:, None]
            g[sel, :] = np.minimum(g[sel, :], val)
    target = min(int(c[0, j + 1]) + int(g[1 << j, j]) for j in range(n))
    opt, order, S, last = target, [0], 0, 0
    for _ in range(n):
        for j in range(n):
            if not S >> j & 1 and int(c[last, j + 1]) + int(g[S | 1 << j, j]) == target:
                S |= 1 << j
                last = j + 1
                target = int(g[S, j])
                order.append(last)
                break
    return order, opt


def brute_force(c):
    """the lexicographically smallest optimal order over all permutations (d <= 8)"""
    d = len(c)
    best = None
    for p in itertools.permutations(range(1, d)):
        o = [0] + list(p)
        v = tour_cost(c, o)
        if best is None or v < best[1]:
            best = (o, v)
    return best


# ---- heuristic ----------------------------------------------------------------------------------------------------------
def mix(z):
    """splitmix64's step"""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def kick_points(seed, r, k, d):
    h = mix((seed ^ mix(((r << 32) | k) & M64)) & M64)
    pts, t = [], 0
    while len(pts) < 3:
        x = 1 + mix((h + t) & M64) % (d - 1)
        if x not in pts:
            pts.append(x)
        t += 1
    return sorted(pts)


def double_bridge(order, p1, p2, p3):
    o = list(order)
    return o[:p1] + o[p2:p3] + o[p1:p2] + o[p3:]


def nearest_neighbour(c):
    d = len(c)
    order, seen = [0], {0}
    for _ in range(d - 1):
        row = c[order[-1]]
        j = min((int(row[j]), j) for j in range(d) if j not in seen)[1]
        order.append(j)
        seen.add(j)
    return order


class _Moves:
    """the neighbourhood of a d-node tour as position arrays, and each move's key (type, i, j, k) encoded as the device
    does: type 0 i*6d + 6j, type 1 6d^2 + i*6d + 6j + k"""

    def __init__(self, d):
        self.d = d
        i, j = np.triu_indices(d, 1)
        keep = i >= 1
        self.i2, self.j2 = i[keep], j[keep]
        self.k2 = self.i2 * (6 * d) + self.j2 * 6
        s, L, rev, g = [], [], [], []
        for ss in range(1, d):
            for LL in (1, 2, 3):
                e = ss + LL - 1
                if e > d - 1:
                    continue
                gg = np.array([x for x in range(d) if not (ss - 1 <= x <= e)], dtype=np.int64)
                for rr in ((0,) if LL == 1 else (0, 1)):
                    s.append(np.full(len(gg), ss))
                    L.append(np.full(len(gg), LL))
                    rev.append(np.full(len(gg), rr))
                    g.append(gg)
        cat = (lambda a: np.concatenate(a).astype(np.int64)) if s else (lambda a: np.zeros(0, np.int64))
        self.s, self.L, self.rev, self.g = cat(s), cat(L), cat(rev), cat(g)
        self.k1 = 6 * d * d + self.s * (6 * d) + self.g * 6 + (self.L - 1) * 2 + self.rev


_MOVES = {}


def _moves(d):
    if d not in _MOVES:
        _MOVES[d] = _Moves(d)
    return _MOVES[d]


def move_deltas(c, order):
    """(delta, key) of every move of both neighbourhoods from `order` (int64 arrays)"""
    c = np.asarray(c, dtype=np.int64)
    o = np.asarray(order, dtype=np.int64)
    d = len(o)
    mv = _moves(d)
    nxt = np.roll(o, -1)
    F = np.concatenate([[0], np.cumsum(c[o, nxt])])
    B = np.concatenate([[0], np.cumsum(c[o[1:], o[:-1]])])
    i, j = mv.i2, mv.j2
    jn = np.where(j + 1 == d, 0, j + 1)
    d2 = (c[o[i - 1], o[j]] + c[o[i], o[jn]] - (F[i] - F[i - 1]) - (F[j + 1] - F[j]) + (B[j] - B[i]) - (F[j] - F[i]))
    s, L, rev, g = mv.s, mv.L, mv.rev, mv.g
    e = s + L - 1
    first, last, p = o[s], o[e], o[s - 1]
    nx = o[np.where(e + 1 == d, 0, e + 1)]
    u, v = o[g], o[np.where(g + 1 == d, 0, g + 1)]
    rem = (F[s] - F[s - 1]) + (F[e + 1] - F[e]) - c[p, nx]
    gap = F[g + 1] - F[g]
    fwd = c[u, first] + c[last, v] - gap - rem
    bwd = c[u, last] + c[first, v] - gap + (B[e] - B[s]) - (F[e] - F[s]) - rem
    d1 = np.where(rev == 1, bwd, fwd)
    return np.concatenate([d2, d1]), np.concatenate([mv.k2, mv.k1])


def apply_move(order, key):
    d = len(order)
    o = list(order)
    if key < 6 * d * d:
        i, j = key // (6 * d), (key % (6 * d)) // 6
        return o[:i] + o[i:j + 1][::-1] + o[j + 1:]
    r = key - 6 * d * d
    s, g, k = r // (6 * d), (r % (6 * d)) // 6, r % 6
    L, rev = k // 2 + 1, k & 1
    seg = o[s:s + L]
    if rev:
        seg = seg[::-1]
    rest = o[:s] + o[s + L:]
    gp = g if g < s else g - L
    return rest[:gp + 1] + seg + rest[gp + 1:]


def move_type(d, key):
    """"2opt", "or_fwd" or "or_rev" of a move key"""
    if key < 6 * d * d:
        return "2opt"
    return "or_rev" if (key - 6 * d * d) % 6 & 1 else "or_fwd"


def local_search(c, order, counts=None):
    """best improvement until no move has delta < 0; ties by the smallest key.  counts: a dict that gains one per
    applied move under its move_type"""
    order = list(order)
    while True:
        delta, key = move_deltas(c, order)
        if len(delta) == 0:
            break
        m = delta.min()
        if m >= 0:
            break
        k = int(key[delta == m].min())
        if counts is not None:
            t = move_type(len(order), k)
            counts[t] = counts.get(t, 0) + 1
        order = apply_move(order, k)
    return order, tour_cost(c, order)


def ils(c, restarts, kicks, seed, start=None):
    """start: local_search(c, nearest_neighbour(c)) when the caller has it already (it depends on c alone)"""
    c = np.asarray(c, dtype=np.int64)
    d = len(c)
    start, start_cost = local_search(c, nearest_neighbour(c)) if start is None else start  # the same for every restart
    best_all = None
    for r in range(restarts):
        best, bcost = list(start), start_cost
        for k in range(kicks):
            cand, cc = local_search(c, double_bridge(best, *kick_points(seed, r, k, d)))
            if cc < bcost:
                best, bcost = cand, cc
        if best_all is None or bcost < best_all[1]:
            best_all = (best, bcost)
    return best_all


def local_optimum_violations(c, order):
    """the moves of either neighbourhood that would still improve `order` (empty for a local optimum)"""
    delta, key = move_deltas(c, order)
    return [(int(dv), int(kv)) for dv, kv in zip(delta[delta < 0], key[delta < 0])]


# ---- the reference's file route -------------------------------------------------------------------------------------------
def ref_int_matrix(mat, scale=100):
    """int int_cost = cost_mat(i, j) * scale (fast_exploration_manager.cpp:370-371): truncation toward zero"""
    return [[int(float(v) * scale) for v in row] for row in np.asarray(mat, dtype=np.float64)]


def write_tsp(mat, scale=100):
    """single.tsp as findGlobalTour writes it (:342-375)"""
    im = ref_int_matrix(mat, scale)
    d = len(im)
    s = ("NAME : single\nTYPE : ATSP\nDIMENSION : " + str(d) + "\nEDGE_WEIGHT_TYPE : "
         "EXPLICIT\nEDGE_WEIGHT_FORMAT : FULL_MATRIX\nEDGE_WEIGHT_SECTION\n")
    for row in im:
        s += "".join("%d " % v for v in row) + "\n"
    return s + "EOF"


def read_tour(text):
    """the ATSP branch of findGlobalTour's parse (:382-410): lines after TOUR_SECTION, id 1 skipped, stop at -1,
    indices id - 2"""
    lines = text.split("\n")
    k = 0
    while k < len(lines) and lines[k] != "TOUR_SECTION":
        k += 1
    out = []
    for line in lines[k + 1:]:
        if line == "":
            continue
        idx = int(line)
        if idx == 1:
            continue
        if idx == -1:
            break
        out.append(idx - 2)
    return out


def feasible_matrix(rng, d, lo=0, hi=1000):
    return rng.integers(lo, hi, size=(d, d)).astype(np.int64)


def fuel_like_matrix(rng, n, vm=2.0, yd=60 * math.pi / 180.0, w_dir=1.5, box=(40.0, 40.0, 10.0), vel=(0.8, -0.4, 0.1)):
    """n seeded viewpoints in a box, ViewNode::computeCost on straight-line lengths (v = 0 between viewpoints, row 0
    from the current state with a velocity), column 0 zero: the (n+1) x (n+1) double matrix getFullCostMatrix gives"""
    import refine_ref as rr
    pts = rng.random((n + 1, 3)) * np.array(box)
    yaws = rng.uniform(-math.pi, math.pi, n + 1)
    m = np.zeros((n + 1, n + 1))
    for i in range(n + 1):
        v1 = vel if i == 0 else (0.0, 0.0, 0.0)
        for j in range(1, n + 1):
            if i != j:
                m[i, j] = rr.compute_cost(float(np.linalg.norm(pts[j] - pts[i])), pts[i], pts[j], yaws[i], yaws[j], v1,
                                          vm, yd, w_dir)
    return m


def cycle_matrix(workload, seed=42, vm=2.0, yd=60 * 3.1415926 / 180.0, w_dir=1.5):
    """getFullCostMatrix of a headline workload's first cycle, as the facade computes it with
    frontier/device_path_cost (needs the device): the best viewpoint of every active cluster, searchPath lengths from
    SDFMap.path_costs (one search per pair), ViewNode::computeCost on the host; row 0 from a current state beside
    cluster 0's viewpoint with a velocity, column 0 zero"""
    import bench
    import fuel_amd
    import refine_ref as rr
    map_size, box, occ, _, _ = bench.build_inputs(workload, seed=seed)
    gm = fuel_amd.SDFMap(map_size, box[0], box[1], device=0)
    gm.uploadOccupancy(occ)
    nv = gm.nvox
    gm.setLocalBound((0, 0, 0), (nv[0] - 1, nv[1] - 1, nv[2] - 1))
    gm.clearAndInflateLocalMap()
    gf = fuel_amd.FrontierFinder(gm, cluster_min=100, cluster_size_xy=2.0, down_sample=3, split=True)
    gf.setViewpointConfig(gf.viewpointConfig())
    gm.setUpdatedBox(box[0], box[1])
    gf.searchFrontiers()
    na, _ = gf.computeFrontiersToVisit()
    vp = np.array([gf.viewpoints(1, k)[0][0, :4] for k in range(na)])
    gf.close()
    n = len(vp)
    a, b = np.triu_indices(n, 1)
    length, _, _ = gm.path_costs(vp[a, :3], vp[b, :3], max_points=0)
    cur, vel, yaw = vp[0, :3] + np.array([0.3, -0.2, 0.0]), np.array([0.5, -0.3, 0.1]), 0.3
    l0, _, _ = gm.path_costs(np.repeat([cur], n, axis=0), vp[:, :3], max_points=0)
    gm.close()
    m = np.zeros((n + 1, n + 1))
    zero = (0.0, 0.0, 0.0)
    for k in range(len(a)):
        i, j = a[k], b[k]
        m[i + 1, j + 1] = m[j + 1, i + 1] = rr.compute_cost(length[k], vp[i, :3], vp[j, :3], vp[i, 3], vp[j, 3], zero,
                                                            vm, yd, w_dir)
    for j in range(n):
        m[0, j + 1] = rr.compute_cost(l0[j], cur, vp[j, :3], yaw, vp[j, 3], vel, vm, yd, w_dir)
    return m


def planted_matrix(d, seed, n_traps=4):
    """A d x d instance (d >= 64) with a cheap seeded Hamiltonian cycle and traps that send the nearest-neighbour start
    astray, so that the local search needs many moves of every type and stays cheap to restate at d ~ 1024:
      cycle      perm[t] <-> perm[t+1] costs 10..19 both ways (reversing a stretch of it costs nothing inside), but
                 0 -> perm[d-1] costs 30, so the start runs forwards
      elsewhere  2000..2999
      2-opt trap perm[k] -> perm[k+5] costs 1 and perm[k+5] -> perm[k+4] is cheaper than -> perm[k+6]: the start runs
                 perm[k+5] .. perm[k+1] backwards, then perm[k+1] -> perm[k+6] (100); reversing the stretch repairs it
      Or-opt trap perm[k] -> perm[k+2] (1) skips perm[k+1], left for a jump (column 600): moved back forwards
      pair trap  perm[k] -> perm[k+3] (1) skips perm[k+1], perm[k+2]; a jump enters perm[k+2] (column 500) first and
                 leaves by perm[k+1]: moved back reversed
    Returns (int64 matrix, perm)."""
    assert d >= 64
    rng = np.random.default_rng(seed)
    perm = np.concatenate([[0], 1 + rng.permutation(d - 1)]).astype(np.int64)
    c = rng.integers(2000, 3000, (d, d)).astype(np.int64)
    nxt = np.roll(perm, -1)
    w = rng.integers(10, 20, d)
    c[perm, nxt] = w
    c[nxt, perm] = w
    c[0, perm[d - 1]] = 30
    spots = (rng.choice((d - 16) // 12, 3 * n_traps, replace=False) + 1) * 12  # trap starts, 12 apart, off the ends
    P = lambda t: int(perm[t])  # noqa: E731
    for t, k in enumerate(spots.tolist()):
        kind = t % 3
        if kind == 0:  # 2-opt
            c[P(k), P(k + 5)] = 1
            c[P(k + 5), P(k + 4)] = 5
            c[P(k + 1), P(k + 6)] = 100
        elif kind == 1:  # Or-opt forward
            c[P(k), P(k + 2)] = 1
            col = c[:, P(k + 1)]
            col[col >= 2000] = 600
        else:  # Or-opt reversed
            c[P(k), P(k + 3)] = 1
            col = c[:, P(k + 2)]
            col[col >= 2000] = 500
    return c, perm
