"""HeadingPlanner's information gain and yaw search (active_perception/src/heading_planner.cpp) restated in Python
floats, operation by operation: what fuel_amd/csrc/info_gain.hip is compared with (tests/test_heading_gpu.py) and what
is itself compared with recordings of the reference's own code (tests/test_heading_cpu.py, tests/golden/heading).

  Map                the members of SDFMap the planner reads: the unknown and occupied cells, the exploration box
  view_setup         :240-255 and calcFovAABB (:401-418): rotated normals, the index box
  view               calcInformationGain (:236-322) / calcInfoGain (:324-391): the cells in x, y, z order with their
                     verdicts; rays go through a memo per camera position (the CastFlags cache, :280-308)
  gain_of            the sum of a view, in the reference's order or in the device's
  search             Graph::dijkstraSearch (:52-100) as the layered recurrence, with every replace test's margin
  search_fifo        the same function literally: the queue, the open map, the close set
  search_path_of_yaw searchPathOfYaw (:170-234)
  parity_tolerance   the measured tolerance of a NON_UNIFORM gain

math.sin / cos / tan / exp / sqrt are the C library's.  Nothing here needs a GPU."""
import math
from collections import deque

import numpy as np

NON_UNIFORM, UNIFORM = 0, 1
MAX_CELLS, MAX_YAW, MAX_CTRL, MAX_LAYER = 12288, 31, 256, 64  # include/fuelmi.h FUELMI_GAIN_* / FUELMI_YAWPATH_*
DEFAULT_CFG = dict(weight_type=UNIFORM, in_box=True, factor=4, far=4.5, top_ang=0.56125, left_ang=0.69222,
                   right_ang=0.68901, lambda1=2.0, lambda2=1.0)
_TOL = {}


def gain_cfg(**kw):
    c = dict(DEFAULT_CFG)
    c.update(kw)
    return c


class Map:
    """unk / occ: bool [nx, ny, nz]; box_min / box_max: the exploration box in metres (SDFMap::box_mind_ / box_maxd_)"""

    def __init__(self, origin, res, unk, occ, box_min, box_max, res_inv=None):
        self.origin = tuple(float(v) for v in origin)
        self.res = float(res)
        self.res_inv = float(res_inv) if res_inv is not None else 1.0 / self.res
        self.unk, self.occ = np.asarray(unk, dtype=bool), np.asarray(occ, dtype=bool)
        self.nvox = self.unk.shape
        self.box_mind, self.box_maxd = tuple(float(v) for v in box_min), tuple(float(v) for v in box_max)
        self.box_min, self.box_max = self.pos_to_index(self.box_mind), self.pos_to_index(self.box_maxd)
        self.offset = tuple(0.5 - self.origin[k] / self.res for k in range(3))

    def pos_to_index(self, p):  # sdf_map.h:127-130
        return tuple(math.floor((p[k] - self.origin[k]) * self.res_inv) for k in range(3))

    def index_to_pos(self, i):  # :132-135
        return tuple((i[k] + 0.5) * self.res + self.origin[k] for k in range(3))

    def in_map(self, i):
        return all(0 <= i[k] <= self.nvox[k] - 1 for k in range(3))

    def in_box(self, i):  # isInBox(Vector3i) :171-178
        return all(self.box_min[k] <= i[k] < self.box_max[k] for k in range(3))


def _rot(R, v):
    return tuple(R[r][0] * v[0] + R[r][1] * v[1] + R[r][2] * v[2] for r in range(3))


def view_setup(m, cfg, pt, yaw):
    """(the four rotated normals top, bottom, left, right; lbi; ubi) of :240-255.  T_wc = T_wb * T_bc with
    T_bc = T_cb^-1 = [[0, 0, 1], [-1, 0, 0], [0, 1, 0]]: R_wc = [[sin, 0, cos], [-cos, 0, sin], [0, 1, 0]], t_wc = pt"""
    sn, cs = math.sin(yaw), math.cos(yaw)
    R = ((sn, 0.0, cs), (-cs, 0.0, sn), (0.0, 1.0, 0.0))
    h = math.pi / 2  # M_PI_2
    top, left, right, far = cfg["top_ang"], cfg["left_ang"], cfg["right_ang"], cfg["far"]
    normals = ((0.0, math.sin(h - top), math.cos(h - top)), (0.0, -math.sin(h - top), math.cos(h - top)),
               (math.sin(h - left), 0.0, math.cos(h - left)), (-math.sin(h - right), 0.0, math.cos(h - right)))
    normals = tuple(_rot(R, n) for n in normals)
    verts = ((-far * math.tan(left), -far * math.sin(top), far), (-far * math.sin(left), far * math.sin(top), far),
             (far * math.sin(right), -far * math.sin(top), far), (far * math.sin(right), far * math.sin(top), far))
    pts = [tuple(a + b for a, b in zip(_rot(R, v), pt)) for v in verts] + [tuple(pt)]
    lbd = [min(p[k] for p in pts) for k in range(3)]
    ubd = [max(p[k] for p in pts) for k in range(3)]
    for k in range(3):  # SDFMap::boundBox
        lbd[k] = max(lbd[k], m.box_mind[k])
        ubd[k] = min(ubd[k], m.box_maxd[k])
    return normals, m.pos_to_index(lbd), m.pos_to_index(ubd)


def inside_fov(pw, pc, normals, far):  # :475-487
    d = (pw[0] - pc[0], pw[1] - pc[1], pw[2] - pc[2])
    if math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) > far:
        return False
    for n in normals:
        if d[0] * n[0] + d[1] * n[1] + d[2] * n[2] < 0.1:
            return False
    return True


def _intbound(s, ds):  # raycast.cpp:10-23
    if ds < 0:
        s, ds = -s, -ds
    s = math.fmod(math.fmod(s, 1.0) + 1.0, 1.0)
    return (1 - s) / ds if ds != 0 else math.inf  # 1 - s > 0


def ray_blocked(m, check_pt, pt):
    """:290-299: setInput(check_pt / resolution, pt / resolution), every voxel step() hands out read at int(ray + offset).
    A walk that misses its end voxel (the reference never returns) counts as blocked."""
    s = [check_pt[k] / m.res for k in range(3)]
    e = [pt[k] / m.res for k in range(3)]
    x = [math.floor(v) for v in s]
    end = [math.floor(v) for v in e]
    d = [float(end[k] - x[k]) for k in range(3)]
    step = [0 if v == 0 else (-1 if v < 0 else 1) for v in d]
    tmax = [_intbound(s[k], d[k]) for k in range(3)]
    tdel = [step[k] / d[k] if d[k] != 0 else math.nan for k in range(3)]
    limit = sum(abs(end[k] - x[k]) for k in range(3)) + 2
    for _ in range(limit):
        if x == end:
            return False
        rid = tuple(int(float(x[k]) + m.offset[k]) for k in range(3))
        if m.in_map(rid) and m.occ[rid]:
            return True
        if tmax[0] < tmax[1]:
            a = 0 if tmax[0] < tmax[2] else 2
        else:
            a = 1 if tmax[1] < tmax[2] else 2
        x[a] += step[a]
        tmax[a] += tdel[a]
    return True


def prefix_lengths(ctrl):
    ln = [0.0]
    for i in range(len(ctrl) - 1):
        d = [ctrl[i + 1][k] - ctrl[i][k] for k in range(3)]
        ln.append(ln[-1] + math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))
    return ln


def weight(check_pt, ctrl, lens, lambda1, lambda2):
    """distToPathAndCurPos (:452-473) and :286"""
    min_squ, idx = 1.7976931348623157e308, -1
    for i in range(len(ctrl)):
        d = [ctrl[i][k] - check_pt[k] for k in range(3)]
        squ = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        if squ < min_squ:
            min_squ, idx = squ, i
    return math.exp(-lambda1 * math.sqrt(min_squ) - lambda2 * lens[idx])


def view(m, cfg, pt, yaw, memo=None):
    """the candidate cells of one view in the reference's x, y, z order: [(index, position, visible)].  memo: the rays'
    verdicts by cell for this camera position (shared by the yaws of a group); a cell it does not hold is walked"""
    normals, lb, ub = view_setup(m, cfg, pt, yaw)
    f = cfg["factor"]
    memo = {} if memo is None else memo
    out = []
    # a cell outside the map reads -1 at :275 and is skipped, and int % f == 0 means the same for every sign
    rng = [range(max(lb[k], 0) + (-max(lb[k], 0)) % f, min(ub[k], m.nvox[k] - 1) + 1, f) for k in range(3)]
    for x in rng[0]:
        for y in rng[1]:
            for z in rng[2]:
                i = (x, y, z)
                if not m.unk[i]:  # `!getOccupancy(id) == UNKNOWN` skips every KNOWN cell
                    continue
                if cfg["in_box"] and not m.in_box(i):
                    continue
                p = m.index_to_pos(i)
                if not inside_fov(p, pt, normals, cfg["far"]):
                    continue
                if i not in memo:
                    memo[i] = not ray_blocked(m, p, pt)
                out.append((i, p, memo[i]))
    return out


def device_lane(i, f):
    """the lane of info_gain.hip's second phase that sums cell i"""
    return (((i[1] // f) & 7) << 3) | ((i[2] // f) & 7)


def gain_of(cells, cfg, ctrl=None, order="reference"):
    """(n_cand, n_visible, gain) of view()'s cells.  order: "reference" adds in x, y, z order; "device" adds per lane in
    that order and joins the 64 lanes in a butterfly"""
    vis = [c for c in cells if c[2]]
    if cfg["weight_type"] == UNIFORM:
        return len(cells), len(vis), float(len(vis))
    lens = prefix_lengths(ctrl)
    ws = [weight(c[1], ctrl, lens, cfg["lambda1"], cfg["lambda2"]) for c in vis]
    if order == "reference":
        g = 0.0
        for w in ws:
            g += w
        return len(cells), len(vis), g
    part = [0.0] * 64
    for c, w in zip(vis, ws):
        l = device_lane(c[0], cfg["factor"])
        part[l] = part[l] + w
    o = 32
    while o >= 1:
        part = [part[l] + part[l ^ o] for l in range(64)]
        o >>= 1
    return len(cells), len(vis), part[0]


def info_gains(m, cfg, pt, yaws, ctrl=None, order="device"):
    """one group: dict(gain, n_cand, n_visible: lists per yaw; n_rays; cells: the subsampled cells of the union box or
    None when no view has a cell)"""
    memo = {}
    res = [gain_of(view(m, cfg, pt, y, memo), cfg, ctrl, order) for y in yaws]
    return dict(n_cand=[r[0] for r in res], n_visible=[r[1] for r in res], gain=[r[2] for r in res], n_rays=len(memo),
                cells=union_cells(m, cfg, pt, yaws))


def union_cells(m, cfg, pt, yaws):
    """the cells of the group's union box in subsampled indices (what fuelmi_yawpath_plan's cap is about)"""
    f = cfg["factor"]
    lo, hi = None, None
    for y in yaws:
        _, lb, ub = view_setup(m, cfg, pt, y)
        slo = [-(-max(lb[k], 0) // f) for k in range(3)]
        shi = [min(ub[k], m.nvox[k] - 1) // f if ub[k] >= 0 else -1 for k in range(3)]
        if any(a > b for a, b in zip(slo, shi)):
            continue
        lo = slo if lo is None else [min(a, b) for a, b in zip(lo, slo)]
        hi = shi if hi is None else [max(a, b) for a, b in zip(hi, shi)]
    if lo is None:
        return 0
    return (hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1)


# ---- the graph search -------------------------------------------------------------------------------------------------------
def penal(diff, dt, max_yaw_rate):  # :42-49
    yr = diff / dt
    if yr <= max_yaw_rate:
        return 0.0
    return (yr - max_yaw_rate) * (yr - max_yaw_rate)  # pow(x, 2) is x * x, exactly


def layers_of(yaws, gains, half_vert_num, yaw_diff):
    """[[(yaw, gain)]] per layer (:179-203); gains [L][2h + 1] is read at the inner layers"""
    L = len(yaws)
    out = []
    for i in range(L):
        if i == 0 or i == L - 1:
            out.append([(float(yaws[i]), 0.0)])
        else:
            out.append([(float(yaws[i]) + float(j - half_vert_num) * yaw_diff, float(gains[i][j]))
                        for j in range(2 * half_vert_num + 1)])
    return out


def search(layers, dt, w, max_yaw_rate):
    """the layered recurrence.  dict(g_value [[..]], parent [[..]], path_vertex [..], path [..], margin: the smallest
    |g_tmp - g| over every replace test, inf without one)"""
    g = [[0.0] * len(l) for l in layers]
    par = [[0] * len(l) for l in layers]
    margin = math.inf
    for i in range(1, len(layers)):
        for b, (yb, gb) in enumerate(layers[i]):
            for c, (yc, _) in enumerate(layers[i - 1]):
                g_tmp = g[i - 1][c] - gb + w * penal(abs(yc - yb), dt, max_yaw_rate)
                if c == 0:
                    g[i][b], par[i][b] = g_tmp, 0
                    continue
                margin = min(margin, abs(g_tmp - g[i][b]))
                if g_tmp > g[i][b]:
                    continue
                g[i][b], par[i][b] = g_tmp, c
    pv = [0] * len(layers)
    v = 0
    for i in range(len(layers) - 1, 0, -1):
        pv[i] = v
        v = par[i][v]
    return dict(g_value=g, parent=par, path_vertex=pv, path=[layers[i][pv[i]][0] for i in range(len(layers))], margin=margin)


def search_fifo(layers, dt, w, max_yaw_rate):
    """Graph::dijkstraSearch (:52-100) as written: vertices numbered layer by layer, edges from every vertex of a layer to
    every vertex of the next in that order.  (g_value by id, parent by id, path of ids)"""
    ids, yaw, gain = [], [], []
    for l in layers:
        ids.append(list(range(len(yaw), len(yaw) + len(l))))
        yaw += [v[0] for v in l]
        gain += [v[1] for v in l]
    nbs = {v: [] for v in range(len(yaw))}
    for a, b in zip(ids[:-1], ids[1:]):
        for v1 in a:
            nbs[v1] += b
    g, parent = [None] * len(yaw), [None] * len(yaw)
    start, goal = 0, len(yaw) - 1
    g[start] = 0.0
    open_set, open_map, close = deque([start]), {start}, set()
    while open_set:
        vc = open_set.popleft()
        open_map.discard(vc)
        close.add(vc)
        if vc == goal:
            path, v = [], vc
            while v is not None:
                path.append(v)
                v = parent[v]
            return g, parent, path[::-1]
        for vb in nbs[vc]:
            if vb in close:
                continue
            g_tmp = g[vc] - gain[vb] + w * penal(abs(yaw[vc] - yaw[vb]), dt, max_yaw_rate)
            if vb not in open_map:
                open_map.add(vb)
                open_set.append(vb)
            elif g_tmp > g[vb]:
                continue
            parent[vb], g[vb] = vc, g_tmp
    raise AssertionError("Dijkstra can't find path!")


def search_path_of_yaw(m, gcfg, pts, yaws, dt, ctrl, half_vert_num, yaw_diff, max_yaw_rate, w, gains_in=None,
                       order="device"):
    """searchPathOfYaw.  dict(gains [L][2h + 1], n_rays [L], over: a layer past the cell cap, and search()'s keys)"""
    L, nv = len(yaws), 2 * half_vert_num + 1
    gains = [[0.0] * nv for _ in range(L)]
    n_rays, over = [0] * L, False
    for i in range(1, L - 1):
        if gains_in is not None:
            gains[i] = [float(v) for v in gains_in[i]]
            continue
        ys = [float(yaws[i]) + float(j - half_vert_num) * yaw_diff for j in range(nv)]
        r = info_gains(m, gcfg, tuple(pts[i]), ys, ctrl, order)
        gains[i], n_rays[i] = r["gain"], r["n_rays"]
        over = over or r["cells"] > MAX_CELLS
    out = search(layers_of(yaws, gains, half_vert_num, yaw_diff), dt, w, max_yaw_rate)
    out.update(gains=gains, n_rays=n_rays, over=over)
    return out


def parity_tolerance():
    """(measured, tolerance) of a NON_UNIFORM gain, relative to the gain: the largest disagreement, over every
    NON_UNIFORM view of tests/heading_cases.py's scenes, between the sum in the reference's order and the sum in the
    device's, and 100 x that -- the margin of waypoint_traj_ref.parity_tolerance, for the same reason: the C library's exp
    against the device's (one unit in the last place of each term) and the order of the sum"""
    if not _TOL:
        import heading_cases as hc
        worst = 0.0
        for a, b in hc.parity_pairs():
            if a != 0.0:
                worst = max(worst, abs(a - b) / abs(a))
        _TOL["measured"], _TOL["tol"] = worst, 100.0 * worst
    return _TOL["measured"], _TOL["tol"]
