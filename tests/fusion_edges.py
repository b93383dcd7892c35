"""Depth fusion at the edges of its kernels (fuel_amd/csrc/insert.hip): the scenarios test_fusion_edges_cpu.py pins
to the real reference through the oracle and test_fusion_edges_gpu.py runs on the device, and the pure-numpy
predicates that prove a scenario reaches the edge it is drawn for.

A scenario is a dict: "map_size", "map_kw" (keywords of fa.SDFMap / OracleMap / RefMap alike), "frames" -- a list of
(points float32 [n, 3], camera f64 [3]) -- and "compare", the 0-based indices of the frames after which the maps are
compared.  Nothing here needs a GPU or the oracle; the kernels' geometry (lanes per ray, slots per workgroup, cube
extents) comes from the library's host-only fuelmi_map_insert_plan, so that the conditions follow a retuned kernel."""
import math

import numpy as np

import helpers  # noqa: F401  (puts the repository root on sys.path)
import fuel_amd
from fuel_amd.host import DEFAULT_MAP

PLAN = fuel_amd.SDFMap.insertPlan()
LANES = PLAN["lanes_per_ray"]
RAY_SLOTS = PLAN["ray_slots"]
CLASSIFY_SLOTS = PLAN["classify_slots"]
CUBE = PLAN["cube"]
WAVE = 64  # lanes of a wavefront on gfx950 (the __shfl_up de-duplication works inside one)
BRANCHES = ("fits", "low", "high", "middle")


# ---- the map's geometry and inputPointCloud's per-point classification, restated in numpy f64 ----
class Geo:
    def __init__(self, map_size, **kw):
        p = dict(DEFAULT_MAP)
        p.update(kw)
        self.res = float(p["resolution"])
        self.res_inv = 1 / self.res
        self.max_ray = float(p["max_ray_length"])
        self.inflate = max(self.res, float(p["local_bound_inflate"]))
        self.org = np.array([-map_size[0] / 2.0, -map_size[1] / 2.0, p["ground_height"]])
        self.nv = np.array([int(math.ceil(map_size[i] / self.res)) for i in range(3)])
        self.minb, self.maxb = self.org, self.org + np.array(map_size, dtype=float)
        self.N = int(self.nv[0]) * int(self.nv[1]) * int(self.nv[2])

    def index(self, p):
        """posToIndex: floor((p - origin) * resolution_inv)"""
        return np.floor((np.asarray(p, dtype=float) - self.org) * self.res_inv).astype(np.int64)

    def address(self, idx):
        idx = np.asarray(idx, dtype=np.int64)
        return (idx[..., 0] * self.nv[1] + idx[..., 1]) * self.nv[2] + idx[..., 2]


def classify(g, pts, cam):
    """(kept [n] bool, end points [n, 3] f64, hit flag [n], end voxel address [n]) of a frame, point by point as
    inputPointCloud classifies them: in-map test, closetPointInMap, clip to max_ray_length, the z < 0.2 drop"""
    p = np.asarray(pts, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    cam = np.asarray(cam, dtype=np.float64)
    n = len(p)
    with np.errstate(all="ignore"):
        inmap = ~np.any(p < g.minb + 1e-4, axis=1) & ~np.any(p > g.maxb - 1e-4, axis=1)
        diff = p - cam
        min_t = np.full(n, 1000000.0)
        for k in range(3):
            mov = np.abs(diff[:, k]) > 0
            for bound in (g.maxb[k], g.minb[k]):
                t = (bound - cam[k]) / diff[:, k]
                use = mov & (t > 0) & (t < min_t)
                min_t = np.where(use, t, min_t)
        out = np.where(inmap[:, None], p, cam + (min_t - 1e-3)[:, None] * diff)
        d = out - cam
        length = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        far = length > g.max_ray
        out = np.where(far[:, None], d / length[:, None] * g.max_ray + cam, out)
        clipped = far | ~inmap
        kept = ~np.isnan(p[:, 0]) & ~(clipped & (out[:, 2] < 0.2))
        out = np.where(kept[:, None], out, 0.0)
        adr = g.address(g.index(out))
        kept &= (adr >= 0) & (adr < g.N)
    return kept, out, kept & ~clipped, np.where(kept, adr, -1)


# ---- RayCaster::input / nextId, restated ----
def _mod1(v):
    return math.fmod(math.fmod(v, 1.0) + 1.0, 1.0)


def _intbound(s, ds):
    if ds < 0:
        s, ds = -s, -ds
    s = _mod1(s)
    return (1 - s) / ds if ds != 0 else math.inf


def ray_params(pt, cam, res):
    """c, ec, step, tMax, tDelta of the ray from end point pt to the camera, as RayCaster::input forms them"""
    s = [float(pt[k]) / res for k in range(3)]
    e = [float(cam[k]) / res for k in range(3)]
    c = [int(math.floor(v)) for v in s]
    ec = [int(math.floor(v)) for v in e]
    d = [float(ec[k] - c[k]) for k in range(3)]
    step = [0 if v == 0 else (-1 if v < 0 else 1) for v in d]
    tmax = [_intbound(s[k], d[k]) for k in range(3)]
    tdel = [step[k] / d[k] if d[k] != 0 else math.nan for k in range(3)]
    return c, ec, step, tmax, tdel


def ray_walk(pt, cam, res):
    """the walk of nextId: {"crossings": the parameter of every step in order, "ties": per step the number of axes that
    share the smallest tMax, "cells": the (ray-frame) cells the fusion marks as misses, "moving": moving axes,
    "octant": the step signs}"""
    c, ec, step, tmax, tdel = ray_params(pt, cam, res)
    c, t = list(c), list(tmax)
    crossings, ties, cells = [], [], []
    guard = sum(abs(ec[k] - c[k]) for k in range(3)) + 4
    first = True
    while c != ec and guard >= 0:
        if not first:
            cells.append(tuple(c))
        first = False
        if t[0] < t[1]:
            k = 0 if t[0] < t[2] else 2
        else:
            k = 1 if t[1] < t[2] else 2
        crossings.append(t[k])
        ties.append(sum(1 for q in range(3) if t[q] == t[k]))
        c[k] += step[k]
        t[k] += tdel[k]
        guard -= 1
    return {"crossings": crossings, "ties": ties, "cells": cells, "moving": sum(1 for v in step if v),
            "octant": tuple(step)}


def handover_exact(walk, lanes=None):
    """the step parameters of the walk that equal j / lanes exactly, 0 < j < lanes: the lane hand-over's own values"""
    lanes = lanes or LANES
    edges = {j / lanes for j in range(1, lanes)}
    return [t for t in walk["crossings"] if t in edges]


# ---- the LDS miss cube of a ray-walk workgroup ----
def cube_origin(block_box_lo, block_box_hi, cam_cell, ext):
    """one axis of the cube's placement: (origin, branch).  block_box_lo / _hi: the index range of the end points of
    the classify workgroup (None: it kept no point); the camera's cell always joins the range"""
    lo = cam_cell if block_box_lo is None else min(cam_cell, int(block_box_lo))
    hi = cam_cell if block_box_hi is None else max(cam_cell, int(block_box_hi))
    if hi - lo < ext:
        return lo, "fits"
    if cam_cell == lo:
        return lo, "low"
    if cam_cell == hi:
        return hi - ext + 1, "high"
    return cam_cell - ext // 2, "middle"


def frame_cubes(g, pts, cam, box_slots=None):
    """per ray-walk workgroup of a frame: {"casts": it walks at least one ray (a slot that is the first of its end
    voxel), "origin": (x, y, z), "branch": (bx, by, bz)}.  The box is the one of the classify workgroup the slots
    belong to (box_slots = CLASSIFY_SLOTS); box_slots = RAY_SLOTS gives what the workgroup's own points would."""
    box_slots = box_slots or CLASSIFY_SLOTS
    kept, end, _, adr = classify(g, pts, cam)
    idx = g.index(end)
    cam_c = g.index(cam)
    first = np.zeros(len(kept), dtype=bool)
    _, where = np.unique(np.where(kept, adr, -1 - np.arange(len(kept))), return_index=True)
    first[where] = True
    first &= kept
    out = []
    for b in range(-(-len(kept) // RAY_SLOTS)):
        s0 = (b * RAY_SLOTS) // box_slots * box_slots
        sel = kept[s0:s0 + box_slots]
        org, br = [], []
        for k in range(3):
            v = idx[s0:s0 + box_slots, k][sel]
            o, name = cube_origin(v.min() if len(v) else None, v.max() if len(v) else None, int(cam_c[k]), CUBE[k])
            org.append(o)
            br.append(name)
        out.append({"casts": bool(first[b * RAY_SLOTS:(b + 1) * RAY_SLOTS].any()), "origin": tuple(org),
                    "branch": tuple(br)})
    return out


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)


def exploration_box(sc, margin=0.3):
    """the exploration box every map of this suite is created with: the map less a margin on every side (fusion does
    not read it; the frontier search at the end of a scenario does)"""
    g = Geo(sc["map_size"], **sc["map_kw"])
    return tuple(g.minb + margin), tuple(g.maxb - margin)


def scenario(map_size, frames, compare=None, **map_kw):
    frames = [(f32(p), np.asarray(c, dtype=np.float64)) for p, c in frames]
    return {"map_size": tuple(map_size), "map_kw": map_kw, "frames": frames,
            "compare": sorted(range(len(frames)) if compare is None else compare)}


# ---- A: the char frame counter ----
A_MAP = (4.0, 4.0, 2.0)
A_CAM = (0.05, 0.05, 0.05)
A_JUNK = (-1.05, -0.85, 0.35)
# end voxels of the directed part and the (1-based) frames they end a ray in
A_VOXELS = {"first_and_257": ((1.25, 0.35, 0.45), (1, 257)), "first_in_255": ((0.35, 1.25, -0.35), (255,)),
            "first_in_256": ((-0.45, 1.15, 0.55), (256,)), "first_in_128": ((1.05, -1.15, 0.25), (128,))}
A_COMPARE = (1, 127, 128, 129, 254, 255, 256, 257, 258, 300)


def dropped_cloud(cam, n=40, seed=11, reach=8.0):
    """points far outside every map of this suite, steeply below a camera under z = 1.5: each is clipped (to the map,
    then to max_ray_length) and ends below z = 0.2"""
    rng = np.random.default_rng(seed)
    d = np.stack([rng.uniform(-0.6, 0.6, n), rng.uniform(-0.6, 0.6, n), rng.uniform(-1.0, -0.6, n)], axis=1)
    d /= np.linalg.norm(d, axis=1)[:, None]
    return f32(np.asarray(cam) + reach * d)


def scenario_counter_directed(dropped_at=None):
    """300 frames of one junk point; the voxels of A_VOXELS join in their frames.  dropped_at (1-based): an all-dropped
    frame takes that place and every later frame moves back by one (scenario F)."""
    frames = []
    for k in range(1, 301):
        pts = [A_JUNK] + [p for p, at in A_VOXELS.values() if k in at]
        frames.append((pts, A_CAM))
    compare = [k - 1 for k in A_COMPARE]
    if dropped_at is not None:
        frames.insert(dropped_at - 1, (dropped_cloud(A_CAM), A_CAM))
        compare = sorted(set(compare) | {k + 1 for k in compare} | {dropped_at - 1, dropped_at})
    return scenario(A_MAP, frames, compare)


def scenario_counter_random():
    """the 300 frames of test_char_wrap_of_raycast_num (same seed)"""
    rng = np.random.default_rng(1)
    frames = []
    for _ in range(300):
        pts = (rng.random((30, 3)) * np.array([3.6, 3.6, 1.6]) - np.array([1.8, 1.8, 0.8])).astype(np.float32)
        frames.append((pts, (0.0, 0.0, 0.0)))
    return scenario(A_MAP, frames, [k - 1 for k in A_COMPARE])


def counter_mid_cell(g, name):
    """a cell in the middle of the ray from voxel `name` of A_VOXELS to the camera that no other ray of the directed
    part crosses: map index (x, y, z)"""
    walks = {n: ray_walk(np.float32(p).astype(float), A_CAM, g.res)["cells"] for n, (p, _) in A_VOXELS.items()}
    walks["junk"] = ray_walk(np.float32(A_JUNK).astype(float), A_CAM, g.res)["cells"]
    others = {c for n, w in walks.items() if n != name for c in w}
    ends = {tuple(int(math.floor(float(np.float32(v)) / g.res)) for v in p) for p, _ in A_VOXELS.values()}
    mine = [c for c in walks[name] if c not in others and c not in ends]
    c = mine[len(mine) // 2]
    return tuple(int(c[k] + 0.5 - g.org[k] / g.res) for k in range(3))


# ---- B: the hand-over between the lanes of one ray ----
B_GRIDS = {"r0.25": ((8.0, 8.0, 4.0), 0.25, (0, 0, 4)), "r0.125": ((4.0, 4.0, 2.0), 0.125, (0, 0, 0))}


def _signs(v):
    out = {()}
    for a in v:
        out = {s + (q,) for s in out for q in ((a, -a) if a else (0,))}
    return sorted(out)


def _perms(v):
    a, b, c = v
    return sorted({(a, b, c), (a, c, b), (b, a, c), (b, c, a), (c, a, b), (c, b, a)})


def lane_rays(grid):
    """(map size, map keywords, camera, [(label, point)]): end points whose cell differences to the camera's cell are
    multiples of LANES in every sign octant -- axis-aligned rays, face and space diagonals, (8, 4, 0) and (8, 8, 4) --
    on voxel faces (crossings land exactly on j / LANES) and voxel centres; rays of 0..3 cells; the camera itself; a
    point in its voxel; points beyond max_ray_length and outside the map.  Cell units times a power-of-two resolution:
    every coordinate is exact in float32."""
    map_size, res, cam_cell = B_GRIDS[grid]
    L = LANES
    cam = (np.array(cam_cell) + 0.5) * res
    dirs = []
    for base in ((L, 0, 0), (2 * L, 0, 0), (L, L, 0), (2 * L, 2 * L, 0), (L, L, L), (2 * L, 2 * L, L), (2 * L, L, 0)):
        for p in _perms(base):
            dirs += _signs(p)
    dirs = sorted(set(dirs))
    rays = []
    for d in dirs:
        cell = np.array(cam_cell) + np.array(d)
        rays.append(("face%s" % (d,), cell * res))                       # s integer on every axis
        rays.append(("centre%s" % (d,), (cell + 0.5) * res))
        mixed = cell + np.where(np.array(d) != 0, 0.0, 0.5)               # faces on the moving axes only
        rays.append(("mixed%s" % (d,), mixed * res))
    for d in ((0, 0, 0), (1, 0, 0), (0, -1, 0), (1, 1, 0), (-2, 0, 0), (0, 1, -1), (1, 1, 1), (-1, 2, 0), (0, 0, 3),
              (2, -1, 1), (-2, -2, 0), (4, 0, 0), (1, -1, 2)):
        cell = np.array(cam_cell) + np.array(d)
        rays.append(("short%s" % (d,), (cell + 0.5) * res))
        rays.append(("shortface%s" % (d,), (cell + np.where(np.array(d) != 0, 0.0, 0.5)) * res))
    rays.append(("camera", cam.copy()))
    rays.append(("cam_voxel", cam + 0.25 * res))
    for d in ((1, 0.5, 0.1), (-1, -1, 0.2), (0.3, -1, 0.05), (-1, 0.2, -0.1), (1, 1, 0.25), (0, 1, 0), (-1, 0, 0)):
        u = np.array(d) / np.linalg.norm(d)
        rays.append(("far%s" % (d,), cam + u * 6.0))                     # beyond max_ray_length (and the map)
    return map_size, dict(resolution=res), cam, [(n, np.float32(p)) for n, p in rays]


def scenario_lanes(grid, single):
    """single: one frame per ray, fused into one map; else all rays in one frame"""
    map_size, kw, cam, rays = lane_rays(grid)
    if single:
        return scenario(map_size, [([p], cam) for _, p in rays], None, **kw)
    return scenario(map_size, [([p for _, p in rays], cam)], None, **kw)


# ---- C: where the cube goes ----
C_MAP = (16.0, 12.0, 4.8)
C_KW = dict(max_ray_length=10.0)


def _box_cloud(rng, lo, hi, n):
    return rng.uniform(lo, hi, size=(n, 3))


def cube_frames():
    """[(label, points, camera)]: one frame per (axis, branch) pair that needs one, the two cubes whose z origin lies
    below 0, the two that overhang the top, the corner columns, and the frame whose last slot widens the box"""
    g = Geo(C_MAP, **C_KW)
    rng = np.random.default_rng(5)
    zc = lambda i: g.org[2] + (i + 0.5) * g.res  # noqa: E731
    out = []
    c0 = (0.05, 0.05, 1.05)
    out.append(("fits", _box_cloud(rng, (1, -1, 0.5), (3, 1, 2.0), 200), c0))
    out.append(("x_low", _box_cloud(rng, (-7.5, -1, 0.5), (1.0, 1, 2.0), 256), (-7.55, 0.05, 1.05)))
    out.append(("x_high", _box_cloud(rng, (-1.0, -1, 0.5), (7.5, 1, 2.0), 256), (7.55, 0.05, 1.05)))
    out.append(("x_middle", _box_cloud(rng, (-5, -1, 0.5), (5, 1, 2.0), 256), c0))
    out.append(("y_low", _box_cloud(rng, (-1, -5.5, 0.5), (1, 2.0, 2.0), 256), (0.05, -5.55, 1.05)))
    out.append(("y_high", _box_cloud(rng, (-1, -2.0, 0.5), (1, 5.5, 2.0), 256), (0.05, 5.55, 1.05)))
    out.append(("y_middle", _box_cloud(rng, (-1, -4.5, 0.5), (1, 4.5, 2.0), 256), c0))
    out.append(("z_low", _box_cloud(rng, (-1.5, -1.5, zc(3)), (1.5, 1.5, zc(47)), 256), (0.05, 0.05, zc(2))))
    out.append(("z_high", _box_cloud(rng, (-1.5, -1.5, zc(0)), (1.5, 1.5, zc(44)), 256), (0.05, 0.05, zc(45))))
    # z origin below 0: camera z index 5, end points from index 0 to 47 (the cube starts at 5 - CUBE_Z / 2)
    p = _box_cloud(rng, (-1.5, -1.5, zc(0)), (1.5, 1.5, zc(47)), 256)
    p[0, 2], p[1, 2] = zc(0), zc(47)
    out.append(("z_below_0", p, (0.05, 0.05, zc(5))))
    # a cube overhanging the top: camera z index 40
    p = _box_cloud(rng, (-1.5, -1.5, zc(0)), (1.5, 1.5, zc(47)), 256)
    p[0, 2], p[1, 2] = zc(0), zc(47)
    out.append(("z_over_top", p, (0.05, 0.05, zc(40))))
    # the corner columns: rays running along (0, 0, *) and (nx - 1, ny - 1, *), the cube's z origin below 0 / its top
    # above the map; the line's bitmap word straddles two words of the miss plane
    for label, ix, iy, iz, sx in (("corner_first", 0, 0, 5, 1.0), ("corner_last", g.nv[0] - 1, g.nv[1] - 1, 40, -1.0)):
        cam = (g.org[0] + (ix + 0.5) * g.res, g.org[1] + (iy + 0.5) * g.res, zc(iz))
        col = np.array([[cam[0], cam[1], zc(i)] for i in range(0, 48, 2)])
        col[::2, :2] += 0.03 * sx
        lo = (min(cam[0], cam[0] + 3 * sx), min(cam[1], cam[1] + 3 * sx), zc(0))
        hi = (max(cam[0], cam[0] + 3 * sx), max(cam[1], cam[1] + 3 * sx), zc(47))
        out.append((label, np.vstack([col, _box_cloud(rng, lo, hi, 200)]), cam))
    # slot coupling: slots 0 .. CLASSIFY_SLOTS - 2 are a narrow fan on the camera's -x side, the last slot lies far on
    # its +x side: the box of the classify workgroup straddles the camera, the first ray workgroup's own box does not
    fan = _box_cloud(rng, (-2.5, -1, 0.5), (-0.5, 1, 2.0), CLASSIFY_SLOTS - 1)
    out.append(("slot_coupling", np.vstack([fan, [[7.0, 0.3, 1.2]]]), c0))
    return [(n, f32(p), np.asarray(c, dtype=float)) for n, p, c in out]


def scenario_cubes():
    return scenario(C_MAP, [(p, c) for _, p, c in cube_frames()], None, **C_KW)


# ---- D: counts at the wave and workgroup edges ----
D_MAP = (4.0, 4.0, 2.0)
D_CAM = (-1.75, -1.75, -0.55)
D_HM_CAM = (-1.75, -1.75, 0.25)
D_COUNTS = (1, 63, 64, 65, 255, 256, 257, 513)
D_RUNS = (1, 2, 63, 64, 65, 128)
D_REGROW = (10, 3000, 10, 5000)


def _d_cloud(n, seed=21):
    """in-map points, a third of them beyond max_ray_length from D_CAM, and a few outside the map"""
    rng = np.random.default_rng(seed)
    p = rng.uniform((-1.9, -1.9, -0.9), (1.9, 1.9, 0.9), size=(n, 3))
    out = rng.random(n) < 0.1
    p[out] = np.array(D_CAM) + (p[out] - np.array(D_CAM)) * 3.0
    return f32(p)


def scenario_counts():
    cloud = _d_cloud(max(D_COUNTS))
    return scenario(D_MAP, [(cloud[:n], D_CAM) for n in D_COUNTS])


def run_cloud():
    """300 points, constant per run of D_RUNS equal points (the last run cut at 300)"""
    base = f32([(0.5, 0.3, 0.2), (1.8, 1.8, 0.8), (-0.5, 0.8, 0.5), (1.85, 1.5, 0.9), (1.0, -0.5, -0.3), (1.3, 1.9, 0.7)])
    return np.repeat(base, D_RUNS, axis=0)[:300]  # (runs of hits and of points beyond max_ray_length in turn)


def scenario_runs():
    cloud = run_cloud()
    return scenario(D_MAP, [(cloud, D_CAM), (cloud[::-1], (0.35, -0.25, 0.15)), (cloud[37:], D_CAM)])


def hit_miss_cloud(g, n_vox=6, reps=22):
    """alternating records of a point within max_ray_length (a hit) and of the same point pushed along its ray beyond
    max_ray_length, whose clipped end lies in the same voxel (a miss): n_vox voxels, reps pairs each, interleaved so
    that the two kinds are neighbours in every slot pair"""
    cam = np.array(D_HM_CAM)
    pts = []
    rng = np.random.default_rng(25)
    for _ in range(2000):  # directions whose point at max_ray_length lies well inside a voxel
        d = np.array([3.3, 2.9, 0.5]) + rng.uniform(-1, 1, 3) * np.array([0.8, 0.3, 0.3])
        u = d / np.linalg.norm(d)
        frac = (cam + u * g.max_ray - g.org) * g.res_inv % 1.0
        if np.all((frac > 0.3) & (frac < 0.7)) and len(pts) < n_vox:
            pts.append((cam + u * (g.max_ray - 0.012), cam + u * (g.max_ray + 0.15)))
    assert len(pts) == n_vox
    out = []
    for _ in range(reps):
        for hit, miss in pts:
            out += [hit, miss]
    return f32(out)


def scenario_hit_miss():
    g = Geo(D_MAP)
    cloud = hit_miss_cloud(g)
    return scenario(D_MAP, [(cloud, D_HM_CAM), (cloud[1:], D_HM_CAM), (cloud[::-1], D_HM_CAM)])


def one_voxel_cloud(n=513, seed=23):
    rng = np.random.default_rng(seed)
    return f32(np.array([0.85, 0.65, 0.35]) + rng.uniform(-0.045, 0.045, size=(n, 3)))


def scenario_one_voxel():
    return scenario(D_MAP, [(one_voxel_cloud(), D_CAM), (one_voxel_cloud(seed=24), (0.35, -0.25, 0.15))])


def scenario_regrow():
    return scenario(D_MAP, [(_d_cloud(n, seed=30 + k), D_CAM) for k, n in enumerate(D_REGROW)])


def nan_frames():
    """[(records with NaN slots, the same records without them, camera)]: NaN in slot 0, in the last slot and between
    equal neighbours (device only: the oracle defines nothing for NaN)"""
    out = []
    for cloud in (_d_cloud(257, seed=40), run_cloud()):
        cloud = cloud.copy()
        bad = np.zeros(len(cloud), dtype=bool)
        bad[[0, len(cloud) - 1]] = True
        same = np.where(np.all(cloud[1:-1] == cloud[:-2], axis=1) & np.all(cloud[1:-1] == cloud[2:], axis=1))[0] + 1
        bad[same[::7]] = True
        bad[[WAVE - 1, WAVE, CLASSIFY_SLOTS - 1]] = True
        dirty = cloud.copy()
        dirty[bad, 0] = np.nan
        out.append((dirty, cloud[~bad], np.array(D_CAM)))
    return out


# ---- E: an origin that is no multiple of the resolution ----
E_MAP = (10.05, 8.03, 4.07)
E_KW = dict(ground_height=-0.97)


def _outside_frames(g, map_size, seed=4):
    """two frames built like outside_camera_frames (test_gpu_parity_r2.py) on this map: the camera 0.3 m beyond the +z
    and the +y face, end points inside the map, within max_ray_length and 1 m away from the x faces (every ray cell
    then has an address inside the grid)"""
    rng = np.random.default_rng(seed)
    top = g.org + np.array(map_size)
    lo, hi = g.org + 0.15, top - 0.15
    lo[0] += 1.0
    hi[0] -= 1.0
    for cam in ((0.3, 0.2, top[2] + 0.3), (0.0, top[1] + 0.3, 0.5)):
        cam = np.array(cam) + rng.normal(scale=0.03, size=3)
        d = rng.normal(size=(900, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        pts = cam + d * rng.uniform(0.5, 4.3, size=(900, 1))
        yield pts[np.all((pts > lo) & (pts < hi), axis=1)], cam


def scenario_unaligned(dropped_in_middle=False):
    g = Geo(E_MAP, **E_KW)
    rng = np.random.default_rng(6)
    size = np.array(E_MAP)
    frames = []
    for _ in range(8):
        cam = g.org + size * rng.uniform(0.2, 0.8, size=3)
        frames.append((cam + rng.normal(scale=3.0, size=(500, 3)), cam))
    if dropped_in_middle:
        cam = np.array([0.4, -0.3, 1.1])
        frames.insert(4, (dropped_cloud(cam), cam))
    frames += list(_outside_frames(g, E_MAP))
    # one far-away junk point: a mark an earlier frame left in the hit / miss planes would be applied now
    frames.append(([g.org + size * np.array([0.08, 0.9, 0.7])], g.org + size * np.array([0.1, 0.85, 0.6])))
    return scenario(E_MAP, frames, None, **E_KW)


# ---- F: a frame whose points are all dropped ----
def scenario_all_dropped_first():
    return scenario(A_MAP, [(dropped_cloud(A_CAM), A_CAM), ([A_JUNK], A_CAM)])


SCENARIOS = {
    "A_counter_directed": scenario_counter_directed,
    "A_counter_random": scenario_counter_random,
    "B_lanes_r0.25_single": lambda: scenario_lanes("r0.25", True),
    "B_lanes_r0.25_frame": lambda: scenario_lanes("r0.25", False),
    "B_lanes_r0.125_single": lambda: scenario_lanes("r0.125", True),
    "B_lanes_r0.125_frame": lambda: scenario_lanes("r0.125", False),
    "C_cubes": scenario_cubes,
    "D_counts": scenario_counts,
    "D_runs": scenario_runs,
    "D_hit_miss": scenario_hit_miss,
    "D_one_voxel": scenario_one_voxel,
    "D_regrow": scenario_regrow,
    "E_unaligned": scenario_unaligned,
    "F_dropped_first": scenario_all_dropped_first,
    "F_dropped_in_E": lambda: scenario_unaligned(True),
    "F_dropped_as_255": lambda: scenario_counter_directed(dropped_at=255),
}
STATE_PLANES = ("A_counter_directed", "A_counter_random", "C_cubes", "E_unaligned")  # inflation + ESDF + one frontier search at the end
