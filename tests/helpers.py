"""Shared fixtures for the parity tests: seeded synthetic maps built with the ORACLE
(test infrastructure), and helpers to push the same state into the GPU map."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import fuel_oracle as fo  # noqa: E402


def explored_oracle_map(map_size, n_obstacles, n_frames, seed=42, cam_seed=7, width=160, height=120,
                        box_margin=1.0, extent=0.7, **kw):
    """Oracle map whose known region was carved by its own inputPointCloud on synthetic frames.

    Exploration box = map shrunk by box_margin in x,y and z in [0, 0.8*sz-1]."""
    org = (-map_size[0] / 2.0, -map_size[1] / 2.0, -1.0)
    box_min = (org[0] + box_margin, org[1] + box_margin, 0.0)
    box_max = (-org[0] - box_margin, -org[1] - box_margin, max(0.8 * map_size[2] - 1.0, 1.0))
    m = fo.OracleMap(map_size, box_min, box_max, **kw)
    truth = m.fixture_world(seed, n_obstacles)
    frames = []
    for k in range(n_frames):
        pose = m.fixture_camera(truth, cam_seed, k, n_frames, extent)
        pts = m.fixture_render(truth, pose, width, height, 2, 2)
        frames.append((pts, pose[:3].copy()))
        m.input_points(pts, pose[:3])
    return m, truth, frames, (box_min, box_max)


def esdf_plan_kernels(fa, gm, lo, hi):
    """the kernels the last updateESDF3d of gm ran over the box [lo, hi]: fuelmi_map_esdf_plan with the family that
    update reported (a PLAIN update the packed pair did not take reports PLAIN32 and ran PLAIN32's plan)"""
    fam = gm.lastEsdfFamily()
    p = fa.SDFMap.esdfPlan(gm.nvox, lo, hi, fam, gm.cfg.optimistic, gm.cfg.signed_dist)
    assert p["family"] == fam
    return [launch["kernel"] for launch in p["launches"]]


def full_box(nvox):
    return (0, 0, 0), (nvox[0] - 1, nvox[1] - 1, nvox[2] - 1)


def make_trajectories(rng, n_traj, n_pts, lo, hi, seg_len=6.0, noise=0.3):
    """Candidate control-point sets: straight segments of seg_len between seeded points plus
    lateral perturbation; returns ctrl [C][N][3]."""
    ctrl = np.empty((n_traj, n_pts, 3))
    lo = np.asarray(lo, dtype=float)
    hi = np.asarray(hi, dtype=float)
    for c in range(n_traj):
        a = lo + (hi - lo) * rng.random(3)
        d = rng.normal(size=3)
        d[2] *= 0.2
        d /= np.linalg.norm(d)
        b = np.clip(a + seg_len * d, lo, hi)
        t = np.linspace(0, 1, n_pts)[:, None]
        ctrl[c] = a + (b - a) * t + rng.normal(scale=noise, size=(n_pts, 3))
    return ctrl


def bspline_inputs(ctrl, dt, mintime=True):
    """NLopt-layout variable vectors + boundary states for a batch of control-point sets."""
    C, N, dim = ctrl.shape
    x = ctrl.reshape(C, N * dim)
    if mintime:
        x = np.concatenate([x, np.full((C, 1), dt)], axis=1)
    pt_dist = np.array([fo.bspline_pt_dist(ctrl[c]) for c in range(C)])
    start = np.zeros((C, 3, 3))
    end = np.zeros((C, 3, 3))
    for c in range(C):
        q = ctrl[c]
        start[c, 0] = (q[0] + 4 * q[1] + q[2]) / 6.0 + 0.05
        start[c, 1] = (q[2] - q[0]) / (2 * dt) * 0.9
        start[c, 2] = (q[0] - 2 * q[1] + q[2]) / (dt * dt) * 0.5
        end[c, 0] = (q[-1] + 4 * q[-2] + q[-3]) / 6.0 - 0.03
        end[c, 1] = 0.1
        end[c, 2] = 0.0
    return np.ascontiguousarray(x), pt_dist, start, end


# ---- a G400-geometry map whose number of kept frontier clusters is chosen (test_frontier_capacity_*) ----
# 40 x 40 x 10 m at 0.1 m, bench.exploration_box; everything known free except isolated unknown blocks, each of which
# leaves one frontier cluster of a known size.  Blocks are placed against the tiles of the fast chain's full-box search.
CAP_MAP = (40.0, 40.0, 10.0)
CAP_CUBE = 5                    # side of a cube: its six faces are one 26-connected shell of 6 * 5 * 5 cells
CUBE_SHELL = 6 * CAP_CUBE ** 2  # (150 > cluster_min = 100)
CAP_SLAB = (8, 13, 5)           # a slab above the box's top face: its underside + the NQ seed that claims it
SLAB_SHELL = CAP_SLAB[0] * CAP_SLAB[1] + 1
CAP_SWEEP = (8, 32, 42, 43, 64, 128, 255, 256, 257)  # kept-cluster counts test_frontier_capacity_gpu runs
_FAST_MENU = ((16, 32), (8, 32), (8, 16), (4, 8))  # frontier_tile.hip kFastMenu: (x-rows, y-lines) per tile


def capacity_map():
    """Oracle map of the fixture's geometry; its occupancy is left to capacity_occupancy."""
    import bench
    return fo.OracleMap(CAP_MAP, *bench.exploration_box(CAP_MAP))


def capacity_tiles(om):
    """(x0, y0, TX, TY, ntx) of the fast chain's tiles for a search whose updated box is the whole exploration box, as
    fuelmi_frontier_search_begin derives them: the scan box (updated box +- (1, 1) m clipped to the exploration box,
    as indices) joined with the Q box (min <= id < max) and cut to [Q lo, Q hi + 1]; the first menu tile that leaves
    at least 512 tiles."""
    blo, bhi = om.box_index()
    p0, p1 = [], []
    for k in range(2):
        s_lo = int(np.floor((max(om.cfg.box_min[k] - 1.0, om.cfg.box_min[k]) - om.origin[k]) / om.res + 1e-9))
        s_hi = int(np.floor((min(om.cfg.box_max[k] + 1.0, om.cfg.box_max[k]) - om.origin[k]) / om.res + 1e-9))
        q_lo, q_hi = max(blo[k], 0), min(bhi[k] - 1, om.nvox[k] - 1)
        p0.append(max(min(s_lo, q_lo), q_lo))
        p1.append(min(max(s_hi, q_hi), q_hi + 1))
    qx, qy = p1[0] - p0[0] + 1, p1[1] - p0[1] + 1
    tiles = lambda t: -(-qx // t[0]) * -(-qy // t[1])  # noqa: E731
    tx, ty = next((t for t in _FAST_MENU if tiles(t) >= 512), _FAST_MENU[-1])
    return p0[0], p0[1], tx, ty, -(-qx // tx)


def capacity_layout(om, n, faces=True, slabs=False, seed=3):
    """n unknown blocks [(lo, hi)] (index boxes, hi exclusive) whose frontier shells are n separate clusters, and the
    straddle counts the layout was planned with: {"x": crosses an x tile boundary only, "y": a y boundary only,
    "corner": both (the shell lies in four tiles), "none"}.

    slabs=False: cubes of side CAP_CUBE (shell CUBE_SHELL, claimed by one of their own cells) on two z layers, three of
    every four across tile boundaries in the order corner, x, y, none; faces=True puts six of them against the
    exploration box: its x / y low faces (the face outside the box is not a frontier), x / y / z high faces (frontier
    cells one voxel outside the box: NQ seeds that stay one-cell clusters) and one slab above the top face (a cluster an
    NQ seed claims, SLAB_SHELL cells).  slabs=True: n slabs only, inside one tile each (every shell SLAB_SHELL, every
    cluster seed-claimed).  Blocks are >= 8 voxels apart: shells never touch."""
    x0, y0, TX, TY, _ = capacity_tiles(om)
    blo, bhi = om.box_index()
    assert (TX, TY) == (8, 32), "the layout below is drawn for 8 x 32 tiles"
    C = CAP_CUBE
    blocks, plan = [], {"x": 0, "y": 0, "corner": 0, "none": 0}
    sx, sy, sz = CAP_SLAB
    if slabs:
        for k in range(n):  # one per tile: x rows 1..8 of every fourth tile column, y lines 5..17 of a tile row
            i, j = k % 11, k // 11
            lo = (x0 + TX * (4 * i + 1), y0 + TY * (j + 1) + 5, bhi[2])
            blocks.append((lo, (lo[0] + sx, lo[1] + sy, lo[2] + sz)))
            plan["x"] += 1  # (the seeds either side of the slab lie in the tiles either side of its own)
        assert blocks[-1][1][1] < bhi[1] - 1
        return blocks, plan
    if faces:
        zf = 68
        for lo, size, cat in (((blo[0], y0 + TY * 3 + 10, zf), (C, C, C), "none"),            # x low face
                              ((x0 + TX * 17 + 1, blo[1], zf), (C, C, C), "none"),            # y low face
                              ((bhi[0] - 4, y0 + TY * 6 + 5, zf), (4, C, C), "x"),            # x high face
                              ((x0 + TX * 30 + 1, bhi[1] - C, zf), (C, C, C), "none"),        # y high face
                              ((x0 + TX * 14 + 1, y0 + TY * 9 + 1, bhi[2] - C), (C, C, C), "none"),  # z high face
                              ((x0 + TX * 36, y0 + TY * 9 + 1, bhi[2]), (sx, sy, sz), "x")):  # above the box
            blocks.append((lo, tuple(lo[q] + size[q] for q in range(3))))
            plan[cat] += 1
    # grid slots: x slot i around the boundary of tile columns 2 i + 1 / 2 i + 2, y slot j (even: across the boundary
    # of tile rows j / 2, j / 2 + 1; odd: inside tile row j / 2 + 1), z layers 30 and 50 (faces: 68 and above)
    bxs = [x0 + TX * (2 * i + 1) for i in range(23)]
    bys = [y0 + TY * (j // 2 + 1) for j in range(22)]
    slots = [(i, j, z) for i in range(23) for j in range(22) for z in (30, 50)]
    order = np.random.default_rng(seed).permutation(len(slots))
    used = np.zeros(len(slots), dtype=bool)
    for k in range(n - len(blocks)):
        cat = ("corner", "x", "y", "none")[k % 4]
        ystr = cat in ("corner", "y")
        s = next(s for s in order if not used[s] and (slots[s][1] % 2 == 0) == ystr)
        used[s] = True
        i, j, z = slots[s]
        xl = bxs[i] - 2 if cat in ("corner", "x") else bxs[i] + 1
        yl = bys[j] - 2 if ystr else bys[j] + 14
        blocks.append(((xl, yl, z), (xl + C, yl + C, z + C)))
        plan[cat] += 1
    return blocks, plan


def capacity_occupancy(om, blocks):
    """log-odds of the fixture: known free (l_min) everywhere, unknown (l_min - 0.01) in the blocks"""
    o3 = np.full(om.nvox, om.l_min)
    for lo, hi in blocks:
        o3[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = om.l_min - 0.01
    return o3.reshape(-1)


def block_straddle(om, lo, hi):
    """which tile boundaries of the full-box search the frontier shell of block [lo, hi) crosses (the voxels one step
    outside the block, inside the tiles' rectangle): "x", "y", "corner" or "none" -- from the tile origin alone"""
    x0, y0, TX, TY, ntx = capacity_tiles(om)
    blo, bhi = om.box_index()
    span = lambda k, t0, T: (max(lo[k] - 1, blo[k]) - t0) // T != (min(hi[k], bhi[k]) - t0) // T  # noqa: E731
    cx, cy = span(0, x0, TX), span(1, y0, TY)
    return "corner" if cx and cy else ("x" if cx else ("y" if cy else "none"))


# ---- the changed-cluster test in front of a search (test_frontier_changed_*) ----
# On the CAP_MAP geometry: a lattice of isolated unknown blocks, one committed cluster each.  An a x b x c block inside
# the box leaves a shell of 2 (ab + bc + ca) frontier cells; a ("slab", a, b) above the box's top face leaves its
# underside plus the NQ seed that claims it, ab + 1.  Blocks fill the lattice x slot first, then y, then z, so their
# clusters come out of a full-box search -- and sit in the candidate table -- in the order of the list; a slab goes
# into the x slot behind every block: it is the last cluster.  cluster_min = 5 keeps every shell (a single unknown
# voxel leaves 6 cells).  frontier_changed.hip picks the test's path from nc (candidates) and total (their cells).
CHG_CLUSTER_MIN = 5
CHG_PITCH = 10                    # lattice pitch: blocks of up to 7 voxels keep 3 free voxels between their shells
CHG_ORIGIN = (12, 12, 20)         # lowest slot; shells stay above min_z = 0.4 m and away from the box's faces
CHG_SLOTS = (37, 37, 5)
RM_ONE_CELLS, RM_BAR_CELLS, RM_LDS = 2048, 512 * 256, 1024
RM_PATHS = ("one", "bar", "staged", "table")
# (clusters, cells, path) of the layouts that pin the edges of the four paths
CHG_EDGES = {
    "one_2048": (24, 2048, "one"),
    "bar_2049": (24, 2049, "bar"),
    "bar_131072": (886, 131072, "bar"),               # 512 workgroups of 256 lanes
    "staged_131073": (886, 131073, "staged"),
    "bar_nc1024": (1024, 6200, "bar"),                # single voxels: a short grid
    "table_nc1025": (1025, 6206, "table"),
    "staged_nc1024": (1024, 151700, "staged"),
    "table_nc1025_big": (1025, 151850, "table"),
}
WAVE_HEAD = 12                    # singles in front of every layout: several clusters in the first 64-lane wave


def shell_size(shape):
    if shape[0] == "slab":
        return shape[1] * shape[2] + 1
    a, b, c = shape
    return 2 * (a * b + b * c + c * a)


def rm_path(nc, total):
    """the path remove_changed_begin takes for nc candidates of total pooled cells"""
    if nc <= RM_LDS and total <= RM_ONE_CELLS:
        return "one"
    if nc <= RM_LDS and -(-total // 256) <= 512:
        return "bar"
    return "staged" if nc <= RM_LDS else "table"


def changed_shapes(n, total, head=WAVE_HEAD, bulk=(5, 5, 5)):
    """n shapes whose shells sum to total: head singles, bulk blocks, one filler block and a last slab"""
    m = n - head - 2
    rest = total - 6 * head - shell_size(bulk) * m
    for a in range(1, 8):
        for b in range(a, 8):
            for c in range(b, 8):
                s = rest - shell_size((a, b, c))
                for sa in range(2, 17):
                    if s - 1 > 0 and (s - 1) % sa == 0 and (s - 1) // sa <= 40:
                        return [(1, 1, 1)] * head + [bulk] * m + [(a, b, c), ("slab", sa, (s - 1) // sa)]
    raise ValueError("no filler for %d clusters of %d cells" % (n, total))


def changed_edge_shapes(name):
    n, total, _ = CHG_EDGES[name]
    return changed_shapes(n, total, bulk=(1, 1, 1) if total < 8 * n else (5, 5, 5))


def changed_blocks(om, shapes):
    """index boxes [(lo, hi)] (hi exclusive) of the shapes, laid out as described above"""
    blo, bhi = om.box_index()
    blocks = []
    nx, ny, nz = CHG_SLOTS
    inner = [s for s in shapes if s[0] != "slab"]
    assert len(inner) <= nx * ny * nz and inner == list(shapes[:len(inner)]), "slabs go last"
    for q, s in enumerate(inner):
        i, j, k = q // (ny * nz), q // nz % ny, q % nz
        lo = (CHG_ORIGIN[0] + CHG_PITCH * i, CHG_ORIGIN[1] + CHG_PITCH * j, CHG_ORIGIN[2] + CHG_PITCH * k)
        assert max(s) <= CHG_PITCH - 3
        blocks.append((lo, (lo[0] + s[0], lo[1] + s[1], lo[2] + s[2])))
    i = (len(inner) - 1) // (ny * nz) + 1 if inner else 0
    for q, s in enumerate(shapes[len(inner):]):
        assert s[0] == "slab"
        lo = (CHG_ORIGIN[0] + CHG_PITCH * (i + 2 * q), CHG_ORIGIN[1], bhi[2])
        blocks.append((lo, (lo[0] + s[1], lo[1] + s[2], bhi[2] + 5)))
    for lo, hi in blocks:
        assert all(blo[q] < lo[q] and hi[q] <= (bhi[q] - 1 if q < 2 else om.nvox[2]) for q in range(3)), (lo, hi)
    return blocks


def have_overlap(min1, max1, min2, max2):
    """haveOverlap (frontier_finder.cpp:353-363), with its 1e-3 slack"""
    return all(max(min1[i], min2[i]) <= min(max1[i], max2[i]) + 1e-3 for i in range(3))


def pooled_cells(om, cells, device_order=True):
    """a committed cluster's cells as the finder's device pool holds them: ascending addresses, an NQ seed (the BFS
    root outside the box) last when the cluster was committed straight from the search (device_order); in plain
    ascending order after the pool was rebuilt from the host lists"""
    blo, bhi = om.box_index()
    x, y, z = np.unravel_index(cells[0], om.nvox)
    seeded = not (blo[0] <= x < bhi[0] and blo[1] <= y < bhi[1] and blo[2] <= z < bhi[2])
    if not (device_order and seeded):
        return np.sort(cells)
    return np.concatenate([np.sort(cells[1:]), cells[:1]])


def changed_candidates(of, om, lo, hi, device_order=True):
    """the candidates of a changed-cluster test against the updated box [lo, hi], from the oracle's committed lists:
    [(which, k, pooled cells)] in table order (frontiers_, then dormant_frontiers_)"""
    out = []
    for which in (1, 2):
        for k, cells in enumerate(of.clusters(which)):
            _, bmin, bmax = of.cluster_info(which, k)
            if have_overlap(bmin, bmax, lo, hi):
                out.append((which, k, pooled_cells(om, cells, device_order)))
    return out


def occupy(om, adrs):
    """a copy of the oracle's log-odds with the cells adrs made occupied: no longer frontier cells"""
    o = om.occ.copy()
    o[np.asarray(adrs, dtype=np.int64)] = om.l_max
    return o


# ---- viewpoint sampling at its wave, candidate and map edges (test_viewpoint_limits_*) ----
# Hand-written states on small maps.  Two families:
#   "patch": obstacles_inflation = 0, everything below min_z occupied except a x b unknown patches in the top floor
#            layer.  The free voxels above a patch are one cluster of exactly a * b cells, all at the same height as
#            their candidates: nothing hides them, so frustum, max_dist and the wave tails alone decide the counts.
#   "room":  default inflation, unknown boxes (their six faces are one shell cluster) and full-height occupied pillars
#            between them and the candidates, given in metres and converted with the map's own posToIndex: rays are
#            stopped, and the scene moves with the resolution and the origin.
# A state is a list of (lo, hi, kind) index boxes (hi exclusive), kind "unknown" / "occupied" / "free", painted in order.
VP_MIN_Z = 0.4
VP_BOX_MARGIN = 0.3


class VpScene:
    """everything both sides need to build a state and run computeFrontiersToVisit on it"""

    def __init__(self, map_size, paint, box=None, map_kw=None, finder=None, vcfg=None):
        self.map_size, self.paint, self.box = tuple(map_size), list(paint), box
        self.map_kw = dict(map_kw or {})
        self.finder = dict(cluster_min=0, min_z=VP_MIN_Z, cluster_size_xy=50.0, down_sample=3)
        self.finder.update(finder or {})
        self.vcfg = dict(min_visib_num=0)
        self.vcfg.update(vcfg or {})

    def variant(self, paint=None, box=None, **vcfg):
        s = VpScene(self.map_size, self.paint if paint is None else paint, self.box if box is None else box,
                    self.map_kw, self.finder, self.vcfg)
        s.vcfg.update(vcfg)
        return s

    def box_args(self):
        """the exploration box; by default the map less VP_BOX_MARGIN on every side (a box that touches a map face
        makes the reference's search loop read one voxel past the map)"""
        if self.box is not None:
            return tuple(self.box[0]), tuple(self.box[1])
        org = np.array([-self.map_size[0] / 2.0, -self.map_size[1] / 2.0,
                        self.map_kw.get("ground_height", fo.DEFAULT_MAP["ground_height"])])
        return tuple(org + VP_BOX_MARGIN), tuple(org + np.array(self.map_size) - VP_BOX_MARGIN)


def vp_map(scene, cls=None):
    """a map of the scene's geometry: fo.OracleMap, ref.RefMap, ... (anything with their constructor)"""
    return (cls or fo.OracleMap)(scene.map_size, *scene.box_args(), **scene.map_kw)


def vp_occupancy(om, paint):
    """log-odds of a painted state on the oracle map's geometry: known free, then the boxes in order"""
    o3 = np.full(om.nvox, om.l_min)
    val = {"unknown": om.l_min - 0.01, "occupied": om.l_max, "free": om.l_min}
    for lo, hi, kind in paint:
        lo = [max(int(v), 0) for v in lo]
        hi = [min(int(hi[q]), om.nvox[q]) for q in range(3)]
        o3[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = val[kind]
    return o3.reshape(-1)


def vp_whole_map(om):
    """(lo, hi) in metres of the whole map: the updated box every search of this suite uses"""
    org = np.asarray(om.origin)
    return tuple(org), tuple(org + np.array(om.nvox) * om.res)


def vp_oracle(scene, reference_order=False, paint=None, vcfg=None):
    """the oracle's run of the scene: (om, of) after inflate, search and computeFrontiersToVisit"""
    om = vp_map(scene)
    om.occ[:] = vp_occupancy(om, scene.paint if paint is None else paint)
    om.set_local_bound(*full_box(om.nvox))
    om.inflate_local()
    of = fo.OracleFrontier(om, split=True, canonical_order=not reference_order, **scene.finder)
    of.set_viewpoint_cfg(fo.viewpoint_cfg(**(scene.vcfg if vcfg is None else vcfg)))
    om.set_updated_box(*vp_whole_map(om))
    of.search()
    of.compute_to_visit()
    return om, of


def vp_views(of):
    """[(which, k, pos_yaw [n, 4], visib [n], filtered [nf, 3])] of every committed cluster, active ones first"""
    return [(w, k) + of.viewpoints(w, k) + (of.filtered(w, k),) for w in (1, 2) for k in range(len(of.clusters(w)))]


def vp_candidate_offsets(vcfg):
    """the candidate table of sampleViewpoints (frontier_finder.cpp:664-667), its two accumulation loops restated:
    [ns, 2] offsets (rc cos phi, rc sin phi) in evaluation order"""
    import math
    c = fo.viewpoint_cfg(**vcfg)
    out = []
    rc, dr = c.candidate_rmin, (c.candidate_rmax - c.candidate_rmin) / c.candidate_rnum
    while rc <= c.candidate_rmax + 1e-3:
        phi = -math.pi
        while phi < math.pi:
            out.append((rc * math.cos(phi), rc * math.sin(phi)))
            phi += c.candidate_dphi
        rc += dr
    return np.array(out).reshape(-1, 2)


def vp_candidates(of, which, k, vcfg):
    """[ns, 3] candidate positions of a committed cluster: average_ + offsets, as the reference adds them"""
    avg = of.cluster_info(which, k)[0]
    off = vp_candidate_offsets(vcfg)
    return np.stack([avg[0] + off[:, 0], avg[1] + off[:, 1], np.full(len(off), avg[2] + 0.0)], axis=1)


def vp_cell_geometry(pos, cells):
    """sampleViewpoints' own arithmetic for one candidate, in the reference's order of operations:
    (distances n [nf], unit directions [nf, 3], cross z of (ref x dir) [nf], dot (dir . ref) [nf], pre-wrap yaw)"""
    import math
    d = cells - np.asarray(pos)[None, :]
    n = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    u = d / n[:, None]
    ref = u[0]
    dot = u[:, 0] * ref[0] + u[:, 1] * ref[1] + u[:, 2] * ref[2]
    cross = ref[0] * u[:, 1] - ref[1] * u[:, 0]
    acc = 0.0
    for i in range(1, len(cells)):
        y = math.acos(dot[i]) if abs(dot[i]) <= 1.0 else float("nan")
        acc += -y if cross[i] < 0 else y
    return n, u, cross, dot, acc / len(cells) + math.atan2(ref[1], ref[0])


def vp_min_cell_distance(of, vcfg):
    """smallest distance between a candidate and a filtered cell of its cluster, over every committed cluster: a
    coincidence would make normalized() divide by zero (the stand-in's caveat)"""
    best = np.inf
    for w, k, _, _, cells in vp_views(of):
        cand = vp_candidates(of, w, k, vcfg)
        best = min(best, np.sqrt(((cand[:, None, :] - cells[None, :, :]) ** 2).sum(-1)).min())
    return best


def vp_floor_top(om):
    """z index of the highest layer whose centre lies below min_z: the top floor layer of a patch scene"""
    return int(np.floor((VP_MIN_Z - om.origin[2]) / om.res - 0.5 - 1e-9))


def vp_patch_paint(om, patches):
    """patch family: the floor (every layer below min_z) occupied, [(x0, y0, a, b)] unknown in its top layer"""
    zt = vp_floor_top(om)
    paint = [((0, 0, 0), (om.nvox[0], om.nvox[1], zt + 1), "occupied")]
    for x0, y0, a, b in patches:
        paint.append(((x0, y0, zt), (x0 + a, y0 + b, zt + 1), "unknown"))
    return paint


def vp_patch_scene(patches, map_size=(16.0, 14.0, 3.0), **kw):
    map_kw = dict(obstacles_inflation=0.0)
    map_kw.update(kw.pop("map_kw", {}))
    s = VpScene(map_size, [], map_kw=map_kw, **kw)
    s.paint = vp_patch_paint(vp_map(s), patches)
    return s


def vp_metric_box(om, lo, hi, kind):
    """a box given in metres as an index box of om (posToIndex of both corners, hi inclusive)"""
    a = np.floor((np.asarray(lo, dtype=float) - om.origin) / om.res).astype(int)
    b = np.floor((np.asarray(hi, dtype=float) - om.origin) / om.res).astype(int) + 1
    return tuple(a), tuple(b), kind


def vp_room_scene(map_size=(16.0, 14.0, 4.0), pillars=True, scale=1.0, **kw):
    """room family: three unknown boxes and full-height pillars around them, laid out in fractions of the map so that
    the same scene exists at every resolution, map size and origin; scale shrinks the boxes with the map"""
    s = VpScene(map_size, [], **kw)
    om = vp_map(s)
    org, top = np.asarray(om.origin), np.asarray(om.origin) + np.asarray(map_size)
    sx, sy = map_size[0] / 16.0, map_size[1] / 14.0
    z0, z1 = 0.62 * scale + (1 - scale) * 0.45, 0.62 * scale + (1 - scale) * 0.45 + 0.8 * scale
    paint = []
    for cx, cy, hx, hy in ((-3.1, -1.4, 0.55, 0.75), (3.3, 1.2, 0.7, 0.4), (0.2, 3.9, 0.35, 0.35)):
        paint.append(vp_metric_box(om, (cx * sx - hx * scale, cy * sy - hy * scale, z0),
                                   (cx * sx + hx * scale, cy * sy + hy * scale, z1), "unknown"))
    if pillars:
        for px, py in ((-1.6, -0.3), (-3.0, 1.1), (-4.6, -2.9), (1.7, 0.2), (3.6, 3.0), (4.9, -0.6), (0.9, 2.4),
                       (-1.1, 4.6), (1.5, 5.3), (-4.4, -0.2), (2.2, -1.5), (0.1, -2.6)):
            paint.append(vp_metric_box(om, (px * sx - 0.14 * scale, py * sy - 0.14 * scale, org[2]),
                                       (px * sx + 0.14 * scale, py * sy + 0.14 * scale, top[2]), "occupied"))
    s.paint = paint
    return s


# -- the scenes of the suite, one builder per edge, and the oracle-only guards that the edge was reached --
VP_NF_CLASSES = ((1, 1), (2, 2), (63, 64), (65, 65), (128, 129), (193, 1 << 30))
VP_GRIDS = {  # name: (resolution, map size, ground height, scale of the room scene, viewpoint overrides)
    "r0.10_aligned": (0.1, (16.0, 14.0, 4.0), -1.0, 1.0, {}),
    "r0.10_offset": (0.1, (16.05, 14.15, 3.7), -1.03, 1.0, {}),
    "r0.15_offset": (0.15, (16.05, 14.15, 3.7), -1.03, 1.0, {}),
    "r0.05_offset": (0.05, (8.05, 7.15, 1.85), -0.52, 0.5, dict(rmin=0.75, rmax=1.25, max_dist=2.25, clearance=0.105)),
}
VP_TABLES = {"default": {}, "rnum1": dict(rnum=1), "rnum5": dict(rnum=5), "dphi0.5": dict(dphi=0.5),
             "dphi7": dict(dphi=7.0), "rmin0.05": dict(rmin=0.05)}
VP_CLEARANCES = {"v0": (0.05, 0), "v1": (0.1, 1), "v2": (0.21, 2), "v2_nominal3": (0.3, 2), "v4": (0.45, 4)}
VP_TABLE_NS = {"default": 100, "rnum1": 50, "rnum5": 150, "dphi0.5": 52, "dphi7": 4, "rmin0.05": 100}  # candidates
VP_MIN_VISIB_TIES = 3   # candidates that must share the count the min_visib_num edge is put on
VP_YAW_MIN = 4          # viewpoints a yaw case must have at each end it is drawn for
VP_NARROW = dict(top_angle=0.25, left_angle=0.45, right_angle=0.20)


def vp_pos_to_idx(om, pos):
    """SDFMap::posToIndex: floor((pos - origin) * resolution_inv)"""
    return np.floor((np.asarray(pos, dtype=float) - om.origin) * (1.0 / om.res)).astype(int)


def vp_positions(of):
    """{(x, y, z) of every accepted viewpoint: visib_num}"""
    return {tuple(p[:3]): int(v) for _, _, py, vis, _ in vp_views(of) for p, v in zip(py, vis)}


def vp_scene_cells(down_sample=1):
    """item 1: patches of 1, 2, 63, 64, 65 (two shapes), 128, 129 and 193 cells, one cluster each; at down_sample = 1
    every cell is its own leaf and nf is the cell count"""
    return vp_patch_scene([(30, 30, 1, 1), (30, 60, 1, 2), (30, 90, 7, 9), (60, 30, 8, 8), (60, 60, 5, 13),
                           (60, 95, 8, 8), (68, 95, 1, 1), (95, 25, 8, 16), (95, 60, 8, 16), (103, 60, 1, 1),
                           (110, 95, 12, 16), (122, 95, 1, 1)], finder=dict(down_sample=down_sample))


def vp_guard_cells(of):
    got = {c: 0 for c in VP_NF_CLASSES}
    for _, _, _, vis, cells in vp_views(of):
        for c in VP_NF_CLASSES:
            if c[0] <= len(cells) <= c[1] and len(vis) > 0:
                got[c] += 1
    assert all(got.values()), "a class of cells per cluster has no cluster with a viewpoint: %s" % got
    nfs = {len(cells) for _, _, _, _, cells in vp_views(of)}
    assert {1, 2, 64, 65, 129, 193} <= nfs, nfs


def vp_scene_clearance(name):
    """item 2: (scene with lone unknown voxels, flips, stays).  Each speck is the corner x = y = +v, z = +1 of one
    accepted candidate's clearance block (the last voxel isNearUnknown visits) and the only unknown voxel in it:
    `flips` are those candidates.  For the clearance that is nominally three voxels, `stays` are candidates with a
    speck at +3, +3, +1: outside the block of floor(0.3 / 0.1) = 2."""
    clearance, v = VP_CLEARANCES[name]
    base = vp_patch_scene([(40, 40, 4, 4), (90, 80, 5, 3), (100, 30, 3, 6), (45, 95, 6, 6)],
                          finder=dict(cluster_min=6), vcfg=dict(clearance=clearance))
    om, of = vp_oracle(base)
    assert int(np.floor(clearance / om.res)) == v
    views = vp_views(of)
    assert len(views) == 4 and all(w == 1 for w, *_ in views)
    flips, stays, specks = [], [], []
    for k, (_, _, py, _, _) in enumerate(views):
        order = np.lexsort((py[:, 1], py[:, 0]))  # a fixed choice: lowest x, spread over the rings by k
        for j, off, into in ((order[k], v, flips), (order[-1 - k], v + 1, stays)):
            if into is stays and name != "v2_nominal3":
                continue
            p = py[j, :3]
            id_ = vp_pos_to_idx(om, p + np.array([off, off, 1]) * om.res)
            specks.append((tuple(id_), tuple(id_ + 1), "unknown"))
            into.append(tuple(p))
    return base.variant(paint=base.paint + specks), flips, stays


def vp_guard_clearance(name, scene, flips, stays):
    v = VP_CLEARANCES[name][1]
    om, of = vp_oracle(scene)
    _, of0 = vp_oracle(scene, paint=[b for b in scene.paint if not (b[2] == "unknown" and b[0][2] > vp_floor_top(om))])
    with_, without = vp_positions(of), vp_positions(of0)
    assert len(flips) >= 3 and all(p in without and p not in with_ for p in flips), "a speck did not flip its candidate"
    assert all(p in without and p in with_ for p in stays), "a speck outside the block flipped its candidate"
    assert (name == "v2_nominal3") == bool(stays)
    w, unk = 2 * v + 1, om.occ.reshape(om.nvox) < om.l_min - 1e-3
    for p in flips:  # the block as isNearUnknown walks it: the speck is its only unknown voxel and its last one
        hit = []
        for t in range(w * w * 3):
            z, r = t % 3 - 1, t // 3
            y, x = r % w - v, r // w - v
            id_ = vp_pos_to_idx(om, np.array(p) + np.array([x, y, z]) * om.res)
            if unk[tuple(id_)]:
                hit.append(t)
        assert hit == [w * w * 3 - 1], (p, hit)
    return om, of


def vp_scene_box_face(face, ulps, reference_order=False):
    """item 3, box faces: one symmetric patch; the box face is the coordinate of a ring-0 candidate itself (x of the
    phi = -pi candidate: avg_x - rmin exactly, for the box's low x face; the largest candidate y for its high y face)
    or its neighbour `ulps` away.  Returns (scene, the candidate, whether isInBox must accept it)."""
    base = vp_patch_scene([(77, 67, 6, 6)])
    _, of = vp_oracle(base, reference_order)
    cand = vp_candidates(of, 1, 0, base.vcfg)
    ns0 = len(cand) // 4  # ring 0
    lo, hi = [list(v) for v in base.box_args()]
    if face == "x_min":
        p = cand[0]
        assert p[0] == of.cluster_info(1, 0)[0][0] - 1.5
        lo[0] = p[0] if ulps == 0 else np.nextafter(p[0], np.inf * ulps)
        inside = lo[0] < p[0]
    else:
        p = cand[np.argmax(cand[:ns0, 1])]
        hi[1] = p[1] if ulps == 0 else np.nextafter(p[1], np.inf * ulps)
        inside = p[1] < hi[1]
    assert tuple(p) in vp_positions(of)
    return base.variant(box=(lo, hi)), tuple(p), bool(inside)


def vp_scene_occluded(grid="r0.10_aligned", pillars=True, **vcfg):
    """item 6: the room scene at one of VP_GRIDS"""
    res, ms, gh, sc, over = VP_GRIDS[grid]
    v = dict(over)
    v.update(vcfg)
    return vp_room_scene(ms, pillars=pillars, scale=sc, map_kw=dict(resolution=res, ground_height=gh), vcfg=v)


def vp_guard_occluded(grid, of, reference_order=False, **vcfg):
    _, of0 = vp_oracle(vp_scene_occluded(grid, pillars=False, **vcfg), reference_order)
    a, b = vp_positions(of), vp_positions(of0)
    stopped = sum(1 for p in b if a.get(p, 0) != b[p])
    assert stopped >= 10, "the pillars stop the rays of %d candidates only" % stopped
    assert len(of.clusters(1)) >= 3 and len(a) >= 60 and sum(a.values()) >= 500, (len(of.clusters(1)), len(a))


def vp_min_visib_edge(grid="r0.10_aligned", reference_order=False):
    """item 3, min_visib_num: (v, n) -- a count v that n >= 3 candidates of the occluded scene have exactly, in the
    cell order the caller runs in (the VoxelGrid centroids, and with them the counts, differ between the orders)"""
    _, of = vp_oracle(vp_scene_occluded(grid), reference_order)
    counts = np.array(sorted(vp_positions(of).values()))
    vals, n = np.unique(counts[counts >= 2], return_counts=True)
    v = int(vals[np.argmax(n >= 3)])
    assert (counts == v).sum() >= VP_MIN_VISIB_TIES
    return v, int((counts == v).sum())


def vp_guard_min_visib(v, n, reference_order=False, grid="r0.10_aligned"):
    """the oracle keeps exactly the n >= 3 candidates of count v at min_visib_num = v - 1 and drops them at v"""
    tot = [len(vp_positions(vp_oracle(vp_scene_occluded(grid, min_visib_num=m), reference_order)[1])) for m in (v, v - 1)]
    assert tot[1] - tot[0] == n >= VP_MIN_VISIB_TIES, (tot, n)


def vp_max_dist_edges(down_sample=1, reference_order=False):
    """item 3, max_dist: (base scene, candidate, {"between": between the nearest and the farthest cell of the cluster
    seen from it, "equal": the distance of one cell, and one cell only, as sampleViewpoints computes it, "below": one
    ulp less}), from a run in the cell order the caller runs in: in the other order the centroids differ in their last
    float ulp and no cell lies at that distance any more"""
    base = vp_patch_scene([(70, 60, 8, 16), (30, 30, 6, 6)], finder=dict(down_sample=down_sample))
    _, of = vp_oracle(base, reference_order)
    _, _, py, _, cells = vp_views(of)[0]
    j = len(py) // 2
    n = vp_cell_geometry(py[j, :3], cells)[0]
    vals, cnt = np.unique(n, return_counts=True)
    once = vals[cnt == 1]
    d = float(once[np.argmin(np.abs(once - np.median(n)))])
    return base, tuple(py[j, :3]), {"between": 0.5 * (n.min() + n.max()), "equal": d, "below": float(np.nextafter(d, 0.0))}


def vp_guard_max_dist(base, p, edges, reference_order=False):
    """the oracle's counts of candidate p at the three bounds: the cell at exactly max_dist is kept, one ulp less
    drops it and it alone; `between` cuts the cluster"""
    c = {k: vp_positions(vp_oracle(base.variant(max_dist=d), reference_order)[1])[p] for k, d in edges.items()}
    full = vp_positions(vp_oracle(base, reference_order)[1])[p]
    assert c["equal"] == c["below"] + 1 and 0 < c["between"] < full, (c, full)
    return c


def vp_scene_collinear():
    """item 3, collinear cells: a 12 x 1 row of cells along x whose y (4.25 m) is a float and lies in [4, 8): every
    filtered cell has the row's y exactly, and so has the phi = -pi candidate of every ring (rc sin(-pi) is below half
    an ulp of 4.25): all cross products are exactly 0"""
    return vp_patch_scene([(60, 112, 12, 1), (100, 27, 1, 12)])


def vp_guard_collinear(scene, of):
    views = vp_views(of)
    w, k, py, _, cells = views[0]
    assert np.all(cells[:, 1] == 4.25) and len(cells) >= 4, cells
    seen = 0
    for rc in (1.5, 1.5 + 1.0 / 3.0):
        p = (of.cluster_info(w, k)[0][0] - rc, 4.25, of.cluster_info(w, k)[0][2])
        hit = [i for i in range(len(py)) if abs(py[i, 0] - p[0]) < 1e-9 and py[i, 1] == 4.25]
        if not hit:
            continue
        _, _, cross, dot, _ = vp_cell_geometry(py[hit[0], :3], cells)
        assert np.all(cross == 0.0) and np.all(np.abs(dot) >= 1.0 - 1e-15), (cross, dot)
        seen += 1
    assert seen >= 1, "no phi = -pi candidate on the row's line was accepted"


def vp_scene_frustum(family, swapped=False, **kw):
    """item 4: a narrow asymmetric frustum on big patches (left / right planes cut them) or on the room scene (all
    four do); swapped: left and right exchanged"""
    f = dict(VP_NARROW)
    if swapped:
        f["left_angle"], f["right_angle"] = f["right_angle"], f["left_angle"]
    if family == "patch":
        return vp_patch_scene([(30, 30, 14, 14), (95, 25, 8, 16), (60, 90, 12, 16), (72, 90, 1, 1), (115, 95, 5, 13)],
                              vcfg=f, **kw)
    return vp_scene_occluded("r0.10_aligned", **f)


def vp_guard_frustum(family, of, reference_order=False):
    _, ofs = vp_oracle(vp_scene_frustum(family, swapped=True), reference_order)
    cut = tot = 0
    for _, _, _, vis, cells in vp_views(of):
        cut += int((vis < len(cells)).sum())
        tot += len(vis)
    assert tot >= 40 and 4 * cut >= tot, (cut, tot)
    a, b = vp_positions(of), vp_positions(ofs)
    assert sum(1 for p in set(a) | set(b) if a.get(p) != b.get(p)) >= 10, "exchanging left and right moved nothing"


def vp_scene_yaw_wrap(family="patch"):
    """item 5.  patch: patches symmetric in y; their candidates near phi = 0 lie due +x of them and look along -x.  The
    reference direction is the first filtered cell, the one of lowest z, then y, then x: on a flat patch it is the
    most clockwise cell seen from +x, so the sums only ever leave [-pi, pi] below -pi.  step: an unknown block whose
    lowest cells lie on its +y side -- there the reference direction is just under +pi and sums end above +pi."""
    if family == "patch":
        return vp_patch_scene([(40, 40, 6, 6), (40, 90, 3, 9), (100, 60, 8, 16), (100, 20, 2, 2)])
    s = VpScene((16.0, 14.0, 4.0), [])
    om = vp_map(s)
    s.paint = [vp_metric_box(om, (-0.5, 0.3, 0.6), (0.5, 0.89, 1.39), "unknown"),
               vp_metric_box(om, (-0.5, -0.9, 0.9), (0.5, 0.29, 1.39), "unknown")]
    return s


def vp_guard_yaw_wrap(of):
    """{+1 / -1: yaws within 1e-6 of +pi / -pi, "below" / "above": sums that left [-pi, pi] at either end before the
    wrap loops}, recomputed from the filtered cells"""
    import math
    got = {1: 0, -1: 0, "below": 0, "above": 0}
    for _, _, py, _, cells in vp_views(of):
        for p in py:
            pre = vp_cell_geometry(p[:3], cells)[4]
            wrapped = pre
            while wrapped < -math.pi:
                wrapped += 2 * math.pi
            while wrapped > math.pi:
                wrapped -= 2 * math.pi
            d = abs(wrapped - p[3])
            assert min(d, 2 * math.pi - d) <= 1e-9  # (the restatement above is the oracle's)
            got["below"] += int(pre < -math.pi)
            got["above"] += int(pre > math.pi)
            if math.pi - abs(p[3]) <= 1e-6:
                got[1 if p[3] > 0 else -1] += 1
    assert got["below"] + got["above"] >= 1, "no mean bearing left [-pi, pi] before the wrap"
    return got


VP_DPHI_ABOVE = 15 * 3.1415927 / 180.0  # 12 steps from -pi end just above 0 (the default's 3.1415926 ends just below)


def vp_guard_tables(of, vcfg):
    """item 8: every accepted viewpoint is, bit for bit, an entry of the candidate table restated in numpy, in the
    table's order within equal counts; returns ns"""
    ns = len(vp_candidate_offsets(vcfg))
    for w, k, py, _, _ in vp_views(of):
        cand = {tuple(c): i for i, c in enumerate(vp_candidates(of, w, k, vcfg))}
        assert len(cand) == ns or ns == 0
        assert all(tuple(p[:3]) in cand for p in py), "a viewpoint that is not in the restated table"
    return ns


VP_FACE_BLOCKS = {  # index boxes on the 120 x 100 x 30 map of vp_scene_faces, one voxel thick, against every map face
    "x_low": ((0, 45, 10), (1, 55, 16)), "x_high": ((119, 30, 12), (120, 42, 18)),
    "y_low": ((50, 0, 8), (60, 1, 14)), "y_high": ((70, 99, 14), (82, 100, 20)),
    "z_low": ((30, 20, 0), (50, 22, 1)), "z_high": ((80, 60, 29), (100, 62, 30)),
}


def vp_scene_faces(beyond=False):
    """item 7: the exploration box is the whole map (beyond: 0.55 m more on every side; map creation does not clamp it),
    a thin unknown block against each of the six map faces, no z cut (min_z far below the map).  Oracle only: the
    real reference's search loop reads one voxel past a map face its box touches, and its z cut is fixed at 0.4 m."""
    ms, gh = (12.0, 10.0, 3.0), -1.0
    org = np.array([-6.0, -5.0, gh])
    pad = 0.55 if beyond else 0.0
    box = (tuple(org - pad), tuple(org + np.array(ms) + pad))
    return VpScene(ms, [(lo, hi, "unknown") for lo, hi in VP_FACE_BLOCKS.values()], box=box,
                   map_kw=dict(ground_height=gh), finder=dict(min_z=-5.0, cluster_min=10))


def vp_scene_floor_probe():
    """item 7, posToIndex below the map: the box reaches beyond the map, no inflation, candidate_dphi = 0.5.  Some
    accepted candidates then lie less than a voxel outside the low x face: posToIndex floors them to x = -1, outside
    the map, where nothing is inflated.  The voxel a truncating cast would give them, (0, y, z), is made occupied.
    Returns (scene, those candidates)."""
    base = vp_scene_faces(True)
    base.map_kw["obstacles_inflation"] = 0.0
    base.vcfg["dphi"] = 0.5
    om, of = vp_oracle(base)
    hit = [p for p in vp_positions(of) if -om.res < p[0] - om.origin[0] < 0.0]
    walls = []
    for p in hit:
        id_ = vp_pos_to_idx(om, p)
        assert id_[0] == -1
        walls.append(((0, id_[1], id_[2]), (1, id_[1] + 1, id_[2] + 1), "occupied"))
    return base.variant(paint=base.paint + walls), hit


def vp_guard_floor_probe(om, of, hit):
    pos = vp_positions(of)
    assert len(hit) >= 1 and all(p in pos for p in hit), "a probed candidate is no longer accepted"
    for p in hit:
        id_ = vp_pos_to_idx(om, p)
        assert om.infl.reshape(om.nvox)[0, id_[1], id_[2]] == 1


def vp_guard_faces(om, of, vcfg, beyond):
    v = int(np.floor(fo.viewpoint_cfg(**vcfg).min_candidate_clearance / om.res))
    ids = np.array([vp_pos_to_idx(om, p) for p in vp_positions(of)])
    n = np.array(om.nvox)
    assert len(of.clusters(1)) + len(of.clusters(2)) == 6
    for q in range(2):
        assert ((ids[:, q] >= 0) & (ids[:, q] < v)).any() and ((ids[:, q] <= n[q] - 1) & (ids[:, q] > n[q] - 1 - v)).any(), q
    assert (ids[:, 2] == 0).any() and (ids[:, 2] == n[2] - 1).any()
    outside = ((ids < 0) | (ids > n - 1)).any(axis=1)
    assert outside.any() == beyond, "accepted candidates outside the map: %d" % outside.sum()


# item 9: three states of one patch map; a 1 x 2 patch whose two cells can never beat min_visib_num = 3 goes dormant
VP_ROUNDS = (
    [(40, 40, 6, 6), (90, 80, 5, 3), (30, 100, 1, 2)],
    [(40, 40, 6, 6), (30, 100, 1, 2)] + [(20 + 24 * i, 15 + 30 * j, 8, 16) for i in range(5) for j in range(3)
                                          if (i, j) != (1, 1)] + [(130, 120, 2, 1)],
    [(40, 40, 6, 6), (20, 15, 8, 16), (100, 100, 4, 4)],
)


def vp_scene_rounds(r):
    return vp_patch_scene(VP_ROUNDS[r], vcfg=dict(min_visib_num=3))


def vp_stage_bytes(ncl, ns, nf):
    """bytes one sampling call stages on the device: means, candidate table, cell offsets, cells, results"""
    pad8 = lambda b: (b + 7) // 8 * 8  # noqa: E731
    return 24 * ncl + 16 * ns + pad8(4 * (ncl + 1)) + pad8(12 * nf) + 40 * ncl * ns


def vp_guard_stage_growth(need):
    """the staging bytes of the three rounds: the second outgrows what the first allocated (view_stage takes a quarter
    and 4 KiB more than asked), the third fits again"""
    assert need[1] > 1.25 * need[0] + 4096 and need[2] < need[1], need
