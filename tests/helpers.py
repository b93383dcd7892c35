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
