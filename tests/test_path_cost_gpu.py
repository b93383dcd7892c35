"""fuelmi_map_path_costs on the device against the CPU restatement (tests/path_cost_ref.py): the straight line bit for
bit on the headline map, the lattice search bit for bit on small maps, path properties, the limits, batching
invariance, and every viewpoint pair of the headline cycle."""
import os
import sys
import time

import numpy as np
import pytest

import path_cost_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


def _device_world(map_size, box, occ_fn):
    """device map + oracle twin (for its ray walk) + the restatement's view of the device planes"""
    import fuel_amd
    from oracle import fuel_oracle as fo
    gm = fuel_amd.SDFMap(map_size, box[0], box[1], device=0)
    om = fo.OracleMap(map_size, box[0], box[1])
    nv = gm.nvox
    occ = np.full(nv, gm.info.clamp_min_log)
    occ_fn(occ, gm.info.clamp_max_log, gm.info.clamp_min_log - 0.01)
    gm.uploadOccupancy(occ.reshape(-1))
    gm.setLocalBound((0, 0, 0), (nv[0] - 1, nv[1] - 1, nv[2] - 1))
    gm.clearAndInflateLocalMap()
    return gm, om, pr.PathMap.from_device(gm)


def _g400():
    import bench
    import fuel_amd
    from oracle import fuel_oracle as fo
    map_size, box, occ, _, _ = bench.build_inputs("G400", seed=42)
    gm = fuel_amd.SDFMap(map_size, box[0], box[1], device=0)
    gm.uploadOccupancy(occ)
    nv = gm.nvox
    gm.setLocalBound((0, 0, 0), (nv[0] - 1, nv[1] - 1, nv[2] - 1))
    gm.clearAndInflateLocalMap()
    om = fo.OracleMap(map_size, box[0], box[1])
    return gm, om, pr.PathMap.from_device(gm), box


@pytest.fixture(scope="module")
def g400():
    gm, om, pm, box = _g400()
    yield gm, om, pm, box
    gm.close()


def _check_properties(pm, kind, length, path):
    """consecutive lattice points are 26-neighbours over usable edges; length = pathLength of the points"""
    assert kind == 1
    assert length == pr.path_length(path)
    for a, b in zip(path[:-2], path[1:-1]):
        assert pr.edge_ok(pm, a, b), (a, b)


def _compare(pm, om, p1, p2, length, kind, paths, lattices=None):
    lattices = {} if lattices is None else lattices
    for i in range(len(p1)):
        key = p1[i].tobytes()
        lat = lattices.get(key)
        if lat is None and not pr.straight_line_safe(pm, om, p1[i], p2[i]):
            lat = lattices[key] = pr.Lattice(pm, p1[i])
            lat.d = lat.dijkstra()
        k, L, P = pr.search_path(pm, om, p1[i], p2[i], lattice=lat)
        assert kind[i] == k, (i, p1[i], p2[i], kind[i], k)
        assert length[i] == L, (i, length[i], L)
        assert np.array_equal(paths[i], P), i
        if k == 1:
            _check_properties(pm, k, length[i], paths[i])


# ---- 1. the straight line, bit for bit, on the headline map ----------------------------------------------------------
def test_straight_line_bit_exact_g400(g400):
    gm, om, pm, box = g400
    rng = np.random.default_rng(11)
    lo, hi = np.array(box[0]), np.array(box[1])
    n = 4096
    # few sources (the lattice search of the blocked pairs runs per source); ends anywhere, a tenth outside the box,
    # some p1 in unknown space, some ends nudged next to inflated voxels
    srcs = lo + (hi - lo) * rng.random((12, 3))
    p1 = srcs[rng.integers(0, len(srcs), n)]
    p2 = lo + (hi - lo) * rng.random((n, 3))
    out = rng.random(n) < 0.1
    p2[out] = lo - 2.0 + (hi - lo + 4.0) * rng.random((out.sum(), 3))
    short = rng.random(n) < 0.5
    p2[short] = p1[short] + rng.normal(scale=1.5, size=(short.sum(), 3))
    bad = np.argwhere(pm.bad)
    graze = bad[rng.integers(0, len(bad), 300)]
    p2[:300] = pm.origin + (graze + 0.5) * pm.res + rng.uniform(-0.12, 0.12, size=(300, 3))
    length, kind, paths = gm.path_costs(p1, p2, max_points=0)
    assert paths is None
    n_line = 0
    for i in range(n):
        safe = pr.straight_line_safe(pm, om, p1[i], p2[i])
        assert (kind[i] == 0) == safe, (i, p1[i], p2[i], kind[i])
        if safe:
            n_line += 1
            assert length[i] == pr.norm3(*(p1[i] - p2[i]))
    assert 50 < n_line < n - 50  # both outcomes are exercised (the headline map is mostly unknown)
    # the paths of the straight pairs: {p1, p2}
    sel = np.flatnonzero(kind == 0)[:256]
    _, k2, P2 = gm.path_costs(p1[sel], p2[sel], max_points=4)
    assert (k2 == 0).all()
    for j, i in enumerate(sel):
        assert np.array_equal(P2[j], [p1[i], p2[i]])


# ---- 2./3. the lattice, bit for bit, on small maps -------------------------------------------------------------------
SMALL = ((8.0, 8.0, 4.0), ((-3.9, -3.9, 0.05), (3.9, 3.9, 2.9)))


def _walls(occ, solid, unknown):
    free = occ[0, 0, 0]
    occ[38:40, :, :] = solid          # wall at x ~ -0.2 ... with a door
    occ[38:40, 52:60, 10:26] = free
    occ[50:52, 20:70, 10:40] = solid  # a second wall, open at low y
    occ[60:62, 10:40, 10:20] = solid  # a low wall and a raised floor: a staircase in z
    occ[62:70, 10:40, 10:18] = solid
    occ[64:66, 30:32, 22:24] = unknown


def test_lattice_bit_exact_small_maps():
    gm, om, pm = _device_world(*SMALL, lambda occ, solid, unk: _walls(occ, solid, unk))
    rng = np.random.default_rng(5)
    srcs = np.array([[-1.0, 0.0, 1.0], [-2.3, -1.1, 0.7], [1.05, 1.6, 0.45], [0.3, -2.2, 2.1]])
    p1 = srcs[rng.integers(0, len(srcs), 96)]
    p2 = np.array([-3.5, -3.5, 0.2]) + np.array([7.0, 7.0, 2.6]) * rng.random((96, 3))
    length, kind, paths = gm.path_costs(p1, p2, max_points=512)
    assert (kind == 1).sum() >= 20, np.bincount(kind)
    _compare(pm, om, p1, p2, length, kind, paths)
    gm.close()


# ---- 4. no path, start in goal, the point limit ---------------------------------------------------------------------
def test_sealed_start_in_goal_and_point_limit():
    def fill(occ, solid, unk):
        occ[38:40, :, :] = solid    # a full wall: nothing crosses x ~ -0.2
        occ[10:35, 30:32, :] = solid  # a wall across y, open only at x < -3.2 after inflation
        occ[30, 40, 20] = unk       # one unknown voxel beside a source
    gm, om, pm = _device_world(*SMALL, fill)
    p1 = np.array([[-1.0, 0.0, 1.0], [-1.0, 0.0, 1.0], [-3.0, -3.0, 1.0]])
    p2 = np.array([[1.0, 0.5, 1.2], [-1.0 - 0.25, 0.0, 1.0], [-1.5, 2.5, 1.5]])
    # pair 1: the line from voxel 28 to voxel 31 crosses the unknown voxel 30; p1 and p2 share lattice index 7
    p1[1] = (-1.15, 0.05, 1.05)
    p2[1] = (-0.9, 0.05, 1.05)
    length, kind, paths = gm.path_costs(p1, p2, max_points=64)
    assert kind[0] == 2 and length[0] == 1000.0 and np.array_equal(paths[0], [p1[0], p2[0]])
    _compare(pm, om, p1, p2, length, kind, paths)
    assert kind[1] == 1 and np.array_equal(paths[1], [p1[1], p2[1]])  # the start is a goal node
    assert kind[2] == 1 and len(paths[2]) > 4
    n3 = len(paths[2])
    import fuel_amd
    with pytest.raises(fuel_amd.FuelmiError) as e:
        gm.path_costs(p1, p2, max_points=n3 - 1)
    assert "-5" in str(e.value)
    # path_len still carries the full count
    import ctypes as C
    from fuel_amd import _lib
    c = _lib.PathCfg(0.4, 0.1, 1000.0, n3 - 1)
    L, K = np.empty(3), np.empty(3, dtype=np.int32)
    PL = np.empty(3, dtype=np.int32)
    buf = np.zeros((3, n3 - 1, 3))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731
    rc = gm.L.fuelmi_map_path_costs(gm.h, C.byref(c), 3, dp(p1), dp(p2), dp(L), ip(K), ip(PL), dp(buf))
    assert rc == -5
    # a real map with a NULL configuration is refused before any work
    assert gm.L.fuelmi_map_path_costs(gm.h, None, 3, dp(p1), dp(p2), dp(L), ip(K), ip(PL), dp(buf)) == -1
    assert list(PL) == [2, 2, n3] and np.array_equal(L, length) and np.array_equal(K, kind)
    gm.close()


# ---- 5. batching invariance -----------------------------------------------------------------------------------------
def test_batching_invariance():
    gm, om, pm = _device_world(*SMALL, lambda occ, solid, unk: _walls(occ, solid, unk))
    rng = np.random.default_rng(9)
    srcs = np.array([[-1.0, 0.0, 1.0], [1.05, 1.6, 0.45], [-2.3, -1.1, 0.7]])
    p1 = srcs[rng.integers(0, len(srcs), 40)]
    p2 = np.array([-3.5, -3.5, 0.2]) + np.array([7.0, 7.0, 2.6]) * rng.random((40, 3))
    single = [gm.path_costs(p1[i:i + 1], p2[i:i + 1], max_points=512) for i in range(40)]
    perm = rng.permutation(40)
    idx = np.concatenate([perm, perm[:15]])  # shuffled, with duplicates
    L, K, P = gm.path_costs(p1[idx], p2[idx], max_points=512)
    for j, i in enumerate(idx):
        assert K[j] == single[i][1][0] and L[j].tobytes() == single[i][0][0].tobytes()
        assert np.array_equal(P[j], single[i][2][0])
    gm.close()


# ---- 6. every viewpoint pair of the headline cycle ------------------------------------------------------------------
def test_headline_cycle_all_viewpoint_pairs(g400):
    import fuel_amd
    gm, om, pm, box = g400
    gf = fuel_amd.FrontierFinder(gm, cluster_min=100, cluster_size_xy=2.0, down_sample=3, split=True)
    gf.setViewpointConfig(gf.viewpointConfig())
    gm.setUpdatedBox(box[0], box[1])
    gf.searchFrontiers()
    na, _ = gf.computeFrontiersToVisit()
    vps = np.array([gf.viewpoints(1, k)[0][0, :3] for k in range(na)])
    gf.close()
    assert len(vps) >= 100
    a, b = np.triu_indices(len(vps), 1)
    # the facade issues an old x new link from the new side: sources are the rows
    p1, p2 = vps[a], vps[b]
    t0 = time.perf_counter()
    length, kind, paths = gm.path_costs(p1, p2, max_points=1024)
    dt = time.perf_counter() - t0
    assert dt < 120.0, dt
    assert set(np.unique(kind)) <= {0, 1, 2}
    assert (kind == 1).sum() > 0
    lat_pairs = np.flatnonzero(kind == 1)
    for i in lat_pairs:
        assert length[i] == pr.path_length(paths[i])
        assert np.array_equal(paths[i][0], p1[i]) and np.array_equal(paths[i][-1], p2[i])
        steps = np.rint((paths[i][2:-1] - paths[i][1:-2]) / 0.4)
        assert np.abs(steps).max(initial=1) <= 1
    # the edge-safety rule on one lattice pair of every source and 1 500 more drawn at random
    first = {}
    for i in lat_pairs:
        first.setdefault(a[i], i)
    rng = np.random.default_rng(3)
    sample = set(first.values()) | set(rng.choice(lat_pairs, min(1500, len(lat_pairs)), replace=False).tolist())
    for i in sorted(sample):
        _check_properties(pm, kind[i], length[i], paths[i])
    # two sources in full: csgraph distances, then the restatement's goal / backtrack
    blocked_src = [s for s in np.unique(a) if (kind[a == s] == 1).any()][:2]
    assert blocked_src
    for s in blocked_src:
        lat = pr.Lattice(pm, vps[s])
        lat.d = lat.csgraph_dist()
        for i in np.flatnonzero(a == s):
            k, L, P = pr.search_path(pm, om, p1[i], p2[i], lattice=lat)
            assert kind[i] == k and length[i] == L and np.array_equal(paths[i], P), i
            if k == 1:
                _check_properties(pm, k, length[i], paths[i])


# ---- 7. the facade: frontier/device_path_cost -----------------------------------------------------------------------
def _facade_run(scen, opt_in):
    import subprocess
    exe = os.path.join(ROOT, "fuel_amd", "facade", "facade_pathcost")
    out = subprocess.run([exe, scen, str(int(opt_in))], check=True, capture_output=True, text=True, timeout=300).stdout
    res = {"vp": [], "row": [], "pt": []}
    for line in out.splitlines():
        f = line.split()
        if not f:
            continue
        if f[0] == "clusters":
            res["n1"], res["removed"], res["n"] = (int(v) for v in f[1:4])
        elif f[0] == "tour":
            res["tour"] = [int(v) for v in f[1:]]
        elif f[0] == "cur":
            res["cur"] = [float(v) for v in f[1:]]
        elif f[0] in res:
            res[f[0]].append([float(v) for v in f[1:]])
    return {k: (np.array(v) if k in ("vp", "row", "pt") else v) for k, v in res.items()}


def _host_cost(length, p1, p2, y1, y2, v1, vm=2.0, yd=60 * 3.1415926 / 180.0, w_dir=1.5):
    """ViewNode::computeCost (graph_node.cpp:63-88) on the device length, as the facade computes it"""
    import math
    pos_cost = length / vm
    if pr.norm3(*v1) > 1e-3:
        d = [p2[k] - p1[k] for k in range(3)]
        nd = pr.norm3(*d)
        d = [d[k] / nd for k in range(3)]
        nv = pr.norm3(*v1)
        vd = [v1[k] / nv for k in range(3)]
        pos_cost += w_dir * math.acos(vd[0] * d[0] + vd[1] * d[1] + vd[2] * d[2])
    diff = abs(y2 - y1)
    diff = min(diff, 2 * math.pi - diff)
    return max(pos_cost, diff / yd)


def test_facade_device_path_cost(tmp_path):
    import fuel_amd
    from fuel_amd import synth
    map_size, box = (10.0, 8.0, 4.0), ((-4.0, -3.0, 0.0), (4.0, 3.0, 2.2))
    w = synth.World.for_map_size(map_size)
    truth = w.world(3, 14)
    occ1, _ = w.known_state(truth, 3, 3, 1.5, 2.5)
    occ2, _ = w.known_state(truth, 3, 6, 1.5, 2.5)
    scen = str(tmp_path / "scen.bin")
    with open(scen, "wb") as f:
        np.array(list(map_size) + list(box[0]) + list(box[1]), dtype=np.float64).tofile(f)
        np.ascontiguousarray(occ1, dtype=np.float64).tofile(f)
        np.ascontiguousarray(occ2, dtype=np.float64).tofile(f)
    dev = _facade_run(scen, True)
    ref = _facade_run(scen, False)
    n, n_old = dev["n"], dev["n1"] - dev["removed"]
    assert n >= 4 and n_old >= 2 and n > n_old, (dev["n1"], dev["removed"], n)
    assert np.array_equal(dev["vp"], ref["vp"]) and dev["tour"] == ref["tour"]
    vp, cur = dev["vp"], dev["cur"]
    cpos, cvel, cyaw = cur[0:3], cur[3:6], cur[6:8]

    def device_map(occ):
        gm = fuel_amd.SDFMap(map_size, box[0], box[1], device=0)
        gm.uploadOccupancy(np.ascontiguousarray(occ, dtype=np.float64).reshape(-1))
        nv = gm.nvox
        gm.setLocalBound((0, 0, 0), (nv[0] - 1, nv[1] - 1, nv[2] - 1))
        gm.clearAndInflateLocalMap()
        return gm
    gm1, gm2 = device_map(occ1), device_map(occ2)
    # the stored link of i -> j: old x old from round 1 (searched from the earlier), old x new searched from the new
    # one in round 2 (reversed for the old record), new x new from the earlier
    link = {}
    for i in range(n):
        for j in range(i + 1, n):
            if j < n_old:
                gm, src, dst, rev = gm1, i, j, False
            elif i < n_old:
                gm, src, dst, rev = gm2, j, i, True
            else:
                gm, src, dst, rev = gm2, i, j, False
            L, K, P = gm.path_costs(vp[src:src + 1, :3], vp[dst:dst + 1, :3], max_points=1024)
            path = P[0][::-1] if rev else P[0]  # i -> j
            c = _host_cost(L[0], vp[i, :3], vp[j, :3], vp[i, 3], vp[j, 3], (0.0, 0.0, 0.0))
            link[(i, j)] = (c, path)
            link[(j, i)] = (c, path[::-1])
    mat = dev["row"]
    assert mat.shape == (n + 1, n + 1)
    L0, _, P0 = gm2.path_costs(np.repeat([cpos], n, axis=0), vp[:, :3], max_points=1024)
    for j in range(n):
        assert mat[0, j + 1] == _host_cost(L0[j], cpos, vp[j, :3], cyaw[0], vp[j, 3], cvel), j
        assert mat[j + 1, 0] == 0.0
        for i in range(n):
            assert mat[i + 1, j + 1] == (0.0 if i == j else link[(i, j)][0]), (i, j)
    tour = dev["tour"]
    want = [P0[tour[0]]] + [link[(a, b)][1] for a, b in zip(tour[:-1], tour[1:])]
    assert np.array_equal(dev["pt"], np.concatenate(want))
    # the default: ViewNode as the driver defines it (straight flight + 0.1 |yaw difference|, end points)
    m = ref["row"]
    for j in range(n):
        assert m[0, j + 1] == pr.norm3(*(vp[j, :3] - cpos)) + 0.1 * abs(vp[j, 3] - cyaw[0])
        for i in range(n):
            if i != j:
                a, b = min(i, j), max(i, j)
                assert m[i + 1, j + 1] == pr.norm3(*(vp[b, :3] - vp[a, :3])) + 0.1 * abs(vp[b, 3] - vp[a, 3])
    want = [np.array([cpos, vp[tour[0], :3]])] + [np.array([vp[a, :3], vp[b, :3]]) for a, b in zip(tour[:-1], tour[1:])]
    assert np.array_equal(ref["pt"], np.concatenate(want))
    gm1.close()
    gm2.close()
