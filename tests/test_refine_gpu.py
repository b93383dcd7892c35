"""fuelmi_map_refine_tours on the device against the restatement (tests/refine_ref.py) fed with the device's own
searchPath lengths (SDFMap.path_costs): the headline cycle, batching invariance, every rule of the reference on small
maps, the polyline, and the facade's refineLocalTour / refineSingleDestination."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import refine_ref as rr
from test_refine_cpu import nan_edge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
VM, YD, WDIR = 2.0, 60 * 3.1415926 / 180.0, 1.5


def _device_world(map_size, box, occ_fn=None):
    import fuel_amd
    gm = fuel_amd.SDFMap(map_size, box[0], box[1], device=0)
    nv = gm.nvox
    occ = np.full(nv, gm.info.clamp_min_log)
    if occ_fn is not None:
        occ_fn(occ, gm.info.clamp_max_log, gm.info.clamp_min_log - 0.01)
    gm.uploadOccupancy(occ.reshape(-1))
    gm.setLocalBound((0, 0, 0), (nv[0] - 1, nv[1] - 1, nv[2] - 1))
    gm.clearAndInflateLocalMap()
    return gm


def _lengths(gm, g, res=0.4):
    """the device's searchPath lengths of every edge of g: {(u, v): length}, and their kinds"""
    pairs = g.edge_pairs()
    p1 = np.array([g.pts[u] for u, _ in pairs])
    p2 = np.array([g.pts[v] for _, v in pairs])
    length, kind, _ = gm.path_costs(p1, p2, res=res, max_points=0)
    return dict(zip(pairs, length)), kind


def _restated(gm, pos, vel, yaw, layers, argmin=False):
    g = rr.Graph(pos, vel, yaw, layers, last_argmin=argmin)
    lengths, kind = _lengths(gm, g)
    cost = g.costs(lengths, VM, YD, WDIR)
    ch, c = rr.layer_dp(g, cost)
    return g, cost, ch, c, kind


def _refine(gm, problems, **kw):
    return gm.refine_tours(problems, VM, YD, WDIR, **kw)


def _assert_same(dev_ch, dev_c, ch, c, exact=True):
    if ch is None:
        assert list(dev_ch) == [-1] * len(dev_ch) and dev_c == math.inf
        return
    assert list(dev_ch) == ch
    if exact:
        assert dev_c == c
    else:  # device acos against glibc's: within an ulp per direction term
        assert abs(dev_c - c) <= 1e-12 * abs(c)


def _near_ties(g, cost, ch, rel=1e-12):
    """candidates at a node of the chosen route whose key (total, g(u)) lies within rel of the winner's without being
    equal: only those could flip under an ulp of acos (everything else is computed in the same operation order)"""
    gv = {0: 0.0}
    prev = [0]
    for ids in g.layer_ids:
        for v in ids:
            t = [gv[u] + cost[(u, v)] for u in prev]
            t = [x for x in t if x < rr.G_INIT]
            gv[v] = min(t) if t else rr.G_INIT
        prev = ids
    near, prev = [], [0]
    for i, ids in enumerate(g.layer_ids):
        v = ids[ch[i]]
        win = prev[ch[i - 1]] if i > 0 else 0
        t0, g0 = gv[win] + cost[(win, v)], gv[win]
        for u in prev:
            if u == win:
                continue
            t = gv[u] + cost[(u, v)]
            if (t != t0 and abs(t - t0) <= rel * t0) or (t == t0 and g0 != gv[u] and abs(gv[u] - g0) <= rel * g0):
                near.append((i, u, t - t0))
        prev = ids
    return near


# ---- 1. the headline cycle -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g400():
    import bench
    import fuel_amd
    map_size, box, occ, _, _ = bench.build_inputs("G400", seed=42)
    gm = fuel_amd.SDFMap(map_size, box[0], box[1], device=0)
    gm.uploadOccupancy(occ)
    nv = gm.nvox
    gm.setLocalBound((0, 0, 0), (nv[0] - 1, nv[1] - 1, nv[2] - 1))
    gm.clearAndInflateLocalMap()
    gf = fuel_amd.FrontierFinder(gm, cluster_min=100, cluster_size_xy=2.0, down_sample=3, split=True)
    cfg = gf.viewpointConfig()
    gf.setViewpointConfig(cfg)
    gm.setUpdatedBox(box[0], box[1])
    gf.searchFrontiers()
    na, _ = gf.computeFrontiersToVisit()
    views = {}
    for k in range(na):
        py, vis = gf.viewpoints(1, k)
        views[k] = [(py[i, :3], py[i, 3], int(vis[i])) for i in range(len(py))]
    gf.close()
    yield gm, views, cfg.min_candidate_dist
    gm.close()


def _layers(views, cur, ids, min_dist):
    P, Y = rr.viewpoints_info(cur, views, ids, 15, 0.8, min_dist)
    return [np.concatenate([np.array(p), np.array(y)[:, None]], axis=1) for p, y in zip(P, Y)]


def test_headline_cycle(g400):
    gm, views, min_dist = g400
    assert len(views) >= 20
    vel, yaw = np.array([0.5, -0.3, 0.1]), 0.3
    ids = list(range(7))
    done, seen = False, []
    for s in range(10, 20):  # a free start (another cluster's best viewpoint) whose answer has no near-tie
        cur = views[s][0][0]
        layers = _layers(views, cur, ids, min_dist)
        assert max(len(l) for l in layers) > 1
        g, cost, ch, c, kind = _restated(gm, cur, vel, yaw, layers)
        assert ch is not None
        near = _near_ties(g, cost, ch)
        seen.append((s, ch, c, near[:3]))
        if near:
            continue
        assert rr.dijkstra(g, cost) == (ch, c)
        assert (kind == 1).sum() > 0  # some edges took the lattice
        (dev_ch,), dev_c, tours = _refine(gm, [(cur, vel, yaw, layers)])
        _assert_same(dev_ch, dev_c[0], ch, c, exact=False)
        assert tours is None
        done = True
        break
    assert done, seen


# ---- 2. batching invariance ------------------------------------------------------------------------------------------
def test_batching_invariance(g400):
    gm, views, min_dist = g400
    rng = np.random.default_rng(7)
    probs = []
    starts = [views[s][0][0] for s in (10, 11, 12)]
    for b in range(16):
        cur = starts[b % 2] if b < 8 else starts[2] + (0.0 if b % 4 else 0.05 * b)  # shared and distinct starts
        ids = list(rng.choice(len(views), 3, replace=False))
        layers = [l[:6] for l in _layers(views, cur, ids, min_dist)]
        probs.append((cur, rng.normal(size=3) * (b % 3 != 0), float(rng.uniform(-3, 3)), layers))
    ch, c, tours = _refine(gm, probs, tour_res=0.2, max_tour_points=4096, last_argmin=False)
    for b in range(16):
        ch1, c1, t1 = _refine(gm, probs[b:b + 1], tour_res=0.2, max_tour_points=4096)
        assert np.array_equal(ch[b], ch1[0]) and c[b].tobytes() == c1[0].tobytes(), b
        assert np.array_equal(tours[b], t1[0]), b


# ---- 3. edge cases on small maps ------------------------------------------------------------------------------------
SMALL = ((8.0, 8.0, 4.0), ((-3.9, -3.9, 0.05), (3.9, 3.9, 2.9)))


@pytest.fixture(scope="module")
def open_map():
    gm = _device_world(*SMALL)
    yield gm
    gm.close()


def _L(points, yaws):
    return [np.concatenate([np.asarray(points, dtype=float), np.asarray(yaws, dtype=float)[:, None]], axis=1)]


def _check(gm, pos, vel, yaw, layers, argmin=False, exact=True):
    g, cost, ch, c, _ = _restated(gm, pos, vel, yaw, layers, argmin)
    (dev_ch,), dev_c, _ = _refine(gm, [(pos, vel, yaw, layers)], last_argmin=argmin)
    _assert_same(dev_ch, dev_c[0], ch, c, exact=exact)
    return list(dev_ch), dev_c[0], cost


def test_one_layer_tie_and_the_flag(open_map):
    gm = open_map
    pos, z = np.array([0.0, 0.0, 1.0]), np.zeros(3)
    layers = _L([(2.0, 0.0, 1.0), (0.0, 1.0, 1.0), (-1.0, 0.0, 1.0)], [0.0, 0.0, 0.0])
    assert _check(gm, pos, z, 0.0, layers, argmin=True)[:2] == ([1], 0.5)  # exact tie: the first index
    assert _check(gm, pos, z, 0.0, layers)[:2] == ([0], 1.0)                # only node 0 of the last layer


def test_last_layer_beyond_node_0_is_ignored(open_map):
    gm = open_map
    pos, vel = np.array([0.0, 0.0, 1.0]), np.array([0.3, 0.1, 0.0])
    l1 = _L([(1.0, 1.0, 1.0), (1.5, -1.0, 1.2), (0.5, 0.5, 0.8)], [0.2, -0.4, 1.0])[0]
    last = _L([(2.5, 0.3, 1.0), (0.1, 0.1, 1.0), (-2.0, 2.0, 1.0)], [0.0, 1.0, 2.0])[0]
    a = _refine(gm, [(pos, vel, 0.1, [l1, last])])
    last2 = last.copy()
    last2[1:] = [[2.6, 0.0, 1.0, 0.0], [0.0, 0.0, 1.0, 0.0]]
    b = _refine(gm, [(pos, vel, 0.1, [l1, last2])])
    assert np.array_equal(a[0][0], b[0][0]) and a[1].tobytes() == b[1].tobytes()
    _check(gm, pos, vel, 0.1, [l1, last], exact=False)


def test_direction_term_threshold_and_zero_length_edge(open_map):
    gm = open_map
    pos = np.array([0.0, 0.0, 1.0])
    layers = _L([(-1.0, 0.0, 1.0)], [0.0])
    assert _check(gm, pos, np.array([1e-3, 0.0, 0.0]), 0.0, layers)[1] == 0.5
    _, c, _ = _check(gm, pos, np.array([2e-3, 0.0, 0.0]), 0.0, layers, exact=False)
    assert c > 0.5 + WDIR * 3.14
    # a viewpoint at the start: real Eigen's rule, pi / 2 (the restatement, not the stand-in's hostCost)
    _, c, _ = _check(gm, pos, np.array([0.3, 0.0, 0.0]), 0.0, _L([pos], [0.0]), exact=False)
    assert abs(c - WDIR * math.pi / 2) <= 1e-15


def test_nan_edge_flips_the_choice_and_unreached_goal(open_map):
    gm = open_map
    v, d = nan_edge(np.random.default_rng(4), max_len=0.8)
    pos = np.array([0.0, 0.0, 1.0])
    perp = np.array([d[1], -d[0], 0.0])
    far = pos + perp * (2.0 * rr.norm3(*d) / rr.norm3(*perp))
    near = pos + d
    assert gm.path_costs([pos, pos], [near, far], max_points=0)[1].tolist() == [0, 0]
    layers = _L([near, far], [0.0, 0.0])
    ch, _, cost = _check(gm, pos, v, 0.0, layers, argmin=True, exact=False)
    assert math.isnan(cost[(0, 1)]) and ch == [1]
    assert _check(gm, pos, np.zeros(3), 0.0, layers, argmin=True)[0] == [0]
    ch, c, _ = _check(gm, pos, v, 0.0, _L([near], [0.0]))
    assert ch == [-1] and c == math.inf


def test_yaw_wrap(open_map):
    gm = open_map
    _, c, _ = _check(gm, np.array([0.0, 0.0, 1.0]), np.zeros(3), 3.1, _L([(0.05, 0.0, 1.0)], [-3.1]))
    assert c == (2 * math.pi - 6.2) / YD


def test_sealed_viewpoint():
    gm = _device_world(*SMALL, lambda occ, solid, unk: occ.__setitem__((slice(38, 40), slice(None), slice(None)), solid))
    pos = np.array([-1.0, 0.0, 1.0])
    _, c, _ = _check(gm, pos, np.zeros(3), 0.0, _L([(1.0, 0.0, 1.0)], [0.0]))
    assert c == 1000.0 / VM
    gm.close()


def test_refusals_on_a_real_map(open_map):
    import fuel_amd
    gm = open_map
    pos = np.array([0.0, 0.0, 1.0])
    one = _L([(1.0, 0.0, 1.0)], [0.0])[0]
    _refine(gm, [(pos, np.zeros(3), 0.0, [one, one])])
    before = gm.path_stats()
    assert before["launches"] == 0  # straight lines only
    for layers, code in (([one, np.zeros((0, 4))], "-1"), ([one] * 65, "-5"), ([np.tile(one, (257, 1))], "-5")):
        with pytest.raises(fuel_amd.FuelmiError) as e:
            _refine(gm, [(pos, np.zeros(3), 0.0, layers)], last_argmin=True)
        assert code in str(e.value)
    # refused before any device work: the stats of the last call are untouched
    _, _, _ = gm.path_costs([pos], [(-3.0, 2.0, 2.0)], max_points=0)
    st = gm.path_stats()
    with pytest.raises(fuel_amd.FuelmiError):
        _refine(gm, [(pos, np.zeros(3), 0.0, [one] * 65)])
    assert gm.path_stats() == st


def _door_map():
    def fill(occ, solid, unk):
        free = occ[0, 0, 0]
        occ[38:40, :, :] = solid  # a wall at x ~ -0.2 with a door near y = 1.6, z < 1.4
        occ[38:40, 52:60, 10:26] = free
    return _device_world(*SMALL, fill)


def test_polyline_is_the_legs_at_0_2():
    gm = _door_map()
    pos, vel = np.array([-1.0, 0.0, 1.0]), np.array([0.2, 0.0, 0.0])
    layers = [_L([(0.6, 0.0, 1.0), (0.7, 0.8, 1.3)], [0.0, 0.5])[0],
              _L([(0.6, 0.0, 1.0), (0.6, -1.0, 1.0)], [0.0, 0.2])[0],  # a repeated point: a zero-length leg
              _L([(-2.0, 1.0, 1.2), (0.0, 0.0, 0.0)], [1.0, 0.0])[0]]
    (ch,), c, (tour,) = _refine(gm, [(pos, vel, 0.0, layers)], tour_res=0.2, max_tour_points=4096)
    assert ch[0] >= 0
    pts = [layers[i][ch[i], :3] for i in range(3)]
    p1 = np.array([pos] + pts[:-1])
    L, K, P = gm.path_costs(p1, np.array(pts), res=0.2, max_points=4096)
    assert (K == 1).sum() >= 2 and (L == 0.0).any(), (K, L)  # through the door both ways; the repeated point
    want = rr.polyline(pos, pts, list(zip(L, P)))
    assert np.array_equal(tour, want)
    # the limit: fills what fits, FUELMI_ELIMIT
    import fuel_amd
    with pytest.raises(fuel_amd.FuelmiError) as e:
        _refine(gm, [(pos, vel, 0.0, layers)], tour_res=0.2, max_tour_points=len(want) - 1)
    assert "-5" in str(e.value)
    gm.close()


# ---- 4. the facade --------------------------------------------------------------------------------------------------
def _facade_run(scen, with_params):
    exe = os.path.join(ROOT, "fuel_amd", "facade", "facade_refine")
    out = subprocess.run([exe, scen, str(int(with_params))], check=True, capture_output=True, text=True,
                         timeout=300).stdout
    res = {"layer": [], "refined": [], "pt": []}
    for line in out.splitlines():
        f = line.split()
        if not f:
            continue
        if f[0] == "layer":
            res["layer"].append(np.array([float(v) for v in f[2:]]).reshape(-1, 4))
        elif f[0] in ("refined", "pt"):
            res[f[0]].append([float(v) for v in f[1:]])
        elif f[0] == "cur":
            res["cur"] = [float(v) for v in f[1:]]
        elif f[0] in ("refine", "clusters"):
            res[f[0]] = int(f[1])
        elif f[0] == "single":
            res["single"] = (int(f[1]), int(f[2]))
    return res


def test_facade_refine(tmp_path):
    import fuel_amd
    from fuel_amd import synth
    map_size, box = (10.0, 8.0, 4.0), ((-4.0, -3.0, 0.0), (4.0, 3.0, 2.2))
    w = synth.World.for_map_size(map_size)
    truth = w.world(3, 14)
    occ, _ = w.known_state(truth, 3, 6, 1.5, 2.5)
    scen = str(tmp_path / "scen.bin")
    with open(scen, "wb") as f:
        np.array(list(map_size) + list(box[0]) + list(box[1]), dtype=np.float64).tofile(f)
        np.ascontiguousarray(occ, dtype=np.float64).tofile(f)
    assert _facade_run(scen, False)["refine"] == 0  # the ViewNode parameters are required
    res = _facade_run(scen, True)
    assert res["refine"] == 1 and res["clusters"] >= 2 and len(res["layer"]) >= 2
    cur = res["cur"]
    pos, vel, yaw = np.array(cur[0:3]), np.array(cur[3:6]), cur[6]
    layers = res["layer"]
    gm = fuel_amd.SDFMap(map_size, box[0], box[1], device=0)
    gm.uploadOccupancy(np.ascontiguousarray(occ, dtype=np.float64).reshape(-1))
    nv = gm.nvox
    gm.setLocalBound((0, 0, 0), (nv[0] - 1, nv[1] - 1, nv[2] - 1))
    gm.clearAndInflateLocalMap()
    (ch,), c, (tour,) = gm.refine_tours([(pos, vel, yaw, layers)], VM, YD, WDIR, tour_res=0.2)
    g, cost, rch, rc, _ = _restated(gm, pos, vel, yaw, layers)
    assert list(ch) == rch
    refined = np.array([layers[i][ch[i]] for i in range(len(layers))])
    assert np.array_equal(np.array(res["refined"]), refined)
    assert np.array_equal(np.array(res["pt"]), tour)
    # the single-destination branch on the first cluster (the driver asks getViewpointsInfo for cluster 0 again,
    # which gives layer 0)
    (ch1,), _, _ = gm.refine_tours([(pos, vel, yaw, layers[:1])], VM, YD, WDIR, last_argmin=True)
    g1, cost1, rch1, _, _ = _restated(gm, pos, vel, yaw, layers[:1], argmin=True)
    ids = g1.layer_ids[0]
    lengths1 = {v: cost1[(0, v)] for v in ids}
    i_ref, _ = rr.single_destination(pos, vel, yaw, [g1.pts[v] for v in ids], [g1.yaws[v] for v in ids],
                                     [_lengths(gm, g1)[0][(0, v)] for v in ids], VM, YD, WDIR)
    assert res["single"] == (1, int(ch1[0])) and rch1 == [i_ref] == [int(ch1[0])], lengths1
    gm.close()
