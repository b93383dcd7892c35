"""fuelmi_map_goal_paths on the device against the restatement (tests/goal_path_ref.py), bit for bit in status, counts,
way-points, next_goal, raw path and length: the wall-and-door map, k_goal_shorten's window edges, every threshold at
its value and the value's neighbours, rays that leave the map, a goal in an unknown voxel, batching invariance, the
limits and refusals, the headline cycle, and the facade's planPathToViewpoint.  tests/test_goal_path_cpu.py asserts on
the restatement alone that these scenes hold what they claim."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import goal_path_ref as gr
import path_cost_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


def _device_twin(om, size, box):
    """the device map of an oracle map's occupancy; its inflated / unknown voxels must be the oracle's"""
    import fuel_amd
    gm = fuel_amd.SDFMap(size, box[0], box[1], device=0)
    gm.uploadOccupancy(np.array(om.occ, dtype=np.float64))
    nv = gm.nvox
    gm.setLocalBound((0, 0, 0), (nv[0] - 1, nv[1] - 1, nv[2] - 1))
    gm.clearAndInflateLocalMap()
    assert np.array_equal(pr.PathMap.from_device(gm).bad, pr.PathMap.from_oracle(om).bad)
    return gm


def _run(gm, case, **kw):
    cfg = dict(gr.DEFAULTS, **case.get("cfg", {}))
    cfg.update(kw)
    return gm.goal_paths(case["starts"], case["goals"], **cfg)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def _assert_problem(out, b, r, tag=""):
    """device problem b = restatement r, every bit"""
    where = (tag, b)
    assert out["status"][b] == r["status"], (where, out["status"][b], r["status"])
    assert out["raw_len"][b] == r["raw_len"], (where, out["raw_len"][b], r["raw_len"])
    assert out["n_way"][b] == len(r["way"]), (where, out["n_way"][b], len(r["way"]))
    assert _bits(out["length"][b]) == _bits(r["length"]), (where, out["length"][b], r["length"])
    assert _bits(out["next_goal"][b]) == _bits(r["next_goal"]), (where, out["next_goal"][b], r["next_goal"])
    assert _bits(out["way"][b]) == _bits(np.array(r["way"]).reshape(-1, 3)), (where, out["way"][b], r["way"])
    assert _bits(out["raw"][b]) == _bits(np.array(r["raw"]).reshape(-1, 3)), where


def _forms_agree(pm, om, case, ref):
    """the literal loop = the first-push form, for scenes whose inputs only exist on the device (the others:
    tests/test_goal_path_cpu.py)"""
    cfg = dict(gr.DEFAULTS, **case.get("cfg", {}))
    for r in ref:
        if r["status"] in (gr.NO_PATH, gr.RAW_OVER):
            continue
        fp = gr.first_push_shorten(pm, om, r["raw"], cfg["shorten_dist"], cfg["end_eps"])
        assert len(fp) == len(r["short"]) and all(np.array_equal(a, b) for a, b in zip(fp, r["short"]))


def _assert_case(gm, pm, om, case, sources=None, tag="", **kw):
    out = _run(gm, case, **kw)
    ref = gr.solve_case(pm, om, case, sources)
    assert len(ref) == len(out["status"]) > 0
    _forms_agree(pm, om, case, ref)
    for b, r in enumerate(ref):
        _assert_problem(out, b, r, tag)
    return out, ref


# ---- 1. the wall-and-door map ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def door():
    om, pm, size, box, case = gr.door_scene()
    gm = _device_twin(om, size, box)
    sources = {}
    ref = gr.solve_case(pm, om, case, sources)
    yield gm, om, pm, case, ref, sources
    gm.close()


def test_door_scene_bit_exact(door):
    gm, om, pm, case, ref, sources = door
    assert len(ref) >= 80 and len(sources) >= 2
    out = _run(gm, case)
    for b, r in enumerate(ref):
        _assert_problem(out, b, r, "door")
    st = gm.path_stats()
    assert st["sources"] == len(sources) and st["chunks"] == 1 and st["launches"] > 0, st
    assert {gr.CLOSE, gr.MID, gr.FAR, gr.NO_PATH} <= set(out["status"].tolist())
    ms = gm.goal_path_times()
    assert ms[0] > 0.0 and ms[1] > 0.0
    # without the raw path: the same answers
    lean = _run(gm, case, raw=False)
    assert "raw" not in lean
    for k in ("status", "length", "n_way", "next_goal"):
        assert _bits(lean[k]) == _bits(out[k]), k
    assert all(_bits(a) == _bits(b) for a, b in zip(lean["way"], out["way"]))


# ---- 2. the window edges of k_goal_shorten ---------------------------------------------------------------------------
def test_window_edges():
    om, pm = gr.corridor_map()
    gm = _device_twin(om, gr.CORRIDOR_SIZE, gr.CORRIDOR_BOX)
    cases, src = gr.window_cases(pm)
    sources = {(gr.CORRIDOR_START.tobytes(), gr.CORRIDOR_RES, 0.1): src}
    seen = []
    for case in cases:
        out, ref = _assert_case(gm, pm, om, case, sources, tag=str(case.get("run", case.get("points"))))
        seen.append(tuple(out["raw_len"].tolist()))
    assert seen[-1] == (2, 3, 64, 65, 66)
    assert all(n[0] > 2 * gr.WINDOW + 3 for n in seen[:-1])
    gm.close()


# ---- 3. the thresholds -----------------------------------------------------------------------------------------------
def test_thresholds_at_the_value_and_its_neighbours(door):
    gm, om, pm, case, ref, _ = door
    b = next(i for i, r in enumerate(ref) if r["status"] == gr.MID and r["raw_len"] >= 12)
    cases, src = gr.threshold_cases(pm, om, case["starts"][b], case["goals"][b])
    sources = {(case["starts"][b].tobytes(), 0.2, 0.1): src}
    got = {}
    for name, v, three in cases:
        got[name] = [_assert_case(gm, pm, om, c, sources, tag="%s %d" % (name, k))[0] for k, c in enumerate(three)]
    assert [int(o["status"][0]) for o in got["radius_close"]] == [gr.MID, gr.MID, gr.CLOSE]
    assert [int(o["status"][0]) for o in got["radius_far"]] == [gr.FAR, gr.MID, gr.MID]
    lo, at, hi = got["shorten_dist"]
    assert _bits(lo["way"][0]) != _bits(at["way"][0]) and _bits(at["way"][0]) == _bits(hi["way"][0])
    lo, at, hi = got["end_eps"]
    assert _bits(lo["way"][0]) != _bits(at["way"][0]) and _bits(at["way"][0]) == _bits(hi["way"][0])


# ---- 4. a ray that leaves the map, a goal in an unknown voxel ---------------------------------------------------------
def test_ray_outside_the_map_and_goal_in_unknown():
    om, pm = gr.face_map()
    gm = _device_twin(om, gr.FACE_SIZE, gr.FACE_BOX)
    out, ref = _assert_case(gm, pm, om, gr.face_case(), tag="face")
    assert gr.NO_PATH not in out["status"].tolist()
    gm.close()


# ---- 5. batching invariance, the limits, the refusals ----------------------------------------------------------------
def test_alone_equals_batched(door):
    gm, om, pm, case, ref, _ = door
    batch = dict(starts=case["starts"][12:76], goals=case["goals"][12:76], cfg={})  # 64 problems, both starts
    assert len(batch["starts"]) == 64 and len({s.tobytes() for s in batch["starts"]}) == 2
    out = _run(gm, batch)
    for b in range(64):
        one = _run(gm, dict(starts=batch["starts"][b:b + 1], goals=batch["goals"][b:b + 1], cfg={}))
        for k in ("status", "length", "n_way", "next_goal", "raw_len"):
            assert _bits(one[k][0]) == _bits(out[k][b]), (b, k)
        assert _bits(one["way"][0]) == _bits(out["way"][b]) and _bits(one["raw"][0]) == _bits(out["raw"][b]), b
        _assert_problem(one, 0, ref[12 + b], "alone")


def test_batch_over_several_source_chunks():
    om, pm = pr.chunk_map()
    p1, p2, chunk = pr.chunk_case(pm, om)
    assert max(chunk) >= 1
    gm = _device_twin(om, pr.CHUNK_SIZE, pr.CHUNK_BOX)
    case = dict(starts=p1, goals=p2, cfg=dict(res=pr.CHUNK_RES))
    out = _run(gm, case)
    st = gm.path_stats()
    assert st["sources"] == len(p1) and st["chunks"] == max(chunk) + 1, st
    assert gr.NO_PATH not in out["status"].tolist()
    last1 = max(i for i in range(len(p1)) if chunk[i] == 0)
    for b in (0, last1, last1 + 1, len(p1) - 1):
        one = _run(gm, dict(starts=p1[b:b + 1], goals=p2[b:b + 1], cfg=case["cfg"]))
        for k in ("status", "length", "n_way", "next_goal", "raw_len"):
            assert _bits(one[k][0]) == _bits(out[k][b]), (b, k)
        assert _bits(one["way"][0]) == _bits(out["way"][b]) and _bits(one["raw"][0]) == _bits(out["raw"][b]), b
    # the two sides of the chunk boundary in full (csgraph distances: 0.8 M nodes each)
    for b in (last1, last1 + 1):
        src = {(p1[b].tobytes(), pr.CHUNK_RES, 0.1): gr.Source(pm, p1[b], pr.CHUNK_RES, 0.1, csgraph=True)}
        one = dict(starts=p1[b:b + 1], goals=p2[b:b + 1], cfg=case["cfg"])
        r = gr.solve_case(pm, om, one, src)[0]
        _forms_agree(pm, om, one, [r])
        _assert_problem(out, b, r, "chunk")
    gm.close()


def test_limits_fill_counts_and_keep_fitting_problems(door):
    import fuel_amd
    gm, om, pm, case, ref, _ = door
    far = [i for i, r in enumerate(ref) if r["status"] == gr.FAR]
    big = max(far, key=lambda i: ref[i]["raw_len"])      # the longest raw path
    small = next(i for i, r in enumerate(ref) if r["status"] == gr.CLOSE and r["raw_len"] < ref[big]["raw_len"] - 1
                 and len(r["way"]) < len(ref[big]["way"]))
    ids = [small, big]
    two = dict(starts=case["starts"][ids], goals=case["goals"][ids], cfg={})
    n_raw, n_way = ref[big]["raw_len"], len(ref[big]["way"])
    # exactly at the counts: complete
    out = _run(gm, two, max_path_points=n_raw, max_way_points=n_way)
    assert not out["limit"]
    for k, i in enumerate(ids):
        _assert_problem(out, k, ref[i], "at the limit")
    # one below the raw count: FUELMI_ELIMIT, the count filled, the fitting problem complete
    with pytest.raises(fuel_amd.FuelmiError) as e:
        _run(gm, two, max_path_points=n_raw - 1)
    assert "-5" in str(e.value)
    out = _run(gm, two, max_path_points=n_raw - 1, allow_limit=True)
    assert out["limit"] and out["status"][1] == gr.RAW_OVER and out["raw_len"][1] == n_raw and out["n_way"][1] == 0
    _assert_problem(out, 0, ref[small], "beside a raw overflow")
    # one below the way-point count: the count filled, what fits written, status / length / next_goal complete
    out = _run(gm, two, max_way_points=n_way - 1, allow_limit=True)
    r = ref[big]
    assert out["limit"] and out["n_way"][1] == n_way and out["status"][1] == r["status"]
    assert _bits(out["length"][1]) == _bits(r["length"]) and _bits(out["next_goal"][1]) == _bits(r["next_goal"])
    assert _bits(out["way"][1]) == _bits(np.array(r["way"][:n_way - 1]))
    _assert_problem(out, 0, ref[small], "beside a way-point overflow")


def test_refusals(door):
    import fuel_amd
    gm, om, pm, case, ref, _ = door
    s, g = case["starts"][:1], case["goals"][:1]
    empty = gm.goal_paths(np.zeros((0, 3)), np.zeros((0, 3)))
    assert len(empty["status"]) == 0 and not empty["limit"]
    _run(gm, dict(starts=s, goals=g, cfg={}))
    st = gm.path_stats()
    assert st["launches"] > 0
    bad = [dict(starts=np.array([[math.nan, 0.0, 1.0]])), dict(goals=np.array([[0.0, math.inf, 1.0]])),
           dict(goals=np.array([[0.0, 1e7, 1.0]])), dict(res=0.0), dict(res=-0.2), dict(res=math.nan),
           dict(edge_step=0.0), dict(shorten_dist=0.0), dict(radius_close=-1.5), dict(radius_far=0.0),
           dict(radius_far=math.inf), dict(end_eps=-1e-3), dict(end_eps=math.nan), dict(max_path_points=1),
           dict(max_way_points=0)]
    for kw in bad:
        kw = dict(kw)
        a, b = kw.pop("starts", s), kw.pop("goals", g)
        with pytest.raises(fuel_amd.FuelmiError) as e:
            gm.goal_paths(a, b, **kw)
        assert "-1" in str(e.value), kw
        assert gm.path_stats() == st, kw  # refused before any device work


# ---- 6. the headline cycle -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g400():
    import bench
    import fuel_amd
    from oracle import fuel_oracle as fo
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
    om = fo.OracleMap(map_size, box[0], box[1])  # geometry only: the restatement's ray walk
    yield gm, om, pr.PathMap.from_device(gm), views
    gm.close()


def _ray_clear(pm, om, a, b):
    return not gr.ray_blocked(pm, om, a, b)


def test_headline_cycle(g400):
    gm, om, pm, views = g400
    assert len(views) >= 20
    cur = views[10][0][0]  # the current position: a free viewpoint; the next viewpoints: every cluster's best
    goals = np.array([views[k][0][0] for k in sorted(views)])
    case = dict(starts=np.repeat([cur], len(goals), axis=0), goals=goals, cfg={})
    out = _run(gm, case, max_path_points=4096)
    assert gm.path_stats()["sources"] == 1
    status = out["status"]
    assert (status != gr.NO_PATH).sum() >= len(goals) // 2
    for b in range(len(goals)):
        if status[b] == gr.NO_PATH:
            assert out["n_way"][b] == 0 and out["raw_len"][b] == 0
            continue
        raw, way = out["raw"][b], out["way"][b]
        assert _bits(raw[0]) == _bits(cur) and _bits(raw[-1]) == _bits(goals[b])
        index = {_bits(p): i for i, p in reversed(list(enumerate(raw)))}
        mid = len(way) == 3 and _bits(way[1]) not in index
        if mid:
            assert _bits(way[1]) == _bits(0.5 * (way[0] + way[2]))
            way = way[[0, 2]]
        ids = [index[_bits(p)] for p in way]
        assert ids[0] == 0 and all(i < j for i, j in zip(ids[:-1], ids[1:])), (b, ids)
        for i, j in zip(ids[:-1], ids[1:]):  # the candidate before a push did not push: the ray to raw[j] was clear
            assert j == i + 1 or _ray_clear(pm, om, raw[i], raw[j]), (b, i, j)
        # pathLength(short) <= pathLength(raw) by the triangle inequality; both are sums of at most len(raw) rounded
        # norms, each term and each addition within 2^-53 relative: an allowance of len(raw) * 2^-51 of the raw length
        raw_length = pr.path_length(raw)
        assert out["length"][b] <= raw_length * (1.0 + len(raw) * 2.0 ** -51), (b, out["length"][b], raw_length)
        if status[b] == gr.FAR:
            assert _bits(out["next_goal"][b]) in index and _bits(out["next_goal"][b]) == _bits(way[-1])
            assert out["length"][b] > 5.0
        else:
            assert _bits(out["next_goal"][b]) == _bits(goals[b])
            assert (out["length"][b] < 1.5) == (status[b] == gr.CLOSE)
    # in full: one source, csgraph distances, then the restatement's goal / backtrack / shortenPath for every goal
    src = {(cur.tobytes(), 0.2, 0.1): gr.Source(pm, cur, csgraph=True)}
    ref = gr.solve_case(pm, om, case, src)
    _forms_agree(pm, om, case, ref)
    for b, r in enumerate(ref):
        _assert_problem(out, b, r, "G400")


# ---- 7. the facade ---------------------------------------------------------------------------------------------------
def _facade_run(scen):
    exe = os.path.join(ROOT, "fuel_amd", "facade", "facade_goalpath")
    p = subprocess.run([exe, scen], check=True, capture_output=True, text=True, timeout=300)
    res = {}
    for line in p.stdout.splitlines():
        f = line.split()
        if not f:
            continue
        if f[0] == "goal":
            res[int(f[1])] = dict(branch=int(f[2]), n=int(f[3]), next_goal=[float(v) for v in f[4:7]], way=[])
        elif f[0] == "way":
            res[int(f[1])]["way"].append([float(v) for v in f[2:5]])
    return res, p.stderr


def test_facade_goal_path(tmp_path):
    import fuel_amd
    from fuel_amd import synth
    from oracle import fuel_oracle as fo
    map_size, box = (10.0, 8.0, 4.0), ((-4.0, -3.0, 0.0), (4.0, 3.0, 2.2))
    w = synth.World.for_map_size(map_size)
    truth = w.world(3, 14)
    occ, _ = w.known_state(truth, 3, 6, 1.5, 2.5)
    occ = np.ascontiguousarray(occ, dtype=np.float64).reshape(-1)
    gm = fuel_amd.SDFMap(map_size, box[0], box[1], device=0)
    gm.uploadOccupancy(occ)
    nv = gm.nvox
    gm.setLocalBound((0, 0, 0), (nv[0] - 1, nv[1] - 1, nv[2] - 1))
    gm.clearAndInflateLocalMap()
    pm = pr.PathMap.from_device(gm)
    om = fo.OracleMap(map_size, box[0], box[1])
    # a free start; candidate goals all over the box; one problem of every kind the driver must hand back
    rng = np.random.default_rng(11)
    cand = np.array(box[0]) + 0.1 + (np.array(box[1]) - np.array(box[0]) - 0.2) * rng.random((400, 3))
    free = cand[~pm.blocked(cand)]
    cur = free[24]  # near the middle of the known space: goals beyond 5 m exist
    all_out = gm.goal_paths(np.repeat([cur], len(cand), axis=0), cand)
    pick = {}
    for b, s in enumerate(all_out["status"].tolist()):
        pick.setdefault(s, b)
    assert gr.FAR in pick and gr.NO_PATH in pick and (gr.CLOSE in pick or gr.MID in pick), sorted(pick)
    ids = [pick[s] for s in sorted(pick)]
    scen = str(tmp_path / "scen.bin")
    with open(scen, "wb") as f:
        np.array(list(map_size) + list(box[0]) + list(box[1]), dtype=np.float64).tofile(f)
        occ.tofile(f)
        for b in ids:
            np.concatenate([cur, cand[b]]).tofile(f)
    res, err = _facade_run(scen)
    assert len(res) == len(ids)
    case = dict(starts=np.repeat([cur], len(ids), axis=0), goals=cand[ids], cfg={})
    out, ref = _assert_case(gm, pm, om, case, tag="facade")
    for k, b in enumerate(ids):
        got = res[k]
        assert got["branch"] == out["status"][k] == all_out["status"][b]
        assert got["n"] == out["n_way"][k] == len(got["way"])
        assert _bits(got["next_goal"]) == _bits(out["next_goal"][k])
        assert _bits(np.array(got["way"]).reshape(-1, 3)) == _bits(out["way"][k])
        if got["branch"] == gr.NO_PATH:  # a value, and nothing to index
            assert got["n"] == 0 and "no path" in err
        else:
            assert got["n"] >= 1
    gm.close()
