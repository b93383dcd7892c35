"""fuelmi_map_waypoint_trajs / fuelmi_bspline_dev_load_waypoints on the device against the restatement
(tests/waypoint_traj_ref.py).

Bit for bit against the dense restatement: status, seg_times, duration, seg_num, dt given seg_num, n_samples.
Coefficients, samples, derivatives and length: within 100 x the dense-vs-structured disagreement the restatement
measures on the same tours (waypoint_traj_ref.parity_tolerance; tests/test_waypoint_traj_cpu.py prints it), tours
whose shortest segment takes >= 0.2 s.  Shorter segments: the invariants of the fit, within 100 x the structured
restatement's own residuals.  Then the edges, batching, the device chain into the spline fit, way-points straight from
goal_paths, and the facade's planThroughWaypoints."""
import os
import subprocess
import sys

import numpy as np
import pytest

import goal_path_ref as gr
import path_cost_ref as pr
import waypoint_traj_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

MAP_SIZE, BMIN, BMAX = (10.0, 8.0, 4.0), (-4.0, -3.0, 0.0), (4.0, 3.0, 2.2)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


@pytest.fixture(scope="module")
def gm():
    import fuel_amd
    m = fuel_amd.SDFMap(MAP_SIZE, BMIN, BMAX, device=0)
    yield m
    m.close()


def _one(gm, p, **kw):
    cfg = dict(p["cfg"], **kw)
    return gm.waypoint_trajs([p["way"]], [p["vel"]], [p["acc"]], **cfg)


def _assert_exact(out, b, r, tag="", counts=True):
    """the discrete results and the left-to-right sums, every bit (counts=False: a tour with a segment shorter than
    0.2 s, where the dense inverses' own noise reaches the length: seg_num and n_samples only have to be consistent)"""
    w = (tag, b)
    assert out["status"][b] == r["status"], (w, out["status"][b], r["status"])
    assert _bits(out["duration"][b]) == _bits(r["duration"]), (w, out["duration"][b], r["duration"])
    if counts:
        assert out["n_samples"][b] == r["n_samples"], (w, out["n_samples"][b], r["n_samples"])
        assert out["seg_num"][b] == r["seg_num"], (w, out["seg_num"][b], r["seg_num"])
        assert _bits(out["dt"][b]) == _bits(r["dt"]), (w, out["dt"][b], r["dt"])
    else:
        assert out["n_samples"][b] == out["seg_num"][b] + 1 >= 9, w
    if r["status"] in (wr.OK, wr.OVER):
        assert _bits(out["dt"][b]) == _bits(out["duration"][b] / float(out["seg_num"][b])), w
        assert _bits(out["seg_times"][b]) == _bits(r["seg_times"]), (w, out["seg_times"][b], r["seg_times"])
        assert len(out["samples"][b]) == out["n_samples"][b], w


def _as_result(out, b):
    return {k: out[k][b] for k in ("seg_times", "coef", "samples", "derivs", "length")}


def _assert_close(out, b, r, tol, tag=""):
    d = wr.disagreement(r, _as_result(out, b))
    print("parity %s: device vs dense %s, tolerance %s" % (tag, d, tol))
    for k in d:
        assert d[k] <= tol[k], (tag, b, k, d[k], tol[k])


def _assert_residuals(p, out, b, bound, tag=""):
    res = wr.joint_residuals(p["way"], p["vel"], p["acc"], out["seg_times"][b], out["coef"][b])
    print("residuals %s: device %s, bound %s" % (tag, res, bound))
    for k, v in res.items():
        assert v <= bound[k], (tag, b, k, v, bound[k])


def _assert_seg_num_safe(r, p):
    q = r["length"] / p["cfg"]["ctrl_pt_dist"]
    assert abs(q - round(q)) > 1e-6, (q, "length / ctrl_pt_dist too close to an integer for an exact seg_num")


# ---- 1. parity with the dense formulation ----------------------------------------------------------------------------
def test_parity_with_dense(gm):
    measured, tol = wr.parity_tolerance()
    print("dense vs structured on the parity tours: %s -> tolerance %s" % (measured, tol))
    for i, p in enumerate(wr.parity_cases()):
        r = wr.solve(p, "dense")
        assert r["status"] == wr.OK and min(r["seg_times"]) >= 0.2
        _assert_seg_num_safe(r, p)
        out = _one(gm, p, max_samples=256)
        _assert_exact(out, 0, r, "parity %d" % i)
        _assert_close(out, 0, r, tol, "%d (%d way-points)" % (i, len(p["way"])))


# ---- 2. short segments: the invariants ---------------------------------------------------------------------------------
def test_short_segments_keep_the_invariants(gm):
    measured, bound = wr.residual_bound()
    print("structured restatement's residuals on the short tours: %s -> bound %s" % (measured, bound))
    for i, p in enumerate(wr.short_cases()):
        r = wr.solve(p, "structured")
        assert r["status"] == wr.OK and min(r["seg_times"]) < 0.02
        out = _one(gm, p, max_samples=2048)
        assert out["status"][0] == wr.OK
        assert _bits(out["seg_times"][0]) == _bits(r["seg_times"])
        assert _bits(out["duration"][0]) == _bits(r["duration"])
        assert _bits(out["dt"][0]) == _bits(out["duration"][0] / float(out["seg_num"][0]))
        assert out["n_samples"][0] == out["seg_num"][0] + 1
        _assert_residuals(p, out, 0, bound, "short %d" % i)
    # ... and the parity tours keep them as well
    for i, p in enumerate(wr.parity_cases()[:6]):
        out = _one(gm, p, max_samples=256)
        _assert_residuals(p, out, 0, bound, "parity %d" % i)


# ---- 3. edges ------------------------------------------------------------------------------------------------------------
def test_few_and_degenerate(gm):
    two = wr.problem(70, 2, 0.5, 1.0)
    one = dict(two, way=two["way"][:1])
    for p in (two, one):
        out = _one(gm, p, max_way_points=8)
        assert out["status"][0] == wr.FEW == gm.WPTRAJ_FEW
        for k in ("duration", "length", "dt", "derivs"):
            assert not np.any(out[k][0]), k
        assert out["n_samples"][0] == 0 and out["seg_num"][0] == 0 and len(out["samples"][0]) == 0
    for i, p in enumerate(wr.zero_cases()):
        r = wr.solve(p, "dense")
        assert r["status"] == wr.DEGENERATE == gm.WPTRAJ_DEGENERATE
        out = _one(gm, p)
        _assert_exact(out, 0, r, "zero %d" % i)
        for k in ("duration", "length", "dt", "derivs"):
            assert not np.any(out[k][0]), k
        assert len(out["samples"][0]) == 0
    # three points: one interior way-point, a 2 x 2 system
    p = wr.parity_cases()[0]
    assert len(p["way"]) == 3
    assert _one(gm, p)["status"][0] == wr.OK


def test_way_point_cap(gm):
    import fuel_amd
    p = wr.parity_cases()[-1]
    assert len(p["way"]) == wr.MAX_WAY == gm.waypoint_traj_plan(wr.MAX_WAY)[2]
    out = _one(gm, p, max_samples=256)
    assert out["status"][0] == wr.OK and len(out["coef"][0]) == wr.MAX_WAY - 1
    over = wr.problem(71, wr.MAX_WAY + 1, 0.21, 0.4)
    with pytest.raises(fuel_amd.FuelmiError):
        _one(gm, over)
    with pytest.raises(fuel_amd.FuelmiError):  # more points than the stride
        _one(gm, wr.parity_cases()[3], max_way_points=7)


def test_host_checks(gm):
    import fuel_amd
    p = wr.parity_cases()[2]
    for kw in (dict(max_vel=0.0), dict(max_vel=float("inf")), dict(ctrl_pt_dist=0.0), dict(ctrl_pt_dist=float("nan")),
               dict(min_seg=0), dict(seg_num=-1), dict(max_samples=0)):
        with pytest.raises(fuel_amd.FuelmiError):
            _one(gm, p, **kw)
    for key, val in (("way", float("nan")), ("way", 1e7), ("vel", float("inf")), ("acc", -1e7)):
        q = dict(p, **{key: np.array(p[key], copy=True)})
        q[key].reshape(-1)[1] = val
        with pytest.raises(fuel_amd.FuelmiError):
            _one(gm, q)
    far = dict(p, way=np.array([[0.0, 0, 0], [9e6, 0, 0], [0.0, 9e6, 0]]))  # longer than FUELMI_WPTRAJ_MAX_DURATION
    with pytest.raises(fuel_amd.FuelmiError):
        _one(gm, far)
    out = gm.waypoint_trajs([], np.zeros((0, 3)), np.zeros((0, 3)))
    assert len(out["status"]) == 0


def test_sample_cap_and_forced_seg_num(gm):
    import fuel_amd
    ps = [wr.parity_cases()[k] for k in (3, 4, 1)]
    ways, vels, accs = [p["way"] for p in ps], [p["vel"] for p in ps], [p["acc"] for p in ps]
    full = gm.waypoint_trajs(ways, vels, accs, max_samples=64, **wr.DEFAULTS)
    counts = full["n_samples"].tolist()
    assert counts == [wr.solve(p)["n_samples"] for p in ps] and counts[1] == max(counts) > counts[0]
    with pytest.raises(fuel_amd.FuelmiError):
        gm.waypoint_trajs(ways, vels, accs, max_samples=counts[1] - 1, **wr.DEFAULTS)
    cut = gm.waypoint_trajs(ways, vels, accs, max_samples=counts[1] - 1, allow_limit=True, **wr.DEFAULTS)
    assert cut["limit"] and cut["status"].tolist() == [0, -1, 0] and cut["n_samples"].tolist() == counts
    assert _bits(cut["samples"][1]) == _bits(full["samples"][1][:counts[1] - 1])
    for k in ("duration", "length", "dt", "derivs"):
        assert _bits(cut[k]) == _bits(full[k]), k
    for b in (0, 2):
        assert _bits(cut["samples"][b]) == _bits(full["samples"][b])
    for b in range(3):
        assert _bits(cut["coef"][b]) == _bits(full["coef"][b])
    # a forced seg_num: seg_num + 1 samples whatever the length
    p = ps[0]
    r = wr.solve(p, "dense", seg_num=20)
    out = _one(gm, p, seg_num=20)
    assert r["n_samples"] == 21
    _assert_exact(out, 0, r, "forced")
    _assert_close(out, 0, r, wr.parity_tolerance()[1], "forced seg_num")


def test_batches_equal_single_problems(gm):
    probs = wr.mixed_batch(300)
    kw = dict(wr.DEFAULTS, max_way_points=40, max_samples=160)
    ways, vels, accs = [p["way"] for p in probs], [p["vel"] for p in probs], [p["acc"] for p in probs]
    out = gm.waypoint_trajs(ways, vels, accs, **kw)
    seen = set(out["status"].tolist())
    assert seen == {wr.OK, wr.FEW, wr.DEGENERATE}, seen
    for b, p in enumerate(probs):
        alone = gm.waypoint_trajs([p["way"]], [p["vel"]], [p["acc"]], **kw)
        for k in ("status", "n_samples", "seg_num", "duration", "length", "dt", "derivs"):
            assert alone[k][0].tobytes() == out[k][b].tobytes(), (b, k)
        for k in ("samples", "seg_times", "coef"):
            assert _bits(alone[k][0]) == _bits(out[k][b]), (b, k)
    # one problem, and the same problems in another order
    assert gm.waypoint_trajs(ways[:1], vels[:1], accs[:1], **kw)["length"][0] == out["length"][0]
    rev = gm.waypoint_trajs(ways[::-1], vels[::-1], accs[::-1], **kw)
    assert _bits(rev["length"][::-1]) == _bits(out["length"])
    for b in range(0, 300, 37):
        r = wr.solve(probs[b], "dense")
        if r["status"] == wr.OK:
            _assert_seg_num_safe(r, probs[b])
        _assert_exact(out, b, r, "batch")


# ---- 4. the device chain into the spline fit -------------------------------------------------------------------------
def _batch(gm, C, N=14):
    import fuel_amd
    rng = np.random.default_rng(9)
    ctrl = np.array(BMIN) + 0.5 + (np.array(BMAX) - np.array(BMIN) - 1.0) * rng.random((C, N, 3))
    x = np.concatenate([ctrl.reshape(C, 3 * N), np.full((C, 1), 0.2)], axis=1)
    cf = fuel_amd.NORMAL_PHASE | fuel_amd.MINTIME
    opt = fuel_amd.BsplineOptimizer()
    opt.setEnvironment(gm)
    prob = fuel_amd.BsplineBatchProblem(x, N, cf, np.full(C, 0.3), rng.normal(size=(C, 3, 3)), rng.normal(size=(C, 3, 3)),
                                        3, 3, 0.2)
    return opt.deviceProblem(prob)


def _state(dev, max_eval=25):
    dev.eval()
    cost, grad = dev.download()
    x, c, ev = dev.optimize(max_eval=max_eval)
    return cost.tobytes(), grad.tobytes(), x.tobytes(), c.tobytes(), ev.tobytes()


def _in_box(p):
    """a tour moved into the map's box (the solve's variables are clipped to it)"""
    w = p["way"] - p["way"].mean(axis=0)
    w = w / max(1.0, np.abs(w).max() / 1.2) + np.array([0.0, 0.0, 1.1])
    return dict(p, way=w)


def test_load_waypoints_equals_load_samples(gm):
    nv = gm.nvox
    gm.setLocalBound((0, 0, 0), (nv[0] - 1, nv[1] - 1, nv[2] - 1))
    gm.clearAndInflateLocalMap()
    gm.updateESDF3d()
    C, N = 6, 14
    seg = N - 3
    ps = [_in_box(wr.problem(300 + i, n, 0.3, 0.9)) for i, n in enumerate((3, 4, 5, 6, 8, 11))]
    ways, vels, accs = [p["way"] for p in ps], [p["vel"] for p in ps], [p["acc"] for p in ps]
    dev = _batch(gm, C, N)
    status, duration = dev.load_waypoints(ways, vels, accs, **wr.DEFAULTS)
    assert not status.any()
    chain = _state(dev)
    host = gm.waypoint_trajs(ways, vels, accs, seg_num=seg, max_samples=seg + 1, **wr.DEFAULTS)
    assert host["n_samples"].tolist() == [seg + 1] * C and _bits(host["duration"]) == _bits(duration)
    dev2 = _batch(gm, C, N)
    dev2.loadSamples(host["dt"], np.array(host["samples"]), host["derivs"])
    assert _state(dev2) == chain
    # candidates 1 (two points) and 4 (a zero-length segment) keep the state they had; the others are reloaded
    ps2 = [_in_box(wr.problem(320 + i, n, 0.3, 0.9)) for i, n in enumerate((4, 2, 5, 7, 6, 3))]
    ps2[4]["way"][3] = ps2[4]["way"][2]
    ways2, vels2, accs2 = [p["way"] for p in ps2], [p["vel"] for p in ps2], [p["acc"] for p in ps2]
    dev3 = _batch(gm, C, N)
    dev3.load_waypoints(ways, vels, accs, **wr.DEFAULTS)
    status2, duration2 = dev3.load_waypoints(ways2, vels2, accs2, max_way_points=12, **wr.DEFAULTS)
    assert status2.tolist() == [0, wr.FEW, 0, 0, wr.DEGENERATE, 0] and duration2[1] == 0.0 == duration2[4]
    mixed_w = [ways[b] if b in (1, 4) else ways2[b] for b in range(C)]
    mixed_v = [vels[b] if b in (1, 4) else vels2[b] for b in range(C)]
    mixed_a = [accs[b] if b in (1, 4) else accs2[b] for b in range(C)]
    host2 = gm.waypoint_trajs(mixed_w, mixed_v, mixed_a, seg_num=seg, max_samples=seg + 1, **wr.DEFAULTS)
    dev4 = _batch(gm, C, N)
    dev4.loadSamples(host2["dt"], np.array(host2["samples"]), host2["derivs"])
    assert _state(dev3) == _state(dev4)
    import fuel_amd
    with pytest.raises(fuel_amd.FuelmiError):  # a seg_num the batch cannot hold
        wc = fuel_amd._lib.WptrajCfg(2.0, 0.45, 8, seg + 1, 12, 1)
        import ctypes as C_
        n_way = np.array([len(w) for w in ways], dtype=np.int32)
        way = np.zeros((C, 12, 3))
        st = np.zeros(C, dtype=np.int32)
        fuel_amd._lib.check(dev.L.fuelmi_bspline_dev_load_waypoints(
            dev.h, C_.byref(wc), n_way.ctypes.data_as(C_.POINTER(C_.c_int)), way.ctypes.data_as(C_.POINTER(C_.c_double)),
            way.ctypes.data_as(C_.POINTER(C_.c_double)), way.ctypes.data_as(C_.POINTER(C_.c_double)),
            st.ctypes.data_as(C_.POINTER(C_.c_int)), None))
    for d in (dev, dev2, dev3, dev4):
        d.close()


# ---- 5. way-points straight from goal_paths ---------------------------------------------------------------------------
def test_goal_path_scenes(gm):
    import fuel_amd
    om, pm, size, box, case = gr.door_scene()
    dm = fuel_amd.SDFMap(size, box[0], box[1], device=0)
    dm.uploadOccupancy(np.array(om.occ, dtype=np.float64))
    nv = dm.nvox
    dm.setLocalBound((0, 0, 0), (nv[0] - 1, nv[1] - 1, nv[2] - 1))
    dm.clearAndInflateLocalMap()
    gp = dm.goal_paths(case["starts"], case["goals"], **dict(gr.DEFAULTS, **case.get("cfg", {})))
    pick = [b for b in range(len(gp["status"])) if gp["status"][b] in (gr.CLOSE, gr.FAR)]
    assert {int(gp["status"][b]) for b in pick} == {gr.CLOSE, gr.FAR}
    rng = np.random.default_rng(4)
    ways = [gp["way"][b] for b in pick]
    vels, accs = rng.normal(scale=0.5, size=(len(pick), 3)), rng.normal(scale=0.3, size=(len(pick), 3))
    out = dm.waypoint_trajs(ways, vels, accs, max_way_points=64, max_samples=512, **wr.DEFAULTS)
    probs = [dict(way=ways[i], vel=vels[i], acc=accs[i], cfg=dict(wr.DEFAULTS)) for i in range(len(pick))]
    dense = [wr.solve(p, "dense") for p in probs]
    long_enough = [i for i, r in enumerate(dense) if r["status"] == wr.OK and min(r["seg_times"]) >= 0.2]
    worst = dict(wr.parity_tolerance()[0])
    for i in long_enough:
        d = wr.disagreement(dense[i], wr.solve(probs[i], "structured"))
        worst = {k: max(worst[k], d[k]) for k in worst}
    tol = {k: 100.0 * v for k, v in worst.items()}
    bound = wr.residual_bound()[1]
    assert len(long_enough) >= 4
    for i, (p, r) in enumerate(zip(probs, dense)):
        assert r["status"] == (wr.OK if len(p["way"]) >= 3 else wr.FEW), (i, r["status"])  # ({p, p} is shortened to {p})
        if r["status"] != wr.OK:
            assert out["status"][i] == r["status"] and out["n_samples"][i] == 0
            continue
        _assert_exact(out, i, r, "door %d" % pick[i], counts=i in long_enough)
        if i in long_enough:
            _assert_seg_num_safe(r, p)
            _assert_close(out, i, r, tol, "door %d" % pick[i])
        else:
            _assert_residuals(p, out, i, bound, "door %d" % pick[i])
    dm.close()


# ---- 6. the facade -------------------------------------------------------------------------------------------------------
def _facade_run(scen):
    exe = os.path.join(ROOT, "fuel_amd", "facade", "facade_wptraj")
    p = subprocess.run([exe, scen], check=True, capture_output=True, text=True, timeout=300)
    res, empty = {}, None
    for line in p.stdout.splitlines():
        f = line.split()
        if not f:
            continue
        if f[0] == "empty":
            empty = int(f[1])
        elif f[0] == "goal":
            res[int(f[1])] = dict(branch=int(f[2]), way=[], init=[], ctrl=[])
        elif f[0] == "traj":
            res[int(f[1])].update(status=int(f[2]), rows=int(f[3]), dt0=float(f[4]), dt1=float(f[5]), cost=float(f[6]))
        elif f[0] in ("way", "init", "ctrl"):
            res[int(f[1])][f[0]].append([float(v) for v in f[2:5]])
    return res, empty


def test_facade_plan_through_waypoints(tmp_path):
    """FrontierFinder::planPathToViewpoint then BsplineOptimizer::planThroughWaypoints (the facade's driver) against the
    Python route goal_paths -> waypoint_trajs -> parameterizeToBspline -> getBoundaryStates(2, 0) -> optimize on the same
    map: the spline handed to the solve within the parity tolerance, the final cost within the 0.1 % the optimiser tests
    allow between two routes of the same solve (tests/test_gpu_parity.py)."""
    import fuel_amd
    from fuel_amd import synth
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
    gm.updateESDF3d()
    pm = pr.PathMap.from_device(gm)
    rng = np.random.default_rng(11)
    cand = np.array(box[0]) + 0.1 + (np.array(box[1]) - np.array(box[0]) - 0.2) * rng.random((400, 3))
    cur = cand[~pm.blocked(cand)][24]
    all_out = gm.goal_paths(np.repeat([cur], len(cand), axis=0), cand)
    pick = {}
    for b, s in enumerate(all_out["status"].tolist()):
        if s in (gr.CLOSE, gr.FAR) and all_out["n_way"][b] >= 3:
            pick.setdefault(s, b)
    assert gr.FAR in pick and gr.CLOSE in pick, sorted(pick)
    ids = [pick[gr.CLOSE], pick[gr.FAR]]
    vel, acc = np.array([0.4, -0.2, 0.05]), np.array([0.1, 0.3, -0.1])
    scen = str(tmp_path / "scen.bin")
    with open(scen, "wb") as f:
        np.array(list(map_size) + list(box[0]) + list(box[1]), dtype=np.float64).tofile(f)
        occ.tofile(f)
        for b in ids:
            np.concatenate([cur, cand[b], vel, acc]).tofile(f)
    res, empty = _facade_run(scen)
    assert empty == wr.FEW and len(res) == len(ids)
    tol = wr.parity_tolerance()[1]["samples"]
    cf = fuel_amd.NORMAL_PHASE | fuel_amd.MINTIME
    opt = fuel_amd.BsplineOptimizer()
    opt.setEnvironment(gm)
    for k, b in enumerate(ids):
        got = res[k]
        way = all_out["way"][b]
        assert got["branch"] == all_out["status"][b] and _bits(np.array(got["way"])) == _bits(way)
        assert got["status"] == wr.OK
        t = gm.waypoint_trajs([way], [vel], [acc], max_samples=256, **wr.DEFAULTS)
        assert t["status"][0] == wr.OK
        ctrl = fuel_amd.NonUniformBspline.parameterizeToBspline(gm, t["dt"], np.array(t["samples"]), t["derivs"], 3)
        assert got["rows"] == ctrl.shape[1] == t["n_samples"][0] + 2
        assert abs(got["dt0"] - t["dt"][0]) <= tol and np.abs(np.array(got["init"]) - ctrl[0]).max() <= tol
        st, en = fuel_amd.NonUniformBspline.getBoundaryStates(gm, ctrl, t["dt"], 3, 2, 0)
        en3 = np.zeros((1, 3, 3))
        en3[0, 0] = en[0, 0]
        n = ctrl.shape[1]
        ptd = np.linalg.norm(np.diff(ctrl[0], axis=0), axis=1).sum() / n
        x = np.concatenate([ctrl[0].reshape(-1), t["dt"]])[None, :]
        pb = fuel_amd.BsplineBatchProblem(x, n, cf, np.array([ptd]), st, en3, 1, 3, t["dt"])
        xs, cs, ev = opt.optimize(pb, max_eval=100)
        print("facade %d: final cost %.9g, python route %.9g" % (k, got["cost"], cs[0]))
        assert abs(got["cost"] - cs[0]) <= 1e-3 * abs(cs[0]), (got["cost"], cs[0])
        assert len(got["ctrl"]) == n and got["dt1"] > 0.0
    gm.close()
