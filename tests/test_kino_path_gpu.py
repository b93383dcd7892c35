"""fuelmi_map_kino_paths / fuelmi_bspline_dev_load_kino on the device against the restatement (tests/kino_ref.py, which
tests/test_kino_path_cpu.py pins to the reference's own code): every discrete output exactly -- status, answering
search, iter_num, use_node_num, the path's voxels, inputs and durations, shot flag, seg_num, n_samples -- and every
output that involves no libm bit for bit (the path's states, T_sum and the samples without a shot).  The device's libm
is not glibc's: outputs behind cbrt / acos / cos / pow(., 3) are compared within 100 x the largest disagreement between
the restatement's plain run and its eight runs with every libm result nudged by -4 .. +4 ulp (kino_ref.robustness); the
CPU test asserts that every scene used here keeps its discrete outputs under those nudges, and that the edge scenes reach
their edges (lists of 1 .. 256 primitives, colliding and wrapping tables, a full pool, refused starts and goals, the
sample-count edges of getSamples).  Beside the scenes: one launch with every outcome, calls of changing workspace layout
on one map, the device chain at other degrees and at its smallest batch."""
import faulthandler
import os
import sys

import numpy as np
import pytest

import kino_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

_maps = {}


def _device_map(sc, esdf=False):
    """the device map of a scene; its inflated / unknown voxels must be the restatement's"""
    import fuel_amd
    key = (repr(sc.get("blocks", ())), repr(sc.get("unknown", ())), repr(sc.get("box", kr.BOX)))
    if key not in _maps:
        box = sc.get("box", kr.BOX)
        gm = fuel_amd.SDFMap(kr.MAP_SIZE, box[0], box[1], device=0)
        gm.uploadOccupancy(kr.occupancy(sc.get("blocks", ()), sc.get("unknown", ())))
        nv = gm.nvox
        gm.setLocalBound((0, 0, 0), (nv[0] - 1, nv[1] - 1, nv[2] - 1))
        gm.clearAndInflateLocalMap()
        km, dev = kr.scene_map(sc), kr.KMap.from_device(gm)
        assert np.array_equal(dev.infl, km.infl) and np.array_equal(dev.unk, km.unk)
        assert np.array_equal(dev.box_mind, km.box_mind) and np.array_equal(dev.box_maxd, km.box_maxd)
        assert np.array_equal(dev.origin, km.origin) and np.array_equal(dev.map_size, km.map_size)
        _maps[key] = gm
    if esdf:
        _maps[key].updateESDF3d()
    return _maps[key]


@pytest.fixture(scope="module", autouse=True)
def _close_maps():
    yield
    for gm in _maps.values():
        gm.close()
    _maps.clear()


@pytest.fixture
def time_limit():
    """a search that does not return ends the run (with every thread's stack) instead of holding the device"""
    faulthandler.dump_traceback_later(120, exit=True, file=sys.__stderr__)
    yield
    faulthandler.cancel_dump_traceback_later()


def _fresh_map(sc):
    """a device map of a scene that nothing has been called on (the caller closes it)"""
    import fuel_amd
    box = sc.get("box", kr.BOX)
    gm = fuel_amd.SDFMap(kr.MAP_SIZE, box[0], box[1], device=0)
    gm.uploadOccupancy(kr.occupancy(sc.get("blocks", ()), sc.get("unknown", ())))
    nv = gm.nvox
    gm.setLocalBound((0, 0, 0), (nv[0] - 1, nv[1] - 1, nv[2] - 1))
    gm.clearAndInflateLocalMap()
    return gm


KEYS_I = ("status", "which", "iter_num", "use_node_num", "n_nodes", "shot", "seg_num", "n_samples")
KEYS_D = ("t_shot", "T_sum", "ts", "coef", "derivs", "samples", "node_state", "node_input", "node_duration")


def _assert_same_bits(a, ia, b, ib, where):
    for k in KEYS_I:
        assert a[k][ia] == b[k][ib], (where, k, a[k][ia], b[k][ib])
    for k in KEYS_D:
        assert _bits(a[k][ia]) == _bits(b[k][ib]), (where, k)


def _cfg(sc, **kw):
    c = dict(kr.DEFAULTS)
    c.update(sc.get("cfg", {}))
    c.update(kw)
    return c


def _run(gm, probs, cfg, **kw):
    return gm.kino_paths([p["start"] for p in probs], [p["vel"] for p in probs], [p["acc"] for p in probs],
                         [p["goal"] for p in probs], [p["goal_vel"] for p in probs], **dict(cfg, **kw))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def _assert_problem(out, b, r, worst, tag=""):
    where = (tag, b)
    for k in ("status", "which", "iter_num", "use_node_num", "n_nodes", "shot", "seg_num", "n_samples"):
        assert out[k][b] == r[k], (where, k, out[k][b], r[k])
    nodes = r["nodes"]
    if nodes:
        st = np.array([n["state"] for n in nodes])
        assert _bits(out["node_state"][b]) == _bits(st), (where, "states")
        assert _bits(out["node_input"][b]) == _bits(np.array([n["input"] for n in nodes])), (where, "inputs")
        assert _bits(out["node_duration"][b]) == _bits(np.array([n["duration"] for n in nodes])), (where, "durations")
        org = np.array((-kr.MAP_SIZE[0] / 2.0, -kr.MAP_SIZE[1] / 2.0, kr.GROUND))
        vox = np.floor((out["node_state"][b][:, :3] - org) * (1.0 / 0.1)).astype(int)
        assert np.array_equal(vox, np.array([n["index"] for n in nodes])), (where, "voxels")
    tol = kr.tolerance(worst)
    got = dict(t_shot=out["t_shot"][b], coef=out["coef"][b], T_sum=out["T_sum"][b], ts=out["ts"][b],
               samples=out["samples"][b], derivs=out["derivs"][b])
    for k in kr.CONTINUOUS:
        x, y = np.asarray(got[k], dtype=np.float64), np.asarray(r[k], dtype=np.float64)
        if k == "samples" and r["status"] == kr.OVER and len(y) > len(x):  # over max_samples: the first max_samples are kept
            assert len(x) == len(y) - 1, (where, len(x), len(y))
            y = y[:len(x)]
        assert x.shape == y.shape, (where, k, x.shape, y.shape)
        if x.size == 0:
            continue
        err = float(np.abs(x - y).max())
        print("%s problem %d %s: device vs restatement %.3e, tolerance %.3e" % (tag, b, k, err, tol[k]))
        if tol[k] == 0.0:  # no libm behind it in this problem
            assert _bits(x) == _bits(y), (where, k, err)
        else:
            assert err <= tol[k], (where, k, err, tol[k])
    if not r["shot"]:  # g-derived: no libm
        n = len(out["samples"][b])
        assert _bits(out["T_sum"][b]) == _bits(r["T_sum"]) and _bits(out["samples"][b]) == _bits(r["samples"][:n]), where


# ---- 1. every scene against the restatement --------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(kr.scenes()))
def test_scene(name, time_limit):
    sc = kr.scenes()[name]
    gm = _device_map(sc)
    over = sc.get("over", False)  # a scene over max_samples: the call reports the limit, everything else is compared
    out = _run(gm, sc["probs"], _cfg(sc), allow_limit=over)
    ref = kr.scene_results(name, sc)
    assert len(ref) == len(out["status"]) > 0 and out["limit"] == over
    for b, (r, robust, worst) in enumerate(ref):
        assert robust, (name, b)
        _assert_problem(out, b, r, worst, name)


def test_scenes_hold_what_they_claim():
    """on the device's own answers (the CPU test asserts the same on the restatement)"""
    sc = kr.scenes()
    st = {}
    for name in ("open", "near_start", "pillar_start", "near_end", "horizon", "enclosed", "alloc_at", "alloc_over"):
        o = _run(_device_map(sc[name]), sc[name]["probs"], _cfg(sc[name]))
        st[name] = (int(o["status"][0]), int(o["which"][0]), int(o["n_nodes"][0]), int(o["shot"][0]))
    assert st["open"][0] == kr.REACH_END and st["open"][3] == 1 and st["open"][2] > 2
    assert st["near_start"] == (kr.REACH_END, 0, 1, 1)
    assert st["pillar_start"][:2] == (kr.NO_PATH, 1) and st["enclosed"][:2] == (kr.NO_PATH, 1)
    assert st["near_end"][0] == kr.NEAR_END and st["horizon"][0] == kr.REACH_HORIZON
    assert st["alloc_at"][0] == kr.NO_PATH and st["alloc_over"][0] == kr.REACH_END


# ---- 2. caps and refusals ----------------------------------------------------------------------------------------------
def test_caps():
    import fuel_amd
    sc = kr.scenes()["bookkeeping"]
    gm = _device_map(sc)
    with pytest.raises(fuel_amd.FuelmiError) as e:  # 257 init primitives: refused before anything is launched
        _run(gm, sc["probs"], _cfg(sc, time_res_init=1 / 257.0))
    assert "error -5" in str(e.value)
    assert kr.primitives(_cfg(sc, time_res_init=1 / 257.0)) is None and kr.primitives(_cfg(sc, time_res_init=1 / 256.0))
    _run(gm, sc["probs"], _cfg(sc, time_res_init=1 / 256.0))  # 256 are accepted
    (r, robust, worst), = kr.scene_results("bookkeeping", sc)
    full = _run(gm, sc["probs"], _cfg(sc))
    assert full["n_nodes"][0] == r["n_nodes"] > 2 and full["n_samples"][0] == r["n_samples"]
    two = [sc["probs"][0], kr.scenes()["near_start"]["probs"][0]]
    near = _run(gm, two[1:], _cfg(sc))
    for kw, key in ((dict(max_path_nodes=r["n_nodes"] - 1), "node_state"), (dict(max_samples=r["n_samples"] - 1), "samples")):
        cut = _run(gm, two, _cfg(sc, **kw), allow_limit=True)
        assert cut["limit"] and cut["status"][0] == -1
        assert cut["n_nodes"][0] == r["n_nodes"] and cut["n_samples"][0] == r["n_samples"]
        assert _bits(cut[key][0]) == _bits(full[key][0][:len(cut[key][0])]) and len(cut[key][0]) == len(full[key][0]) - 1
        assert _bits(cut["derivs"][0]) == _bits(full["derivs"][0]) and _bits(cut["T_sum"][0]) == _bits(full["T_sum"][0])
        # the other problem is complete
        assert cut["status"][1] == near["status"][0] == kr.REACH_END
        assert _bits(cut["samples"][1]) == _bits(near["samples"][0])
        with pytest.raises(fuel_amd.FuelmiError):
            _run(gm, two, _cfg(sc, **kw))
    # exactly at the caps: accepted
    fit = _run(gm, sc["probs"], _cfg(sc, max_path_nodes=r["n_nodes"], max_samples=r["n_samples"]))
    assert fit["status"][0] == r["status"] and not fit["limit"]
    # without the node arrays max_path_nodes caps nothing
    bare = _run(gm, sc["probs"], _cfg(sc, max_path_nodes=1), nodes=False)
    assert bare["status"][0] == r["status"] and bare["n_nodes"][0] == r["n_nodes"]
    for bad in (dict(check_num=0), dict(allocate_num=1), dict(max_vel=0.0), dict(ts=float("nan")), dict(horizon=-1.0)):
        with pytest.raises(fuel_amd.FuelmiError) as e:
            _run(gm, sc["probs"], _cfg(sc, **bad))
        assert "error -1" in str(e.value), bad
    with pytest.raises(fuel_amd.FuelmiError):
        _run(gm, [dict(sc["probs"][0], goal=(float("inf"), 0.0, 0.0))], _cfg(sc))
    empty = _run(gm, [], _cfg(sc))
    assert len(empty["status"]) == 0


# ---- 3. a result does not depend on the problem's place in the batch -----------------------------------------------------
def test_batch_invariance():
    sc = kr.scenes()["open"]
    gm = _device_map(sc)
    probs = kr.batch65()
    out = _run(gm, probs, _cfg(sc))
    alone = _run(gm, probs[:1], _cfg(sc))
    ref = kr.problem_results("open", probs)
    _assert_problem(alone, 0, ref[0][0], ref[0][2], "alone")
    # every block of the batch against the restatement (each of its eight distinct problems is checked for robustness
    # by tests/test_kino_path_cpu.py) ...
    for b, (r, robust, worst) in enumerate(ref):
        assert robust, b
        _assert_problem(out, b, r, worst, "batch65")
    # ... and the same problem at another place bit for bit: 0 / 64 / alone, and the seven others nine times over
    keys_i = ("status", "which", "iter_num", "use_node_num", "n_nodes", "shot", "seg_num", "n_samples")
    keys_d = ("t_shot", "T_sum", "ts", "coef", "derivs", "samples", "node_state", "node_input", "node_duration")
    for b in (0, 64):
        assert all(out[k][b] == alone[k][0] for k in keys_i), b
        assert all(_bits(out[k][b]) == _bits(alone[k][0]) for k in keys_d), b
    for b in range(8, 64):
        assert all(out[k][b] == out[k][b - 7] for k in keys_i), b
        assert all(_bits(out[k][b]) == _bits(out[k][b - 7]) for k in keys_d), b
    # and the call leaves nothing behind: the same batch again gives the same bits
    again = _run(gm, probs, _cfg(sc))
    for b in range(65):
        assert _bits(again["samples"][b]) == _bits(out["samples"][b]) and again["use_node_num"][b] == out["use_node_num"][b]


# ---- 3b. one launch with every outcome; calls of another layout on one map ----------------------------------------------
def test_outcome_batch(time_limit):
    """72 problems on the wall map in one launch: REACH_END, NEAR_END, REACH_HORIZON, NO_PATH after the retry, CLOSE_GOAL
    (its workgroup returns before the first barrier) and one problem over max_samples side by side -- each against the
    restatement, and bit for bit what the same problem gives alone"""
    sc = kr.scenes()[kr.OUTCOME_SCENE]
    gm = _device_map(sc)
    cfg = _cfg(sc, **kr.OUTCOME_CFG)
    names, distinct = kr.outcome_problems()
    ref = dict(zip(names, kr.problem_results(kr.OUTCOME_SCENE, distinct, kr.OUTCOME_CFG)))
    bn, probs = kr.outcome_batch()
    assert len(probs) == 72
    out = _run(gm, probs, cfg, allow_limit=True)
    assert out["limit"] and {int(v) for v in out["status"]} == {kr.REACH_END, kr.NEAR_END, kr.REACH_HORIZON, kr.NO_PATH,
                                                                 kr.CLOSE_GOAL, kr.OVER}
    alone = {n: _run(gm, [p], cfg, allow_limit=True) for n, p in zip(names, distinct)}
    assert [n for n in names if alone[n]["limit"]] == ["back"]
    for b, n in enumerate(bn):
        r, robust, worst = ref[n]
        assert robust, n
        _assert_problem(out, b, r, worst, "outcomes/" + n)
        _assert_same_bits(out, b, alone[n], 0, (n, b))


def test_layout_change_between_calls(time_limit):
    """the workspace is laid out anew per call in the map's pool: a call with 4096 nodes a problem, then 70 problems of 16
    nodes (their tables lie where node records were), then a 256-primitive list -- each bit for bit the same call on a
    map nothing else has run on"""
    sc = kr.scenes()["bookkeeping"]
    names, distinct = kr.outcome_problems()
    calls = [(distinct[:3], _cfg(sc, allocate_num=4096)),
             ([dict(distinct[i % 10]) for i in range(70)], _cfg(sc, allocate_num=16)),
             (distinct[:2], _cfg(sc, **dict(kr.REG_LISTS["reg256"][1])))]
    gm = _fresh_map(sc)
    fresh = []
    try:
        seq = [_run(gm, p, c) for p, c in calls]
        for p, c in calls:
            fresh.append(_fresh_map(sc))
            want = _run(fresh[-1], p, c)
            got = seq[len(fresh) - 1]
            assert len(got["status"]) == len(p)
            for b in range(len(p)):
                _assert_same_bits(got, b, want, b, (len(fresh) - 1, b))
        # the calls did what they are here for: paths in the first, every pool of 16 used up or unused in the second
        assert set(seq[0]["status"].tolist()) == {kr.REACH_END, kr.NEAR_END}
        assert set(seq[1]["status"].tolist()) <= {kr.NO_PATH, kr.CLOSE_GOAL, kr.REACH_END}
        assert set(seq[1]["use_node_num"].tolist()) >= {0, 1, 16}
        # and the sequence once more on the same map, in reverse
        for (p, c), want in list(zip(calls, seq))[::-1]:
            again = _run(gm, p, c)
            for b in range(len(p)):
                _assert_same_bits(again, b, want, b, ("again", b))
    finally:
        for m in [gm] + fresh:
            m.close()


# ---- 4. the device chain into the spline fit -----------------------------------------------------------------------------
def _batch(gm, n_cand, N=14, degree=3):
    import fuel_amd
    rng = np.random.default_rng(9)
    lo, hi = np.array(kr.BOX[0]), np.array(kr.BOX[1])
    ctrl = lo + 0.5 + (hi - lo - 1.0) * rng.random((n_cand, N, 3))
    x = np.concatenate([ctrl.reshape(n_cand, 3 * N), np.full((n_cand, 1), 0.2)], axis=1)
    cf = fuel_amd.NORMAL_PHASE | fuel_amd.MINTIME
    opt = fuel_amd.BsplineOptimizer() if degree == 3 else fuel_amd.BsplineOptimizer(bspline_degree=degree)
    opt.setEnvironment(gm)
    prob = fuel_amd.BsplineBatchProblem(x, N, cf, np.full(n_cand, 0.3), rng.normal(size=(n_cand, 3, 3)),
                                        rng.normal(size=(n_cand, 3, 3)), 3, 3, 0.2)
    return opt.deviceProblem(prob)


def _state(dev, max_eval=25):
    dev.eval()
    cost, grad = dev.download()
    x, c, ev = dev.optimize(max_eval=max_eval)
    return cost.tobytes(), grad.tobytes(), x.tobytes(), c.tobytes(), ev.tobytes()


def _cols(probs):
    return [[p[k] for p in probs] for k in ("start", "vel", "acc", "goal", "goal_vel")]


def test_load_kino_equals_load_samples():
    import fuel_amd
    sc = kr.scenes()[kr.LOAD_SCENE]
    gm = _device_map(sc, esdf=True)
    n_cand, N, seg = 4, kr.LOAD_CTRL, kr.LOAD_SEG
    assert seg == N - 3
    pa, pb = kr.load_problems()
    # what the restatement says of both loads (seg_num forced); tests/test_kino_path_cpu.py asserts each problem robust
    ra, rb = (kr.problem_results(kr.LOAD_SCENE, ps, dict(seg_num=seg)) for ps in (pa, pb))
    assert all(robust for _, robust, _ in ra + rb)
    cfg = _cfg(sc)
    load_cfg = {k: v for k, v in cfg.items() if k not in ("seg_num", "max_samples", "max_path_nodes")}
    dev = _batch(gm, n_cand, N)
    status, t_sum = dev.load_kino(*_cols(pa), **load_cfg)
    assert status.tolist() == [r["status"] for r, _, _ in ra]
    chain = _state(dev)
    host = _run(gm, pa, cfg, seg_num=seg, max_samples=seg + 1)
    assert host["n_samples"].tolist() == [seg + 1] * n_cand and _bits(host["T_sum"]) == _bits(t_sum)
    assert host["status"].tolist() == status.tolist()
    for b, (r, _, worst) in enumerate(ra):
        _assert_problem(host, b, r, worst, "load, first")
    dev2 = _batch(gm, n_cand, N)
    dev2.loadSamples(host["ts"], np.array(host["samples"]), host["derivs"])
    assert _state(dev2) == chain
    # candidate 1 finds no path (the shot from its start crosses the wall, twice) and candidate 3 is refused as a close
    # goal: both keep the state they had; the others are reloaded
    dev3 = _batch(gm, n_cand, N)
    dev3.load_kino(*_cols(pa), **load_cfg)
    status2, t_sum2 = dev3.load_kino(*_cols(pb), **load_cfg)
    assert status2.tolist() == [r["status"] for r, _, _ in rb] and t_sum2[1] == 0.0 == t_sum2[3]
    assert (rb[1][0]["status"], rb[3][0]["status"]) == (kr.NO_PATH, kr.CLOSE_GOAL)
    for b, (r, _, worst) in enumerate(rb):
        tol = kr.tolerance(worst)["T_sum"]
        assert abs(t_sum2[b] - r["T_sum"]) <= tol, (b, t_sum2[b], r["T_sum"], tol)
    mixed = [pa[b] if b in (1, 3) else pb[b] for b in range(n_cand)]
    host2 = _run(gm, mixed, cfg, seg_num=seg, max_samples=seg + 1)
    dev4 = _batch(gm, n_cand, N)
    dev4.loadSamples(host2["ts"], np.array(host2["samples"]), host2["derivs"])
    assert _state(dev3) == _state(dev4)
    with pytest.raises(fuel_amd.FuelmiError):  # a seg_num the batch cannot hold
        dev.load_kino(*_cols(pa), **dict(load_cfg, seg_num=seg + 1))
    for d in (dev, dev2, dev3, dev4):
        d.close()


@pytest.mark.parametrize("degree,N", kr.LOAD_SIZES)
def test_load_kino_other_sizes(degree, N, time_limit):
    """degrees 4 and 5, and the smallest batch N = degree + 1 (one segment, two samples): load_kino leaves the state
    kino_paths + loadSamples leave, and the samples it is compared through are the restatement's"""
    import fuel_amd
    sc = kr.scenes()[kr.LOAD_SCENE]
    gm = _device_map(sc, esdf=True)
    seg, n_cand = N - degree, 4
    pa, _ = kr.load_problems()
    ref = kr.problem_results(kr.LOAD_SCENE, pa, dict(seg_num=seg))
    assert all(robust for _, robust, _ in ref) and all(r["n_samples"] == seg + 1 for r, _, _ in ref)
    cfg = _cfg(sc)
    load_cfg = {k: v for k, v in cfg.items() if k not in ("seg_num", "max_samples", "max_path_nodes")}
    dev, dev2 = _batch(gm, n_cand, N, degree), _batch(gm, n_cand, N, degree)
    try:
        status, t_sum = dev.load_kino(*_cols(pa), **load_cfg)
        assert status.tolist() == [r["status"] for r, _, _ in ref]
        host = _run(gm, pa, cfg, seg_num=seg, max_samples=seg + 1)
        assert host["n_samples"].tolist() == [seg + 1] * n_cand and _bits(host["T_sum"]) == _bits(t_sum)
        for b, (r, _, worst) in enumerate(ref):
            _assert_problem(host, b, r, worst, "load, degree %d, N %d" % (degree, N))
        dev2.loadSamples(host["ts"], np.array(host["samples"]), host["derivs"])
        assert _state(dev, max_eval=8) == _state(dev2, max_eval=8)
        with pytest.raises(fuel_amd.FuelmiError):  # a seg_num the batch cannot hold
            dev.load_kino(*_cols(pa), **dict(load_cfg, seg_num=seg + 1))
    finally:
        dev.close()
        dev2.close()


# ---- 5. the facade: a MID problem out of planPathToViewpoint takes planKinodynamic -----------------------------------------
def test_facade_plan_kinodynamic(tmp_path):
    """FrontierFinder::planPathToViewpoint then, on the MID branch, BsplineOptimizer::planKinodynamic (the facade's driver
    facade_kino) against the Python route goal_paths -> kino_paths -> parameterizeToBspline -> getBoundaryStates(2, 0) ->
    optimize on the same map: the search's status and counters and the spline handed to the solve exactly (both routes run
    the same kernels), the final cost within the 0.1 % the optimiser tests allow between two routes of the same solve."""
    import subprocess
    import fuel_amd
    sc = kr.scenes()[kr.FACADE_SCENE]
    gm = _device_map(sc, esdf=True)
    fp = kr.facade_problem()
    (r, robust, worst), = kr.problem_results(kr.FACADE_SCENE, [fp])  # (robust: asserted by tests/test_kino_path_cpu.py too)
    assert robust
    start, goal, vel, acc = (np.array(fp[k], dtype=np.float64) for k in ("start", "goal", "vel", "acc"))
    gp = gm.goal_paths([start], [goal])
    assert gp["status"][0] == fuel_amd.SDFMap.GOAL_MID and _bits(gp["next_goal"][0]) == _bits(goal)
    scen = str(tmp_path / "scen.bin")
    with open(scen, "wb") as f:
        np.array(list(kr.MAP_SIZE) + list(kr.BOX[0]) + list(kr.BOX[1]), dtype=np.float64).tofile(f)
        kr.occupancy(sc["blocks"]).reshape(-1).tofile(f)
        np.concatenate([start, goal, vel, acc]).tofile(f)
    exe = os.path.join(ROOT, "fuel_amd", "facade", "facade_kino")
    p = subprocess.run([exe, scen], check=True, capture_output=True, text=True, timeout=300)
    got = dict(init=[], ctrl=[])
    for line in p.stdout.splitlines():
        f = line.split()
        if f and f[0] == "goal":
            got["branch"] = int(f[2])
        elif f and f[0] == "kino":
            got.update(status=int(f[2]), which=int(f[3]), iter_num=int(f[4]), use_node_num=int(f[5]), rows=int(f[6]),
                       dt0=float(f[7]), dt1=float(f[8]), cost=float(f[9]))
        elif f and f[0] in ("init", "ctrl"):
            got[f[0]].append([float(v) for v in f[2:5]])
    assert got["branch"] == fuel_amd.SDFMap.GOAL_MID and "status" in got, p.stdout[-2000:]
    k = _run(gm, [dict(fp, goal=gp["next_goal"][0])], _cfg(sc))
    _assert_problem(k, 0, r, worst, "facade")
    for key in ("status", "which", "iter_num", "use_node_num"):
        assert got[key] == k[key][0] == r[key], key
    ctrl = fuel_amd.NonUniformBspline.parameterizeToBspline(gm, k["ts"], np.array(k["samples"]), k["derivs"], 3)
    n = ctrl.shape[1]
    assert got["rows"] == n == k["n_samples"][0] + 2
    assert got["dt0"] == k["ts"][0] and _bits(np.array(got["init"])) == _bits(ctrl[0])
    st, en = fuel_amd.NonUniformBspline.getBoundaryStates(gm, ctrl, k["ts"], 3, 2, 0)
    en3 = np.zeros((1, 3, 3))
    en3[0, 0] = en[0, 0]
    ptd = np.linalg.norm(np.diff(ctrl[0], axis=0), axis=1).sum() / n
    x = np.concatenate([ctrl[0].reshape(-1), k["ts"]])[None, :]
    cf = fuel_amd.NORMAL_PHASE | fuel_amd.MINTIME
    opt = fuel_amd.BsplineOptimizer()
    opt.setEnvironment(gm)
    pb = fuel_amd.BsplineBatchProblem(x, n, cf, np.array([ptd]), st, en3, 1, 3, k["ts"])
    xs, cs, ev = opt.optimize(pb, max_eval=100)
    print("facade_kino: final cost %.9g, python route %.9g" % (got["cost"], cs[0]))
    assert abs(got["cost"] - cs[0]) <= 1e-3 * abs(cs[0]), (got["cost"], cs[0])
    assert len(got["ctrl"]) == n and got["dt1"] > 0.0
