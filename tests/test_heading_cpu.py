"""HeadingPlanner's information gain and yaw search without a GPU: the restatement (tests/heading_ref.py) against the
recordings of the reference's own heading_planner.cpp / raycast.cpp (tests/golden/heading, made by
tests/golden/make_heading_golden.py); the layered recurrence against Graph::dijkstraSearch restated literally; the scenes
of tests/heading_cases.py on the edges they are drawn for; the measured tolerance and the decision margins; the kernels'
own text built for the host under sanitizers (tests/golden/check_heading_host_build.py); fuelmi_yawpath_plan, the exported
symbols and every refusal that needs no device."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import heading_cases as hc
import heading_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "heading")
SCENES = hc.all_scenes()
# what tests/golden/make_heading_golden.py cannot give the reference: a subsampling factor other than its constant 4
NOT_RECORDED = tuple(s["tag"] for s in SCENES if s["cfg"]["factor"] != 4)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def _close(a, b, tol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all(np.abs(a - b) <= tol * np.abs(b)))


def test_every_scene_sits_on_its_edge():
    tags = [s["tag"] for s in SCENES]
    assert len(set(tags)) == len(tags) >= 45
    for sc in SCENES:
        r = hc.restate(sc)
        for k, v in sc["expect"].items():
            assert r[k] == v, (sc["tag"], k, r[k], v)
    by = {s["tag"]: s for s in SCENES}
    res = {t: hc.restate(by[t]) for t in tags}
    # an empty map: every candidate is visible; in_box changes nothing when the box is the map
    for t in ("open_1", "open_2", "open_11", "open_cap", "open_pi"):
        assert res[t]["n_cand"] == res[t]["n_visible"] and min(res[t]["n_cand"]) > 0
    assert res["open_1"]["gain"] == res["open_1_nobox"]["gain"]
    assert res["open_pi"]["n_cand"][0] == res["open_pi"]["n_cand"][1]  # +pi and -pi
    assert len(by["open_cap"]["yaws"]) == hr.MAX_YAW
    # shadows, the known-free bubble
    assert 0 < sum(res["wall_11"]["n_visible"]) < sum(res["wall_11"]["n_cand"])
    assert sum(res["bubble_3"]["n_cand"]) < sum(hr.info_gains(hc.spec("wall").ref(), by["bubble_3"]["cfg"], hc.CAM,
                                                              by["bubble_3"]["yaws"])["n_cand"])
    # the exploration box: boundBox clamps the view's box, isInBox cuts cells, ub < lb
    m = hc.spec("inner").ref()
    _, lb, ub = hr.view_setup(m, by["inner_edge"]["cfg"], by["inner_edge"]["pos"], 0.0)
    assert ub[0] == m.box_max[0] and m.pos_to_index((by["inner_edge"]["pos"][0] + 1.4, 0, 0))[0] > ub[0]
    assert sum(res["inner_edge"]["n_cand"]) < sum(res["inner_edge_nobox"]["n_cand"])
    _, lb, ub = hr.view_setup(m, by["inner_empty"]["cfg"], by["inner_empty"]["pos"], 0.0)
    assert ub[0] < lb[0]
    # rays that leave the map below index 0: int() truncates toward zero where floor would leave the map
    sc = by["stripes_below"]
    ms = hc.spec("stripes").ref()
    real_int, seen = int, [0]

    def floor_int(v):
        seen[0] += v < 0
        return math.floor(v)
    hr.int = floor_int  # (ray_blocked's cast, for this one comparison)
    try:
        floored = hr.info_gains(ms, sc["cfg"], sc["pos"], sc["yaws"])
    finally:
        del hr.int
    assert int is real_int and seen[0] > 0 and floored["n_visible"] != res["stripes_below"]["n_visible"]
    # the ballot windows: exactly N candidates
    for n in hc.COUNTS:
        assert res["count_%d" % n]["n_cand"] == [n] and res["count_%d_3" % n]["n_rays"] == n
    # the weights: one control point; the nearest first / last; two equally near, where the first wins
    a, b = res["nu_nearest_first"]["gain"][0], res["nu_nearest_last"]["gain"][0]
    assert b < a and _close(b, a * math.exp(-1.0 * hr.prefix_lengths(by["nu_nearest_last"]["ctrl"])[2]), 1e-12)
    assert res["nu_equal_first_wins"]["gain"][0] == a  # d2 = 0: the copy at index 2 did not win
    assert len(by["nu_one_ctrl"]["ctrl"]) == 1 and res["nu_one_ctrl"]["gain"][0] > 0
    # the layers
    assert sorted({len(s["yaws"]) for s in hc.path_scenes()})[:3] == [1, 2, 3]
    assert {1, 2, 3, 7, hr.MAX_LAYER} <= {len(s["yaws"]) for s in hc.path_scenes()}
    assert {0, 1, 5} <= {s["h"] for s in SCENES if s["kind"] == "path"}
    assert res["layers_2"]["n_rays"] == [0, 0]
    # given gains: the tie goes to the later predecessor; a worse first predecessor is replaced; yr exactly at the rate
    assert res["in_all_equal"]["margin"] == 0.0 and res["in_all_equal"]["path_vertex"] == [0, 4, 4, 0]
    assert res["in_first_worse"]["parent"][2] == [1, 1, 1]
    sc = by["in_at_rate"]
    assert sc["yaw_diff"] / sc["dt"] == sc["max_yaw_rate"] and hr.penal(sc["yaw_diff"], sc["dt"], sc["max_yaw_rate"]) == 0.0
    assert hr.penal(2 * sc["yaw_diff"], sc["dt"], sc["max_yaw_rate"]) > 0.0
    assert res["in_at_rate"]["g_value"] != res["in_over_rate"]["g_value"]
    # the scene at the reference's defaults
    mid = hc.mid_scene()
    assert mid["cfg"]["far"] == 4.5 and mid["h"] == 5 and len(mid["yaws"]) == 7 and hc.spec("mid").nvox == (128, 128, 32)
    assert min(res["mid_defaults"]["n_rays"][1:6]) > 500 and not res["mid_defaults"]["over"]


def test_recurrence_is_the_fifo_search():
    """Graph::dijkstraSearch restated literally (queue, open map, close set) gives the recurrence's labels, parents and
    path on every path scene: all of layer i is popped before any of layer i + 1"""
    for sc in SCENES:
        if sc["kind"] != "path":
            continue
        r = hc.restate(sc)
        layers = hr.layers_of(sc["yaws"], r["gains"], sc["h"], sc["yaw_diff"])
        g, parent, path = hr.search_fifo(layers, sc["dt"], sc["w"], sc["max_yaw_rate"])
        first = np.cumsum([0] + [len(l) for l in layers])
        for i, l in enumerate(layers):
            for j in range(len(l)):
                assert _bits(g[first[i] + j]) == _bits(r["g_value"][i][j]), (sc["tag"], i, j)
                if i:
                    assert parent[first[i] + j] == first[i - 1] + r["parent"][i][j], (sc["tag"], i, j)
        assert path == [first[i] + v for i, v in enumerate(r["path_vertex"])], sc["tag"]


def test_tolerance_and_decision_margins():
    measured, tol = hr.parity_tolerance()
    assert 0.0 < measured < 1e-13 and tol == 100.0 * measured  # a few units in the last place of a sum of <= 1000 terms
    checked = 0
    for sc in SCENES:
        if sc["kind"] == "path" and sc["cfg"]["weight_type"] == hr.NON_UNIFORM and sc["gains_in"] is None and sc["assert_path"]:
            r = hc.restate(sc)
            scale = max(1.0, max(abs(g) for row in r["gains"] for g in row))
            assert r["margin"] >= 1000.0 * tol * scale, (sc["tag"], r["margin"], tol)
            checked += 1
    assert checked >= 3


def test_restatement_equals_the_recorded_reference():
    """UNIFORM gains, n_cand, n_visible, every chosen vertex and the path: equal.  NON_UNIFORM gains: the sum in the
    reference's order equals the recording bit for bit (the same exp, the same order), the sum in the device's order lies
    within the measured tolerance.  g_value: bit for bit on the recorded gains -- pow(x, 2) of the reference's build is
    x * x."""
    names = [s["tag"] for s in SCENES if s["tag"] not in NOT_RECORDED]
    missing = [n for n in names if not os.path.exists(os.path.join(GOLDEN, n + ".npz"))]
    if missing:
        pytest.skip("tests/golden/heading has no recording of %s: run tests/golden/make_heading_golden.py (it needs the "
                    "reference's sources)" % ", ".join(missing[:4]))
    assert len(names) >= 35
    tol = hr.parity_tolerance()[1]
    for sc in SCENES:
        if sc["tag"] in NOT_RECORDED:
            continue
        z = np.load(os.path.join(GOLDEN, sc["tag"] + ".npz"))
        ro, rd = hc.restate(sc, "reference"), hc.restate(sc, "device")
        if sc["kind"] == "gain":
            assert list(z["n_cand"]) == rd["n_cand"] and list(z["n_visible"]) == rd["n_visible"], sc["tag"]
            assert _bits(z["gain"]) == _bits(ro["gain"]), (sc["tag"], z["gain"], ro["gain"])
            if sc["cfg"]["weight_type"] == hr.UNIFORM:
                assert _bits(z["gain"]) == _bits(rd["gain"]), sc["tag"]
            else:
                assert _close(rd["gain"], z["gain"], tol), sc["tag"]
            continue
        L, nv = len(sc["yaws"]), 2 * sc["h"] + 1
        gains = z["gains"]
        if sc["gains_in"] is None:
            assert _bits(gains) == _bits(ro["gains"]), sc["tag"]
            assert _close(rd["gains"], gains, tol), sc["tag"]
            assert _bits(z["search_path_of_yaw"]) == _bits(z["path"]), sc["tag"]  # searchPathOfYaw itself
        # the recurrence on the recorded gains
        s = hr.search(hr.layers_of(sc["yaws"], gains, sc["h"], sc["yaw_diff"]), sc["dt"], sc["w"], sc["max_yaw_rate"])
        flat = [g for row in s["g_value"] for g in row]
        assert _bits(z["g_value"]) == _bits(flat), sc["tag"]
        first = np.cumsum([0] + [len(row) for row in s["g_value"]])
        assert list(z["path_ids"]) == [first[i] + v for i, v in enumerate(s["path_vertex"])], sc["tag"]
        assert _bits(z["path"]) == _bits(s["path"]), sc["tag"]
        # ... and the restatement's own gains choose the same vertices
        assert rd["path_vertex"] == s["path_vertex"] and _bits(rd["path"]) == _bits(z["path"]), sc["tag"]


def test_host_build_of_the_kernels():
    """the two kernels' own text and the host's view setup, built for the host under the address and undefined-behaviour
    sanitizers as a stand-alone program, on every scene: bit for bit the restatement"""
    script = os.path.join(ROOT, "tests", "golden", "check_heading_host_build.py")
    p = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "identical" in p.stdout and "DIFFERS" not in p.stdout and "FAILED" not in p.stdout


def test_plan_call_and_symbols():
    import fuel_amd
    L = fuel_amd.lib()
    for name in ("fuelmi_map_info_gains", "fuelmi_map_yaw_paths", "fuelmi_yawpath_plan"):
        assert getattr(L, name)
    p = fuel_amd.yawpath_plan()
    assert p["lanes"] == 256 and p["groups_per_workgroup"] == 1 and p["search_lanes"] == 64
    assert (p["max_cells"], p["max_yaw"], p["max_ctrl"], p["max_layer"]) == (hr.MAX_CELLS, hr.MAX_YAW, hr.MAX_CTRL, hr.MAX_LAYER)
    assert p["max_cells"] % 64 == 0
    big = fuel_amd.yawpath_plan(fuel_amd.yawpath_cfg(max_ctrl=hr.MAX_CTRL))
    assert big["lds_bytes"] == hr.MAX_CELLS * 12 + 4 * hr.MAX_CTRL * 8 + 16 <= 160 * 1024  # weights, masks, control points
    uni = fuel_amd.yawpath_plan(fuel_amd.yawpath_cfg(weight_type=hr.UNIFORM))
    assert uni["lds_bytes"] == hr.MAX_CELLS * 4 + 16
    out = (C.c_int * 10)()
    EINVAL, ELIMIT = -1, -5
    cfg = fuel_amd.yawpath_cfg
    for over in (dict(half_vert_num=16), dict(max_layer=hr.MAX_LAYER + 1), dict(max_ctrl=hr.MAX_CTRL + 1)):
        assert L.fuelmi_yawpath_plan(C.byref(cfg(**over)), out) == ELIMIT, over
    for bad in (dict(half_vert_num=-1), dict(max_layer=0), dict(w=float("nan")), dict(yaw_diff=float("inf")),
                dict(weight_type=2), dict(factor=0), dict(far=0.0), dict(far=float("nan")), dict(lambda1=float("inf")),
                dict(max_ctrl=0)):
        assert L.fuelmi_yawpath_plan(C.byref(cfg(**bad)), out) == EINVAL, bad
    assert L.fuelmi_yawpath_plan(None, out) == EINVAL and L.fuelmi_yawpath_plan(C.byref(cfg()), None) == EINVAL


def test_refusals_that_need_no_device():
    """every FUELMI_EINVAL / FUELMI_ELIMIT of both calls comes before the map is touched: m = NULL"""
    import fuel_amd
    L = fuel_amd.lib()
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731
    EINVAL, ELIMIT = -1, -5
    n, my = 2, 3

    def gains(cfg=None, n_group=n, pos=None, n_yaw=(3, 1), yaws=None, n_path=0, n_ctrl=None, ctrl=None, path_of=None, null=()):
        cfg = cfg if cfg is not None else fuel_amd.gain_cfg(max_yaw=my)
        pos = np.zeros((n, 3)) if pos is None else np.array(pos, dtype=np.float64)
        yaws = np.zeros((n, my)) if yaws is None else np.array(yaws, dtype=np.float64)
        o = dict(status=np.zeros(n, np.int32), gain=np.zeros((n, my)), n_cand=np.zeros((n, my), np.int32),
                 n_visible=np.zeros((n, my), np.int32), n_rays=np.zeros(n, np.int32))
        P = lambda k: None if k in null else (ip(o[k]) if o[k].dtype == np.int32 else dp(o[k]))  # noqa: E731
        return L.fuelmi_map_info_gains(None, None if "cfg" in null else C.byref(cfg), n_group, None if "pos" in null else dp(pos),
                                       ip(np.array(n_yaw, dtype=np.int32)), dp(yaws), n_path, ip(n_ctrl), dp(ctrl), ip(path_of),
                                       P("status"), P("gain"), P("n_cand"), P("n_visible"), P("n_rays"))

    assert gains() == EINVAL and ": m (" in L.fuelmi_last_error().decode()  # everything valid: only the map is missing
    assert gains(n_group=0) == 0
    assert gains(n_group=-1) == EINVAL
    for null in ("cfg", "pos", "status", "gain", "n_cand", "n_visible", "n_rays"):
        assert gains(null=(null,)) == EINVAL and ": m (" not in L.fuelmi_last_error().decode(), null
    for bad in (dict(n_yaw=(4, 1)), dict(n_yaw=(-1, 1)), dict(pos=[[0, 0, 0], [0, np.nan, 0]]), dict(pos=[[1e7, 0, 0], [0, 0, 0]]),
                dict(yaws=[[0, 0, np.inf], [0, 0, 0]])):
        assert gains(**bad) == EINVAL and ": m (" not in L.fuelmi_last_error().decode(), bad
    assert gains(yaws=[[0, 0, 0], [0, np.nan, np.inf]]) == EINVAL and ": m (" in L.fuelmi_last_error().decode()  # past n_yaw
    assert gains(cfg=fuel_amd.gain_cfg(max_yaw=hr.MAX_YAW + 1)) == ELIMIT
    nu = fuel_amd.gain_cfg(max_yaw=my, weight_type=hr.NON_UNIFORM, max_ctrl=2)
    ok = dict(cfg=nu, n_path=1, n_ctrl=np.array([2], np.int32), ctrl=np.zeros((1, 2, 3)), path_of=np.zeros(n, np.int32))
    assert gains(**ok) == EINVAL and ": m (" in L.fuelmi_last_error().decode()
    for bad in (dict(n_path=0), dict(n_ctrl=np.array([3], np.int32)), dict(n_ctrl=np.array([0], np.int32)), dict(ctrl=None),
                dict(path_of=None), dict(path_of=np.array([0, 1], np.int32)), dict(ctrl=np.full((1, 2, 3), np.nan))):
        assert gains(**dict(ok, **bad)) == EINVAL and ": m (" not in L.fuelmi_last_error().decode(), bad

    ml, nv = 4, 3

    def paths(cfg=None, n_prob=n, n_layer=(4, 1), pts=None, yaws=None, dt=(0.5, 0.5), n_ctrl=None, ctrl=None, gin=None, null=()):
        cfg = cfg if cfg is not None else fuel_amd.yawpath_cfg(half_vert_num=1, max_layer=ml, weight_type=hr.UNIFORM)
        pts = np.zeros((n, ml, 3)) if pts is None else np.array(pts, dtype=np.float64)
        yaws = np.zeros((n, ml)) if yaws is None else np.array(yaws, dtype=np.float64)
        o = dict(status=np.zeros(n, np.int32), path=np.zeros((n, ml)), path_vertex=np.zeros((n, ml), np.int32),
                 gains=np.zeros((n, ml, nv)), g_value=np.zeros((n, ml, nv)), n_rays=np.zeros((n, ml), np.int32))
        P = lambda k: None if k in null else (ip(o[k]) if o[k].dtype == np.int32 else dp(o[k]))  # noqa: E731
        return L.fuelmi_map_yaw_paths(None, None if "cfg" in null else C.byref(cfg), n_prob, ip(np.array(n_layer, dtype=np.int32)),
                                      dp(pts), dp(yaws), dp(np.array(dt, dtype=np.float64)), ip(n_ctrl), dp(ctrl), dp(gin),
                                      P("status"), P("path"), P("path_vertex"), P("gains"), P("g_value"), P("n_rays"))

    assert paths() == EINVAL and ": m (" in L.fuelmi_last_error().decode()
    assert paths(n_prob=0) == 0
    for null in ("cfg", "status", "path", "path_vertex", "gains", "g_value", "n_rays"):
        assert paths(null=(null,)) == EINVAL and ": m (" not in L.fuelmi_last_error().decode(), null
    nan_y = np.zeros((n, ml))
    nan_y[0, 2] = np.nan
    for bad in (dict(n_layer=(0, 1)), dict(n_layer=(5, 1)), dict(dt=(0.0, 0.5)), dict(dt=(np.nan, 0.5)), dict(dt=(0.5, -1.0)),
                dict(yaws=nan_y), dict(gin=np.full((n, ml, nv), np.nan))):
        assert paths(**bad) == EINVAL and ": m (" not in L.fuelmi_last_error().decode(), bad
    assert paths(gin=np.zeros((n, ml, nv))) == EINVAL and ": m (" in L.fuelmi_last_error().decode()
    nuc = fuel_amd.yawpath_cfg(half_vert_num=1, max_layer=ml, max_ctrl=2)  # NON_UNIFORM: control points per problem
    assert paths(cfg=nuc) == EINVAL and ": m (" not in L.fuelmi_last_error().decode()
    assert paths(cfg=nuc, n_ctrl=np.array([2, 1], np.int32), ctrl=np.zeros((n, 2, 3))) == EINVAL and \
        ": m (" in L.fuelmi_last_error().decode()
    assert paths(cfg=nuc, gin=np.zeros((n, ml, nv))) == EINVAL and ": m (" in L.fuelmi_last_error().decode()  # no weights needed
    assert paths(cfg=fuel_amd.yawpath_cfg(half_vert_num=16, max_layer=ml)) == ELIMIT
