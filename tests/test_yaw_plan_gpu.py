"""fuelmi_map_plan_yaws / fuelmi_bspline_dev_plan_yaws on the device against the restatement (tests/yaw_plan_ref.py).

Bit- or integer-equal to the restatement: status, duration, seg_num, dt_yaw, n_waypt (everything the accumulated knots
decide), and the way-points where the case says so (exact pi, stalls).  Way-points, control points and cost: within
yaw_plan_ref.parity_tolerance() of the DENSE restatement (100 x the larger of the dense-vs-banded disagreement and the
effect of 6 ulp of atan2; tests/test_yaw_plan_cpu.py prints it).  Optimality is checked apart from the restatement, by
the oracle's gradient and by the cost the iterative solve reaches.  Then batching, the device chain behind
_dev_optimize and the facade."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import yaw_plan_ref as yr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

MAP_SIZE, BMIN, BMAX = (10.0, 8.0, 4.0), (-4.0, -3.0, 0.0), (4.0, 3.0, 2.2)
OUT_KEYS = ("status", "duration", "seg_num", "dt_yaw", "yaw_ctrl", "n_waypt", "waypts", "end_yaw", "cost", "yawdot_ctrl",
            "yawddot_ctrl")
_REF = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def ref(pr, form="dense"):
    """the restatement of one problem, computed once"""
    key = (id(pr), form)
    if key not in _REF:
        _REF[key] = (pr, yr.solve(pr, form))
    return _REF[key][1]


@pytest.fixture(scope="module")
def gm():
    import fuel_amd
    m = fuel_amd.SDFMap(MAP_SIZE, BMIN, BMAX, device=0)
    yield m
    m.close()


def run(gm, prs, **kw):
    """one call for problems that share their configuration"""
    p0 = prs[0]
    cfg = dict(mode=p0["mode"], pos_degree=p0["degree"], seg_num=p0["seg_num"], lookfwd=p0["lookfwd"],
               relax_time=p0["relax_time"], forward_t=p0["forward_t"], dt_target=p0["dt_target"], end_back=p0["end_back"],
               max_seg=p0["max_seg"])
    cfg.update(kw)
    return gm.plan_yaws([p["ctrl"] for p in prs], [p["dt"] for p in prs], [p["start"] for p in prs],
                        [p["end"] for p in prs], weights=p0["weights"], **cfg)


def assert_exact(out, b, r, tag=""):
    assert out["status"][b] == r["status"], (tag, out["status"][b], r["status"])
    assert _bits(out["duration"][b]) == _bits(r["duration"]), (tag, out["duration"][b], r["duration"])
    assert out["seg_num"][b] == r["seg_num"], (tag, out["seg_num"][b], r["seg_num"])
    assert _bits(out["dt_yaw"][b]) == _bits(r["dt_yaw"]), (tag, out["dt_yaw"][b], r["dt_yaw"])
    if r["status"] != yr.OVER:
        assert out["n_waypt"][b] == r["n_waypt"], (tag, out["n_waypt"][b], r["n_waypt"])


def assert_close(out, b, r, tol, tag=""):
    N, nw = r["seg_num"] + 3, r["n_waypt"]
    d = {"waypts": float(np.abs(out["waypts"][b, :nw] - np.array(r["waypts"])).max()) if nw else 0.0,
         "yaw_ctrl": float(np.abs(out["yaw_ctrl"][b, :N] - r["yaw_ctrl"]).max()),
         "cost": abs(out["cost"][b] - r["cost"]),
         "end_yaw": abs(out["end_yaw"][b] - r["end_yaw"])}
    print("parity %s: device vs dense %s, tolerance %s" % (tag, d, tol))
    for k in ("waypts", "yaw_ctrl", "cost"):
        assert d[k] <= tol[k], (tag, b, k, d[k], tol[k])
    assert d["end_yaw"] <= tol["waypts"], (tag, d["end_yaw"])
    # the derivative control points are the control points' differences over dt_yaw (a few ulp of them)
    p, dt = r["degree_yaw"], r["dt_yaw"]
    d1, d2 = yr.derivative_ctrl(out["yaw_ctrl"][b, :N], p, dt)
    assert np.abs(out["yawdot_ctrl"][b, :N - 1] - d1).max() <= 8 * 2.0 ** -52 * max(np.abs(d1).max(), 1.0), tag
    assert np.abs(out["yawddot_ctrl"][b, :N - 2] - d2).max() <= 32 * 2.0 ** -52 * max(np.abs(d2).max(), np.abs(d1).max() / dt, 1.0), tag
    assert not out["yaw_ctrl"][b, N:].any() and not out["waypts"][b, nw:].any(), tag


PARITY = yr.parity_cases()
FOLLOW = yr.follow_cases()
EDGE = yr.edge_cases()


# ---- 1. parity, EXPLORE ----------------------------------------------------------------------------------------------
def test_parity_explore(gm):
    tol = yr.parity_tolerance()[1]
    for pr in PARITY:
        assert yr.parity_ok(pr), pr["tag"]
        out = run(gm, [pr])
        r = ref(pr)
        assert r["status"] == yr.OK
        assert_exact(out, 0, r, pr["tag"])
        assert_close(out, 0, r, tol, pr["tag"])


# ---- 2. accumulated knots --------------------------------------------------------------------------------------------
def test_accumulated_knots(gm):
    pr = yr.problem(yr.curve(40, 31), 0.1, (0.3, 0.0, 0.0), 1.0)
    out = run(gm, [pr])
    want = float.fromhex("0x1.d99999999999ep+1")
    assert _bits(out["duration"][0]) == _bits(want) and out["duration"][0] != 3.7, out["duration"][0].hex()
    assert _bits(out["dt_yaw"][0]) == _bits(want / 12.0)
    assert_exact(out, 0, ref(pr), "n40")
    for n, seg in ((9, 2), (18, 6)):
        pf = yr.problem(yr.curve(n, 30 + n), 0.1, (0.1, 0.0, 0.0), mode=yr.FOLLOW)
        o = run(gm, [pf])
        assert o["seg_num"][0] == seg and o["n_waypt"][0] == seg, (n, o["seg_num"][0])
        assert_exact(o, 0, ref(pf), "follow n%d" % n)
        assert_close(o, 0, ref(pf), yr.follow_tolerance()[1], "follow n%d" % n)


# ---- 3. unwrap -------------------------------------------------------------------------------------------------------
def test_unwrap(gm):
    tol = yr.parity_tolerance()[1]
    outs = {k: run(gm, [EDGE[k]]) for k in ("spiral", "start_7", "start_m7", "end_plus", "end_minus", "line_mx")}
    for k, o in outs.items():
        assert_exact(o, 0, ref(EDGE[k]), k)
        assert_close(o, 0, ref(EDGE[k]), tol, k)
    w = outs["spiral"]["waypts"][0, :11]
    assert outs["spiral"]["n_waypt"][0] == 11 and w[-1] > 1.5 * math.pi and np.all(np.diff(w) > 0.0)
    assert np.abs(np.diff(w)).max() < 1.0  # no +-2 pi jump between neighbours
    # the wrap loops: the start state of the fit is the wrapped yaw
    for k, s0 in (("start_7", 7.0 - 2 * math.pi), ("start_m7", -7.0 + 2 * math.pi)):
        q = outs[k]["yaw_ctrl"][0]
        assert abs((q[0] + 4 * q[1] + q[2]) / 6.0 - s0) < 0.05, (k, q[:3])  # (a soft constraint; 7.0 is 6.28 away)
    assert _bits(outs["end_plus"]["end_yaw"][0]) == _bits(math.pi + (-3.0 - math.pi) + 2 * math.pi)
    assert abs(outs["end_minus"]["end_yaw"][0] - (3.5 - 2 * math.pi)) <= tol["waypts"]
    # straight along -x from yaw 0: atan2(+0, -x) is pi exactly, diff == pi takes the <= branch
    assert _bits(outs["line_mx"]["waypts"][0, :11]) == _bits([math.pi] * 11)


# ---- 4. stalls and odd geometry ---------------------------------------------------------------------------------------
def test_stall_and_odd_geometry(gm):
    tol = yr.parity_tolerance()[1]
    for k in ("stall_late", "stall_all", "climb"):
        o = run(gm, [EDGE[k]])
        r = ref(EDGE[k])
        assert_exact(o, 0, r, k)
        assert_close(o, 0, r, tol, k)
        w = o["waypts"][0, :11]
        if k == "stall_late":
            assert _bits(w[-1]) == _bits(w[-2]) == _bits(w[-3]) and w[0] != w[1]
            stalled = [i for i in range(1, 11) if r["waypts"][i] == r["waypts"][i - 1]]
            assert len(stalled) >= 2 and all(_bits(w[i]) == _bits(w[i - 1]) for i in stalled)
        elif k == "stall_all":
            assert _bits(w) == _bits([0.7] * 11)  # the first way-point stalls: last_yaw, the (wrapped) start yaw
        else:
            assert _bits(w) == _bits([0.0] * 11)  # |pd| = dz > 1e-6, atan2(0, 0) = 0, unwrapped against 2.0


# ---- 5. relax and lookfwd ---------------------------------------------------------------------------------------------
def test_relax_and_lookfwd(gm):
    tol = yr.parity_tolerance()[1]
    base = PARITY[3]
    dur = yr.front(base)["duration"]
    outs = []
    for relax, lookfwd, want in ((0.0, True, 11), (10.5 * dur / 12, True, 1), (dur, True, 0), (dur + 5.0, True, 0),
                                 (0.0, False, 0)):
        pr = dict(base, relax_time=relax, lookfwd=lookfwd)
        o = run(gm, [pr])
        r = yr.solve(pr)
        assert o["n_waypt"][0] == want == r["n_waypt"], (relax, lookfwd, o["n_waypt"][0])
        assert_exact(o, 0, r, "relax %g" % relax)
        assert_close(o, 0, r, tol, "relax %g" % relax)
        outs.append(o)
    for k in OUT_KEYS:
        assert _bits(outs[2][k]) == _bits(outs[4][k]) == _bits(outs[3][k]), k


# ---- 6. degenerate ----------------------------------------------------------------------------------------------------
def test_degenerate_among_neighbours(gm):
    import fuel_amd
    deg = EDGE["degenerate"]
    a, c = dict(PARITY[3], lookfwd=False), dict(PARITY[4], lookfwd=False)
    out = run(gm, [a, deg, c])
    assert list(out["status"]) == [fuel_amd.SDFMap.YAW_OK, fuel_amd.SDFMap.YAW_DEGENERATE, fuel_amd.SDFMap.YAW_OK]
    r = yr.solve(deg)
    assert_exact(out, 1, r, "degenerate")
    assert out["cost"][1] == 0.0 and _bits(out["yaw_ctrl"][1, :15]) == _bits(r["q0"]) and not out["yaw_ctrl"][1].any()
    assert out["end_yaw"][1] == 0.0 and not out["yawdot_ctrl"][1].any()
    for b, pr in ((0, a), (2, c)):
        alone = run(gm, [pr])
        for k in OUT_KEYS:
            assert _bits(out[k][b]) == _bits(alone[k][0]), (b, k)
    # with way-points the degenerate problem still reports them
    dw = dict(deg, lookfwd=True, relax_time=0.0)
    o = run(gm, [dw])
    rw = yr.solve(dw)
    assert o["status"][0] == rw["status"] == yr.DEGENERATE  # (pt_dist_ comes from the initial control points alone)
    assert o["n_waypt"][0] == 11 and np.abs(o["waypts"][0, :11] - rw["waypts"]).max() <= yr.parity_tolerance()[1]["waypts"]


# ---- 7. FOLLOW --------------------------------------------------------------------------------------------------------
def test_follow(gm):
    tol = yr.follow_tolerance()[1]
    one = yr.problem(yr.curve(4, 42), 0.25, (0.2, 0.1, 0.0), mode=yr.FOLLOW, tag="seg1")
    short = yr.problem(yr.curve(4, 43), 0.05, (0.2, 0.1, 0.0), mode=yr.FOLLOW, tag="duration < end_back")
    for pr in FOLLOW + [one, short]:
        o = run(gm, [pr])
        r = ref(pr)
        assert r["status"] == yr.OK
        assert_exact(o, 0, r, pr["tag"])
        assert_close(o, 0, r, tol, pr["tag"])
    o = run(gm, [one])
    assert o["seg_num"][0] == 1 and o["n_waypt"][0] == 1 and not o["yaw_ctrl"][0, 4:].any() and o["yaw_ctrl"][0, :4].all()
    assert ref(FOLLOW[1])["n_waypt"] >= 65 and ref(short)["duration"] < 0.1
    assert {p["degree"] for p in FOLLOW} == {3, 4, 5}


def test_follow_at_and_over_the_segment_limit(gm):
    import fuel_amd
    big = yr.problem(yr.curve(1024, 40, scale=0.01), 0.075, (0.2, 0.0, 0.0), mode=yr.FOLLOW, tag="seg256")
    over = yr.problem(yr.curve(1024, 41, scale=0.01), 0.08, (0.2, 0.0, 0.0), mode=yr.FOLLOW, tag="over")
    rb, ro = ref(big, "banded"), ref(over)
    assert rb["seg_num"] == 256 and ro["status"] == yr.OVER and ro["seg_num"] > 256
    o = run(gm, [big])
    assert_exact(o, 0, rb, "seg256")
    # 259 unknowns: the tolerance recipe on this very problem (dense vs banded, 6 ulp of atan2), nothing from the device
    m, tol = yr.tolerance_for("seg256", [big])
    print("seg256: measured %s" % m)
    assert_close(o, 0, ref(big), tol, "seg256")
    p0, p2 = FOLLOW[0], yr.problem(yr.curve(14, 13), 0.3, (2.0, 0.0, 0.0), mode=yr.FOLLOW)
    with pytest.raises(fuel_amd.FuelmiError, match="error -5"):
        run(gm, [p0, over])
    o = run(gm, [p0, over, p2], allow_limit=True)
    assert o["limit"] and list(o["status"]) == [0, -1, 0]
    assert o["seg_num"][1] == ro["seg_num"] and _bits(o["duration"][1]) == _bits(ro["duration"])
    assert not o["yaw_ctrl"][1].any() and not o["waypts"][1].any()
    for b, pr in ((0, p0), (2, p2)):
        alone = run(gm, [pr])
        for k in OUT_KEYS:
            assert _bits(o[k][b]) == _bits(alone[k][0]), (b, k)


# ---- 8. optimality, independent of the restatement ---------------------------------------------------------------------
def test_optimality_by_the_oracle_and_the_iterative_solve(gm):
    import fuel_amd
    from oracle import fuel_oracle as fo
    om = fo.OracleMap((4.0, 4.0, 2.0), (-1.5, -1.5, 0.0), (1.5, 1.5, 1.5))
    opt = fuel_amd.BsplineOptimizer(**yr.WEIGHTS)
    opt.setEnvironment(gm)
    flags = fuel_amd.SMOOTHNESS | fuel_amd.START | fuel_amd.END | fuel_amd.WAYPOINTS
    for pr in (PARITY[0], PARITY[4], PARITY[6], dict(PARITY[3], lookfwd=False), FOLLOW[0], FOLLOW[2]):
        o = run(gm, [pr])
        r = yr.solve(pr)
        N, nw = r["seg_num"] + 3, r["n_waypt"]
        st, en = np.zeros((3, 3)), np.zeros((3, 3))
        st[:, 0] = r["start"]
        en[0, 0] = o["end_yaw"][0]
        wp = np.zeros((nw, 3))
        wp[:, 0] = o["waypts"][0, :nw]
        args = (N, flags, r["pt_dist"], st, en, r["end_n"], 1, r["dt_yaw"], -1.0, None, wp if nw else None,
                np.array(r["idx"], dtype=np.int32) if nw else None)
        en_r, wp_r = np.zeros((3, 3)), np.zeros((nw, 3))
        en_r[0, 0] = r["end_yaw"]
        wp_r[:, 0] = r["waypts"]
        args_r = args[:4] + (en_r,) + args[5:10] + (wp_r if nw else None,) + args[11:]
        _, g_dev = fo.bspline_cost_grad(om, o["yaw_ctrl"][0, :N], *args)
        _, g_ref = fo.bspline_cost_grad(om, r["yaw_ctrl"], *args_r)
        n_dev, n_ref = float(np.linalg.norm(g_dev)), float(np.linalg.norm(g_ref))
        print("optimality %s: |grad| at the device's result %.3e, at the dense restatement's %.3e" % (pr["tag"], n_dev, n_ref))
        assert n_dev <= 100.0 * n_ref, (pr["tag"], n_dev, n_ref)
        pb = fuel_amd.BsplineBatchProblem(np.array(r["q0"])[None, :], N, flags, np.array([r["pt_dist"]]), st[None], en[None],
                                          r["end_n"], 1, r["dt_yaw"], None, None, wp[None] if nw else None,
                                          np.array(r["idx"], dtype=np.int32)[None] if nw else None)
        _, c_lbfgs, ev = opt.optimize(pb, max_eval=2000)
        print("optimality %s: cost %.12g, iterative solve %.12g after %d evaluations" % (pr["tag"], o["cost"][0], c_lbfgs[0], ev[0]))
        assert o["cost"][0] <= c_lbfgs[0] * (1.0 + 1e-9), (pr["tag"], o["cost"][0], c_lbfgs[0])


# ---- 9. batch independence ----------------------------------------------------------------------------------------------
def test_batch_independence(gm):
    pool = [dict(p, relax_time=1.0) for p in PARITY]
    prs = [pool[1]] + [pool[(3 * i) % len(pool)] for i in range(69)] + [pool[1]]
    out = run(gm, prs)
    assert len(out["status"]) == 71 and not out["status"].any()
    for k in OUT_KEYS:
        assert _bits(out[k][0]) == _bits(out[k][70]), k
    alone = run(gm, [pool[1]], max_ctrl=35)
    for k in OUT_KEYS:
        assert _bits(out[k][0]) == _bits(alone[k][0]), k
    assert out["n_waypt"][0] >= 1 and out["yaw_ctrl"][0, :15].all()


# ---- 10. the device chain ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mintime", [True, False])
def test_device_chain(gm, mintime):
    import fuel_amd
    C, N, dt = 8, 16, 0.31
    rng = np.random.default_rng(17)
    ctrl = helpers.make_trajectories(rng, C, N, np.array(BMIN) + 0.5, np.array(BMAX) - 0.5)
    x, ptd, st, en = helpers.bspline_inputs(ctrl, dt, mintime)
    cf = fuel_amd.SMOOTHNESS | fuel_amd.FEASIBILITY | fuel_amd.START | fuel_amd.END | (fuel_amd.MINTIME if mintime else 0)
    opt = fuel_amd.BsplineOptimizer()
    opt.setEnvironment(gm)
    pb = fuel_amd.BsplineBatchProblem(x, N, cf, ptd, st, en, 3, 3, dt)
    dev = opt.deviceProblem(pb)
    start = np.stack([rng.uniform(-3, 3, C), rng.uniform(-0.3, 0.3, C), rng.uniform(-0.2, 0.2, C)], axis=1)
    end = rng.uniform(-3, 3, C)
    with pytest.raises(fuel_amd.FuelmiError, match="error -1"):
        dev.plan_yaws(start, end, relax_time=0.5)
    xo, co, ev = dev.optimize(max_eval=40)
    got = dev.plan_yaws(start, end, relax_time=0.5)
    pos = xo[:, :3 * N].reshape(C, N, 3)
    knot = xo[:, -1] if mintime else np.full(C, dt)
    if mintime:
        assert np.abs(knot - dt).max() > 0.0  # the knot span really comes from the variables
    want = gm.plan_yaws(list(pos), knot, start, end, relax_time=0.5)
    assert not got["status"].any() and got["n_waypt"].min() >= 1
    for k in OUT_KEYS:
        assert _bits(got[k]) == _bits(want[k]), k
    # FOLLOW through the same chain, without an end yaw
    gf = dev.plan_yaws(start, None, mode=1)
    wf = gm.plan_yaws(list(pos), knot, start, None, mode=1)
    for k in OUT_KEYS:
        assert _bits(gf[k]) == _bits(wf[k]), k
    # a reload invalidates what the last solve left
    K = N - 2
    dev.loadSamples(np.full(C, dt), np.ascontiguousarray(ctrl[:, :K]), np.zeros((C, 4, 3)))
    with pytest.raises(fuel_amd.FuelmiError, match="error -1"):
        dev.plan_yaws(start, end, relax_time=0.5)
    dev.optimize(max_eval=5)
    assert not dev.plan_yaws(start, end, relax_time=0.5)["status"].any()
    dev.close()


def test_device_chain_refuses_other_batches(gm):
    import fuel_amd
    rng = np.random.default_rng(3)
    opt = fuel_amd.BsplineOptimizer()
    opt.setEnvironment(gm)
    N = 15
    x = rng.normal(size=(2, N))
    st, en = np.zeros((2, 3, 3)), np.zeros((2, 3, 3))
    flags = fuel_amd.SMOOTHNESS | fuel_amd.START | fuel_amd.END
    pb = fuel_amd.BsplineBatchProblem(x, N, flags, np.array([0.3, 0.3]), st, en, 2, 1, 0.3)
    dev = opt.deviceProblem(pb)
    dev.optimize(max_eval=5)
    with pytest.raises(fuel_amd.FuelmiError, match="error -1"):  # dim 1
        dev.plan_yaws(np.zeros((2, 3)) + 0.1, np.ones(2))
    dev.close()


# ---- 11. the facade ---------------------------------------------------------------------------------------------------
def test_facade_plan_yaw_explore(tmp_path):
    """facade_yaw: planPathToViewpoint -> planThroughWaypoints -> planYawExplore on the close and the far branch of
    tests/test_waypoint_traj_gpu.py's scene, against SDFMap.plan_yaws on the position spline the driver printed"""
    import fuel_amd
    from fuel_amd import synth
    import goal_path_ref as gr
    import path_cost_ref as pc
    map_size, box = (10.0, 8.0, 4.0), ((-4.0, -3.0, 0.0), (4.0, 3.0, 2.2))
    w = synth.World.for_map_size(map_size)
    truth = w.world(3, 14)
    occ, _ = w.known_state(truth, 3, 6, 1.5, 2.5)
    occ = np.ascontiguousarray(occ, dtype=np.float64).reshape(-1)
    m = fuel_amd.SDFMap(map_size, box[0], box[1], device=0)
    m.uploadOccupancy(occ)
    nv = m.nvox
    m.setLocalBound((0, 0, 0), (nv[0] - 1, nv[1] - 1, nv[2] - 1))
    m.clearAndInflateLocalMap()
    m.updateESDF3d()
    pm = pc.PathMap.from_device(m)
    rng = np.random.default_rng(11)
    cand = np.array(box[0]) + 0.1 + (np.array(box[1]) - np.array(box[0]) - 0.2) * rng.random((400, 3))
    cur = cand[~pm.blocked(cand)][24]
    all_out = m.goal_paths(np.repeat([cur], len(cand), axis=0), cand)
    pick = {}
    for b, s in enumerate(all_out["status"].tolist()):
        if s in (gr.CLOSE, gr.FAR) and all_out["n_way"][b] >= 3:
            pick.setdefault(s, b)
    assert gr.FAR in pick and gr.CLOSE in pick, sorted(pick)
    ids = [pick[gr.CLOSE], pick[gr.FAR]]
    vel, acc = np.array([0.4, -0.2, 0.05]), np.array([0.1, 0.3, -0.1])
    yaws = [((0.4, 0.1, 0.0), 2.0, 1.0), ((-2.8, 0.0, 0.05), 3.0, 0.5)]
    scen = str(tmp_path / "scen.bin")
    with open(scen, "wb") as f:
        np.array(list(map_size) + list(box[0]) + list(box[1]), dtype=np.float64).tofile(f)
        occ.tofile(f)
        for b, (sy, ey, relax) in zip(ids, yaws):
            np.concatenate([cur, cand[b], vel, acc, sy, [ey, relax]]).tofile(f)
    exe = os.path.join(ROOT, "fuel_amd", "facade", "facade_yaw")
    p = subprocess.run([exe, scen], check=True, capture_output=True, text=True, timeout=300)
    res = json.loads(p.stdout[p.stdout.index("{"):])["problems"]
    assert len(res) == 2
    tol = yr.parity_tolerance()[1]
    for got, b, (sy, ey, relax) in zip(res, ids, yaws):
        assert got["branch"] == all_out["status"][b] and got["traj_status"] == 0
        assert got["yaw_status"] == 0 and got["yaw_rows"] == 15 == len(got["yaw_ctrl"])
        o = m.plan_yaws([np.array(got["pos_ctrl"])], [got["pos_dt"]], [sy], [ey], relax_time=relax)
        assert o["status"][0] == 0
        assert abs(got["dt_yaw"] - o["dt_yaw"][0]) <= tol["waypts"]
        assert np.abs(np.array(got["yaw_ctrl"]) - o["yaw_ctrl"][0, :15]).max() <= tol["yaw_ctrl"]
        # statuses are propagated and a refused call leaves the outputs alone
        assert got["hover_status"] == fuel_amd.SDFMap.YAW_DEGENERATE and got["hover_untouched"] == 1
        fo_ = m.plan_yaws([np.array(got["pos_ctrl"])], [got["pos_dt"]], [sy], None, mode=1)
        assert got["follow_status"] == 0 and got["follow_rows"] == fo_["seg_num"][0] + 3
        assert got["follow_path_yaw"] == fo_["n_waypt"][0] and abs(got["follow_dt_yaw"] - fo_["dt_yaw"][0]) <= tol["waypts"]
    m.close()
