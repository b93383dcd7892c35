"""fuelmi_map_local_segments / fuelmi_bspline_dev_load_local_segments on the device against the restatement
(tests/localseg_ref.py, product form) on the scenes of tests/localseg_cases.py.

Every output but the control points is compared BIT FOR BIT with the restatement: the call is + - * /, floor and a
correctly rounded f64 square root, compiled without FMA contraction, so there is no tolerance to measure.  The control
points are compared bit for bit with fuelmi_bspline_parameterize fed this call's own points, derivatives and dt, and
within the existing 1e-9 with the oracle's parameterizeToBspline.  Then the recordings of the reference's own code (with
the tolerance tests/test_local_segment_cpu.py measures), the workgroup packing (2 problems per workgroup), batch
independence and reversal, shared and interleaved states, wider strides, the defined failures among good neighbours, the
chain way-points -> local segment -> collision ranges -> topological search -> guide points -> reparameterisation on a
tests/topo_cases.py map, and the batch loader against loadSamples."""
import os
import sys

import numpy as np
import pytest

import collide_ref as cr
import localseg_cases as lc
import localseg_ref as lr
import topo_cases as tcs
import waypoint_traj_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "localseg")
PACK = 2  # problems per workgroup (local_segment.hip LS_WAVES)
SCENES = lc.scenes()
INTS = ("status", "n_steps", "seg_num", "n_points", "n_ctrl")
MAP_SIZE, BMIN, BMAX = (10.0, 8.0, 4.0), (-4.0, -3.0, 0.0), (4.0, 3.0, 2.2)
_REF = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


@pytest.fixture(scope="module")
def gm():
    import fuel_amd
    m = fuel_amd.SDFMap(MAP_SIZE, BMIN, BMAX, device=0)
    yield m
    m.close()


def ref(sc, max_points=None):
    mp = sc["max_points"] if max_points is None else max_points
    if (sc["tag"], mp) not in _REF:
        _REF[sc["tag"], mp] = lr.solve(sc["state"], sc["mode"], sc["start_t"], sc["arg0"], sc["arg1"], max_points=mp)
    return _REF[sc["tag"], mp]


def run(gm, scs, states=None, index=None, max_points=None, **kw):
    """one call for scenes that share their degree and max_points; states / index: the scenes' states given once, each
    scene naming its own"""
    s0 = scs[0]
    assert all(s["degree"] == s0["degree"] and (max_points or s["max_points"] == s0["max_points"]) for s in scs)
    if states is None:
        states, index = [s["state"] for s in scs], list(range(len(scs)))
    return gm.local_segments([st.as_dict() for st in states], [lc.problem(s, i) for s, i in zip(scs, index)],
                             degree=s0["degree"], max_points=max_points or s0["max_points"], **kw)


def parameterize(gm, dt, points, derivs, degree):
    import fuel_amd
    return fuel_amd.NonUniformBspline.parameterizeToBspline(gm, np.array([dt]), points[None], derivs[None], degree)[0]


def assert_same(gm, out, b, r, tag, fit=True):
    mp = out["points"].shape[1]
    degree = out["ctrl"].shape[1] - mp + 1
    for k in INTS:
        assert out[k][b] == r[k], (tag, k, out[k][b], r[k])
    for k in ("segment_len", "duration", "dt"):
        assert _bits(out[k][b]) == _bits(r[k]), (tag, k, out[k][b], r[k])
    assert _bits(out["derivs"][b]) == _bits(r["derivs"]), (tag, "derivs")
    rows = np.array(r["points"], dtype=np.float64).reshape(-1, 3)
    assert len(rows) == min(r["n_points"], mp)
    assert _bits(out["points"][b][:len(rows)]) == _bits(rows), (tag, "points")
    assert not out["points"][b][len(rows):].any(), (tag, "points")  # rows that are not written are zero
    n = int(out["n_ctrl"][b])
    assert not out["ctrl"][b][n:].any(), (tag, "ctrl")
    if r["status"] != lr.OK:
        assert n == 0
    elif fit:  # the fit: fuelmi_bspline_parameterize's bits on this call's own outputs, the oracle within 1e-9
        from oracle import fuel_oracle as fo
        assert n == r["n_points"] + degree - 1
        want = parameterize(gm, out["dt"][b], out["points"][b][:r["n_points"]], out["derivs"][b], degree)
        assert _bits(out["ctrl"][b][:n]) == _bits(want), (tag, "ctrl")
        oracle = fo.spline_parameterize(out["dt"][b], out["points"][b][:r["n_points"]], out["derivs"][b], degree)
        assert np.abs(out["ctrl"][b][:n] - oracle).max() <= 1e-9, (tag, np.abs(out["ctrl"][b][:n] - oracle).max())


# ---- 1. every scene alone -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sc", SCENES, ids=[s["tag"] for s in SCENES])
def test_scene_alone(gm, sc):
    out = run(gm, [sc], allow_limit=True)
    assert out["limit"] == (ref(sc)["status"] == -1)
    assert_same(gm, out, 0, ref(sc), sc["tag"])


# ---- 2. packing, order, shared states, strides --------------------------------------------------------------------------
def test_packed_reversed_shared_and_strided(gm):
    seen = shared_states = 0
    for (degree, mp), scs in lc.groups(SCENES).items():
        whole = run(gm, scs, allow_limit=True)
        for b, sc in enumerate(scs):
            assert_same(gm, whole, b, ref(sc), sc["tag"], fit=False)
        seen += len(scs)
        for count in (1, PACK, PACK + 1):  # one workgroup half full, full, and one problem into the next
            if count <= len(scs):
                part = run(gm, scs[:count], allow_limit=True)
                for b in range(count):
                    for k in whole:
                        if k != "limit":
                            assert part[k][b].tobytes() == whole[k][b].tobytes(), (scs[b]["tag"], count, k)
        rev = run(gm, scs[::-1], allow_limit=True)
        for k in whole:
            if k != "limit":
                assert rev[k][::-1].tobytes() == whole[k].tobytes(), (degree, mp, k)
        # the states once each: several problems on one state, problems on interleaved states, in both orders
        uniq = []
        for sc in scs:
            if not any(sc["state"] is u for u in uniq):
                uniq.append(sc["state"])
        index = [next(i for i, u in enumerate(uniq) if u is sc["state"]) for sc in scs]
        shared_states += len(uniq) < len(scs)
        shared = run(gm, scs, states=uniq, index=index, allow_limit=True)
        order = list(range(len(scs)))[::2] + list(range(len(scs)))[1::2]
        mixed = run(gm, [scs[i] for i in order], states=uniq[::-1], index=[len(uniq) - 1 - index[i] for i in order],
                    allow_limit=True)
        wide = run(gm, scs, allow_limit=True, max_seg=max(len(s["state"].seg_times) for s in scs) + 3,
                   max_ctrl=max([len(s["state"].local_ctrl or []) for s in scs] + [degree + 1]) + 5)
        for k in whole:
            if k != "limit":
                assert shared[k].tobytes() == whole[k].tobytes(), (degree, mp, k)
                assert wide[k].tobytes() == whole[k].tobytes(), (degree, mp, k)
                assert mixed[k].tobytes() == whole[k][order].tobytes(), (degree, mp, k)
    assert seen == len(SCENES) and shared_states >= 1


def test_no_problem(gm):
    out = gm.local_segments([lc.line().as_dict()], [], degree=3, max_points=8)
    assert len(out["status"]) == 0 and not out["limit"]
    out = gm.local_segments([], [], degree=3, max_points=8)
    assert len(out["status"]) == 0


# ---- 3. the fit: several point counts in one call ------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [3, 4, 5])
def test_three_point_counts_in_one_call(gm, degree):
    by = {s["tag"]: s for s in SCENES}
    scs = [dict(by[t], degree=degree) for t in ("points_2", "points_63", "points_65", "exit_step_129", "points_129")]
    for s in scs:
        s["state"] = lc.line(degree=degree)
    out = run(gm, scs)
    assert out["n_points"].tolist() == [2, 63, 65, 29, 129] and out["n_ctrl"].tolist() == [k + degree - 1 for k in (2, 63, 65, 29, 129)]
    for b, sc in enumerate(scs):
        r = lr.solve(sc["state"], sc["mode"], sc["start_t"], sc["arg0"], sc["arg1"], max_points=sc["max_points"])
        assert_same(gm, out, b, r, (sc["tag"], degree))


# ---- 4. the defined failures between good neighbours ---------------------------------------------------------------------
def test_failures_between_good_neighbours(gm):
    by = {s["tag"]: s for s in SCENES}
    tags = ["points_2", "over_max_points", "exit_step_64", "start_at_end", "points_63", "no_local_points", "one_segment",
            "no_local_first", "dt_zero", "one_point", "no_local_deriv", "points_64"]
    scs = [by[t] for t in tags]
    out = run(gm, scs, max_points=64, allow_limit=True)
    assert out["limit"]
    assert out["status"].tolist() == [0, -1, 0, lr.DEGENERATE, 0, lr.NO_LOCAL, 0, lr.NO_LOCAL, lr.DEGENERATE, lr.DEGENERATE,
                                      lr.NO_LOCAL, 0]
    for b, sc in enumerate(scs):
        assert_same(gm, out, b, ref(sc, 64), sc["tag"])
    over = tags.index("over_max_points")
    assert out["n_points"][over] == 65 and out["points"][over].any() and out["derivs"][over].any() and not out["ctrl"][over].any()
    for b in (tags.index("no_local_points"), tags.index("no_local_first"), tags.index("no_local_deriv")):
        for k in out:
            if k not in ("limit", "status"):
                assert not np.any(out[k][b]), (tags[b], k)
    import fuel_amd
    with pytest.raises(fuel_amd.FuelmiError):
        run(gm, scs, max_points=64)
    good = run(gm, [s for s in scs if ref(s, 64)["status"] == 0], max_points=64)  # the same neighbours without the failures
    at = [b for b, s in enumerate(scs) if ref(s, 64)["status"] == 0]
    for k in good:
        if k != "limit":
            assert good[k].tobytes() == out[k][at].tobytes(), k


# ---- 5. the recordings of the reference's own code -----------------------------------------------------------------------
def test_against_the_recorded_reference(gm):
    measured, tol = lc.parity()
    assert 0.0 < tol < 1e-12
    worst = 0.0
    for (degree, mp), scs in lc.groups(lc.recorded_scenes()).items():
        out = run(gm, scs, allow_limit=True)
        for b, sc in enumerate(scs):
            z = np.load(os.path.join(GOLDEN, sc["tag"] + ".npz"))
            assert (int(z["n_points"]), int(z["seg_num"])) == (out["n_points"][b], out["seg_num"][b]), sc["tag"]
            rows = min(int(z["n_points"]), mp)
            d = max(abs(float(z["dt"]) - out["dt"][b]), abs(float(z["duration"]) - out["duration"][b]),
                    float(np.abs(z["derivs"] - out["derivs"][b]).max()),
                    float(np.abs(z["points"][:rows] - out["points"][b][:rows]).max()))
            print("%-24s off the recording by %.3e (allowed %.3e)" % (sc["tag"], d, tol))
            assert d <= tol, (sc["tag"], d, tol)
            worst = max(worst, d)
    print("the device is off the recordings by at most %.3e" % worst)


def device_map(map_size, occ, src, k, res):
    """(the device map over the scene's occupancy, its distance field [nx, ny, nz] as read back)"""
    import fuel_amd
    m = fuel_amd.SDFMap(map_size, device=0)
    assert m.nvox == k.shape
    m.uploadOccupancy(occ)
    m.setLocalBound((0, 0, 0), tuple(v - 1 for v in m.nvox))
    m.clearAndInflateLocalMap()
    m.updateESDF3d()
    h = m.syncHost(inflate=True, distance=True)
    assert np.array_equal(h["inflate"].reshape(m.nvox) == 1, src)
    dist = h["distance"].reshape(m.nvox)
    want = res * np.sqrt(k.astype(np.float64))
    assert np.all(np.abs(dist - want) <= 2 * np.spacing(want.astype(np.float32)).astype(np.float64))
    return m, dist


# ---- 6. the chain of guided replanning -----------------------------------------------------------------------------------
def test_chain_of_guided_replanning():
    """waypoint_trajs(coef=True) -> SPHERE at start_t = 0 (planGlobalTraj's call) -> collision_ranges on the returned
    control points -> topo_paths -> guide_points -> one DURATION batch over the guide paths' dt: the point count that
    guide_points restates now meets the function it was restated from"""
    import topo_ref as tpr
    sc = tcs.scenes()["pillar"]
    k = tcs.squared_distance(tcs.sources(sc["blocks"]))
    gm, dist = device_map(tcs.MAP_SIZE, tcs.occupancy(sc["blocks"]), tcs.sources(sc["blocks"]), k, tcs.RES)
    ways = [(-2.5, 0.0, 0.0), (0.0, 0.0, 0.0), (2.5, 0.0, 0.0)]
    wp = gm.waypoint_trajs([ways], [(0.0, 0.0, 0.0)], [(0.0, 0.0, 0.0)], coef=True)
    assert wp["status"][0] == wr.OK
    state = dict(seg_times=wp["seg_times"][0], coef=wp["coef"][0], global_duration=float(wp["duration"][0]))
    st = lr.State(state["seg_times"], state["coef"], state["global_duration"])
    seg = gm.local_segments([state], [(0, lr.SPHERE, 0.0, 100.0, 0.5)], max_points=64)
    want = lr.solve(st, lr.SPHERE, 0.0, 100.0, 0.5, max_points=64)
    assert_same(gm, seg, 0, want, "chain sphere")
    assert seg["status"][0] == lr.OK and _bits(seg["duration"][0]) == _bits(wp["duration"][0])  # the whole trajectory
    n = int(seg["n_ctrl"][0])
    ctrl, dt, duration = seg["ctrl"][0][:n], float(seg["dt"][0]), float(seg["duration"][0])
    clearance = sc["cfg"]["clearance"]
    col = gm.collision_ranges([ctrl], [dt], clearance=clearance)
    cw = cr.collision_ranges(cr.Field(tcs.ORIGIN, tcs.RES, dist, "cut", gm.info.resolution_inv), ctrl, 3, dt, clearance, 8, 64)
    assert col["status"][0] == cw["status"] == cr.OK
    for key in ("n_ticks", "n_start_events", "n_end_events", "n_start_pts", "n_end_pts"):
        assert col[key][0] == cw[key], key
    assert _bits(col["t_s"][0]) == _bits(cw["t_s"]) and _bits(col["t_e"][0]) == _bits(cw["t_e"])
    nsp, nep = int(col["n_start_pts"][0]), int(col["n_end_pts"][0])
    cfg = {key: v for key, v in sc["cfg"].items() if key != "max_sample_num"}
    got = gm.topo_paths(col["first_start"], col["last_end"], [sc["samples"]], [col["start_pts"][0][:nsp]],
                        [col["end_pts"][0][:nep]], **cfg)
    assert got["status"][0] == tpr.OK and len(got["sel"][0]) >= 1
    gp = gm.guide_points(got["sel"][0], [duration] * len(got["sel"][0]))
    assert not gp["status"].any()
    re = gm.local_segments([state], [(0, lr.DURATION, 0.0, duration, float(d)) for d in gp["dt"]], max_points=64)
    assert not re["status"].any()
    assert re["n_points"].tolist() == gp["n_pts"].tolist() and re["n_ctrl"].tolist() == gp["n_ctrl"].tolist()
    for b, d in enumerate(gp["dt"]):
        assert_same(gm, re, b, lr.solve(st, lr.DURATION, 0.0, duration, float(d), max_points=64), "chain duration %d" % b)
    gm.close()


# ---- 7. the batch loader --------------------------------------------------------------------------------------------------
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


def test_load_local_segments_equals_load_samples(gm):
    nv = gm.nvox
    gm.setLocalBound((0, 0, 0), (nv[0] - 1, nv[1] - 1, nv[2] - 1))
    gm.clearAndInflateLocalMap()
    gm.updateESDF3d()
    C, N = 6, 14
    K = N - 2
    plans = [wr.plan(w, (0.2, 0.0, 0.0), (0.0, 0.0, 0.0), 2.0, 0.45, form="structured") for w in
             ([(-1.5, -1.0, 1.0), (0.0, 0.5, 1.2), (1.0, -0.5, 1.0), (1.5, 1.0, 1.3)],
              [(1.0, 1.0, 0.8), (0.0, 0.0, 1.0), (-1.0, 0.8, 1.4)])]
    base = [lr.State(p["seg_times"], p["coef"], p["duration"]) for p in plans]
    states = [base[0], lc.with_local(base[1], ts=0.4, te=0.9, span=0.125)]
    sd = [s.as_dict() for s in states]

    def points(dt, count=K):  # a duration that gives `count` points
        return (count - 1) * dt + dt / 2
    problems = [(0, lr.DURATION, 0.0, points(0.1), 0.1), (1, lr.DURATION, 0.1, points(0.07), 0.07),
                (0, lr.DURATION, 0.5, points(0.12), 0.12), (1, lr.DURATION, 0.0, points(0.09), 0.09),
                (0, lr.DURATION, 0.2, points(0.05), 0.05), (1, lr.DURATION, 0.3, points(0.1), 0.1)]
    dev = _batch(gm, C, N)
    status, duration = dev.load_local_segments(sd, problems)
    assert not status.any()
    chain = _state(dev)
    host = gm.local_segments(sd, problems, max_points=K)
    assert host["n_points"].tolist() == [K] * C and _bits(host["duration"]) == _bits(duration)
    dev2 = _batch(gm, C, N)
    dev2.loadSamples(host["dt"], host["points"], host["derivs"])
    assert _state(dev2) == chain
    # candidate 1 (one point fewer than the batch holds), 3 (one more) and 4 (no local trajectory where the segment
    # ends) keep the state they had; the others are reloaded
    problems2 = [(1, lr.DURATION, 0.2, points(0.08), 0.08), (0, lr.DURATION, 0.0, points(0.1, K - 1), 0.1),
                 (1, lr.DURATION, 0.0, points(0.11), 0.11), (0, lr.DURATION, 0.0, points(0.1, K + 1), 0.1),
                 (0, lr.DURATION, states[0].global_duration - 0.2, points(0.1), 0.1), (0, lr.DURATION, 0.3, points(0.06), 0.06)]
    dev3 = _batch(gm, C, N)
    dev3.load_local_segments(sd, problems)
    status2, duration2 = dev3.load_local_segments(sd, problems2)
    assert status2.tolist() == [0, lr.MISFIT, 0, lr.MISFIT, lr.NO_LOCAL, 0]
    mixed = [problems[b] if b in (1, 3, 4) else problems2[b] for b in range(C)]
    host2 = gm.local_segments(sd, mixed, max_points=K)
    assert not host2["status"].any()
    dev4 = _batch(gm, C, N)
    dev4.loadSamples(host2["dt"], host2["points"], host2["derivs"])
    assert _state(dev3) == _state(dev4)
    for d in (dev, dev2, dev3, dev4):
        d.close()
