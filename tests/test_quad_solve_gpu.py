"""fuelmi_map_solve_quadratic / fuelmi_bspline_dev_solve_quadratic on the device against the restatement
(tests/quad_solve_ref.py), on the scenes of tests/quad_solve_cases.py.

Bit- or integer-equal: status and pt_dist, and every problem of a ragged batch to the same problem alone.  Control points
and cost: within 100 x the disagreement of the band form and the dense form measured on the CPU for that case
(quad_solve_ref.allowance; tests/test_quad_solve_cpu.py prints it), against the DENSE form.  Optimality is checked apart
from the restatement: by the oracle's gradient at the device result and by the cost the iterative solve reaches from the
same start.  Then the yaw planner's own control points, the refusals, and the device batch in front of a NORMAL_PHASE
solve."""
import os
import sys

import numpy as np
import pytest

import quad_solve_cases as qc
import quad_solve_ref as qr
from quad_solve_cases import oracle_cost_grad, pad3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

MAP_SIZE = (10.0, 8.0, 4.0)
_REF, _DEV = {}, {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def ref(pr, form="dense"):
    key = (id(pr), form)
    if key not in _REF:
        _REF[key] = (pr, qr.solve(pr, form))
    return _REF[key][1]


@pytest.fixture(scope="module")
def gm():
    import fuel_amd
    m = fuel_amd.SDFMap(MAP_SIZE, *qr.BOX, device=0)
    yield m
    m.close()


def alone(gm, pr):
    """one problem in a call of its own, computed once"""
    if id(pr) not in _DEV:
        o = gm.solve_quadratic(**qc.call_args([pr]))
        _DEV[id(pr)] = (pr, dict(status=int(o["status"][0]), ctrl=o["ctrl"][0].copy(), cost=float(o["cost"][0]),
                                 pt_dist=float(o["pt_dist"][0]), tail=o["ctrl_out"][0, len(pr["ctrl"]):].copy()))
    return _DEV[id(pr)][1]


# ---- 1. parity with the dense form -----------------------------------------------------------------------------------
def test_numeric_cases_against_the_dense_form(gm):
    """N = 4, 5 (the start and end blocks overlap, one and two jerk rows); N = 2 order and 2 order + 1 at degrees 3, 4, 5
    (no guide point, one); N = 63, 64, 65 (the rows wrap round the wave) and the cap; end_n = 1, 2, 3; way-points at index 0
    and N - 3 and one index twice; dimension 1 with the yaw mask; bounds that hold"""
    bad = []
    for pr in qc.numeric_cases():
        d, r = alone(gm, pr), ref(pr)
        tq, tc = qr.allowance(pr)
        eq, ec = float(np.abs(d["ctrl"] - r["ctrl"]).max()), abs(d["cost"] - r["cost"])
        print("%-24s N %4d status %d  device vs dense: ctrl %.3e (allowed %.3e) cost %.3e (allowed %.3e)" %
              (pr["tag"], len(pr["ctrl"]), d["status"], eq, tq, ec, tc))
        if not (d["status"] == r["status"] == qr.OK and _bits(d["pt_dist"]) == _bits(r["pt_dist"]) and eq <= tq and ec <= tc
                and not d["tail"].any()):
            bad.append(pr["tag"])
    assert not bad, bad


# ---- 2. optimality, apart from the restatement -----------------------------------------------------------------------
def test_oracle_gradient_at_the_device_result(gm):
    from oracle import fuel_oracle as fo
    om = fo.OracleMap(MAP_SIZE, *qr.BOX)
    bad = []
    for pr in qc.numeric_cases():
        d, r = alone(gm, pr), ref(pr)
        g_dev = np.linalg.norm(oracle_cost_grad(om, pr, d["ctrl"], r["pt_dist"])[1])
        g_ref = np.linalg.norm(oracle_cost_grad(om, pr, r["ctrl"], r["pt_dist"])[1])
        print("%-24s oracle |grad|: device %.3e, dense %.3e" % (pr["tag"], g_dev, g_ref))
        if not g_dev <= 100.0 * g_ref:
            bad.append(pr["tag"])
    assert not bad, bad


def iterative(gm, pr, x0, ptd, max_eval):
    """fuelmi_bspline_optimize on one problem of the restatement from x0 -> (x [N, dim], cost)"""
    import fuel_amd
    N, dim, m = len(pr["ctrl"]), pr["dim"], pr["mask"]
    opt = fuel_amd.BsplineOptimizer(**pr["weights"])
    opt.setEnvironment(gm)
    ng = max(qr.n_guide(pr), 1)
    guide = np.zeros((1, ng, 3))
    if (m & qr.GUIDE) and qr.n_guide(pr):
        guide[0, :qr.n_guide(pr)] = pad3(pr["guide"])[:qr.n_guide(pr)]
    nw = len(pr["widx"])
    bp = fuel_amd.BsplineBatchProblem(np.asarray(x0, dtype=np.float64).reshape(1, N * dim), N, m, [ptd], pad3(pr["start"])[None],
                                      pad3(pr["end"])[None], pr["end_n"], dim, [pr["dt"]],
                                      guide_pts=guide if m & qr.GUIDE else None,
                                      waypoints=pad3(pr["waypts"])[None] if nw else None,
                                      waypt_idx=np.array(pr["widx"], dtype=np.int32)[None] if nw else None)
    x, cost, ev = opt.optimize(bp, max_eval=max_eval)
    return x.reshape(N, dim), float(cost[0])


def test_cost_is_not_above_the_iterative_solve(gm):
    """from the same start with 2000 evaluations.  "Except by rounding": both costs are sums of at most 8 N non-negative
    terms of a few operations each, so each carries at most 64 N ulp of itself"""
    import fuel_amd
    bad, refused = [], []
    for pr in qc.numeric_cases():
        d = alone(gm, pr)
        try:
            _, c_it = iterative(gm, pr, pr["ctrl"], d["pt_dist"], 2000)
        except fuel_amd.FuelmiError as e:  # the iterative route has a size limit of its own, below the exact solve's cap
            assert "error -5" in str(e) and "LDS budget of the device optimiser" in str(e), str(e)
            refused.append(pr["tag"])
            continue
        print("%-24s cost: exact %.12g, iterative (2000 evaluations) %.12g" % (pr["tag"], d["cost"], c_it))
        if not d["cost"] <= c_it * (1.0 + 64 * len(pr["ctrl"]) * 2.0 ** -52):
            bad.append(pr["tag"])
    assert not bad, bad
    assert refused == ["n_cap"], refused  # (1024 control points: no iterative solve exists to compare with)


# ---- 3. the yaw planner's own control points -------------------------------------------------------------------------
def test_dim1_yaw_mask_agrees_with_plan_yaws(gm):
    import yaw_plan_ref as yr
    w = dict(ld_smooth=2.0, ld_start=80.0, ld_end=1.5, ld_waypt=0.7)
    start, dt_pos = (0.3, 0.2, -0.1), 0.25
    y = gm.plan_yaws([yr.curve(16, 9)], [dt_pos], [start], [1.2], weights=w, mode=0, seg_num=12, lookfwd=True,
                     relax_time=1.0, forward_t=2.0)
    assert y["status"][0] == 0 and y["n_waypt"][0] >= 3
    seg, nw, dty, e = int(y["seg_num"][0]), int(y["n_waypt"][0]), float(y["dt_yaw"][0]), float(y["end_yaw"][0])
    # planYawExplore's initial control points (planner_manager.cpp:786-789, :850-853): states2pts on the start state and
    # on (end yaw, 0, 0), zeros between
    q0 = np.zeros(seg + 3)
    m02, m12 = (1 / 3.0) * dty * dty, -(1 / 6.0) * dty * dty
    q0[0] = 1.0 * start[0] + (-dty) * start[1] + m02 * start[2]
    q0[1] = 1.0 * start[0] + 0.0 * start[1] + m12 * start[2]
    q0[2] = 1.0 * start[0] + dty * start[1] + m02 * start[2]
    q0[seg:] = e
    pr = qr.problem(q0, dty, qr.YAW_MASK, start, (e, 0.0, 0.0), 2, None, y["waypts"][0, :nw].reshape(-1, 1),
                    list(range(1, 1 + nw)), weights=w, tag="plan_yaws")
    d = alone(gm, pr)
    tq, tc = qr.allowance(pr)
    eq, ec = float(np.abs(d["ctrl"][:, 0] - y["yaw_ctrl"][0, :seg + 3]).max()), abs(d["cost"] - y["cost"][0])
    print("plan_yaws: control points differ by %.3e (allowed %.3e), cost by %.3e (allowed %.3e)" % (eq, tq, ec, tc))
    assert d["status"] == qr.OK and eq <= tq and ec <= tc
    r = ref(pr)
    assert np.abs(d["ctrl"] - r["ctrl"]).max() <= tq and abs(d["cost"] - r["cost"]) <= tc


# ---- 4. a ragged batch -----------------------------------------------------------------------------------------------
def test_ragged_batch_is_bit_equal_to_every_problem_alone(gm):
    prs = qc.ragged_batch()
    assert sorted(len(p["ctrl"]) for p in prs) == [4, 5, 6, 7, 12, 20, 63, 64, 65, 1024]
    o = gm.solve_quadratic(**qc.call_args(prs))
    rev = gm.solve_quadratic(**qc.call_args(prs[::-1]))
    for b, pr in enumerate(prs):
        d = alone(gm, pr)
        for out, k in ((o, b), (rev, len(prs) - 1 - b)):
            assert out["status"][k] == d["status"] == qr.OK, pr["tag"]
            assert _bits(out["ctrl"][k]) == _bits(d["ctrl"]) and _bits(out["cost"][k]) == _bits(d["cost"]), pr["tag"]
            assert _bits(out["pt_dist"][k]) == _bits(d["pt_dist"]), pr["tag"]
            assert not out["ctrl_out"][k, len(pr["ctrl"]):].any(), pr["tag"]
        tq, tc = qr.allowance(pr)
        assert np.abs(d["ctrl"] - ref(pr)["ctrl"]).max() <= tq and abs(d["cost"] - ref(pr)["cost"]) <= tc, pr["tag"]


# ---- 5. the other two statuses ---------------------------------------------------------------------------------------
def test_degenerate(gm):
    for pr in qc.degenerate_cases():
        d, r = alone(gm, pr), ref(pr, "band")
        assert d["status"] == r["status"] == qr.DEGENERATE, pr["tag"]
        assert _bits(d["ctrl"]) == _bits(pr["ctrl"]) and d["cost"] == 0.0 and _bits(d["pt_dist"]) == _bits(r["pt_dist"])
    assert alone(gm, qc.degenerate_cases()[1])["pt_dist"] == 0.0


def test_bounded_returns_q0(gm):
    pr = qc.bounded_case()
    d, r = alone(gm, pr), ref(pr, "band")
    lo, hi = qr.shrunk_box(pr)
    assert d["status"] == r["status"] == qr.BOUNDED
    assert _bits(d["ctrl"]) == _bits(np.clip(pr["ctrl"], lo, hi)) and _bits(d["pt_dist"]) == _bits(r["pt_dist"])
    # the objective at q0: a few dozen terms, each a few operations on the same numbers in the same order
    assert abs(d["cost"] - r["cost"]) <= 64 * len(pr["ctrl"]) * 2.0 ** -52 * r["cost"], (d["cost"], r["cost"])
    free = alone(gm, qc._once("bounded_free", lambda: dict(pr, bounds=False, tag="bounded_free")))
    assert free["status"] == qr.OK and free["ctrl"][:, 0].max() > hi[0] and free["cost"] < d["cost"]


# ---- 6. the refusals, with a map behind them -------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw,rc,piece", qc.refusals(), ids=[r[0] for r in qc.refusals()])
def test_refusals(gm, name, kw, rc, piece):
    import fuel_amd
    with pytest.raises(fuel_amd.FuelmiError) as e:
        gm.solve_quadratic(**kw)
    assert "error %d" % rc in str(e.value) and piece in str(e.value), str(e.value)


def test_no_problem_is_ok(gm):
    assert len(gm.solve_quadratic([], [])["status"]) == 0


# ---- 7. the device batch in front of the next phase ------------------------------------------------------------------
def test_device_batch_then_normal_phase(gm):
    import fuel_amd
    C, N = 3, 14
    prs = [qc.guide_case(N, seed=60 + c, tag="batch%d" % c) for c in range(C)]
    host = gm.solve_quadratic(**qc.call_args(prs))
    ctrl = np.stack([p["ctrl"] for p in prs])
    st, en = np.stack([p["start"] for p in prs]), np.stack([p["end"] for p in prs])
    dts = [p["dt"] for p in prs]
    opt = fuel_amd.BsplineOptimizer(**prs[0]["weights"])
    opt.setEnvironment(gm)
    dev = opt.deviceProblem(fuel_amd.BsplineBatchProblem(ctrl.reshape(C, 3 * N), N, fuel_amd.NORMAL_PHASE,
                                                         [qr.pt_dist(p["ctrl"]) for p in prs], st, en, 3, 3, dts))
    dev.optimize(max_eval=5)  # (sets the flag the call below has to clear)
    o = dev.solve_quadratic(fuel_amd.GUIDE_PHASE, np.stack([p["guide"] for p in prs]))
    assert np.array_equal(o["status"], host["status"]) and not o["status"].any()
    for k in ("ctrl_out", "cost", "pt_dist"):
        assert _bits(o[k]) == _bits(host[k]), k
    with pytest.raises(fuel_amd.FuelmiError):  # the last solve's variables are no longer the batch's
        dev.plan_yaws(np.zeros((C, 3)), np.zeros(C))
    # the next phase starts from the solution, with pt_dist_ of the solution: the host route on the returned points
    x_dev, c_dev, e_dev = dev.optimize(max_eval=40)
    nxt = fuel_amd.BsplineBatchProblem(o["ctrl_out"].reshape(C, 3 * N), N, fuel_amd.NORMAL_PHASE,
                                       [qr.pt_dist(q) for q in o["ctrl_out"]], st, en, 3, 3, dts)
    x_host, c_host, e_host = opt.optimize(nxt, max_eval=40)
    assert np.array_equal(e_dev, e_host) and _bits(x_dev) == _bits(x_host) and _bits(c_dev) == _bits(c_host)
    assert not np.array_equal(x_dev, o["ctrl_out"].reshape(C, 3 * N))  # (it did move)


# ---- 8. the facade ---------------------------------------------------------------------------------------------------
def test_facade_guide_phase_and_closing_yaw_solve(gm, tmp_path):
    """facade_quad: optimizeTopoBspline's first phase for guide paths of different point counts in ONE call
    (BsplineOptimizer::optimizeGuidePhase), the same through optimize() with optimization/exact_quadratic set and without it,
    and planYawActMap's closing solve; the C++ side must return what the Python side gets from the same library"""
    import json
    import subprocess
    prs = [qc.guide_case(n, seed=70 + n, bounds=True, tag="facade_n%d" % n) for n in (9, 14, 6, 31, 14)]
    yaw = qc.yaw_case(13, 8)
    path = tmp_path / "scenario.bin"
    rec = [np.array(MAP_SIZE), np.array(qr.BOX[0]), np.array(qr.BOX[1]), np.array([float(len(prs))])]
    for p in prs:
        rec += [np.array([float(len(p["ctrl"])), p["dt"]]), p["ctrl"].reshape(-1), p["start"].reshape(-1), p["end"].reshape(-1),
                p["guide"].reshape(-1)]
    rec += [np.array([float(len(yaw["ctrl"])), yaw["dt"]]), yaw["ctrl"].reshape(-1), yaw["start"].reshape(-1),
            yaw["end"].reshape(-1)[:2], np.array([float(len(yaw["widx"]))]), np.array(yaw["widx"], dtype=np.float64),
            yaw["waypts"].reshape(-1)]
    np.concatenate(rec).astype(np.float64).tofile(str(path))
    exe = os.path.join(ROOT, "fuel_amd", "facade", "facade_quad")
    p = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    doc = json.loads(p.stdout)
    mine = gm.solve_quadratic(**qc.call_args(prs))
    for b, pr in enumerate(prs):
        got = doc["batch"][b]
        assert got["status"] == mine["status"][b] == qr.OK, pr["tag"]
        assert _bits(np.array(got["ctrl"])) == _bits(mine["ctrl"][b]) and got["cost"] == mine["cost"][b], pr["tag"]
        assert doc["exact"][b]["exact_status"] == qr.OK and doc["exact"][b]["ctrl"] == got["ctrl"], pr["tag"]
        it = doc["iterative"][b]
        assert it["exact_status"] == -1 and it["ctrl"] != got["ctrl"], pr["tag"]
        c_it = qr.combine_cost(pr, np.array(it["ctrl"]), mine["pt_dist"][b])
        print("%-12s cost: exact %.9g, the facade's two evaluations %.9g" % (pr["tag"], got["cost"], c_it))
        assert got["cost"] <= c_it, pr["tag"]
    d = alone(gm, yaw)
    ye, yi = doc["yaw"]["exact"], doc["yaw"]["iterative"]
    assert ye["exact_status"] == qr.OK and _bits(np.array(ye["ctrl"])) == _bits(d["ctrl"])
    assert yi["exact_status"] == -1
    assert d["cost"] <= qr.combine_cost(yaw, np.array(yi["ctrl"]), d["pt_dist"]) * (1.0 + 64 * 13 * 2.0 ** -52)
