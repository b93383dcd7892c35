"""Given knots into the safety check, the sampling and the yaw plan on the device: fuelmi_map_check_trajs_knots,
_sample_trajs_knots, _plan_yaws_knots and, for a device batch, fuelmi_bspline_dev_set_knot_source(FUELMI_KNOTS_ADJUSTED).

  1. every scene of tests/knots_cases.py through each entry against the restatement (tests/knots_ref.py, pinned to the
     reference's class by tests/test_knots_cpu.py);
  2. explicitly accumulated uniform knots through each entry against the existing uniform entry on the same splines: the
     new path tied to the old one with no reference between them;
  3. the host chain: adjust_trajs(REALLOC), its knots_out as they stand into the three entries;
  4. the batch chain, MINTIME and fixed span: solve, adjust, ADJUSTED -- the three batch calls against the entries on the
     x_out / knots_out the host got; another solve or a reload puts the source back to UNIFORM;
  5. a candidate the adjustment marks BADSPLINE among good neighbours.

The safety check and the samples are compared BIT FOR BIT, as are two device results with each other (2, 4, 5) in every
output.  Of the yaw plan against the restatement, the duration, the segments and the way-point count are bit for bit;
what follows atan2 -- way-points, the solve, the cost -- is within knots_ref.yaw_tolerance, the recipe of
tests/test_yaw_plan_gpu.py, because the device's atan2 is not the host's to the last bit."""
import os
import sys

import numpy as np
import pytest

import helpers
import knots_cases as kc
import knots_ref as kr
import traj_adjust_ref as ar
import traj_check_cases as tc
import traj_check_ref as tr
import traj_sample_ref as ts
import yaw_plan_ref as yr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

CHK_INT = ("status", "safe", "n_samples", "hit_index", "end_reason")
CHK_DBL = ("distance", "hit_t", "duration", "hit_pos")
SMP_KEYS = ("status", "pos", "vel", "acc", "jerk", "yaw", "yawdot", "yawddot", "duration", "flight")
YAW_KEYS = ("status", "duration", "seg_num", "dt_yaw", "yaw_ctrl", "n_waypt", "waypts", "end_yaw", "cost", "yawdot_ctrl",
            "yawddot_ctrl")
YAW_START, YAW_END = (0.3, 0.1, 0.0), 1.2
YAW_CTRL = [0.1, 0.25, 0.5, 0.4, 0.2, 0.3, 0.6]  # a uniform yaw spline beside every position spline


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


@pytest.fixture(scope="module")
def env():
    """(the device map "a" with its inflated plane, the restatement's grid on the plane read back from it)"""
    import fuel_amd
    m = tc.spec(kc.MAP)
    gm = fuel_amd.SDFMap(m.map_size, device=0, **m.kw)
    gm.uploadOccupancy(m.occ3.reshape(-1))
    gm.setLocalBound(*helpers.full_box(gm.nvox))
    gm.clearAndInflateLocalMap()
    infl = gm.syncHost(inflate=True)["inflate"].reshape(gm.nvox)
    assert np.array_equal(infl, m.infl3)
    yield gm, m.grid(infl)
    gm.close()


def yaw_cfg(p, mode):
    pr = yr.problem(np.zeros((p + 1, 3)), 1.0, YAW_START, YAW_END, mode=mode, degree=p, relax_time=0.5)
    return dict(mode=mode, pos_degree=p, seg_num=pr["seg_num"], lookfwd=pr["lookfwd"], relax_time=pr["relax_time"],
                forward_t=pr["forward_t"], dt_target=pr["dt_target"], end_back=pr["end_back"], max_seg=40, weights=pr["weights"])


def check_same(out, b, r, tag):
    for k in CHK_INT:
        assert out[k][b] == r[k], (tag, k, out[k][b], r[k])
    for k in CHK_DBL:
        assert _bits(out[k][b]) == _bits(r[k]), (tag, k, out[k][b], r[k])


def sample_same(out, b, r, t, tag, flight0=None):
    nt = len(t)
    assert out["n_t"][b] == nt
    assert out["status"][b, :nt].tolist() == r["status"] and not out["status"][b, nt:].any(), (tag, out["status"][b], r["status"])
    for k in ("pos", "vel", "acc", "jerk", "yaw", "yawdot", "yawddot"):
        assert _bits(out[k][b, :nt]) == _bits(r[k]), (tag, k, np.abs(out[k][b, :nt] - np.array(r[k])).max())
        assert not out[k][b, nt:].any(), (tag, k)
    assert _bits(out["duration"][b]) == _bits(r["duration"]), tag
    if flight0 is not None:
        assert _bits(out["flight"][b]) == _bits(ts.record_windowed(list(flight0), t, r)), (tag, out["flight"][b])


def yaw_same(out, b, r, tol, tag):
    assert out["status"][b] == r["status"], (tag, out["status"][b], r["status"])
    assert _bits(out["duration"][b]) == _bits(r["duration"]), (tag, out["duration"][b], r["duration"])
    assert out["seg_num"][b] == r["seg_num"] and _bits(out["dt_yaw"][b]) == _bits(r["dt_yaw"]), tag
    assert out["n_waypt"][b] == r["n_waypt"], tag
    N, nw = r["seg_num"] + 3, r["n_waypt"]
    d = {"waypts": float(np.abs(out["waypts"][b, :nw] - np.array(r["waypts"])).max()) if nw else 0.0,
         "yaw_ctrl": float(np.abs(out["yaw_ctrl"][b, :N] - r["yaw_ctrl"]).max()),
         "cost": abs(out["cost"][b] - r["cost"]), "end_yaw": abs(out["end_yaw"][b] - r["end_yaw"])}
    print("yaw %s: device vs restatement %s, tolerance %s" % (tag, d, tol))
    for k in ("waypts", "yaw_ctrl", "cost"):
        assert d[k] <= tol[k], (tag, k, d[k], tol[k])
    assert d["end_yaw"] <= tol["waypts"], (tag, d["end_yaw"])
    assert not out["yaw_ctrl"][b, N:].any() and not out["waypts"][b, nw:].any(), tag


_TOL = {}


def yaw_tol():
    if not _TOL:
        cases = [(kc.yaw_problem(sc, mode), sc["u"]) for sc in kc.scenes() for mode in (yr.EXPLORE, yr.FOLLOW)]
        _TOL["t"] = kr.yaw_tolerance(cases)[1]
    return _TOL["t"]


def all_equal(a, b, keys, tag):
    for k in keys:
        if a[k] is None and b[k] is None:
            continue
        assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), (tag, k)


# ---- 1. every scene through each entry ------------------------------------------------------------------------------------
def test_every_scene_check(env):
    gm, grid = env
    seen = 0
    for p, grp in kc.by_degree().items():
        out = gm.check_trajs([sc["ctrl"] for sc in grp], None, [sc["t_now"] for sc in grp], knots=[sc["u"] for sc in grp],
                             degree=p, step=grp[0]["step"], max_radius=grp[0]["max_radius"])
        assert not out["limit"]
        for b, sc in enumerate(grp):
            check_same(out, b, kr.check(grid, sc["ctrl"], p, sc["u"], sc["t_now"], sc["step"], sc["max_radius"]), sc["tag"])
            seen += 1
        for k in CHK_INT + CHK_DBL:  # the first problem again at the end: its place does not matter
            assert _bits(out[k][0]) == _bits(out[k][len(grp) - 1]), (p, k)
    assert seen >= len(kc.scenes()) + 3


@pytest.mark.parametrize("mode", [ts.COMMAND, ts.STATE])
def test_every_scene_sample(env, mode):
    gm, _ = env
    for p, grp in kc.by_degree().items():
        n = len(grp)
        ydt = [float(sc["u"][len(sc["ctrl"])] - sc["u"][p]) / 4.0 for sc in grp]
        flight0 = np.zeros((n, 8)) if mode == ts.COMMAND else None
        out = gm.sample_trajs([sc["ctrl"] for sc in grp], None, [sc["t"] for sc in grp], yaw_ctrl=[YAW_CTRL] * n, yaw_dt=ydt,
                              flight=flight0, knots=[sc["u"] for sc in grp], mode=mode, degree=p, yaw_degree=3)
        for b, sc in enumerate(grp):
            r = kr.sample(mode, sc["ctrl"], p, sc["u"], sc["t"], YAW_CTRL, 3, ydt[b])
            sample_same(out, b, r, sc["t"], sc["tag"], None if flight0 is None else flight0[b])
        for k in SMP_KEYS:
            if out[k] is not None:
                assert _bits(out[k][0]) == _bits(out[k][n - 1]), (p, k)


@pytest.mark.parametrize("mode", [yr.EXPLORE, yr.FOLLOW])
def test_every_scene_yaw(env, mode):
    gm, _ = env
    tol = yaw_tol()
    for p, grp in kc.by_degree().items():
        n = len(grp)
        out = gm.plan_yaws([sc["ctrl"] for sc in grp], None, [YAW_START] * n, [YAW_END] * n, knots=[sc["u"] for sc in grp],
                           **yaw_cfg(p, mode))
        assert not out["limit"]
        for b, sc in enumerate(grp):
            yaw_same(out, b, kr.yaw_solve(kc.yaw_problem(sc, mode), sc["u"]), tol, "%s mode %d" % (sc["tag"], mode))
        for k in YAW_KEYS:
            assert _bits(out[k][0]) == _bits(out[k][n - 1]), (p, k)


# ---- 2. accumulated uniform knots against the uniform entries ---------------------------------------------------------------
def test_uniform_knots_equal_the_uniform_entries(env):
    gm, _ = env
    by_p = {}
    for p, ctrl, dt in kc.uniform_cases():
        by_p.setdefault(p, []).append((ctrl, dt))
    assert len(by_p) == 3
    for p, cases in by_p.items():
        ctrl, dts = [c for c, _ in cases], [d for _, d in cases]
        us = [kr.uniform(len(c), p, d) for c, d in cases]
        n = len(cases)
        now = [0.1 * b for b in range(n)]
        all_equal(gm.check_trajs(ctrl, None, now, knots=us, degree=p), gm.check_trajs(ctrl, dts, now, degree=p),
                  CHK_INT + CHK_DBL, "check p%d" % p)
        t = [np.concatenate([[-0.2, 0.0, d * (len(c) - p) + 1.0], np.arange(70) * d * 0.37]) for c, d in cases]
        for mode in (ts.COMMAND, ts.STATE):
            fl = np.zeros((n, 8)) if mode == ts.COMMAND else None
            kw = dict(yaw_ctrl=[YAW_CTRL] * n, yaw_dt=0.5, flight=fl, mode=mode, degree=p, yaw_degree=3)
            all_equal(gm.sample_trajs(ctrl, None, t, knots=us, **kw), gm.sample_trajs(ctrl, dts, t, **kw), SMP_KEYS,
                      "sample p%d mode %d" % (p, mode))
        for mode in (yr.EXPLORE, yr.FOLLOW):
            cfg = yaw_cfg(p, mode)
            all_equal(gm.plan_yaws(ctrl, None, [YAW_START] * n, [YAW_END] * n, knots=us, **cfg),
                      gm.plan_yaws(ctrl, dts, [YAW_START] * n, [YAW_END] * n, **cfg), YAW_KEYS, "yaw p%d mode %d" % (p, mode))


# ---- 3. the host chain ----------------------------------------------------------------------------------------------------
LIMITS = dict(limit_vel=0.8, limit_acc=0.6)


def test_host_chain_adjust_then_consumers(env):
    gm, grid = env
    p = 3
    ctrl = [kc.flight(n, 300 + n) for n in (9, 16, 31, 12, 61)]
    dts = [0.3, 0.2, 0.1, 0.25, 0.05]
    adj = gm.adjust_trajs(ctrl, dts, ops=ar.REALLOC, degree=p, **LIMITS)
    assert (adj["status"] == ar.OK).all() and adj["iters"].min() >= 1
    rows = list(adj["knots_out"])  # as they stand: the stride's zeros behind a problem's own knots and all
    us = [row[:len(c) + p + 1] for row, c in zip(rows, ctrl)]
    for c, d, u in zip(ctrl, dts, us):
        assert not np.array_equal(u, np.array(kr.uniform(len(c), p, d)))  # the knots really moved
    n = len(ctrl)
    out = gm.check_trajs(ctrl, None, 0.0, knots=rows, degree=p)
    for b in range(n):
        check_same(out, b, kr.check(grid, ctrl[b], p, us[b], 0.0), "chain %d" % b)
    t = [np.concatenate([[-0.1], np.linspace(0.0, float(u[len(c)] - u[p]) + 0.2, 70)]) for c, u in zip(ctrl, us)]
    fl = np.zeros((n, 8))
    out = gm.sample_trajs(ctrl, None, t, flight=fl, knots=rows, degree=p)
    for b in range(n):
        sample_same(out, b, kr.sample(ts.COMMAND, ctrl[b], p, us[b], t[b]), t[b], "chain %d" % b, fl[b])
        assert _bits(out["duration"][b]) == _bits(adj["duration_out"][b])
    for mode in (yr.EXPLORE, yr.FOLLOW):
        prs = [yr.problem(c, 1.0, YAW_START, YAW_END, mode=mode, degree=p, relax_time=0.5) for c in ctrl]
        assert all(kr.yaw_parity_ok(pr, u) for pr, u in zip(prs, us))
        tol = kr.yaw_tolerance(list(zip(prs, us)))[1]
        out = gm.plan_yaws(ctrl, None, [YAW_START] * n, [YAW_END] * n, knots=rows, **yaw_cfg(p, mode))
        for b in range(n):
            yaw_same(out, b, kr.yaw_solve(prs[b], us[b]), tol, "chain %d mode %d" % (b, mode))


# ---- 4. the batch chain ---------------------------------------------------------------------------------------------------
def _batch(gm, mintime, spoil=()):
    import fuel_amd
    C, N, dt = 8, 12, 0.2
    ctrl = np.stack([tc.wiggle((0.1, tc.HIT_Y, tc.HIT_Z) if c % 2 == 0 else (-1.4, tc.FREE_Y, 0.3), N, seed=60 + c, amp=0.03)
                     for c in range(C)])
    x, ptd, st, en = helpers.bspline_inputs(ctrl, dt, mintime)
    for c, v in spoil:
        x[c, -1] = v
    cf = fuel_amd.SMOOTHNESS | fuel_amd.FEASIBILITY | fuel_amd.START | fuel_amd.END | (fuel_amd.MINTIME if mintime else 0)
    opt = fuel_amd.BsplineOptimizer()
    opt.setEnvironment(gm)
    return opt.deviceProblem(fuel_amd.BsplineBatchProblem(x, N, cf, ptd, st, en, 3, 3, dt)), C, N, dt, ctrl


def _consumers(C, N):
    """the arguments the three calls share between the batch route and the host route"""
    now = [0.05 * c for c in range(C)]
    t = [np.concatenate([[-0.1, 0.0], np.linspace(0.01, 4.0, 66 + c)]) for c in range(C)]
    smp = dict(yaw_ctrl=[YAW_CTRL] * C, yaw_dt=0.4, flight=np.zeros((C, 8)), degree=3, yaw_degree=3)
    yaw = [dict(yaw_cfg(3, mode)) for mode in (yr.EXPLORE, yr.FOLLOW)]
    for y in yaw:
        y.pop("weights")  # the batch's own
    return now, t, smp, yaw


def _dev_results(dev, C, N):
    now, t, smp, yaw = _consumers(C, N)
    return (dev.check_trajs(now, degree=3), dev.sample_trajs(t, **smp),
            [dev.plan_yaws([YAW_START] * C, [YAW_END] * C, **y) for y in yaw])


def _host_results(gm, dev, pos, C, N, span=None, knots=None):
    now, t, smp, yaw = _consumers(C, N)
    return (gm.check_trajs(pos, span, now, knots=knots, degree=3), gm.sample_trajs(pos, span, t, knots=knots, **smp),
            [gm.plan_yaws(pos, span, [YAW_START] * C, [YAW_END] * C, knots=knots, **y) for y in yaw])


def _same_results(a, b, tag):
    all_equal(a[0], b[0], CHK_INT + CHK_DBL, tag + " check")
    all_equal(a[1], b[1], SMP_KEYS, tag + " sample")
    for ya, yb, mode in zip(a[2], b[2], ("explore", "follow")):
        all_equal(ya, yb, YAW_KEYS, tag + " yaw " + mode)


@pytest.mark.parametrize("mintime", [True, False])
def test_batch_chain(env, mintime):
    import fuel_amd
    gm, _ = env
    dev, C, N, dt, _ = _batch(gm, mintime)
    U, A = dev.KNOTS_UNIFORM, dev.KNOTS_ADJUSTED
    assert dev.knot_source == U
    with pytest.raises(fuel_amd.FuelmiError, match="error -1"):  # never solved, never adjusted
        dev.set_knot_source(A)
    xo, _, _ = dev.optimize(max_eval=30)
    with pytest.raises(fuel_amd.FuelmiError, match="error -1"):  # solved, not adjusted
        dev.set_knot_source(A)
    assert dev.knot_source == U
    pos = list(xo[:, :3 * N].reshape(C, N, 3))
    span = xo[:, -1] if mintime else np.full(C, dt)
    uniform = _dev_results(dev, C, N)
    _same_results(uniform, _host_results(gm, dev, pos, C, N, span=span), "uniform")
    adj = dev.adjust_trajs(ops=ar.LENGTHEN | ar.REALLOC, **LIMITS)
    assert (adj["status"] == ar.OK).all() and adj["iters"].max() >= 1
    assert dev.knot_source == U  # the adjustment alone changes nothing
    _same_results(_dev_results(dev, C, N), uniform, "adjusted, source still uniform")
    dev.set_knot_source(A)
    assert dev.knot_source == A
    moved = _dev_results(dev, C, N)
    _same_results(moved, _host_results(gm, dev, pos, C, N, knots=list(adj["knots_out"])), "adjusted")
    assert _bits(moved[0]["duration"]) == _bits(adj["duration_out"]) != _bits(uniform[0]["duration"])
    dev.set_knot_source(U)  # back and forth by hand
    _same_results(_dev_results(dev, C, N), uniform, "back to uniform")
    dev.set_knot_source(A)
    # another solve: the source reads UNIFORM, the results are the uniform entries' on the new x_out
    xo2, _, _ = dev.optimize(max_eval=5)
    assert dev.knot_source == U
    with pytest.raises(fuel_amd.FuelmiError, match="error -1"):
        dev.set_knot_source(A)
    pos2 = list(xo2[:, :3 * N].reshape(C, N, 3))
    _same_results(_dev_results(dev, C, N), _host_results(gm, dev, pos2, C, N, span=xo2[:, -1] if mintime else span), "solved again")
    # a reload clears it too
    dev.adjust_trajs(ops=ar.REALLOC, **LIMITS)
    dev.set_knot_source(A)
    smp = np.cumsum(np.random.default_rng(5).normal(scale=0.1, size=(C, N - 2, 3)), axis=1)
    dev.loadSamples(np.full(C, 0.2), smp, np.zeros((C, 4, 3)))
    assert dev.knot_source == U
    with pytest.raises(fuel_amd.FuelmiError, match="error -1"):
        dev.set_knot_source(A)
    dev.close()


# ---- 5. a bad candidate among good neighbours -------------------------------------------------------------------------------
def test_bad_candidate_among_good_neighbours(env):
    """a MINTIME variable that is 0 / not a number: the adjustment marks the candidate BADSPLINE and keeps knots of 0 for
    it, which only the kernels' own check can meet -- each consumer reports its bad-spline status, the others are complete"""
    gm, _ = env
    dev, C, N, dt, _ = _batch(gm, True, spoil=((1, 0.0), (6, float("nan"))))
    xo, _, _ = dev.optimize(max_eval=1)
    knot = xo[:, -1]
    bad = ~(np.isfinite(knot) & (knot > 0.0))
    assert bad[1] and bad[6] and bad.sum() == 2, knot
    adj = dev.adjust_trajs(ops=ar.REALLOC, **LIMITS)
    assert (adj["status"][bad] == ar.BADSPLINE).all() and (adj["status"][~bad] == ar.OK).all()
    assert not adj["knots_out"][bad].any()
    dev.set_knot_source(dev.KNOTS_ADJUSTED)
    chk, smp, yaws = _dev_results(dev, C, N)
    good = np.flatnonzero(~bad)
    pos = xo[:, :3 * N].reshape(C, N, 3)
    now, t, skw, ykw = _consumers(C, N)
    kn = [adj["knots_out"][c] for c in good]
    want = gm.check_trajs(list(pos[good]), None, [now[c] for c in good], knots=kn, degree=3)
    for k in CHK_INT + CHK_DBL:
        assert _bits(chk[k][good]) == _bits(want[k]), k
    skw = dict(skw, yaw_ctrl=[YAW_CTRL] * len(good), flight=np.zeros((len(good), 8)))
    want = gm.sample_trajs(list(pos[good]), None, [t[c] for c in good], knots=kn, max_t=smp["status"].shape[1], **skw)
    for k in SMP_KEYS:
        assert _bits(smp[k][good]) == _bits(want[k]), k
    for got, y in zip(yaws, ykw):
        want = gm.plan_yaws(list(pos[good]), None, [YAW_START] * len(good), [YAW_END] * len(good), knots=kn,
                            **y)
        for k in YAW_KEYS:
            assert _bits(got[k][good]) == _bits(want[k]), k
    for c in np.flatnonzero(bad):
        assert chk["status"][c] == tr.NONFINITE and chk["end_reason"][c] == tr.END_NONFINITE
        assert chk["duration"][c] == 0.0 and chk["n_samples"][c] == 0 and chk["safe"][c] == 0
        nt = len(t[c])
        assert (smp["status"][c, :nt] == ts.BADSPLINE).all() and not smp["status"][c, nt:].any()
        assert not any(smp[k][c].any() for k in ("pos", "vel", "acc", "jerk", "yaw", "yawdot", "yawddot")) and smp["duration"][c] == 0.0
        for got in yaws:
            assert got["status"][c] == yr.DEGENERATE
            assert not any(np.asarray(got[k][c]).any() for k in YAW_KEYS if k != "status")
    dev.close()
