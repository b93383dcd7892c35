"""The restatement of planYawExplore / planYaw (tests/yaw_plan_ref.py) checked against what exists outside it, and the
host side of the new calls: its de Boor evaluation and derivative spline against the real NonUniformBspline
(ref_spline_evaluate of oracle/_ref, where that was built), its dense Hessian against the gradient of the oracle's
combineCost in one dimension, the dense and the banded solve against each other (the measured disagreement and the
tolerance the GPU tests derive from it are printed), the accumulated-knot facts the GPU tests assert, fuelmi_yaw_plan,
the exported symbols and every refusal that needs no device."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import yaw_plan_ref as yr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NEW_SYMBOLS = ("fuelmi_map_plan_yaws", "fuelmi_bspline_dev_plan_yaws", "fuelmi_yaw_plan")
YAW_FLAGS = (1 << 0) | (1 << 3) | (1 << 4) | (1 << 6)  # SMOOTHNESS | START | END | WAYPOINTS


def test_deboor_and_derivative_against_the_real_spline():
    from oracle.ref_build import ref
    if not ref.available():
        pytest.skip("oracle/_ref was not built here")
    L = C.CDLL(ref.SO)
    dp = C.POINTER(C.c_double)
    L.ref_spline_evaluate.restype = None
    L.ref_spline_evaluate.argtypes = [dp, C.c_int, C.c_int, C.c_double, C.c_int, dp, C.c_int, dp]
    for degree, n, dt, seed in ((3, 4, 0.9, 1), (3, 11, 0.4, 2), (3, 35, 0.1, 3), (4, 14, 0.3, 4), (5, 16, 0.25, 5)):
        ctrl = np.ascontiguousarray(yr.curve(n, seed))
        u = yr.knots(n, degree, dt)
        dur = u[n] - u[degree]
        t = np.ascontiguousarray(np.concatenate([np.linspace(-0.2, dur + 0.2, 41), [0.0, dur, dur - 0.1, 12 * (dur / 12)]]))
        du, dpg, dq = yr.derivative(u, degree, ctrl)
        for deriv in (0, 1):
            out = np.zeros((len(t), 3))
            L.ref_spline_evaluate(ctrl.ctypes.data_as(dp), n, degree, dt, deriv, t.ctypes.data_as(dp), len(t),
                                  out.ctypes.data_as(dp))
            mine = np.array([yr.deboor(u, degree, ctrl, tk) if deriv == 0 else yr.deboor(du, dpg, dq, tk) for tk in t])
            assert np.array_equal(mine, out), (degree, n, deriv, np.abs(mine - out).max())


def test_dense_hessian_is_the_oracle_gradient():
    """grad combineCost(q) = 2 (H q - g) for the restatement's dense H, g: the oracle is the device the B-spline tests use"""
    from oracle import fuel_oracle as fo
    om = fo.OracleMap((4.0, 4.0, 2.0), (-1.5, -1.5, 0.0), (1.5, 1.5, 1.5))
    rng = np.random.default_rng(5)
    for pr in yr.parity_cases()[::3] + yr.follow_cases()[:1] + [yr.edge_cases()["end_minus"]]:
        f = yr.solve(pr, "dense")
        w = pr["weights"]
        H, g = yr.hessian_dense(f, w)
        N = len(g)
        assert np.array_equal(H, H.T) and np.all(np.abs(np.triu(H, 4)) == 0.0)  # symmetric, half-bandwidth 3
        np.linalg.cholesky(H)
        st = np.zeros((3, 3))
        st[:, 0] = f["start"]
        en = np.zeros((3, 3))
        en[0, 0] = f["end_yaw"]
        wp = np.zeros((len(f["waypts"]), 3))
        wp[:, 0] = f["waypts"]
        for q in (f["yaw_ctrl"] + rng.normal(size=N), rng.normal(size=N) * 3.0):
            c, gr = fo.bspline_cost_grad(om, q, N, YAW_FLAGS, f["pt_dist"], st, en, f["end_n"], 1, f["dt_yaw"], -1.0, None,
                                         wp if len(wp) else None, np.array(f["idx"], dtype=np.int32) if len(wp) else None)
            mine = 2.0 * (H @ q - g)
            scale = 2.0 * (np.abs(H) @ np.abs(q) + np.abs(g))
            assert np.all(np.abs(gr - mine) <= 1e-12 * scale), (pr["tag"], np.abs(gr - mine).max())
            cm = yr.cost(f, w, q)
            assert abs(c - cm) <= 1e-12 * max(1.0, abs(c)), (pr["tag"], c, cm)


def test_forms_agree_and_the_tolerance():
    measured, tol = yr.parity_tolerance()
    print("EXPLORE: dense vs banded and 6 ulp of atan2, largest change over parity_cases(): %s" % measured)
    print("EXPLORE: tolerance of the GPU tests (100 x): %s" % tol)
    fm, ft = yr.follow_tolerance()
    print("FOLLOW: measured %s, tolerance %s" % (fm, ft))
    # rounding of a system with a condition number below 1e9: nowhere near a visible yaw error
    for m in (measured, fm):
        assert 0.0 < m["waypts"] < 1e-12 and 0.0 < m["yaw_ctrl"] < 1e-7 and 0.0 < m["cost"] < 1e-10
    sizes, clamped, free = set(), 0, 0
    for pr in yr.parity_cases():
        assert yr.parity_ok(pr), pr["tag"]
        a, b = yr.solve(pr, "dense"), yr.solve(pr, "banded")
        assert a["status"] == b["status"] == yr.OK and a["n_waypt"] >= 1
        sizes.add(len(pr["ctrl"]))
        clamped += a["duration"] < pr["forward_t"]
        free += a["duration"] > 2 * pr["forward_t"]
    assert sizes == {4, 11, 35} and clamped >= 2 and free >= 2
    for pr in yr.follow_cases():
        assert yr.parity_ok(pr), pr["tag"]
    assert yr.solve(yr.follow_cases()[1])["n_waypt"] > 64


def test_edge_cases_hold_what_they_claim():
    E = {k: yr.solve(p, "banded") for k, p in yr.edge_cases().items()}
    w = np.array(E["spiral"]["waypts"])
    assert w[-1] > math.pi * 1.5 and np.all(np.diff(w) > 0) and np.abs(np.diff(w)).max() < 1.0
    assert abs(E["start_7"]["start"][0] - (7.0 - 2 * math.pi)) < 1e-15 and abs(E["start_m7"]["start"][0] + 7.0 - 2 * math.pi) < 1e-15
    assert E["end_plus"]["end_yaw"] == math.pi + (-3.0 - math.pi) + 2 * math.pi
    assert abs(E["end_minus"]["end_yaw"] - (3.5 - 2 * math.pi)) < 1e-15
    assert E["line_mx"]["waypts"] == [math.pi] * 11  # atan2(+0, -x) = pi, diff == pi takes the <= branch
    assert not yr.parity_ok(yr.edge_cases()["line_mx"])  # it sits on the branch on purpose
    s = E["stall_late"]["waypts"]
    assert s[-1] == s[-2] == s[-3] and s[0] != s[1]
    assert E["stall_all"]["waypts"] == [0.7] * 11  # the first way-point stalls: last_yaw
    assert E["climb"]["waypts"] == [0.0] * 11
    d = E["degenerate"]
    assert d["status"] == yr.DEGENERATE and d["cost"] == 0.0 and np.all(d["yaw_ctrl"] == 0.0)
    # relax: 11 way-points, exactly one, none
    base = yr.parity_cases()[3]
    dur = yr.front(base)["duration"]
    for relax, want in ((0.0, 11), (10.5 * dur / 12, 1), (dur, 0), (dur + 1.0, 0)):
        assert yr.solve(dict(base, relax_time=relax))["n_waypt"] == want, relax


def test_accumulated_knots():
    u = yr.knots(40, 3, 0.1)
    dur = u[40] - u[3]
    assert dur == float.fromhex("0x1.d99999999999ep+1") and dur != 3.7 and dur != 37 * 0.1
    for n, seg_acc, seg_prod in ((9, 2, 3), (18, 6, 5)):
        u = yr.knots(n, 3, 0.1)
        d = u[n] - u[3]
        assert int(math.ceil(d / 0.3)) == seg_acc and int(math.ceil(((n - 3) * 0.1) / 0.3)) == seg_prod
        f = yr.front(yr.problem(yr.curve(n, 30 + n), 0.1, (0.1, 0.0, 0.0), mode=yr.FOLLOW))
        assert f["seg_num"] == seg_acc
    assert yr.knots(9, 3, 0.1)[9] - 0.0 == 0.6


def _cfg(**kw):
    from fuel_amd.host import yaw_cfg
    return yaw_cfg(**kw)


def test_plan_call():
    import fuel_amd
    L = fuel_amd.lib()
    out = (C.c_int * 3)()
    big = _cfg(mode=1, max_ctrl=1024, max_seg=256)
    assert L.fuelmi_yaw_plan(C.byref(big), out) == 0
    lanes, lds, cap = tuple(out)
    assert cap == fuel_amd._lib.YAW_MAX_CTRL == 1024 and lanes % 64 == 0 and 0 < lds <= 64 * 1024
    assert fuel_amd.SDFMap.yaw_plan(big) == (lanes, lds, cap)
    assert L.fuelmi_yaw_plan(C.byref(_cfg(max_ctrl=35)), out) == 0 and out[1] < lds
    assert L.fuelmi_yaw_plan(C.byref(_cfg(max_ctrl=1025)), out) == -5
    assert L.fuelmi_yaw_plan(C.byref(_cfg(max_ctrl=3)), out) == -1
    assert L.fuelmi_yaw_plan(C.byref(_cfg(mode=2)), out) == -1
    assert L.fuelmi_yaw_plan(C.byref(_cfg(max_seg=257, seg_num=12)), out) == -1
    assert L.fuelmi_yaw_plan(None, out) == -1


def test_refusals_that_need_no_device():
    """every FUELMI_EINVAL / FUELMI_ELIMIT of fuelmi_map_plan_yaws comes before the map is touched: m = NULL"""
    import fuel_amd
    from fuel_amd._lib import BsplineCfg
    from fuel_amd.host import DEFAULT_BSPLINE
    L = fuel_amd.lib()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731
    n = 2
    outs = dict(status=np.zeros(n, np.int32), duration=np.zeros(n), seg=np.zeros(n, np.int32), dt=np.zeros(n),
                ctrl=np.zeros((n, 15)), nw=np.zeros(n, np.int32), wp=np.zeros((n, 12)), e=np.zeros(n), cost=np.zeros(n))

    def call(cfg=None, w=None, n_prob=n, n_ctrl=(11, 4), pos=None, knot=(0.4, 0.5), start=None, end=(0.5, 1.0),
             null=()):
        cfg = cfg if cfg is not None else _cfg(max_ctrl=11)
        wc = BsplineCfg(**dict(DEFAULT_BSPLINE, **(w or {})))
        a = dict(n_ctrl=np.array(n_ctrl, dtype=np.int32), pos=np.zeros((n, max(cfg.max_ctrl, 1), 3)) if pos is None else pos,
                 knot=np.array(knot, dtype=np.float64), start=np.zeros((n, 3)) + 0.1 if start is None else start,
                 end=np.array(end, dtype=np.float64))
        ptr = {k: (None if k in null else (ip(v) if v.dtype == np.int32 else dp(v))) for k, v in a.items()}
        o = {k: (None if k in null else (ip(v) if v.dtype == np.int32 else dp(v))) for k, v in outs.items()}
        return L.fuelmi_map_plan_yaws(None, None if "w" in null else C.byref(wc), None if "cfg" in null else C.byref(cfg),
                                      n_prob, ptr["n_ctrl"], ptr["pos"], ptr["knot"], ptr["start"], ptr["end"], o["status"],
                                      o["duration"], o["seg"], o["dt"], o["ctrl"], o["nw"], o["wp"], o["e"], o["cost"],
                                      None, None)

    EINVAL, ELIMIT = -1, -5
    assert call() == EINVAL  # everything valid: only the map is missing
    assert call(n_prob=0) == 0
    assert call(cfg=_cfg(max_ctrl=1025), n_prob=0) == ELIMIT
    assert call(cfg=_cfg(max_ctrl=1025)) == ELIMIT
    assert "max_ctrl" in L.fuelmi_last_error().decode()
    bad = np.zeros((n, 11, 3))
    bad[1, 3, 2] = np.nan
    far = np.zeros((n, 11, 3))
    far[0, 10, 0] = 1e7
    beyond = np.zeros((n, 11, 3))
    beyond[1, 4, 0] = np.inf  # past n_ctrl[1] = 4: not read
    for kw in (dict(null=("cfg",)), dict(null=("w",)), dict(null=("n_ctrl",)), dict(null=("pos",)), dict(null=("knot",)),
               dict(null=("start",)), dict(null=("end",)), dict(null=("status",)), dict(null=("cost",)), dict(null=("wp",)),
               dict(cfg=_cfg(mode=2, max_ctrl=11)), dict(cfg=_cfg(mode=-1, max_ctrl=11)),
               dict(cfg=_cfg(pos_degree=2, max_ctrl=11)), dict(cfg=_cfg(pos_degree=6, max_ctrl=11)),
               dict(n_ctrl=(11, 3)), dict(n_ctrl=(12, 4)), dict(knot=(0.4, 0.0)), dict(knot=(-0.1, 0.5)),
               dict(knot=(np.inf, 0.5)), dict(knot=(0.4, np.nan)), dict(pos=bad), dict(pos=far),
               dict(start=np.array([[0.1, 0.0, 0.0], [1001.0, 0.0, 0.0]])), dict(start=np.array([[0.1, np.nan, 0.0], [0.0, 0.0, 0.0]])),
               dict(end=(0.5, -1001.0)), dict(end=(np.inf, 0.0)),
               dict(w=dict(ld_start=0.0)), dict(w=dict(ld_smooth=0.0)), dict(w=dict(ld_smooth=-1.0)), dict(w=dict(ld_end=np.nan)),
               dict(w=dict(ld_waypt=np.inf)),
               dict(cfg=_cfg(max_ctrl=11, forward_t=-1.0)), dict(cfg=_cfg(max_ctrl=11, relax_time=np.nan)),
               dict(cfg=_cfg(max_ctrl=11, end_back=-0.1)), dict(cfg=_cfg(max_ctrl=11, dt_target=-0.3)),
               dict(cfg=_cfg(mode=1, max_ctrl=11, dt_target=0.0)),
               dict(cfg=_cfg(max_ctrl=11, seg_num=0)), dict(cfg=_cfg(max_ctrl=11, seg_num=13, max_seg=12)),
               dict(cfg=_cfg(max_ctrl=11, seg_num=12, max_seg=257)), dict(cfg=_cfg(mode=1, max_ctrl=11, max_seg=0)),
               dict(n_prob=-1)):
        outs["status"][:] = 77
        assert call(**kw) == EINVAL, kw
        assert np.all(outs["status"] == 77), kw
    # accepted up to the map: the limits themselves, and garbage past a problem's own control points
    for kw in (dict(start=np.array([[1000.0, -1000.0, 0.0], [0.0, 0.0, 1000.0]])), dict(end=(1000.0, -1000.0)),
               dict(pos=beyond), dict(w=dict(ld_end=0.0, ld_waypt=0.0)), dict(cfg=_cfg(max_ctrl=11, dt_target=0.0)),
               dict(cfg=_cfg(mode=1, max_ctrl=11), null=("end",)), dict(cfg=_cfg(max_ctrl=1024, seg_num=256, max_seg=256),
                                                                         pos=np.zeros((n, 1024, 3)))):
        assert call(**kw) == EINVAL and ": m (" in L.fuelmi_last_error().decode(), kw


def test_new_symbols_exported_and_declared():
    import fuel_amd
    header = open(os.path.join(ROOT, "include", "fuelmi.h")).read()
    L = fuel_amd.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert getattr(L, name) is not None and name in fuel_amd._lib.SYMBOLS
    for word in ("FUELMI_YAW_EXPLORE", "FUELMI_YAW_FOLLOW", "FUELMI_YAW_OK", "FUELMI_YAW_DEGENERATE", "fuelmi_yaw_cfg"):
        assert word in header, word
    exported = subprocess.run(["nm", "-D", "--defined-only", fuel_amd.LIB_PATH], check=True, capture_output=True,
                              text=True).stdout
    for name in NEW_SYMBOLS:
        assert re.search(r"\bT %s\b" % name, exported), name
    for word, val in (("FUELMI_YAW_MAX_SEG", fuel_amd._lib.YAW_MAX_SEG), ("FUELMI_YAW_MAX_CTRL", fuel_amd._lib.YAW_MAX_CTRL)):
        m = re.search(r"#define %s\s+(\d+)" % word, header)
        assert m and int(m.group(1)) == val
