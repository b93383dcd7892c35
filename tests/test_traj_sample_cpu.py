"""The restatement of trajectory sampling (tests/traj_sample_ref.py) and the scenes of tests/traj_sample_cases.py checked on
the host, and the host side of the new calls: the restatement's evaluations of derivative orders 0..3 equal the real
NonUniformBspline bit for bit through ref_spline_evaluate / ref_spline_duration of oracle/_ref, where that was built (yaw
in column 0 of a 3-column spline); every scene reaches the statuses it is drawn for; the literal record equals the
windowed one at any window size and across a split tape; fuelmi_traj_sample_plan, the exported symbols and every refusal
that needs no device."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import traj_sample_cases as tc
import traj_sample_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NEW_SYMBOLS = ("fuelmi_map_sample_trajs", "fuelmi_bspline_dev_sample_trajs", "fuelmi_traj_sample_plan")
QUICK = tc.quick_scenes()
EINVAL, ELIMIT = -1, -5


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def test_evaluations_against_the_real_spline():
    from oracle.ref_build import ref
    if not ref.available():
        pytest.skip("oracle/_ref was not built here")
    L = C.CDLL(ref.SO)
    dp = C.POINTER(C.c_double)
    L.ref_spline_evaluate.restype = None
    L.ref_spline_evaluate.argtypes = [dp, C.c_int, C.c_int, C.c_double, C.c_int, dp, C.c_int, dp]
    L.ref_spline_duration.restype = C.c_double
    L.ref_spline_duration.argtypes = [C.c_int, C.c_int, C.c_double]

    def real(ctrl, p, dt, deriv, t):
        ctrl = np.ascontiguousarray(ctrl, dtype=np.float64)
        t = np.ascontiguousarray(t, dtype=np.float64)
        out = np.zeros((len(t), 3))
        L.ref_spline_evaluate(ctrl.ctypes.data_as(dp), len(ctrl), p, dt, deriv, t.ctypes.data_as(dp), len(t), out.ctypes.data_as(dp))
        return out

    seen = samples = 0
    for sc in QUICK + tc.big_scenes():
        if sc["mode"] != sr.STATE and not sc["tag"].startswith(("cmd_", "big_")):
            continue
        ctrl, p, dt = sc["ctrl"], sc["degree"], sc["dt"]
        n = len(ctrl)
        assert L.ref_spline_duration(n, p, dt) == sr.Spline.uniform(ctrl, p, dt).duration()
        # STATE: every quantity is evaluateDeBoorT(t) of its spline, for any t -- the real class at the scene's own times
        s = sr.sample(sr.STATE, ctrl, p, dt, sc["t"], *((sc["yaw"]["ctrl"], sc["yaw"]["degree"], sc["yaw"]["dt"]) if sc["yaw"] else ()))
        for deriv, name in enumerate(("pos", "vel", "acc", "jerk")):
            want = real(ctrl, p, dt, deriv, sc["t"])
            assert _bits(s[name]) == _bits(want), (sc["tag"], name, np.abs(np.array(s[name]) - want).max())
            samples += len(want)
        if sc["yaw"]:
            y = sc["yaw"]
            col = np.zeros((len(y["ctrl"]), 3))
            col[:, 0] = y["ctrl"]
            assert L.ref_spline_duration(len(col), y["degree"], y["dt"]) == sr.Spline.uniform(col, y["degree"], y["dt"]).duration()
            for deriv, name in enumerate(("yaw", "yawdot", "yawddot")):
                want = real(col, y["degree"], y["dt"], deriv, sc["t"])
                assert _bits(s[name]) == _bits(want[:, 0]), (sc["tag"], name)
                assert not want[:, 1:].any()
                samples += len(want)
        seen += 1
    assert seen >= 25 and samples >= 2000


def test_derivative_family_is_the_class():
    """the members a derivative spline has after getDerivative: one row, one degree and two knots less, the parent's
    accumulated knots (not regenerated ones), the same time span; a cubic's jerk spline has degree 0 and returns a row"""
    ctrl, p, dt = tc.wiggle(9, 5), 3, 0.31
    fam = sr.Spline.uniform(ctrl, p, dt).family(3)
    u = sr.knots(9, p, dt)
    assert any(u[i] != (i - p) * dt for i in range(len(u)))  # accumulation and products differ somewhere
    for o, s in enumerate(fam):
        assert (len(s.ctrl), s.p, s.u) == (9 - o, p - o, u[o:len(u) - o])
        assert s.duration() == fam[0].duration() and s.u[s.p] == 0.0
    jerk = fam[3]
    for k in range(6):
        assert jerk.at(jerk.u[k + 1]) == jerk.ctrl[k]                                  # the strict < at a knot: row k
        assert jerk.at(math.nextafter(jerk.u[k + 1], math.inf)) == jerk.ctrl[min(k + 1, 5)]
    assert jerk.at(-1.0) == jerk.ctrl[0] and jerk.at(1e9) == jerk.ctrl[5]


def test_scenes_reach_their_edges():
    tags = {s["tag"] for s in QUICK}
    assert len(tags) == len(QUICK)
    assert {(s["degree"], len(s["ctrl"])) for s in QUICK} >= {(p, n) for p in (3, 4, 5) for n in (p + 1, p + 2, 9, 40)}
    assert {len(s["t"]) for s in QUICK} >= {0, 1, 63, 64, 65, 129}
    for sc in QUICK:
        s = tc.restate(sc)
        st, t = np.array(s["status"], dtype=int), sc["t"]
        D = tc.duration_of(len(sc["ctrl"]), sc["degree"], sc["dt"])
        assert s["duration"] == D
        if sc["mode"] == sr.STATE:
            assert not st.any() and (len(t) == 0 or (t.min() < 0.0 and t.max() > D))
            continue
        if sc["tag"].startswith(("cmd_", "stop_")):
            T = D if sc["t_stop"] is None else min(sc["t_stop"], D)
            assert set(st.tolist()) >= ({sr.IN, sr.PAST, sr.INVALID} if T > 0 else {sr.PAST, sr.INVALID}), sc["tag"]
            assert st[t == T].tolist() == [sr.PAST] * int((t == T).sum()) and (t == T).any()
            if T > 0:
                assert (st[t == math.nextafter(T, 0.0)] == sr.IN).all() and (t == math.nextafter(T, 0.0)).any()
            past = np.flatnonzero(st == sr.PAST)
            assert all(s["pos"][k] == s["pos"][past[0]] and s["jerk"][k] == [0.0] * 3 for k in past)
            if sc["yaw"]:
                assert any(s["yawddot"][k] != 0.0 for k in np.flatnonzero(st == sr.IN)) or T <= 0
        if sc["tag"].startswith("stop_neg"):
            assert (st[(t < 0) & (t >= sc["t_stop"])] == sr.PAST).all() and (st[t < sc["t_stop"]] == sr.INVALID).all()
    # accumulated knots and products really differ somewhere, in every degree
    for p in (3, 4, 5):
        sc = next(s for s in QUICK if s["tag"] == "cmd_p%d_n40" % p)
        u = sr.knots(40, p, sc["dt"])
        assert any(u[i] - u[p] != (i - p) * sc["dt"] for i in range(p, 41))
    # a yaw duration that differs from the position's by rounding
    assert any(s["yaw"] and len(s["yaw"]["ctrl"]) == 12 + s["yaw"]["degree"] and
               tc.duration_of(len(s["yaw"]["ctrl"]), s["yaw"]["degree"], s["yaw"]["dt"]) !=
               tc.duration_of(len(s["ctrl"]), s["degree"], s["dt"]) for s in QUICK)
    assert any(s["yaw"] and len(s["yaw"]["ctrl"]) == 4 and s["yaw"]["degree"] == 3 for s in QUICK)


def test_record_literal_equals_windowed():
    seen = 0
    for sc in QUICK + tc.big_scenes():
        if sc["mode"] != sr.COMMAND:
            continue
        s = tc.restate(sc)
        lit = sr.record_literal(sc["t"], s)
        assert _bits(lit) == _bits(s["flight"]), (sc["tag"], lit, s["flight"])
        for width in (1, 7, 4096):
            assert _bits(sr.record_windowed([0.0] * 8, sc["t"], s, width)) == _bits(lit), (sc["tag"], width)
        for cut in (1, len(sc["t"]) // 2, tc.WIN):  # a tape split over two calls with the record carried
            if cut < len(sc["t"]):
                a = {k: s[k][:cut] for k in ("status", "pos", "jerk")}
                b = {k: s[k][cut:] for k in ("status", "pos", "jerk")}
                mid = sr.record_windowed([0.0] * 8, sc["t"][:cut], a)
                assert _bits(sr.record_windowed(mid, sc["t"][cut:], b)) == _bits(lit), (sc["tag"], cut)
        seen += 1
    assert seen >= 40


def test_record_scenes():
    by = {s["tag"]: s for s in QUICK}
    sc = by["record_slow"]
    s = tc.restate(sc)
    pos = np.array(s["pos"])
    step = np.sqrt(((pos[1:] - pos[:-1]) ** 2).sum(axis=1))
    assert (step < 1e-6).all() and (step > 0.5e-6).all()  # against the previous sample nothing would ever be pushed
    n_cmd = s["flight"][7]
    assert 0.4 * len(pos) <= n_cmd <= 0.6 * len(pos) and s["flight"][5] > 0.0  # the last pushed one: about every other
    assert s["flight"][4] == sc["t"][-1] and s["flight"][0] == 1.0
    inv = tc.restate(by["record_invalid_mid"])
    assert inv["status"].count(sr.INVALID) == 2 and inv["flight"][4] == by["record_invalid_mid"]["t"][-1]
    assert inv["flight"][7] < s["flight"][7]
    sc = by["record_past_end"]
    s = tc.restate(sc)
    n_in = s["status"].count(sr.IN)
    assert 0 < n_in < len(sc["t"]) - 5 and s["status"].count(sr.PAST) == len(sc["t"]) - n_in
    # the end point is pushed once (it differs from the last IN sample), the repeats are not; energy gains 0 there
    assert s["flight"][7] == n_in + 1 and s["flight"][1:4] == s["pos"][-1] and s["flight"][6] > 0.0
    only_in = {k: s[k][:n_in] for k in ("status", "pos", "jerk")}
    assert sr.record_windowed([0.0] * 8, sc["t"][:n_in], only_in)[6] == s["flight"][6]


def _cfg(**kw):
    from fuel_amd.host import traj_sample_cfg
    return traj_sample_cfg(**kw)


def test_plan_call():
    import fuel_amd
    L = fuel_amd.lib()
    out = (C.c_int * 3)()
    big = _cfg(max_ctrl=1024, max_yaw_ctrl=1024, max_t=64)
    assert L.fuelmi_traj_sample_plan(C.byref(big), out) == 0
    lanes, lds, cap = tuple(out)
    assert cap == fuel_amd._lib.TRAJSMP_MAX_CTRL == sr.MAX_CTRL == 1024 and lanes == tc.WIN == 64
    assert 0 < lds <= 64 * 1024 and lds % 16 == 0
    assert lds == tc.PACK * 2 * (1024 + 6) * 8  # whole waves, each with the knots of its two splines: n + p + 1 <= max + 6
    assert fuel_amd.SDFMap.traj_sample_plan(big) == (lanes, lds, cap)
    assert L.fuelmi_traj_sample_plan(C.byref(_cfg(max_ctrl=1024)), out) == 0 and out[1] == lds // 2  # no yaw: no block
    assert L.fuelmi_traj_sample_plan(C.byref(_cfg(max_ctrl=40, max_yaw_ctrl=15)), out) == 0 and 0 < out[1] < lds // 2
    assert L.fuelmi_traj_sample_plan(C.byref(_cfg(mode=sr.STATE, degree=5, max_ctrl=6, yaw_degree=5, max_yaw_ctrl=6)), out) == 0
    assert L.fuelmi_traj_sample_plan(C.byref(_cfg(yaw_degree=9, max_t=sr.MAX_T)), out) == 0  # yaw_degree is not read
    for bad in (dict(max_ctrl=1025), dict(max_yaw_ctrl=1025), dict(max_t=sr.MAX_T + 1)):
        assert L.fuelmi_traj_sample_plan(C.byref(_cfg(**bad)), out) == ELIMIT, bad
        assert "max_" in L.fuelmi_last_error().decode()
    for bad in (dict(mode=2), dict(mode=-1), dict(degree=2), dict(degree=6, max_ctrl=8), dict(max_ctrl=3),
                dict(degree=5, max_ctrl=5), dict(max_yaw_ctrl=-1), dict(max_yaw_ctrl=3), dict(yaw_degree=2, max_yaw_ctrl=8),
                dict(yaw_degree=6, max_yaw_ctrl=8), dict(yaw_degree=5, max_yaw_ctrl=5), dict(max_t=-1)):
        assert L.fuelmi_traj_sample_plan(C.byref(_cfg(**bad)), out) == EINVAL, bad
    assert L.fuelmi_traj_sample_plan(None, out) == EINVAL
    assert L.fuelmi_traj_sample_plan(C.byref(big), None) == EINVAL


def test_refusals_that_need_no_device():
    """every FUELMI_EINVAL / FUELMI_ELIMIT of fuelmi_map_sample_trajs comes before the map is touched: m = NULL"""
    import fuel_amd
    L = fuel_amd.lib()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731
    n, MT = 2, 5
    names = ("status", "pos", "vel", "acc", "jerk", "yaw", "yawdot", "yawddot", "duration")

    def call(cfg=None, n_prob=n, null=(), mt=MT, **kw):
        cfg = cfg if cfg is not None else _cfg(max_ctrl=11, max_yaw_ctrl=7, max_t=mt)
        a = dict(n_ctrl=np.array([11, 4], dtype=np.int32), pos_ctrl=np.zeros((n, max(cfg.max_ctrl, 1), 3)), knot=np.array([0.4, 0.5]),
                 n_yaw=np.array([7, 0], dtype=np.int32), yaw_ctrl=np.zeros((n, max(cfg.max_yaw_ctrl, 1))), yaw_dt=np.array([0.3, -1.0]),
                 t_stop=np.array([1.0, 2.0]), n_t=np.array([mt, 0], dtype=np.int32), t=np.zeros((n, max(mt, 1))),
                 flight=np.zeros((n, 8)))
        if cfg.mode == sr.STATE:
            null = tuple(null) + tuple(k for k in ("t_stop", "flight") if k not in kw)
        for k, v in kw.items():
            a[k] = np.ascontiguousarray(v, dtype=a[k].dtype)
        o = dict(status=np.full((n, max(mt, 1)), 77, dtype=np.int32), **{k: np.zeros((n, max(mt, 1), 3)) for k in names[1:]})
        call.out = o
        ptr = {k: (None if k in null else (ip(v) if v.dtype == np.int32 else dp(v))) for k, v in list(a.items()) + list(o.items())}
        return L.fuelmi_map_sample_trajs(None, None if "cfg" in null else C.byref(cfg), n_prob, ptr["n_ctrl"], ptr["pos_ctrl"],
                                         ptr["knot"], ptr["n_yaw"], ptr["yaw_ctrl"], ptr["yaw_dt"], ptr["t_stop"], ptr["n_t"],
                                         ptr["t"], *[ptr[k] for k in names], ptr["flight"])

    def at_the_map():
        return ": m (" in L.fuelmi_last_error().decode()

    assert call() == EINVAL and at_the_map(), L.fuelmi_last_error()  # everything valid: only the map is missing
    assert call(n_prob=0) == 0
    assert call(n_t=[0, 0]) == 0 and call(mt=0) == 0  # no sample at all: nothing is launched
    assert call(n_t=[0, 0], null=names + ("flight", "t_stop", "n_yaw")) == 0
    assert call(cfg=_cfg(max_ctrl=1025, max_t=MT), n_prob=0) == ELIMIT
    assert call(cfg=_cfg(max_ctrl=11, max_yaw_ctrl=1025, max_t=MT)) == ELIMIT
    assert call(cfg=_cfg(max_ctrl=11, max_t=sr.MAX_T + 1)) == ELIMIT
    many = _cfg(max_ctrl=11, max_yaw_ctrl=7, max_t=sr.MAX_T)  # 33 * 2^16 > 2^21: refused before any array is read
    assert L.fuelmi_map_sample_trajs(None, C.byref(many), sr.MAX_SAMPLES // sr.MAX_T + 1, *([None] * 19)) == ELIMIT
    assert "n_prob * max_t" in L.fuelmi_last_error().decode()
    pos_nan, pos_far, pos_beyond = np.zeros((n, 11, 3)), np.zeros((n, 11, 3)), np.zeros((n, 11, 3))
    pos_nan[1, 3, 2], pos_far[0, 10, 0], pos_beyond[1, 4, 0] = np.nan, 1e7, np.inf  # (past n_ctrl[1] = 4: not read)
    yaw_nan, yaw_far, yaw_beyond = np.zeros((n, 7)), np.zeros((n, 7)), np.zeros((n, 7))
    yaw_nan[0, 6], yaw_far[0, 0], yaw_beyond[1, 0] = np.nan, -1e7, np.nan     # (problem 1 has no yaw spline: not read)
    t_nan, t_beyond = np.zeros((n, MT)), np.zeros((n, MT))
    t_nan[0, MT - 1], t_beyond[1, 0] = np.nan, np.nan                         # (n_t[1] = 0: not read)
    fl_bad = np.zeros((n, 8))
    fl_bad[1, 6] = np.inf
    state = dict(mode=sr.STATE, max_ctrl=11, max_yaw_ctrl=7, max_t=MT)
    for kw in ([dict(null=(k,)) for k in ("cfg", "n_ctrl", "pos_ctrl", "knot", "yaw_ctrl", "yaw_dt", "n_t", "t") + names] +
               [dict(cfg=_cfg(mode=3, max_ctrl=11, max_t=MT)), dict(cfg=_cfg(degree=2, max_ctrl=11, max_t=MT)),
                dict(cfg=_cfg(degree=6, max_ctrl=11, max_t=MT)), dict(cfg=_cfg(degree=4, max_ctrl=11, max_yaw_ctrl=7, max_t=MT)),
                dict(cfg=_cfg(max_ctrl=11, yaw_degree=2, max_yaw_ctrl=7, max_t=MT)),
                dict(cfg=_cfg(max_ctrl=11, yaw_degree=4, max_yaw_ctrl=7, max_t=MT), n_yaw=[4, 0]),
                dict(cfg=_cfg(max_ctrl=11, max_yaw_ctrl=0, max_t=MT)),  # yaw splines given, no stride for them
                dict(n_ctrl=[11, 3]), dict(n_ctrl=[12, 4]), dict(n_yaw=[8, 0]), dict(n_yaw=[3, 0]), dict(n_yaw=[7, -1]),
                dict(knot=[0.4, 0.0]), dict(knot=[-0.1, 0.5]), dict(knot=[np.inf, 0.5]), dict(knot=[0.4, np.nan]),
                dict(yaw_dt=[0.0, 1.0]), dict(yaw_dt=[np.nan, 1.0]), dict(yaw_dt=[np.inf, 1.0]),
                dict(pos_ctrl=pos_nan), dict(pos_ctrl=pos_far), dict(yaw_ctrl=yaw_nan), dict(yaw_ctrl=yaw_far), dict(t=t_nan),
                dict(n_t=[MT + 1, 0]), dict(n_t=[MT, -1]), dict(t_stop=[np.nan, 1.0]), dict(t_stop=[1.0, np.inf]),
                dict(flight=fl_bad), dict(cfg=_cfg(**state), t_stop=[1.0, 1.0]), dict(cfg=_cfg(**state), flight=np.zeros((n, 8))),
                dict(n_prob=-1)]):
        assert call(**kw) == EINVAL, kw
        assert not at_the_map(), kw
        assert np.all(call.out["status"] == 77), kw
    # accepted up to the map: the limits themselves, garbage nobody reads, the optional arrays left out
    for kw in (dict(pos_ctrl=pos_beyond), dict(yaw_ctrl=yaw_beyond), dict(t=t_beyond), dict(null=("t_stop",)), dict(null=("flight",)),
               dict(null=("n_yaw", "yaw_ctrl", "yaw_dt")), dict(null=("n_yaw",)), dict(knot=[1e308, 5e-324]),
               dict(t=np.full((n, MT), -1e300)), dict(t_stop=[-1e300, 1e300]), dict(cfg=_cfg(**state)),
               dict(cfg=_cfg(max_ctrl=11, max_t=MT), null=("n_yaw",)),
               dict(cfg=_cfg(degree=5, max_ctrl=11, yaw_degree=5, max_yaw_ctrl=7, max_t=MT), n_ctrl=[11, 6], n_yaw=[6, 7], yaw_dt=[1.0, 1.0]),
               dict(cfg=_cfg(max_ctrl=1024, max_yaw_ctrl=1024, max_t=MT))):
        assert call(**kw) == EINVAL and at_the_map(), kw


def test_new_symbols_exported_and_declared():
    import fuel_amd
    header = open(os.path.join(ROOT, "include", "fuelmi.h")).read()
    L = fuel_amd.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert getattr(L, name) is not None and name in fuel_amd._lib.SYMBOLS
    exported = subprocess.run(["nm", "-D", "--defined-only", fuel_amd.LIB_PATH], check=True, capture_output=True,
                              text=True).stdout
    for name in NEW_SYMBOLS:
        assert re.search(r"\bT %s\b" % name, exported), name
    for word, val in (("COMMAND", sr.COMMAND), ("STATE", sr.STATE), ("IN", sr.IN), ("PAST", sr.PAST), ("INVALID", sr.INVALID),
                      ("BADSPLINE", sr.BADSPLINE), ("MAX_CTRL", sr.MAX_CTRL), ("MAX_T", sr.MAX_T), ("MAX_SAMPLES", sr.MAX_SAMPLES)):
        m = re.search(r"#define FUELMI_TRAJSMP_%s\s+(\d+)" % word, header)
        assert m and int(m.group(1)) == val == getattr(fuel_amd._lib, "TRAJSMP_" + word), word
    assert "fuelmi_trajsmp_cfg" in header
    # the facade and its driver
    hdr = open(os.path.join(ROOT, "fuel_amd", "facade", "bspline_opt", "bspline_optimizer.h")).read()
    assert "bool evaluateCommand(" in hdr and "bool replanState(" in hdr
    assert os.access(os.path.join(ROOT, "fuel_amd", "facade", "facade_trajsample"), os.X_OK)
