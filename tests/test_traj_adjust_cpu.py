"""The restatement of trajectory time adjustment and metrics (tests/traj_adjust_ref.py) and the scenes of
tests/traj_adjust_cases.py checked on the host, and the host side of the new calls: the restatement equals, bit for bit,
what the reference's own NonUniformBspline gave for every recorded scene (tests/golden/traj_adjust/*.npz, recorded by
tests/golden/make_traj_adjust_golden.py through the real class built against the stand-ins of compat/); every scene
reaches the edge it is drawn for; fuelmi_traj_adjust_plan, the exported symbols and every refusal that needs no device.

The norm() of the Eigen stand-in (sqrt of the sum taken left to right) against real Eigen's is the project's standing
caveat: the recordings pin the stand-in's."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np

import traj_adjust_cases as tc
import traj_adjust_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NEW_SYMBOLS = ("fuelmi_map_adjust_trajs", "fuelmi_bspline_dev_adjust_trajs", "fuelmi_traj_adjust_plan")
GOLDEN = os.path.join(ROOT, "tests", "golden", "traj_adjust")
QUICK = tc.quick_scenes()
BY = {s["tag"]: s for s in QUICK}
EINVAL, ELIMIT = -1, -5


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def test_restatement_equals_the_real_class():
    scenes = tc.all_scenes()
    recorded = {f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz")}
    assert recorded == {s["tag"] for s in scenes}  # every scene steps by 0.01 and caps at 1.1: all are recorded
    for sc in scenes:
        g = np.load(os.path.join(GOLDEN, sc["tag"] + ".npz"))
        # the recording is of this scene
        assert _bits(g["ctrl"]) == _bits(sc["ctrl"]) and int(g["degree"]) == sc["degree"] and int(g["ops"]) == sc["ops"], sc["tag"]
        assert _bits(g["knots"]) == _bits(sc["knots"] if sc["knots"] is not None else np.zeros(0)), sc["tag"]
        assert sc["knots"] is not None or float(g["dt"]) == sc["dt"]
        assert (sc["ratio_in"] is None and math.isnan(float(g["ratio_in"]))) or float(g["ratio_in"]) == sc["ratio_in"]
        assert dict(zip(g["cfg_keys"].tolist(), g["cfg_vals"].tolist())) == {k: float(v) for k, v in sc["cfg"].items()}
        r = tc.restate(sc)
        for k in ar.INFO[1:]:
            assert int(g[k]) == r[k], (sc["tag"], k, int(g[k]), r[k])
        for k in ar.METRICS:
            assert _bits(g[k]) == _bits(r[k]), (sc["tag"], k, float(g[k]), r[k])
        assert _bits(g["knots_out"]) == _bits(r["knots_out"]), sc["tag"]
        assert _bits(g["samples"]) == _bits(np.array(r["samples"]).reshape(-1, 3)), sc["tag"]


def test_scenes_reach_their_edges():
    assert len(BY) == len(QUICK)
    R = {t: tc.restate(s) for t, s in BY.items()}
    assert {(s["degree"], len(s["ctrl"])) for s in QUICK} >= {(3, 4), (3, 7), (3, 8), (4, 5), (4, 10), (4, 11), (5, 6), (5, 13),
                                                              (5, 14), (3, 59), (3, 60), (3, 61), (3, 124)}
    assert len(tc.big_scenes()[0]["ctrl"]) == ar.MAX_CTRL
    # lengthenTime: a no-op up to n_ctrl = 3p - 2, knots move from 3p - 1 on
    for p in (3, 4, 5):
        for n, moves in ((3 * p - 2, False), (3 * p - 1, True)):
            s = ar.Spline(tc.path(n, 5), p, ar.knots(n, p, 0.2))
            s.lengthen_time(1.01)
            assert (s.u != ar.knots(n, p, 0.2)) == moves, (p, n)
    assert R["lengthen_small_n"]["knots_out"] == ar.knots(7, 3, 0.2)
    base = ar.knots(11, 3, 0.2)
    assert R["lengthen_one"]["knots_out"] == base and R["lengthen_one"]["time_inc"] == 0.0
    assert R["lengthen_below"]["duration_out"] < R["lengthen_one"]["duration_out"] < R["lengthen_above"]["duration_out"]
    capped = ar.Spline(BY["lengthen_above"]["ctrl"], 3, base)
    capped.lengthen_time(1.01)
    assert R["lengthen_above"]["knots_out"] == capped.u  # 1.5 was capped at 1.01
    # feasible at the input: no pass, the built knots come back
    f = R["feasible"]
    assert (f["feasible_in"], f["iters"], f["feasible"], f["feasible_out"]) == (1, 0, 1, 1)
    assert f["knots_out"] == ar.knots(12, 3, 0.25)
    # one velocity violation on the first interval, one on the last (the last knot moves)
    assert tc.violations(BY["vel_first"]) == ([0], []) and tc.violations(BY["vel_last"]) == ([7], [])
    assert len(BY["vel_last"]["ctrl"]) - 2 == 7
    no_len = ar.adjust(BY["vel_last"]["ctrl"], 3, 0.2, ops=ar.REALLOC, **BY["vel_last"]["cfg"])
    built = ar.knots(9, 3, 0.2)
    assert no_len["knots_out"][-1] != built[-1] and no_len["knots_out"][:9] == built[:9]
    # exactly at limit + 1e-4: not infeasible; one ulp above: infeasible
    lim = 2.0 + 1e-4
    at, above = tc.spline_of(BY["vel_at_limit"]), tc.spline_of(BY["vel_ulp_above"])
    assert at._vel(0)[0] == lim and above._vel(0)[0] == math.nextafter(lim, math.inf)
    assert (R["vel_at_limit"]["feasible_in"], R["vel_at_limit"]["iters"]) == (1, 0)
    assert R["vel_at_limit"]["knots_out"] == ar.knots(8, 3, 1.0)
    assert R["vel_ulp_above"]["feasible_in"] == 0 and R["vel_ulp_above"]["iters"] >= 1
    # limit_ratio binds: the first moved interval grows by exactly the cap; never feasible within 3 passes, nor 1
    s = tc.spline_of(BY["cap_binds_it1"])
    assert max(abs(e) for e in s._vel(0)) / 2.0 + 1e-4 > 1.1
    assert (R["cap_binds_it3"]["iters"], R["cap_binds_it3"]["feasible"], R["cap_binds_it3"]["feasible_out"]) == (3, 0, 0)
    assert (R["cap_binds_it1"]["iters"], R["cap_binds_it1"]["feasible"], R["cap_binds_it1"]["feasible_out"]) == (1, 0, 0)
    assert R["cap_binds_it1"]["duration_out"] < R["cap_binds_it3"]["duration_out"]
    # acceleration violations at i = 0 .. 3 on the input knots, the branch for i == 1 || i == 2 taken
    for i in range(4):
        sc = BY["acc_i%d" % i]
        assert tc.violations(sc)[0] == [] and i in tc.violations(sc)[1]
        log = []
        tc.spline_of(sc).reallocate_time(log)
        assert ("acc", i) in log and not any(k == "vel" for k, _ in log)
    for tag, i in (("acc_i1_p4", 1), ("acc_i2_p5", 2)):
        log = []
        tc.spline_of(BY[tag]).reallocate_time(log)
        assert ("acc", i) in log
    # a velocity move flips a later acceleration test: row 5 is over on the input knots and never found in the pass
    sc = BY["vel_flips_acc"]
    assert tc.violations(sc)[1] == [5]
    log = []
    tc.spline_of(sc).reallocate_time(log)
    assert [k for k, _ in log] == ["vel"] * 11
    # given knots: u[p] != 0 and not uniform
    for tag in ("given_knots_offset", "given_knots_p4"):
        u, p = BY[tag]["knots"], BY[tag]["degree"]
        assert u[p] != 0.0 and len(set(np.round(np.diff(u), 9))) > 2 and (np.diff(u) > 0).all()
    # the 64-sample window: getLength's steps and the walks' samples on both sides of 64
    steps = [tc.spline_of(BY["window_%g" % d]).get_length(0.01)[1] for d in (0.625, 0.635, 0.645, 0.655)]
    assert steps == [62, 63, 64, 65]
    assert [R["window_%g" % d]["num_vel"] for d in (0.625, 0.635, 0.645, 0.655)] == [63, 64, 65, 66]
    # the last accumulated t lies inside the 1e-4 margin: one step more than floor(dur / res)
    m = tc.spline_of(BY["margin"])
    assert m.get_length(0.01)[1] == 70 == math.floor(m.time_sum() / 0.01) + 1
    # RESAMPLE: seg_num + 1 and seg_num + 2
    assert R["resample_plus1"]["n_samples"] == 9 - 3 + 1 and R["resample_plus2"]["n_samples"] == 9 - 3 + 2
    assert tc.restate(BY["resample_plus2"], 9 - 3 + 2)["status"] == ar.OK
    assert ar.adjust(BY["resample_plus2"]["ctrl"], 3, 8e-5, ops=ar.RESAMPLE, max_samples=7)["status"] == ar.LONG
    # LONG beside valid
    assert [R[t]["status"] for t in ("long_valid", "long_long", "long_valid_again")] == [ar.OK, ar.LONG, ar.OK]
    lo = R["long_long"]
    assert lo["length"] == 0.0 and lo["num_vel"] == 0 and lo["n_samples"] == 0 and lo["jerk"] > 0 and lo["duration_out"] > 0
    assert lo["knots_out"] != ar.knots(10, 3, 0.2)
    # a jerk that is not a number
    assert math.isnan(R["nan_jerk"]["jerk"]) and R["nan_jerk"]["status"] == ar.OK
    res = [R["finite_jerk_a"], R["nan_jerk"], R["finite_jerk_b"], R["finite_jerk_a"], R["long_long"]]
    assert ar.select([0, 0, 0, 0, 1], res, 3) == [0, -1, -1]          # the tie: the smallest index; LONG alone: none
    assert ar.select([1, 1, 1, 0, 0], res, 2) == [3, 0]
    assert ar.select([0, 0, 1, 1, 1], res, 2) == [0, 3]


def test_one_call_equals_two_chained_calls():
    sc = BY["chain_both"]
    both = tc.restate(sc)
    first = ar.adjust(sc["ctrl"], 3, sc["dt"], ops=ar.LENGTHEN)
    second = ar.adjust(sc["ctrl"], 3, knots_in=first["knots_out"], ops=ar.REALLOC)
    assert first["knots_out"] != ar.knots(16, 3, 0.2) and second["knots_out"] != first["knots_out"]
    assert _bits(second["knots_out"]) == _bits(both["knots_out"])
    for k in ("iters", "feasible", "feasible_out", "duration_out", "length", "jerk", "mean_vel", "max_acc"):
        assert _bits(second[k]) == _bits(both[k]), k


def _cfg(**kw):
    from fuel_amd.host import traj_adjust_cfg
    return traj_adjust_cfg(**kw)


def test_plan_call():
    import fuel_amd
    L = fuel_amd.lib()
    out = (C.c_int * 3)()
    big = _cfg(max_ctrl=1024)
    assert L.fuelmi_traj_adjust_plan(C.byref(big), out) == 0
    lanes, lds, cap = tuple(out)
    assert cap == fuel_amd._lib.TRAJADJ_MAX_CTRL == ar.MAX_CTRL == 1024 and lanes == tc.WIN == 64
    assert lds == (1024 + 6 + 3 * 1024) * 8 <= 64 * 1024  # one problem per workgroup: the knots and the control points
    assert fuel_amd.SDFMap.traj_adjust_plan(big) == (lanes, lds, cap)
    assert fuel_amd.SDFMap.traj_adjust_plan(_cfg(max_ctrl=64))[1] == 4 * (64 + 6 + 3 * 64) * 8  # four waves
    assert fuel_amd.SDFMap.traj_adjust_plan(_cfg(max_ctrl=700))[1] == 2 * (700 + 6 + 3 * 700) * 8
    assert fuel_amd.SDFMap.traj_adjust_plan(_cfg(max_ctrl=5, degree=4))[1] == 4 * (5 + 7 + 15 + 1) * 8  # kept to 16 bytes
    c = _cfg()
    d = ar.DEFAULTS
    assert (c.limit_vel, c.limit_acc, c.limit_ratio, c.lengthen_cap, c.realloc_iters, c.length_res, c.stat_step) == (
        d["limit_vel"], d["limit_acc"], d["limit_ratio"], d["lengthen_cap"], d["realloc_iters"], d["length_res"], d["stat_step"])
    assert (2.0, 2.0, 1.1, 1.01, 3, 0.01, 0.01) == (c.limit_vel, c.limit_acc, c.limit_ratio, c.lengthen_cap, c.realloc_iters,
                                                    c.length_res, c.stat_step)
    assert L.fuelmi_traj_adjust_plan(C.byref(_cfg(max_ctrl=1025)), out) == ELIMIT
    assert L.fuelmi_traj_adjust_plan(C.byref(_cfg(ops=ar.RESAMPLE, max_ctrl=8, max_samples=4097)), out) == ELIMIT
    assert L.fuelmi_traj_adjust_plan(C.byref(_cfg(ops=ar.SELECT, n_group=ar.MAX_PROB + 1)), out) == ELIMIT
    nan, inf = float("nan"), float("inf")
    for bad in (dict(ops=16), dict(ops=-1), dict(degree=2), dict(degree=6, max_ctrl=8), dict(max_ctrl=3), dict(degree=5, max_ctrl=5),
                dict(limit_vel=0.0), dict(limit_vel=-1.0), dict(limit_vel=nan), dict(limit_vel=inf), dict(limit_acc=0.0),
                dict(limit_acc=nan), dict(limit_acc=inf), dict(limit_ratio=1.0), dict(limit_ratio=nan), dict(limit_ratio=inf),
                dict(lengthen_cap=0.99), dict(lengthen_cap=nan), dict(lengthen_cap=inf), dict(realloc_iters=0),
                dict(realloc_iters=17), dict(length_res=0.0), dict(length_res=nan), dict(length_res=inf), dict(stat_step=0.0),
                dict(stat_step=-0.01), dict(stat_step=nan), dict(stat_step=inf),
                dict(ops=ar.RESAMPLE, max_ctrl=9, max_samples=9 - 3 + 1), dict(ops=ar.SELECT, n_group=0)):
        assert L.fuelmi_traj_adjust_plan(C.byref(_cfg(**bad)), out) == EINVAL, bad
    for good in (dict(ops=15, max_ctrl=9, max_samples=8, n_group=1), dict(lengthen_cap=1.0), dict(realloc_iters=16),
                 dict(realloc_iters=1), dict(limit_ratio=math.nextafter(1.0, 2.0)), dict(max_samples=-5), dict(n_group=-1)):
        assert L.fuelmi_traj_adjust_plan(C.byref(_cfg(**good)), out) == 0, good
    assert L.fuelmi_traj_adjust_plan(None, out) == EINVAL
    assert L.fuelmi_traj_adjust_plan(C.byref(big), None) == EINVAL


def test_refusals_that_need_no_device():
    """every FUELMI_EINVAL / FUELMI_ELIMIT of fuelmi_map_adjust_trajs comes before the map is touched: m = NULL"""
    import fuel_amd
    L = fuel_amd.lib()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731
    n, MC = 2, 11
    ks = MC + 3 + 1
    outs = ("info", "metrics", "knots_out", "samples", "best")
    full = dict(ops=15, max_ctrl=MC, max_samples=MC - 3 + 2, n_group=2)

    def good_knots():
        k = np.zeros((n, ks))
        k[0, :MC + 4] = np.array(ar.knots(MC, 3, 0.3)) + 0.2
        k[1, :8] = ar.knots(4, 3, 0.5)
        return k

    def call(cfg=None, n_prob=n, null=("knots_in",), **kw):
        cfg = cfg if cfg is not None else _cfg(**full)
        a = dict(n_ctrl=np.array([MC, 4], dtype=np.int32), pos_ctrl=np.zeros((n, max(cfg.max_ctrl, 1), 3)), knot=np.array([0.4, 0.5]),
                 knots_in=good_knots(), ratio_in=np.array([0.9, 1.2]), group=np.array([1, 0], dtype=np.int32))
        for k, v in kw.items():
            a[k] = np.ascontiguousarray(v, dtype=a[k].dtype)
        o = dict(info=np.full((n, ar.NI), 77, dtype=np.int32), metrics=np.zeros((n, ar.NM)), knots_out=np.zeros((n, ks)),
                 samples=np.zeros((n, max(cfg.max_samples, 1), 3)), best=np.full(max(cfg.n_group, 1), 77, dtype=np.int32))
        call.out = o
        ptr = {k: (None if k in null else (ip(v) if v.dtype == np.int32 else dp(v))) for k, v in list(a.items()) + list(o.items())}
        return L.fuelmi_map_adjust_trajs(None, None if "cfg" in null else C.byref(cfg), n_prob, ptr["n_ctrl"], ptr["pos_ctrl"],
                                         ptr["knot"], ptr["knots_in"], ptr["ratio_in"], ptr["group"], *[ptr[k] for k in outs])

    def at_the_map():
        return ": m (" in L.fuelmi_last_error().decode()

    assert call() == EINVAL and at_the_map(), L.fuelmi_last_error()  # everything valid: only the map is missing
    assert call(n_prob=0) == 0 and call(n_prob=0, null=outs + ("n_ctrl", "pos_ctrl", "knot", "knots_in", "group")) == 0
    assert call(cfg=_cfg(**dict(full, max_ctrl=1025, max_samples=1100)), n_prob=0) == ELIMIT
    assert call(cfg=_cfg(**dict(full, max_samples=ar.MAX_SAMPLES + 1))) == ELIMIT
    assert call(cfg=_cfg(**dict(full, n_group=ar.MAX_PROB + 1))) == ELIMIT
    assert L.fuelmi_map_adjust_trajs(None, C.byref(_cfg(**full)), ar.MAX_PROB + 1, *([None] * 11)) == ELIMIT
    assert "n_prob" in L.fuelmi_last_error().decode()
    pos_nan, pos_far, pos_beyond = np.zeros((n, MC, 3)), np.zeros((n, MC, 3)), np.zeros((n, MC, 3))
    pos_nan[1, 3, 2], pos_far[0, 10, 0], pos_beyond[1, 4, 0] = np.nan, 1e7, np.inf  # (past n_ctrl[1] = 4: not read)
    k_nan, k_equal, k_down, k_inf, k_beyond = (good_knots() for _ in range(5))
    k_nan[0, 5] = np.nan
    k_equal[1, 4] = k_equal[1, 3]
    k_down[0, MC + 3] = k_down[0, MC + 1]
    k_inf[1, 7] = np.inf
    k_beyond[1, 8] = -np.inf  # (past n_ctrl[1] + p + 1 = 8: not read)
    with_knots = dict(null=())
    for kw in ([dict(null=("knots_in", k)) for k in ("cfg", "n_ctrl", "pos_ctrl", "group") + outs] +
               [dict(null=("knots_in", "knot"))] +  # neither a span nor knots
               [dict(cfg=_cfg(**dict(full, **bad))) for bad in (
                   dict(ops=16), dict(degree=2), dict(degree=6), dict(degree=4), dict(max_samples=MC - 3 + 1), dict(n_group=0),
                   dict(n_group=1), dict(limit_vel=0.0), dict(limit_acc=np.nan), dict(limit_ratio=1.0), dict(lengthen_cap=0.5),
                   dict(realloc_iters=0), dict(realloc_iters=17), dict(length_res=0.0), dict(stat_step=np.inf))] +
               [dict(n_ctrl=[MC, 3]), dict(n_ctrl=[MC + 1, 4]), dict(knot=[0.4, 0.0]), dict(knot=[-0.1, 0.5]), dict(knot=[np.inf, 0.5]),
                dict(knot=[0.4, np.nan]), dict(pos_ctrl=pos_nan), dict(pos_ctrl=pos_far), dict(ratio_in=[np.nan, 1.0]),
                dict(ratio_in=[1.0, np.inf]), dict(group=[0, 2]), dict(group=[-1, 0]), dict(n_prob=-1),
                dict(with_knots, knots_in=k_nan), dict(with_knots, knots_in=k_equal), dict(with_knots, knots_in=k_down),
                dict(with_knots, knots_in=k_inf)]):
        assert call(**kw) == EINVAL, kw
        assert not at_the_map(), kw
        assert np.all(call.out["info"] == 77) and np.all(call.out["best"] == 77), kw
    # accepted up to the map: the limits themselves, garbage nobody reads, the optional arrays left out
    for kw in (dict(pos_ctrl=pos_beyond), dict(with_knots), dict(with_knots, knots_in=k_beyond), dict(null=("knot",)),
               dict(null=("knots_in", "ratio_in")), dict(knot=[1e308, 5e-324]), dict(ratio_in=[-1e300, 1e300]),
               dict(null=(), knot=[np.nan, -1.0]),  # with knots_in the spans are not read
               dict(cfg=_cfg(ops=0, max_ctrl=MC), null=("knots_in", "samples", "best", "group", "ratio_in")),
               dict(cfg=_cfg(**dict(full, ops=ar.RESAMPLE)), null=("knots_in", "best", "group")),
               dict(cfg=_cfg(**dict(full, ops=ar.SELECT, max_samples=0)), null=("knots_in", "samples")),
               dict(cfg=_cfg(**dict(full, degree=5)), n_ctrl=[MC, 6], null=("knots_in",)),
               dict(cfg=_cfg(ops=15, max_ctrl=1024, max_samples=1023, n_group=2))):
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
    assert "fuelmi_trajadj_cfg" in header
    for word, val in (("LENGTHEN", ar.LENGTHEN), ("REALLOC", ar.REALLOC), ("RESAMPLE", ar.RESAMPLE), ("SELECT", ar.SELECT),
                      ("OK", ar.OK), ("BADSPLINE", ar.BADSPLINE), ("LONG", ar.LONG), ("MAX_CTRL", ar.MAX_CTRL),
                      ("MAX_SAMPLES", ar.MAX_SAMPLES), ("MAX_PROB", ar.MAX_PROB), ("MAX_STEPS", ar.MAX_STEPS), ("NI", ar.NI),
                      ("NM", ar.NM)):
        m = re.search(r"#define FUELMI_TRAJADJ_%s\s+(\d+)" % word, header)
        assert m and int(m.group(1)) == val == getattr(fuel_amd._lib, "TRAJADJ_" + word), word
    for k, name in enumerate(ar.INFO):
        assert re.search(r"#define FUELMI_TRAJADJ_I_%s %d\b" % (name.upper(), k), header), name
    for k, name in enumerate(ar.METRICS):
        assert re.search(r"#define FUELMI_TRAJADJ_M_%s %d\b" % (name.upper(), k), header), name
    assert fuel_amd._lib.TRAJADJ_INFO == ar.INFO and fuel_amd._lib.TRAJADJ_METRICS == ar.METRICS
    # the facade and its driver
    hdr = open(os.path.join(ROOT, "fuel_amd", "facade", "bspline_opt", "bspline_optimizer.h")).read()
    assert "bool adjustTime(" in hdr and "bool trajectoryMetrics(" in hdr and "int selectBestTraj(" in hdr
    assert os.access(os.path.join(ROOT, "fuel_amd", "facade", "facade_trajadjust"), os.X_OK)
    # what the header calls out of scope is the moved knots as another call's input, no longer the reallocation itself
    assert len(re.findall(r"fuelmi_map_adjust_trajs, below", header)) >= 3
    assert "knots moved by a time reallocation." not in header and "(lengthenTime) is out of scope" not in header
