"""The local segments of the global trajectory, without a GPU: every scene of tests/localseg_cases.py is proven to sit
on the edge it is drawn for (its expectations and predicate, on the restatement tests/localseg_ref.py), with the same
integers and the same getState branches in both forms of the polynomial; the scene list covers the issue; the
restatement against the recordings of the reference's own GlobalTrajData (tests/golden/localseg/*.npz,
tests/golden/make_localseg_golden.py) within a tolerance that is measured; the host build of the kernel's own text under
the address and undefined-behaviour sanitizers (tests/golden/check_localseg_host_build.py); fuelmi_localseg_plan, the
exported symbols and every refusal that needs no device.

The tolerance: the reference calls pow and Eigen's dot, whose bits are not restated, so a double is allowed 100 x the
largest disagreement between the restatement's literal_pow=True and =False forms over the recorded scenes (the x 100 is
waypoint_traj_ref.parity_tolerance's margin).  Measured: 8.9e-16 between the forms, so 8.9e-14 is allowed; the restatement
is 8.9e-16 off the recordings at the most."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import localseg_cases as lc
import localseg_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "localseg")
SCENES = lc.scenes()
INTS = ("status", "n_steps", "seg_num", "n_points", "n_ctrl")
NEW_SYMBOLS = ("fuelmi_map_local_segments", "fuelmi_localseg_plan", "fuelmi_bspline_dev_load_local_segments")
EINVAL, ELIMIT = -1, -5


@pytest.mark.parametrize("sc", SCENES, ids=[s["tag"] for s in SCENES])
def test_scene_reaches_its_edge(sc):
    r, lit = lc.restate(sc), lc.restate(sc, literal_pow=True)
    for k, v in sc["expect"].items():
        assert r[k] == v, (sc["tag"], k, r[k], v)
    assert sc["pred"] is None or sc["pred"](r), sc["tag"]
    # no knife edge: the integers and every getState's branch and segment are the same in both forms
    assert [r[k] for k in INTS] == [lit[k] for k in INTS] and r["trace"] == lit["trace"], sc["tag"]
    assert len(r["points"]) == min(r["n_points"], sc["max_points"])


def test_scene_list_covers_the_issue():
    by = {s["tag"]: s for s in SCENES}
    firsts = {t: lc.restate(by[t])["trace"][0][0] for t in by if t.startswith("t_")}
    for a, b in (("t_minus_1e-3", "t_below_minus_1e-3"), ("t_local_ts", "t_above_local_ts"),
                 ("t_local_te", "t_below_local_te"), ("t_end_plus_1e-3", "t_above_end_plus_1e-3")):
        assert firsts[a] != firsts[b] and lr.LOCAL in (firsts[a], firsts[b]), (a, b)
        assert abs(by[a]["start_t"] - by[b]["start_t"]) <= 2.0 ** -52 * max(1.0, abs(by[a]["start_t"]))  # neighbours
    assert by["time_change_head"]["state"].time_change != 0.0 and by["time_change_head"]["state"].last_time_inc != 0.0
    assert by["no_local_state"]["state"].local_ctrl is None and by["no_local_state"]["state"].local_ts == -1.0
    assert lc.up(by["lookup_on_edge"]["start_t"]) == by["lookup_above_edge"]["start_t"]
    assert len(by["one_segment"]["state"].seg_times) == 1 and by["negative_t"]["start_t"] < 0.0
    assert [lc.restate(by["exit_step_%d" % k])["n_steps"] for k in (1, 63, 64, 65, 128, 129)] == [1, 63, 64, 65, 128, 129]
    assert [lc.restate(by["points_%d" % k])["n_points"] for k in (2, 63, 64, 65, 129)] == [2, 63, 64, 65, 129]
    assert lc.restate(by["over_max_points"])["n_points"] == by["over_max_points"]["max_points"] + 1
    assert [lc.restate(by[t])["seg_num"] for t in ("quotient_6", "quotient_under_7", "quotient_7")] == [6, 6, 7]
    assert {s["degree"] for s in SCENES if s["mode"] == lc.DURATION} == {3, 4, 5}
    assert {s["degree"] for s in SCENES if s["mode"] == lc.SPHERE} == {3, 4, 5}
    assert {lc.restate(s)["status"] for s in SCENES} == {lr.OK, lr.DEGENERATE, lr.NO_LOCAL, -1}
    # what is not recorded is what the reference cannot give
    for s in SCENES:
        if not s["recorded"]:
            assert lc.restate(s)["status"] in (lr.DEGENERATE, lr.NO_LOCAL) or s["tag"] in ("past_total", "t_end_plus_1e-3")
    # the accumulated tp decides: the product k * dt would admit one point more
    d, k = lc.accumulated_edge()
    acc = 0.0
    for _ in range(k):
        acc += 0.1
    assert k * 0.1 <= d + 1e-4 < acc and lc.restate(by["accumulated_tp"])["n_points"] == k


def test_restatement_against_the_recorded_reference():
    """localseg_ref.py against what the reference's own getTrajInfoInSphere / getTrajInfoInDuration computed: all
    integers equal, the doubles within the measured tolerance, under both forms, and no recorded scene left out"""
    measured, tol = lc.parity()
    print("forms disagree by at most %.3e; tolerance %.3e" % (measured, tol))
    assert 0.0 < tol < 1e-12
    worst = 0.0
    for sc in lc.recorded_scenes():
        z = np.load(os.path.join(GOLDEN, sc["tag"] + ".npz"))  # (a missing file is an error: every scene is recorded)
        for lit in (False, True):
            r = lc.restate(sc, literal_pow=lit)
            assert (int(z["n_points"]), int(z["seg_num"])) == (r["n_points"], r["seg_num"]), (sc["tag"], lit)
            rows = len(r["points"])
            assert z["points"].shape == (r["n_points"], 3)
            d = max(abs(float(z["dt"]) - r["dt"]), abs(float(z["duration"]) - r["duration"]),
                    float(np.abs(z["derivs"] - np.array(r["derivs"])).max()),
                    float(np.abs(z["points"][:rows] - np.array(r["points"])).max()))
            assert d <= tol, (sc["tag"], lit, d, tol)
            worst = max(worst, d)
    print("restatement off the recordings by at most %.3e" % worst)
    assert sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz")) == sorted(s["tag"] for s in lc.recorded_scenes())


def test_host_build_of_the_kernel():
    """the kernel's own text, built for the host under the address and undefined-behaviour sanitizers as a stand-alone
    program, on every scene: bit for bit the restatement"""
    script = os.path.join(ROOT, "tests", "golden", "check_localseg_host_build.py")
    p = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "all identical, sanitizers silent" in p.stdout and "DIFFERS" not in p.stdout and "FAILED" not in p.stdout


def _cfg(degree=3, max_seg=4, max_ctrl=8, max_points=16):
    from fuel_amd._lib import LocalSegCfg
    return LocalSegCfg(degree, max_seg, max_ctrl, max_points)


def test_plan_call():
    import fuel_amd
    L = fuel_amd.lib()
    out = (C.c_int * 8)()
    big = _cfg(3, 255, 1024, 1024)
    assert L.fuelmi_localseg_plan(C.byref(big), out) == 0
    lanes, lds, waves, max_seg, max_ctrl, max_points, cap, fit = tuple(out)
    assert (lanes, waves, max_seg, max_ctrl, max_points) == (64, 2, 255, 1024, lr_max_points())
    assert lds == waves * (255 * 19 + 1024 * 3 + 1030) * 8 and lds <= 160 * 1024 and fit <= 160 * 1024
    assert cap == (lr.COUNT_CAP // 64 + 1) * 64 == 2 ** 20 + 64  # the first multiple of 64 above the cap
    assert fuel_amd.SDFMap.localseg_plan(3, 255, 1024, 1024)["lds_bytes"] == lds
    for over in (_cfg(max_seg=256), _cfg(max_ctrl=1025), _cfg(max_points=1025)):
        assert L.fuelmi_localseg_plan(C.byref(over), out) == ELIMIT
    for bad in (_cfg(degree=2), _cfg(degree=6), _cfg(max_seg=0), _cfg(max_ctrl=3), _cfg(degree=5, max_ctrl=5),
                _cfg(max_points=1)):
        assert L.fuelmi_localseg_plan(C.byref(bad), out) == EINVAL
    assert L.fuelmi_localseg_plan(None, out) == EINVAL and L.fuelmi_localseg_plan(C.byref(big), None) == EINVAL


def lr_max_points():
    import fuel_amd
    return fuel_amd._lib.LOCALSEG_MAX_POINTS


def test_refusals_that_need_no_device():
    """every FUELMI_EINVAL / FUELMI_ELIMIT comes before the map is touched: m = NULL"""
    import fuel_amd
    L = fuel_amd.lib()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731
    nt, n = 2, 3
    status = np.zeros(n, np.int32)

    def call(cfg=None, n_traj=nt, n_prob=n, null=(), **kw):
        cfg = cfg if cfg is not None else _cfg()
        ms, mc, mp = max(cfg.max_seg, 1), max(cfg.max_ctrl, 1), max(cfg.max_points, 1)
        a = dict(n_seg=np.array([2, 1], np.int32), seg_times=np.ones((nt, ms)), coef=np.zeros((nt, ms, 3, 6)),
                 gdur=np.array([2.0, 1.0]), n_local=np.array([0, 5], np.int32), local_ctrl=np.zeros((nt, mc, 3)),
                 span=np.array([0.0, 0.25]), lts=np.array([-1.0, 0.2]), lte=np.array([-1.0, 0.7]), tchg=np.zeros(nt),
                 linc=np.zeros(nt), traj_of=np.array([0, 1, 1], np.int32), mode=np.array([0, 1, 0], np.int32),
                 start_t=np.zeros(n), arg0=np.array([1.0, 0.5, 2.0]), arg1=np.array([0.4, 0.1, 0.3]))
        for k, (idx, val) in kw.items():  # one entry of one array changed
            a[k][idx] = val
        o = dict(status=status, n_steps=np.zeros(n, np.int32), segment_len=np.zeros(n), seg_num=np.zeros(n, np.int32),
                 duration=np.zeros(n), dt=np.zeros(n), n_points=np.zeros(n, np.int32), points=np.zeros((n, mp, 3)),
                 derivs=np.zeros((n, 4, 3)), n_ctrl=np.zeros(n, np.int32), ctrl=np.zeros((n, mp + 4, 3)))
        P = lambda k, v: None if k in null else (ip(v) if v.dtype == np.int32 else dp(v))  # noqa: E731
        ins = ("n_seg", "seg_times", "coef", "gdur", "n_local", "local_ctrl", "span", "lts", "lte", "tchg", "linc")
        prs = ("traj_of", "mode", "start_t", "arg0", "arg1")
        outs = ("status", "n_steps", "segment_len", "seg_num", "duration", "dt", "n_points", "points", "derivs", "n_ctrl", "ctrl")
        return L.fuelmi_map_local_segments(None, None if "cfg" in null else C.byref(cfg), n_traj,
                                           *[P(k, a[k]) for k in ins], n_prob, *[P(k, a[k]) for k in prs],
                                           *[P(k, o[k]) for k in outs])

    assert call() == EINVAL and ": m (" in L.fuelmi_last_error().decode()  # everything valid: only the map is missing
    assert call(n_prob=0) == 0
    assert call(cfg=_cfg(max_seg=256)) == ELIMIT and call(cfg=_cfg(max_ctrl=1025)) == ELIMIT
    assert call(cfg=_cfg(max_points=1025), n_prob=0) == ELIMIT
    assert call(gdur=(0, 1.0001e4)) == ELIMIT and "lasts" in L.fuelmi_last_error().decode()
    names = ("cfg", "n_seg", "seg_times", "coef", "gdur", "n_local", "local_ctrl", "span", "lts", "lte", "tchg", "linc",
             "traj_of", "mode", "start_t", "arg0", "arg1", "status", "n_steps", "segment_len", "seg_num", "duration", "dt",
             "n_points", "points", "derivs", "n_ctrl", "ctrl")
    bad = [dict(null=(k,)) for k in names] + \
        [dict(cfg=_cfg(degree=2)), dict(cfg=_cfg(degree=6)), dict(cfg=_cfg(max_points=1)), dict(cfg=_cfg(max_seg=0)),
         dict(n_seg=(0, 0)), dict(n_seg=(1, 5)), dict(n_local=(1, 3)), dict(n_local=(1, 9)), dict(n_local=(0, -1)),
         dict(cfg=_cfg(degree=4), n_local=(1, 4)), dict(span=(1, 0.0)), dict(span=(1, -0.25)), dict(span=(1, np.nan)),
         dict(traj_of=(2, 2)), dict(traj_of=(0, -1)), dict(mode=(1, 2)), dict(mode=(0, -1)),
         dict(seg_times=((0, 1), np.inf)), dict(seg_times=((0, 0), 1e7)), dict(coef=((0, 1, 2, 5), np.nan)),
         dict(coef=((1, 0, 0, 0), -1e7)), dict(gdur=(1, np.nan)), dict(local_ctrl=((1, 4, 2), np.inf)),
         dict(local_ctrl=((1, 0, 0), 1e7)), dict(lts=(0, np.nan)), dict(lte=(1, np.inf)), dict(tchg=(0, 1e7)),
         dict(linc=(1, -np.inf)), dict(start_t=(2, np.nan)), dict(start_t=(0, -1e7)), dict(arg0=(1, np.inf)),
         dict(arg1=(1, np.nan)), dict(arg0=(0, 0.0)), dict(arg0=(2, -1.0)), dict(arg1=(0, 0.0)), dict(arg1=(2, -0.5)),
         dict(n_prob=-1), dict(n_traj=0)]
    for kw in bad:
        status[:] = 77
        assert call(**kw) == EINVAL, kw
        assert ": m (" not in L.fuelmi_last_error().decode(), kw
        assert np.all(status == 77), kw
    # what is NOT refused: values behind a state's own rows, a span without a local spline, DURATION with dt <= 0
    for kw in (dict(seg_times=((1, 1), np.nan)), dict(coef=((1, 1, 0, 0), np.inf)), dict(local_ctrl=((0, 0, 0), np.nan)),
               dict(local_ctrl=((1, 5, 0), 1e9)), dict(span=(0, -1.0)), dict(arg1=(1, 0.0)), dict(arg0=(1, -1.0)),
               dict(gdur=(0, 1e4))):
        assert call(**kw) == EINVAL and ": m (" in L.fuelmi_last_error().decode(), kw


def test_new_symbols_exported_and_declared():
    import fuel_amd
    header = open(os.path.join(ROOT, "include", "fuelmi.h")).read()
    L = fuel_amd.lib()
    exported = subprocess.run(["nm", "-D", "--defined-only", fuel_amd.LIB_PATH], check=True, capture_output=True,
                              text=True).stdout
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert getattr(L, name) is not None and name in fuel_amd._lib.SYMBOLS
        assert re.search(r"\bT %s\b" % name, exported), name
    lib = fuel_amd._lib
    for word, val in (("FUELMI_LOCALSEG_SPHERE", lr.SPHERE), ("FUELMI_LOCALSEG_DURATION", lr.DURATION),
                      ("FUELMI_LOCALSEG_OK", lr.OK), ("FUELMI_LOCALSEG_DEGENERATE", lr.DEGENERATE),
                      ("FUELMI_LOCALSEG_NO_LOCAL", lr.NO_LOCAL), ("FUELMI_LOCALSEG_MISFIT", lr.MISFIT),
                      ("FUELMI_LOCALSEG_MAX_POINTS", lib.LOCALSEG_MAX_POINTS)):
        m = re.search(r"#define %s\s+(\d+)" % word, header)
        assert m and int(m.group(1)) == val, word
    assert (lib.LOCALSEG_SPHERE, lib.LOCALSEG_DURATION, lib.LOCALSEG_OK, lib.LOCALSEG_DEGENERATE, lib.LOCALSEG_NO_LOCAL,
            lib.LOCALSEG_MISFIT) == (lr.SPHERE, lr.DURATION, lr.OK, lr.DEGENERATE, lr.NO_LOCAL, lr.MISFIT)
    assert re.search(r"#define FUELMI_WPTRAJ_MAX_SEG \(1 << 20\)", header) and lr.MAX_SEG == 1 << 20
    # the polynomial's evaluation and the derivative levels live in one place each
    csrc = os.path.join(ROOT, "fuel_amd", "csrc")
    wp, ls, ts = (open(os.path.join(csrc, f)).read() for f in ("waypoint_traj.hip", "local_segment.hip", "traj_sample.hip"))
    assert "poly_eval(" in wp and "poly_eval(" in ls and "T[idx] + 1e-4 < ts" not in wp + ls
    assert open(os.path.join(csrc, "poly_internal.h")).read().count("T[idx] + 1e-4 < ts") == 1
    assert "spline_eval_levels<" in ts and "spline_eval_levels<" in ls and "spline_derive<" not in ts + ls
