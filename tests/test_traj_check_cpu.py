"""The restatement of checkTrajCollision (tests/traj_check_ref.py) and the scenes of tests/traj_check_cases.py checked on
the host, and the host side of the new calls: every scene sits on the edge it is drawn for (its predicate) and gives the
outputs it is drawn for; the literal loop and the first-hit form agree on every scene, at any window size; the point
evaluation (scalar and windowed) equals the real NonUniformBspline bit for bit through ref_spline_evaluate of oracle/_ref,
where that was built, and the duration its getTimeSum; the numpy inflation the predicates read equals the oracle's;
fuelmi_traj_check_plan, the exported symbols and every refusal that needs no device."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import traj_check_cases as tc
import traj_check_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NEW_SYMBOLS = ("fuelmi_map_check_trajs", "fuelmi_bspline_dev_check_trajs", "fuelmi_traj_check_plan")
QUICK = tc.quick_scenes()


@pytest.mark.parametrize("sc", QUICK, ids=[s["tag"] for s in QUICK])
def test_scene_reaches_its_edge(sc):
    s = tc.scene_samples(sc)
    assert sc["pred"](s, tc.spec(sc["map"]).grid(), sc), sc["tag"]
    lit, fh = tc.restate(sc, "literal"), tc.restate(sc, "first_hit")
    for k, v in sc["expect"].items():
        assert lit[k] == v, (sc["tag"], k, lit[k], v)
    assert lit == fh, (sc["tag"], lit, fh)
    for width in (1, 7, 4096):  # the window is the device's layout, not part of the result
        assert tc.restate(sc, "first_hit", width=width) == lit, (sc["tag"], width)
    assert 4 <= len(sc["ctrl"]) <= 40


def test_scene_list_covers_the_issue():
    tags = {s["tag"] for s in QUICK}
    assert {"hit_%d" % k for k in (1, 63, 64, 65, 128, 129)} <= tags
    assert {"face_%s%s" % (a, s) for a in "xyz" for s in "-+"} <= tags
    hits = {s["tag"]: tc.restate(s) for s in QUICK if s["tag"].startswith("hit_")}
    # a hit in lane 0 of a window takes its distance from lane 63 of the window before: r_64 and r_128
    assert hits["hit_65"]["distance"] == float(tc.scene_samples(tc.hit_scene(65))["r"][63]) > 0.0
    assert hits["hit_129"]["distance"] == float(tc.scene_samples(tc.hit_scene(129))["r"][127]) > 0.0
    assert hits["hit_1"]["distance"] == 0.0
    assert {len(s["ctrl"]) for s in QUICK} >= {4, 5, 6, 40}
    assert {s["degree"] for s in QUICK} == {3, 4, 5} and {s["map"] for s in QUICK} == {"a", "b"}
    # map b's origin is off its voxel grid, map a's is on it
    assert not float(tc.spec("b").origin[2] * tc.spec("b").res_inv).is_integer()
    assert all(float(v * tc.spec("a").res_inv).is_integer() for v in tc.spec("a").origin)


def test_cap_scenes():
    """the two walks of 2^20 samples: the first-hit form at the real cap (the literal loop in Python would take minutes);
    literal = first-hit with the cap lowered to 300 bodies, where the same three outcomes exist"""
    cap, exact = tc.long_scenes()
    for sc in (cap, exact):
        assert sc["pred"](None, None, sc)
        got = tc.restate(sc, "first_hit", width=8192)
        for k, v in sc["expect"].items():
            assert got[k] == v, (sc["tag"], k, got[k], v)
    small = 300
    dur = tc.duration_of(40, 3, 30.0)
    for t_now, want in ((0.0, (tr.OVER, 0, small, tr.END_CAP)),
                        (dur - (small + 0.5) * tc.CAP_STEP, (tr.OK, 1, small, tr.END_DURATION)),
                        (dur - (small - 0.5) * tc.CAP_STEP, (tr.OK, 1, small - 1, tr.END_DURATION))):
        sc = tc.scene("cap_small", "a", tc.still(40), 30.0, t_now=t_now, step=tc.CAP_STEP)
        lit, fh = tc.restate(sc, "literal", cap=small), tc.restate(sc, "first_hit", cap=small)
        assert lit == fh and (lit["status"], lit["safe"], lit["n_samples"], lit["end_reason"]) == want, (t_now, lit)


def test_nonfinite_in_the_walk():
    """a point that turns bad in mid-walk (a device batch can hold one: the host route's inputs cannot produce it): both
    forms report the sample, and an inflated voxel behind it is never reached"""
    m = tc.spec("a")
    ctrl = tc.line((tc.BAND_X - 0.6, tc.HIT_Y, tc.HIT_Z), (1, 0, 0), 16)
    ctrl[6, 0] = 2.0e7  # the fourth span's points leave the admitted range (max_radius is out of their way)
    lit = tr.check_literal(m.grid(), ctrl, 3, tc.DT, 0.0, max_radius=1e9)
    fh = tr.check_first_hit(m.grid(), ctrl, 3, tc.DT, 0.0, max_radius=1e9)
    assert lit == fh and lit["status"] == tr.NONFINITE and lit["safe"] == 0 and lit["distance"] == 0.0
    assert lit["n_samples"] == lit["hit_index"] > 1 and lit["end_reason"] == tr.END_NONFINITE and lit["hit_pos"] == [0.0] * 3
    ctrl[:, 0] = np.nan
    lit = tr.check_literal(m.grid(), ctrl, 3, tc.DT, 0.0)
    assert lit == tr.check_first_hit(m.grid(), ctrl, 3, tc.DT, 0.0) and lit["n_samples"] == 0 and lit["status"] == tr.NONFINITE
    for dt in (0.0, -1.0, float("inf"), float("nan")):
        lit = tr.check_literal(m.grid(), tc.still(8), 3, dt, 0.0)
        assert lit == tr.check_first_hit(m.grid(), tc.still(8), 3, dt, 0.0) and lit["duration"] == 0.0


@pytest.mark.parametrize("name", ["a", "b"])
def test_numpy_inflation_is_the_oracles(name):
    from oracle import fuel_oracle as fo
    m = tc.spec(name)
    om = fo.OracleMap(m.map_size, **m.kw)
    assert om.nvox == m.nvox and np.array_equal(om.origin, m.origin)
    om.occ[:] = m.occ3.reshape(-1)
    om.set_local_bound((0, 0, 0), tuple(v - 1 for v in om.nvox))
    om.inflate_local()
    assert np.array_equal(om.infl.reshape(m.nvox), m.infl3)
    assert m.infl3.sum() >= 125 * len(m.occupied) // 2 and (m.occ3 > 0).sum() == len(m.occupied)
    if name == "b":  # every face has its inflated border voxel
        for a in range(3):
            for s in (0, 1):
                assert m.infl3[tc.face_voxel(m.nvox, a, s)] == 1


def test_deboor_against_the_real_spline():
    from oracle.ref_build import ref
    if not ref.available():
        pytest.skip("oracle/_ref was not built here")
    L = C.CDLL(ref.SO)
    dp = C.POINTER(C.c_double)
    L.ref_spline_evaluate.restype = None
    L.ref_spline_evaluate.argtypes = [dp, C.c_int, C.c_int, C.c_double, C.c_int, dp, C.c_int, dp]
    L.ref_spline_duration.restype = C.c_double
    L.ref_spline_duration.argtypes = [C.c_int, C.c_int, C.c_double]
    seen = 0
    for sc in QUICK:
        if sc["tag"] == "nonfinite":
            continue
        ctrl, p, dt = np.ascontiguousarray(sc["ctrl"]), sc["degree"], sc["dt"]
        n = len(ctrl)
        s = tc.scene_samples(sc)
        assert L.ref_spline_duration(n, p, dt) == s["duration"]
        t = np.ascontiguousarray(np.concatenate([[sc["t_now"]], s["t"][:200], [-0.3, 0.0, s["duration"], s["duration"] + 0.3]]))
        out = np.zeros((len(t), 3))
        L.ref_spline_evaluate(ctrl.ctypes.data_as(dp), n, p, dt, 0, t.ctypes.data_as(dp), len(t), out.ctypes.data_as(dp))
        one = np.array([tr.deboor(s["u"], p, ctrl, float(tk)) for tk in t])
        many = tr.deboor_many(s["u"], p, ctrl, t)
        assert np.array_equal(one, out), (sc["tag"], np.abs(one - out).max())
        assert np.array_equal(many, out), (sc["tag"], np.abs(many - out).max())
        assert np.array_equal(np.array(s["cur"]), out[0]) and np.array_equal(s["pos"][:200], out[1:1 + len(s["t"][:200])])
        seen += 1
    assert seen >= 30


def _cfg(**kw):
    from fuel_amd.host import traj_check_cfg
    return traj_check_cfg(**kw)


def test_plan_call():
    import fuel_amd
    L = fuel_amd.lib()
    out = (C.c_int * 3)()
    big = _cfg(max_ctrl=1024)
    assert L.fuelmi_traj_check_plan(C.byref(big), out) == 0
    lanes, lds, cap = tuple(out)
    assert cap == fuel_amd._lib.TRAJCHK_MAX_CTRL == 1024 and lanes == 64 and 0 < lds <= 64 * 1024 and lds % 16 == 0
    assert lds % ((1024 + 6) * 8) == 0  # whole waves, each with the knots of its own problem: n + p + 1 <= max_ctrl + 6
    assert fuel_amd.SDFMap.traj_check_plan(big) == (lanes, lds, cap)
    assert L.fuelmi_traj_check_plan(C.byref(_cfg(max_ctrl=40)), out) == 0 and 0 < out[1] < lds
    assert L.fuelmi_traj_check_plan(C.byref(_cfg(degree=5, max_ctrl=6)), out) == 0
    assert L.fuelmi_traj_check_plan(C.byref(_cfg(step=1e-3, max_radius=1e-300)), out) == 0
    EINVAL, ELIMIT = -1, -5
    assert L.fuelmi_traj_check_plan(C.byref(_cfg(max_ctrl=1025)), out) == ELIMIT
    assert "max_ctrl" in L.fuelmi_last_error().decode()
    for bad in (dict(max_ctrl=3), dict(degree=5, max_ctrl=5), dict(degree=2), dict(degree=6, max_ctrl=8),
                dict(step=0.99e-3), dict(step=0.0), dict(step=-0.02), dict(step=float("nan")), dict(step=float("inf")),
                dict(max_radius=0.0), dict(max_radius=-6.0), dict(max_radius=float("nan")), dict(max_radius=float("inf"))):
        assert L.fuelmi_traj_check_plan(C.byref(_cfg(**bad)), out) == EINVAL, bad
    assert L.fuelmi_traj_check_plan(None, out) == EINVAL
    assert L.fuelmi_traj_check_plan(C.byref(big), None) == EINVAL


def test_refusals_that_need_no_device():
    """every FUELMI_EINVAL / FUELMI_ELIMIT of fuelmi_map_check_trajs comes before the map is touched: m = NULL"""
    import fuel_amd
    L = fuel_amd.lib()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731
    n = 2
    outs = dict(status=np.zeros(n, np.int32), safe=np.zeros(n, np.int32), distance=np.zeros(n), ns=np.zeros(n, np.int32),
                hi=np.zeros(n, np.int32), ht=np.zeros(n), hp=np.zeros((n, 3)), er=np.zeros(n, np.int32), dur=np.zeros(n))

    def call(cfg=None, n_prob=n, n_ctrl=(11, 4), pos=None, knot=(0.4, 0.5), now=(0.0, 1.0), null=()):
        cfg = cfg if cfg is not None else _cfg(max_ctrl=11)
        a = dict(n_ctrl=np.array(n_ctrl, dtype=np.int32), pos=np.zeros((n, max(cfg.max_ctrl, 1), 3)) if pos is None else pos,
                 knot=np.array(knot, dtype=np.float64), now=np.array(now, dtype=np.float64))
        ptr = {k: (None if k in null else (ip(v) if v.dtype == np.int32 else dp(v))) for k, v in a.items()}
        o = {k: (None if k in null else (ip(v) if v.dtype == np.int32 else dp(v))) for k, v in outs.items()}
        return L.fuelmi_map_check_trajs(None, None if "cfg" in null else C.byref(cfg), n_prob, ptr["n_ctrl"], ptr["pos"],
                                        ptr["knot"], ptr["now"], o["status"], o["safe"], o["distance"], o["ns"], o["hi"],
                                        o["ht"], o["hp"], o["er"], o["dur"])

    EINVAL, ELIMIT = -1, -5
    assert call() == EINVAL and ": m (" in L.fuelmi_last_error().decode()  # everything valid: only the map is missing
    assert call(n_prob=0) == 0
    assert call(cfg=_cfg(max_ctrl=1025), n_prob=0) == ELIMIT
    assert call(cfg=_cfg(max_ctrl=1025)) == ELIMIT
    bad = np.zeros((n, 11, 3))
    bad[1, 3, 2] = np.nan
    far = np.zeros((n, 11, 3))
    far[0, 10, 0] = 1e7
    beyond = np.zeros((n, 11, 3))
    beyond[1, 4, 0] = np.inf  # past n_ctrl[1] = 4: not read
    for kw in (dict(null=("cfg",)), dict(null=("n_ctrl",)), dict(null=("pos",)), dict(null=("knot",)), dict(null=("now",)),
               dict(null=("status",)), dict(null=("safe",)), dict(null=("distance",)), dict(null=("ns",)),
               dict(null=("hi",)), dict(null=("ht",)), dict(null=("hp",)), dict(null=("er",)), dict(null=("dur",)),
               dict(cfg=_cfg(degree=2, max_ctrl=11)), dict(cfg=_cfg(degree=6, max_ctrl=11)),
               dict(n_ctrl=(11, 3)), dict(n_ctrl=(12, 4)), dict(cfg=_cfg(degree=4, max_ctrl=11)),
               dict(knot=(0.4, 0.0)), dict(knot=(-0.1, 0.5)), dict(knot=(np.inf, 0.5)), dict(knot=(0.4, np.nan)),
               dict(pos=bad), dict(pos=far), dict(now=(0.0, np.nan)), dict(now=(np.inf, 0.0)), dict(now=(-np.inf, 0.0)),
               dict(cfg=_cfg(max_ctrl=11, step=0.5e-3)), dict(cfg=_cfg(max_ctrl=11, step=np.nan)),
               dict(cfg=_cfg(max_ctrl=11, max_radius=0.0)), dict(cfg=_cfg(max_ctrl=11, max_radius=np.inf)),
               dict(n_prob=-1)):
        outs["status"][:] = 77
        assert call(**kw) == EINVAL, kw
        assert ": m (" not in L.fuelmi_last_error().decode(), kw
        assert np.all(outs["status"] == 77), kw
    # accepted up to the map: the limits themselves, and garbage past a problem's own control points
    for kw in (dict(pos=beyond), dict(now=(-1e300, 1e300)), dict(knot=(1e308, 5e-324)),
               dict(cfg=_cfg(max_ctrl=11, step=1e-3, max_radius=1e-300)), dict(cfg=_cfg(degree=5, max_ctrl=11), n_ctrl=(11, 6)),
               dict(cfg=_cfg(max_ctrl=1024), pos=np.zeros((n, 1024, 3)))):
        assert call(**kw) == EINVAL and ": m (" in L.fuelmi_last_error().decode(), kw


def test_new_symbols_exported_and_declared():
    import fuel_amd
    header = open(os.path.join(ROOT, "include", "fuelmi.h")).read()
    L = fuel_amd.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert getattr(L, name) is not None and name in fuel_amd._lib.SYMBOLS
    for word in ("FUELMI_TRAJCHK_OK", "FUELMI_TRAJCHK_NONFINITE", "FUELMI_TRAJCHK_END_HIT", "FUELMI_TRAJCHK_END_RADIUS",
                 "FUELMI_TRAJCHK_END_DURATION", "FUELMI_TRAJCHK_END_CAP", "FUELMI_TRAJCHK_END_NONFINITE", "fuelmi_trajchk_cfg"):
        assert word in header, word
    exported = subprocess.run(["nm", "-D", "--defined-only", fuel_amd.LIB_PATH], check=True, capture_output=True,
                              text=True).stdout
    for name in NEW_SYMBOLS:
        assert re.search(r"\bT %s\b" % name, exported), name
    for word, val in (("FUELMI_TRAJCHK_MAX_CTRL", fuel_amd._lib.TRAJCHK_MAX_CTRL),
                      ("FUELMI_TRAJCHK_MAX_SAMPLES", fuel_amd._lib.TRAJCHK_MAX_SAMPLES), ("FUELMI_TRAJCHK_MAX_SAMPLES", tr.CAP)):
        m = re.search(r"#define %s\s+(\d+)" % word, header)
        assert m and int(m.group(1)) == val
    for word, val in (("OK", tr.OK), ("NONFINITE", tr.NONFINITE), ("END_HIT", tr.END_HIT), ("END_RADIUS", tr.END_RADIUS),
                      ("END_DURATION", tr.END_DURATION), ("END_CAP", tr.END_CAP), ("END_NONFINITE", tr.END_NONFINITE)):
        m = re.search(r"#define FUELMI_TRAJCHK_%s\s+(\d+)" % word, header)
        assert m and int(m.group(1)) == val == getattr(fuel_amd._lib, "TRAJCHK_" + word)
    # the facade and its driver
    hdr = open(os.path.join(ROOT, "fuel_amd", "facade", "bspline_opt", "bspline_optimizer.h")).read()
    assert "bool checkTrajCollision(const Eigen::MatrixXd& pos_ctrl, int degree, double dt, double t_now, double& distance);" in hdr
    assert os.access(os.path.join(ROOT, "fuel_amd", "facade", "facade_trajcheck"), os.X_OK)
