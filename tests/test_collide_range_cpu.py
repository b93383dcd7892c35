"""The collision ranges and guide points of guided replanning, without a GPU: every scene of tests/collide_cases.py is
proven to sit on the edge it is drawn for (its predicate, on the restatement tests/collide_ref.py over the f64 field); the
scene lists cover the issue; the cut that carries the reference's strict f64 comparison onto f32 values; the restatement
against the recordings of the reference's own functions (tests/golden/collide/*.npz, tests/golden/make_collide_golden.py);
the host build of the two kernels' own text under the address and undefined-behaviour sanitizers
(tests/golden/check_collide_host_build.py); fuelmi_colrange_plan, the exported symbols and every refusal that needs no
device."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import collide_cases as cc
import collide_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "collide")
SCENES = cc.collision_scenes()
GUIDES = cc.guide_scenes()
NEW_SYMBOLS = ("fuelmi_map_collision_ranges", "fuelmi_colrange_plan", "fuelmi_map_guide_points")
_REF = {}


def ref(sc):
    if sc["tag"] not in _REF:
        _REF[sc["tag"]] = cc.restate(sc)
    return _REF[sc["tag"]]


@pytest.mark.parametrize("sc", SCENES, ids=[s["tag"] for s in SCENES])
def test_scene_reaches_its_edge(sc):
    r = ref(sc)
    for k, v in sc["expect"].items():
        assert r[k] == v, (sc["tag"], k, r[k], v)
    assert sc["pred"](r, sc), sc["tag"]
    # what the device does (the cut, on the f32 rounding of the field and on that moved by 2 ulp) decides like the f64 field
    m = cc.spec(sc["map"])
    for ulp in (-2, 0, 2):
        d32 = (m.f32().view(np.int32) + np.where(m.f32() > 0, ulp, 0).astype(np.int32)).view(np.float32)
        got = cc.restate(sc, field=m.field("cut", d32))
        assert [t[2] for t in got["ticks"]] == [t[2] for t in r["ticks"]], (sc["tag"], ulp)


@pytest.mark.parametrize("sc", GUIDES, ids=[s["tag"] for s in GUIDES])
def test_guide_scene_reaches_its_edge(sc):
    r = cc.grestate(sc)
    for k, v in sc["expect"].items():
        assert r[k] == v, (sc["tag"], k, r[k], v)
    assert sc["pred"](r, sc), sc["tag"]


def test_scene_list_covers_the_issue():
    tags = [s["tag"] for s in SCENES]
    assert len(set(tags)) == len(tags)
    for edge, names in cc.COVERAGE.items():
        for n in names:
            assert n in tags, (edge, n)
    assert {s["degree"] for s in SCENES} == {3, 4, 5}
    sizes = {(s["degree"], len(s["ctrl"])) for s in SCENES}
    assert (3, 4) in sizes and max(n for _, n in sizes) >= 24  # n_ctrl = degree + 1, mid sizes, the batch's max_ctrl
    gtags = [s["tag"] for s in GUIDES]
    assert len(set(gtags)) == len(gtags)
    for edge, names in cc.GUIDE_COVERAGE.items():
        for n in names:
            assert n in gtags, (edge, n)
    over_ev, over_pts = cc.limit_scenes()
    for sc in (over_ev, over_pts):
        r = cc.restate(sc)
        for k, v in sc["expect"].items():
            assert r[k] == v, (sc["tag"], k, r[k], v)
    assert cc.restate(over_ev)["n_start_events"] > over_ev["max_events"]
    assert cc.restate(over_pts)["n_start_pts"] > over_pts["max_pts"] and len(cc.restate(over_pts)["start_pts"]) == over_pts["max_pts"]
    nan = cc.nonfinite_scene()
    assert cc.restate(nan)["status"] == cr.NONFINITE and np.isnan(nan["ctrl"]).sum() == 1


def test_strict_cut():
    """res 0.1, clearance 0.8: 0.1 * sqrt(64) = 0.8 is not < 0.8, the largest k that is unsafe is 63 -- a value no voxel
    holds (not a sum of three squares) -- and the cut lies between the f32 values of 63 and 64"""
    assert 0.1 * math.sqrt(64) == 0.8
    assert cr.kmax_strict(0.1, 0.8) == 63 and not any(a * a + b * b + c * c == 63 for a in range(8) for b in range(8) for c in range(8))
    cut = cr.cut_strict(0.1, 0.8)
    f = lambda k: np.float32(0.1) * np.sqrt(np.float32(k))  # noqa: E731
    assert f(63) < cut < f(64)
    assert cr.kmax_strict(0.1, 0.0) == -1 and cr.cut_strict(0.1, 0.0) == np.float32(-1.0)  # nothing is < 0
    assert cr.kmax_strict(0.1, 0.2) == 3 and cr.kmax_strict(0.1, 0.2000001) == 4
    for res in (0.1, 0.15, 0.05):
        for k in range(0, 200):
            c = res * math.sqrt(k)
            assert cr.kmax_strict(res, c) == k - 1, (res, k)  # equality is safe
            assert cr.kmax_strict(res, math.nextafter(c, math.inf)) == k or k == 0


def test_plain_f32_comparison_disagrees():
    a, b, k, c = cc.f32_disagreement()
    d32 = np.float32(0.1) * np.sqrt(np.float32(k))
    assert not 0.1 * math.sqrt(k) < c and float(d32) < c and not d32 <= cr.cut_strict(0.1, c)
    sc = next(s for s in SCENES if s["tag"] == "f32_disagrees")
    r64, r32, rcut = cc.restate(sc), cc.restate(sc, mode="f32"), cc.restate(sc, mode="cut")
    assert cc.first_unsafe(r32) < cc.first_unsafe(r64) == cc.first_unsafe(rcut)
    assert r32["t_s"] != r64["t_s"] and rcut["t_s"] == r64["t_s"]


def _bits(a):
    a = np.ascontiguousarray(a, dtype=np.float64).copy()
    a[np.isnan(a)] = np.nan  # a generated NaN is one NaN: its sign is the processor's choice
    return a.tobytes()


def test_restatement_against_the_recorded_reference():
    """collide_ref.py against what the reference's own findCollisionRange / pathLength / pathToGuidePts /
    getTrajInfoInDuration computed for the scenes, bit for bit"""
    names = [s["tag"] for s in SCENES] + ["guide_" + s["tag"] for s in GUIDES if s["tag"] not in cc_not_recorded()]
    missing = [n for n in names if not os.path.exists(os.path.join(GOLDEN, n + ".npz"))]
    if missing:
        pytest.skip("tests/golden/collide has no recording of %s: run tests/golden/make_collide_golden.py (it needs the "
                    "reference's sources)" % ", ".join(missing[:4]))
    for sc in SCENES:
        z = np.load(os.path.join(GOLDEN, sc["tag"] + ".npz"))
        r = ref(sc)
        assert int(z["n_ticks"]) == r["n_ticks"], sc["tag"]
        for key in ("colli_start", "colli_end", "start_pts", "end_pts"):
            assert _bits(z[key].reshape(-1, 3)) == _bits(np.array(r[key], dtype=np.float64).reshape(-1, 3)), (sc["tag"], key)
        # (t_s and t_e are locals of the reference's function: start_pts and end_pts, which they shape, stand for them)
    for sc in GUIDES:
        if sc["tag"] in cc_not_recorded():
            continue
        z = np.load(os.path.join(GOLDEN, "guide_" + sc["tag"] + ".npz"))
        r = cc.grestate(sc)
        assert (int(z["seg_num"]), int(z["n_pts"]), int(z["n_ctrl"])) == (r["seg_num"], r["n_pts"], r["n_ctrl"]), sc["tag"]
        assert _bits(z["dt"]) == _bits(r["dt"]) and _bits(z["guide_pts"].reshape(-1, 3)) == \
            _bits(np.array(r["guide_pts"], dtype=np.float64).reshape(-1, 3)), sc["tag"]


def cc_not_recorded():
    """the reference indexes with -1 there: undefined behaviour, nothing to record"""
    return ("no_segment", "one_point")


def test_host_build_of_the_kernels():
    """the two kernels' own text, built for the host under the address and undefined-behaviour sanitizers as a
    stand-alone program, on every scene: bit for bit the restatement"""
    script = os.path.join(ROOT, "tests", "golden", "check_collide_host_build.py")
    if not os.path.exists(script):
        pytest.skip("tests/golden/check_collide_host_build.py is not part of this tree")
    p = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "identical" in p.stdout and "DIFFERS" not in p.stdout and "FAILED" not in p.stdout


def _cfg(**kw):
    from fuel_amd.host import colrange_cfg
    return colrange_cfg(**kw)


def test_plan_call():
    import fuel_amd
    L = fuel_amd.lib()
    out = (C.c_int * 6)()
    big = _cfg(max_ctrl=1024)
    assert L.fuelmi_colrange_plan(C.byref(big), out) == 0
    lanes, lds, waves, ticks, max_ctrl, max_pts = tuple(out)
    assert (lanes, waves, ticks, max_ctrl, max_pts) == (64, 4, cr.CAP, 1024, 64)
    assert lds == waves * (1024 + 6) * 8 and lds <= 64 * 1024
    assert fuel_amd.SDFMap.colrange_plan(big) == dict(lanes=64, lds_bytes=lds, waves=4, max_ticks=cr.CAP, max_ctrl=1024, max_pts=64)
    assert ticks % lanes == 0
    EINVAL, ELIMIT = -1, -5
    for over in (dict(max_ctrl=1025), dict(max_events=4097), dict(max_pts=65)):
        assert L.fuelmi_colrange_plan(C.byref(_cfg(**over)), out) == ELIMIT, over
    for bad in (dict(degree=2), dict(degree=6, max_ctrl=8), dict(max_ctrl=3), dict(degree=5, max_ctrl=5), dict(clearance=-0.1),
                dict(clearance=float("nan")), dict(clearance=float("inf")), dict(max_events=0), dict(max_pts=0)):
        assert L.fuelmi_colrange_plan(C.byref(_cfg(**bad)), out) == EINVAL, bad
    assert L.fuelmi_colrange_plan(None, out) == EINVAL and L.fuelmi_colrange_plan(C.byref(big), None) == EINVAL
    assert L.fuelmi_colrange_plan(C.byref(_cfg(clearance=0.0)), out) == 0


def test_refusals_that_need_no_device():
    """every FUELMI_EINVAL / FUELMI_ELIMIT of both calls comes before the map is touched: m = NULL"""
    import fuel_amd
    L = fuel_amd.lib()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731
    EINVAL, ELIMIT = -1, -5
    n = 2
    ints = {k: np.zeros(n, np.int32) for k in ("status", "n_ticks", "nse", "nee", "nsp", "nep")}

    def call(cfg=None, n_prob=n, n_ctrl=(11, 4), pos=None, knot=(0.4, 0.5), null=()):
        cfg = cfg if cfg is not None else _cfg(max_ctrl=11)
        pos = np.zeros((n, max(cfg.max_ctrl, 1), 3)) if pos is None else pos
        d = dict(ts=np.zeros(n), te=np.zeros(n), cs=np.zeros((n, 8, 3)), ce=np.zeros((n, 8, 3)), sp=np.zeros((n, 64, 3)),
                 ep=np.zeros((n, 64, 3)), fs=np.zeros((n, 3)), le=np.zeros((n, 3)))
        nc, kn = np.array(n_ctrl, dtype=np.int32), np.array(knot, dtype=np.float64)
        P = lambda k, v: None if k in null else (ip(v) if v.dtype == np.int32 else dp(v))  # noqa: E731
        return L.fuelmi_map_collision_ranges(
            None, None if "cfg" in null else C.byref(cfg), n_prob, P("n_ctrl", nc), P("pos", pos), P("knot", kn),
            P("status", ints["status"]), P("n_ticks", ints["n_ticks"]), P("nse", ints["nse"]), P("nee", ints["nee"]),
            P("ts", d["ts"]), P("te", d["te"]), P("cs", d["cs"]), P("ce", d["ce"]), P("nsp", ints["nsp"]), P("sp", d["sp"]),
            P("nep", ints["nep"]), P("ep", d["ep"]), P("fs", d["fs"]), P("le", d["le"]))

    assert call() == EINVAL and ": m (" in L.fuelmi_last_error().decode()  # everything valid: only the map is missing
    assert call(n_prob=0) == 0
    assert call(cfg=_cfg(max_ctrl=1025)) == ELIMIT and call(cfg=_cfg(max_ctrl=11, max_pts=65), n_prob=0) == ELIMIT
    far = np.zeros((n, 11, 3))
    far[0, 10, 0] = -1e7
    nan = np.zeros((n, 11, 3))
    nan[1, 2, 1] = np.nan  # not finite: the kernel's FUELMI_COLRANGE_NONFINITE, not a refusal
    for kw in [dict(null=(k,)) for k in ("cfg", "n_ctrl", "pos", "knot", "status", "n_ticks", "nse", "nee", "ts", "te", "cs",
                                         "ce", "nsp", "sp", "nep", "ep", "fs", "le")] + \
            [dict(cfg=_cfg(degree=2, max_ctrl=11)), dict(cfg=_cfg(degree=6, max_ctrl=11)), dict(n_ctrl=(11, 3)),
             dict(n_ctrl=(12, 4)), dict(cfg=_cfg(degree=4, max_ctrl=11)), dict(knot=(0.4, 0.0)), dict(knot=(-0.1, 0.5)),
             dict(pos=far), dict(cfg=_cfg(max_ctrl=11, clearance=-1e-9)), dict(cfg=_cfg(max_ctrl=11, clearance=np.nan)),
             dict(cfg=_cfg(max_ctrl=11, clearance=np.inf)), dict(cfg=_cfg(max_ctrl=11, max_events=0)),
             dict(cfg=_cfg(max_ctrl=11, max_pts=0)), dict(n_prob=-1)]:
        ints["status"][:] = 77
        assert call(**kw) == EINVAL, kw
        assert ": m (" not in L.fuelmi_last_error().decode(), kw
        assert np.all(ints["status"] == 77), kw
    for kw in (dict(pos=nan), dict(knot=(np.inf, 0.5)), dict(knot=(0.4, np.nan)), dict(cfg=_cfg(max_ctrl=11, clearance=0.0)),
               dict(cfg=_cfg(degree=5, max_ctrl=11), n_ctrl=(11, 6))):
        assert call(**kw) == EINVAL and ": m (" in L.fuelmi_last_error().decode(), kw

    gi = {k: np.zeros(n, np.int32) for k in ("status", "seg", "npts", "nctrl", "ng")}

    def gcall(n_path=n, mpp=4, plen=(4, 2), dur=(3.0, 2.0), dist=0.5, degree=3, max_guide=16, null=()):
        a = dict(paths=np.zeros((n, max(mpp, 1), 3)), plen=np.array(plen, dtype=np.int32), dur=np.array(dur, dtype=np.float64),
                 dt=np.zeros(n), gp=np.zeros((n, max(max_guide, 1), 3)))
        P = lambda k, v: None if k in null else (ip(v) if v.dtype == np.int32 else dp(v))  # noqa: E731
        return L.fuelmi_map_guide_points(None, n_path, mpp, P("paths", a["paths"]), P("plen", a["plen"]), P("dur", a["dur"]),
                                         dist, degree, max_guide, P("status", gi["status"]), P("seg", gi["seg"]),
                                         P("dt", a["dt"]), P("npts", gi["npts"]), P("nctrl", gi["nctrl"]), P("ng", gi["ng"]),
                                         P("gp", a["gp"]))

    assert gcall() == EINVAL and ": m (" in L.fuelmi_last_error().decode()
    assert gcall(n_path=0) == 0
    assert gcall(mpp=257) == ELIMIT and gcall(max_guide=65537) == ELIMIT
    for kw in [dict(null=(k,)) for k in ("paths", "plen", "dur", "status", "seg", "dt", "npts", "nctrl", "ng", "gp")] + \
            [dict(degree=2), dict(degree=6), dict(dist=0.0), dict(dist=-0.5), dict(dist=np.nan), dict(dist=np.inf),
             dict(dur=(3.0, 0.0)), dict(dur=(-1.0, 2.0)), dict(dur=(np.nan, 2.0)), dict(dur=(3.0, np.inf)), dict(mpp=0),
             dict(plen=(5, 2)), dict(plen=(4, -1)), dict(max_guide=0), dict(n_path=-1)]:
        gi["status"][:] = 77
        assert gcall(**kw) == EINVAL, kw
        assert ": m (" not in L.fuelmi_last_error().decode(), kw
        assert np.all(gi["status"] == 77), kw
    for kw in (dict(plen=(0, 1)), dict(mpp=256, plen=(256, 2)), dict(max_guide=65536)):
        assert gcall(**kw) == EINVAL and ": m (" in L.fuelmi_last_error().decode(), kw


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
    for word, val in (("FUELMI_COLRANGE_OK", cr.OK), ("FUELMI_COLRANGE_NO_COLLISION", cr.NO_COLLISION),
                      ("FUELMI_COLRANGE_ENDS_IN_OBSTACLE", cr.ENDS_IN_OBSTACLE), ("FUELMI_COLRANGE_NONFINITE", cr.NONFINITE),
                      ("FUELMI_COLRANGE_MAX_EVENTS", fuel_amd._lib.COLRANGE_MAX_EVENTS), ("FUELMI_GUIDE_MAX_PTS", cr.GUIDE_CAP),
                      ("FUELMI_GUIDE_MAX_PTS", fuel_amd._lib.GUIDE_MAX_PTS), ("FUELMI_TRAJCHK_MAX_SAMPLES", cr.CAP),
                      ("FUELMI_TOPO_UNDEFINED", cr.G_UNDEFINED), ("FUELMI_TOPO_MAX_PATH_POINTS", cc.MAX_PATH_POINTS)):
        m = re.search(r"#define %s\s+(\d+)" % word, header)
        assert m and int(m.group(1)) == val, word
    assert (fuel_amd._lib.COLRANGE_OK, fuel_amd._lib.COLRANGE_NO_COLLISION, fuel_amd._lib.COLRANGE_ENDS_IN_OBSTACLE,
            fuel_amd._lib.COLRANGE_NONFINITE) == (cr.OK, cr.NO_COLLISION, cr.ENDS_IN_OBSTACLE, cr.NONFINITE)
    # the two helpers the kernels share with the topological search live in one place
    topo = open(os.path.join(ROOT, "fuel_amd", "csrc", "topo_path.hip")).read()
    shared = open(os.path.join(ROOT, "fuel_amd", "csrc", "path_internal.h")).read()
    assert "path_disc_point(" in topo and "field_cut(" in topo and "cur_l >= len[j] - 1e-4" not in topo
    assert shared.count("cur_l >= len[j] - 1e-4") == 1
