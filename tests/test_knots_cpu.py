"""Given knots into the safety check, the sampling and the yaw plan (include/fuelmi.h fuelmi_map_check_trajs_knots,
_sample_trajs_knots, _plan_yaws_knots, fuelmi_bspline_dev_set_knot_source), without a GPU:

  * the restatement (tests/knots_ref.py) equals the reference's own NonUniformBspline on every scene of
    tests/knots_cases.py, bit for bit (tests/golden/knots/scenes.npz, recorded by tests/golden/make_knots_golden.py);
  * on explicitly accumulated uniform knots it equals the uniform restatements of the three consumers;
  * the new symbols are exported, declared and bound; every host-side refusal of the three entries returns before the map
    is looked at; the three plan functions report the LDS bytes they reported before the kernels took knots;
  * the kernels' own text, built for the host with sanitizers as a stand-alone program, matches the restatement on every
    scene through the given-knots path and on two scenes whose knots only the kernels' own check can refuse, and the
    uniform path's host builds still compile and match."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import knots_cases as kc
import knots_ref as kr
import traj_check_cases as tc
import traj_check_ref as tr
import traj_sample_ref as ts
import yaw_plan_ref as yr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ("fuelmi_map_check_trajs_knots", "fuelmi_map_sample_trajs_knots", "fuelmi_map_plan_yaws_knots",
       "fuelmi_bspline_dev_set_knot_source", "fuelmi_bspline_dev_knot_source")
EINVAL = -1


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    import fuel_amd
    return fuel_amd.lib()


# ---- 1. the restatement against the reference's class ---------------------------------------------------------------------
def test_restatement_equals_the_reference_on_every_scene():
    g = np.load(os.path.join(GOLDEN, "knots", "scenes.npz"))
    scenes = kc.scenes()
    assert sorted(g["tags"]) == sorted(sc["tag"] for sc in scenes)  # every scene is recorded, none is left over
    for sc in scenes:
        tag = sc["tag"]
        for key in ("ctrl", "u", "t"):  # the record is of this very scene
            assert _bits(g[tag + "/" + key]) == _bits(sc[key]), (tag, key)
        assert int(g[tag + "/degree"]) == sc["degree"]
        D, levels = kr.evaluate(sc["ctrl"], sc["degree"], sc["u"], sc["t"])
        assert _bits(D) == _bits(g[tag + "/time_sum"]), (tag, D, float(g[tag + "/time_sum"]))
        assert _bits(levels) == _bits(g[tag + "/levels"]), tag


def test_scenes_reach_their_edges():
    scenes = {sc["tag"]: sc for sc in kc.scenes()}
    assert [len(scenes["lanes_%d" % k]["u"]) for k in (63, 64, 65, 129)] == [63, 64, 65, 129]
    for p in (3, 4, 5):
        assert len(scenes["one_span_p%d" % p]["ctrl"]) == p + 1
    groups = kc.by_degree()
    full = scenes["full_block_p5"]
    assert len(full["ctrl"]) == max(len(sc["ctrl"]) for sc in groups[5])  # n + p + 1 = max_ctrl + 6: the block is full
    for grp in groups.values():
        assert len(grp) % kc.CHECK_WAVES and len(grp) % kc.SAMPLE_WAVES and len({len(sc["ctrl"]) for sc in grp}) > 1
        assert grp[-1]["tag"].startswith(grp[0]["tag"]) and grp[-1]["u"] is grp[0]["u"]
    assert scenes["shift_plus"]["u"][3] > 1.0 and scenes["shift_minus"]["u"][4] < -1.0
    for tag in ("ratio50_cubic", "ratio50_p4", "full_block_p5"):
        d = np.diff(scenes[tag]["u"])
        assert 40.0 < d.max() / d.min() < 60.0, (tag, d.max() / d.min())
    grid = tc.spec(kc.MAP).grid()
    safe = set()
    for sc in kc.scenes():
        u, p, n = sc["u"], sc["degree"], len(sc["ctrl"])
        if sc["dyadic"]:  # the sample times drawn on knots land on them: the strict < of the search is met
            assert all(float(u[k]) in set(sc["t"] + u[p]) for k in range(p + 1, n))
        r = kr.sample(ts.COMMAND, sc["ctrl"], p, u, sc["t"])
        assert {ts.IN, ts.PAST, ts.INVALID} == set(r["status"]), sc["tag"]
        safe.add(kr.check(grid, sc["ctrl"], p, u, sc["t_now"])["safe"])
        for mode in (yr.EXPLORE, yr.FOLLOW):  # one ulp of atan2 flips no branch of the yaw plan
            assert kr.yaw_parity_ok(kc.yaw_problem(sc, mode), u), (sc["tag"], mode)
    assert safe == {0, 1}
    ub = scenes["t_now_on_knot"]
    assert ub["t_now"] + ub["u"][3] == ub["u"][8]
    assert kr.check(grid, scenes["t_now_past_end"]["ctrl"], 3, scenes["t_now_past_end"]["u"], scenes["t_now_past_end"]["t_now"])["n_samples"] == 0
    for sc in kc.bad_scenes():
        assert not kr.knots_ok(sc["u"])


# ---- 2. accumulated uniform knots: the restatement is the uniform one -----------------------------------------------------
def test_uniform_knots_give_the_uniform_restatements():
    grid = tc.spec(kc.MAP).grid()
    for p, ctrl, dt in kc.uniform_cases():
        n = len(ctrl)
        u = kr.uniform(n, p, dt)
        D = u[n] - u[p]
        a, b = kr.check(grid, ctrl, p, u, 0.1), tr.check_literal(grid, ctrl, p, dt, 0.1)
        assert all(_bits(a[k]) == _bits(b[k]) for k in tr.KEYS), (p, n)
        t = [-0.2, 0.0, 0.3 * D, u[p + 1] - u[p], D, D + 1.0]
        for mode in (ts.COMMAND, ts.STATE):
            a, b = kr.sample(mode, ctrl, p, u, t, [0.1 * k for k in range(7)], 3, 0.4), \
                ts.sample(mode, ctrl, p, dt, t, [0.1 * k for k in range(7)], 3, 0.4)
            assert a["status"] == b["status"] and all(_bits(a[k]) == _bits(b[k]) for k in ts.PER_SAMPLE[1:] + ("duration",))
        for mode in (yr.EXPLORE, yr.FOLLOW):
            pr = yr.problem(ctrl, dt, (0.3, 0.1, 0.0), 1.2, mode=mode, degree=p, relax_time=0.5)
            a, b = kr.yaw_solve(pr, u), yr.solve(pr)
            assert (a["status"], a["seg_num"], a["n_waypt"]) == (b["status"], b["seg_num"], b["n_waypt"])
            for k in ("duration", "dt_yaw", "waypts", "end_yaw", "yaw_ctrl", "cost", "yawdot_ctrl", "yawddot_ctrl"):
                assert _bits(a[k]) == _bits(b[k]), (p, n, mode, k)


# ---- 3. the interface ---------------------------------------------------------------------------------------------------
def test_new_symbols_exported_declared_and_bound(L):
    import fuel_amd
    from fuel_amd import _lib
    header = open(os.path.join(ROOT, "include", "fuelmi.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", fuel_amd.LIB_PATH]).decode()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert " T %s\n" % name in out, name
        assert name in _lib.SYMBOLS and getattr(L, name)
    for word, val in (("FUELMI_KNOTS_UNIFORM", _lib.KNOTS_UNIFORM), ("FUELMI_KNOTS_ADJUSTED", _lib.KNOTS_ADJUSTED)):
        assert re.search(r"#define %s\s+%d\b" % (word, val), header), word
    assert (fuel_amd.host.BsplineDeviceProblem.KNOTS_UNIFORM, fuel_amd.host.BsplineDeviceProblem.KNOTS_ADJUSTED) == (0, 1)
    # what the header no longer says, and what it says stays out
    body = re.sub(r"\s+\*?\s*", " ", header)
    assert "feeding the moved knots into this call is out of scope" not in body
    assert "feeding the knots it moved into this call is out of scope" not in body
    assert "Out of scope: feeding moved knots" not in body and "this call takes uniform splines" not in body
    for left_out in ("fuelmi_map_collision_ranges", "fuelmi_map_local_segments", "kinodynamic loader", "given knots for yaw"):
        assert left_out in body, left_out


def test_knot_source_without_a_batch(L):
    assert L.fuelmi_bspline_dev_set_knot_source(None, 1) == EINVAL
    assert L.fuelmi_bspline_dev_set_knot_source(None, 0) == EINVAL
    assert L.fuelmi_bspline_dev_knot_source(None) == 0


def test_plan_functions_report_the_lds_bytes_they_did(L):
    """the LDS footprints do not move: the knot block always had room for max_ctrl + 6 knots.  The constants are what
    fuelmi_traj_check_plan / _traj_sample_plan / _yaw_plan returned before the kernels took knots: 4 waves x stride(max_ctrl)
    doubles; 3 waves x (stride(max_ctrl) + stride(max_yaw_ctrl)); the yaw kernel's blocks (yaw_plan.hip yp_lds)."""
    from fuel_amd import _lib
    out = (C.c_int * 3)()
    for maxc, lds in ((30, 1152), (61, 2176), (1024, 32960)):
        assert L.fuelmi_traj_check_plan(C.byref(_lib.TrajChkCfg(3, maxc, 0.02, 6.0)), out) == 0
        assert tuple(out) == (64, lds, 1024), (maxc, tuple(out))
    for maxc, maxy, lds in ((30, 0, 864), (30, 15, 1392), (1024, 1024, 49440)):
        assert L.fuelmi_traj_sample_plan(C.byref(_lib.TrajSmpCfg(0, 3, 3, maxc, maxy, 16)), out) == 0
        assert tuple(out) == (64, lds, 1024), (maxc, maxy, tuple(out))
    for maxc, maxs, lds in ((30, 12, 1216), (1024, 256, 23808)):
        cfg = _lib.YawCfg(0, 3, maxc, maxs, min(12, maxs), 1, 1.0, 2.0, 0.3, 0.1)
        assert L.fuelmi_yaw_plan(C.byref(cfg), out) == 0
        assert tuple(out) == (64, lds, 1024), (maxc, maxs, tuple(out))


def _entries(L, n, maxc, p, max_t=4, maxs=12):
    """the three _knots entries on NULL maps, every other argument valid: name -> call(n_ctrl, pos, knots)"""
    from fuel_amd import _lib
    dp, ip = (lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))), \
        (lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int)))
    i = lambda *s: np.zeros(s, dtype=np.int32)  # noqa: E731
    d = lambda *s: np.zeros(s)                  # noqa: E731
    keep = dict(now=d(n), nt=np.full(n, 2, dtype=np.int32), t=np.tile(np.array([0.0, 0.1, 0.0, 0.0]), (n, 1)), sy=d(n, 3), ey=d(n),
                oi=[i(n * max_t) for _ in range(6)], od=[d(n * max_t * 3) for _ in range(12)],
                oy=[d(n, maxs + 3) for _ in range(4)])
    oi, od, oy = keep["oi"], keep["od"], keep["oy"]
    tcfg = _lib.TrajChkCfg(p, maxc, 0.02, 6.0)
    scfg = _lib.TrajSmpCfg(0, p, 3, maxc, 0, max_t)
    ycfg = _lib.YawCfg(0, p, maxc, maxs, 12, 1, 1.0, 2.0, 0.3, 0.1)
    import fuel_amd
    w = fuel_amd.host.BsplineCfg(**fuel_amd.host.DEFAULT_BSPLINE)

    def chk(nc, pos, kn):
        return L.fuelmi_map_check_trajs_knots(None, C.byref(tcfg), n, ip(nc), dp(pos), dp(kn), dp(keep["now"]), ip(oi[0]), ip(oi[1]),
                                              dp(od[0]), ip(oi[2]), ip(oi[3]), dp(od[1]), dp(od[2]), ip(oi[4]), dp(od[3]))

    def smp(nc, pos, kn):
        return L.fuelmi_map_sample_trajs_knots(None, C.byref(scfg), n, ip(nc), dp(pos), dp(kn), None, None, None, None,
                                               ip(keep["nt"]), dp(keep["t"]), ip(oi[0]), dp(od[0]), dp(od[1]), dp(od[2]), dp(od[3]),
                                               dp(od[4]), dp(od[5]), dp(od[6]), dp(od[7]), None)

    def yaw(nc, pos, kn):
        return L.fuelmi_map_plan_yaws_knots(None, C.byref(w), C.byref(ycfg), n, ip(nc), dp(pos), dp(kn), dp(keep["sy"]),
                                            dp(keep["ey"]), ip(oi[0]), dp(od[0]), ip(oi[1]), dp(od[1]), dp(oy[0]), ip(oi[2]),
                                            dp(oy[1]), dp(od[2]), dp(od[3]), dp(oy[2]), dp(oy[3]))
    return dict(check=chk, sample=smp, yaw=yaw), keep


def test_host_refusals_come_before_the_map(L):
    n, maxc, p = 3, 9, 3
    ks = maxc + p + 1
    nc = np.array([9, 4, 7], dtype=np.int32)
    pos = np.zeros((n, maxc, 3))
    good = np.zeros((n, ks))
    for b in range(n):
        good[b, :nc[b] + p + 1] = 0.25 + np.cumsum(np.linspace(0.1, 0.9, nc[b] + p + 1))
        good[b, nc[b] + p + 1:] = np.nan  # behind a problem's own knots nothing is read
    entries, keep = _entries(L, n, maxc, p)

    def with_(b, j, v):
        k = good.copy()
        k[b, j] = v
        return k
    last = nc[1] + p  # the last knot of problem 1
    for name, call in entries.items():
        assert call(nc, pos, good) == EINVAL and ": m (" in L.fuelmi_last_error().decode(), name  # only the map is missing
        refused = [None, with_(0, 5, np.nan), with_(2, 0, np.inf), with_(1, last, -np.inf), with_(0, 4, good[0, 3]),
                   with_(1, last, good[1, last - 1]), with_(2, 6, good[2, 4]), with_(0, 1, good[0, 0] - 1.0)]
        for kn in refused:
            assert call(nc, pos, kn) == EINVAL, name
            assert ": m (" not in L.fuelmi_last_error().decode(), (name, L.fuelmi_last_error())
        # the sibling's checks stay: a count outside degree + 1 .. max_ctrl, a coordinate at 1e7
        assert call(np.array([9, 3, 7], dtype=np.int32), pos, good) == EINVAL and ": m (" not in L.fuelmi_last_error().decode()
        far = pos.copy()
        far[2, 6, 1] = 1e7
        assert call(nc, far, good) == EINVAL and ": m (" not in L.fuelmi_last_error().decode()


def test_python_keyword_is_exclusive():
    import fuel_amd
    m = object.__new__(fuel_amd.SDFMap)  # no device: the argument check comes first
    ctrl = [kc.flight(6, 1)]
    u = [np.arange(10.0)]
    for call in (lambda **kw: m.check_trajs(ctrl, t_now=0.0, **kw), lambda **kw: m.sample_trajs(ctrl, t=[[0.0]], **kw),
                 lambda **kw: m.plan_yaws(ctrl, start_yaw=[[0.0, 0.0, 0.0]], end_yaw=0.0, **kw)):
        with pytest.raises(ValueError):
            call(knot_span=0.2, knots=u)
        with pytest.raises(ValueError):
            call(knot_span=None)


# ---- 4. the kernels' own text on the host ---------------------------------------------------------------------------------
def _script(name):
    p = subprocess.run([sys.executable, os.path.join(GOLDEN, name)], capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    return p.stdout.splitlines()


def test_given_knots_host_build():
    last = _script("check_knots_host_build.py")[-1]
    assert "all identical, sanitizers silent" in last, last


@pytest.mark.parametrize("name", ["traj_check", "traj_sample"])
def test_uniform_path_host_builds_still_match(name):
    """the existing drivers, unmodified: SplineSrc's new members are at its end, the cut markers are where they were"""
    assert _script("check_%s_host_build.py" % name)[-1].endswith("all identical, sanitizers silent")
