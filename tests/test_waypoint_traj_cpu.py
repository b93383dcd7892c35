"""The restatement of planExploreTraj's first half (tests/waypoint_traj_ref.py) checked against itself, and the host
side of the new calls: the dense and the structured formulation agree on every scene tests/test_waypoint_traj_gpu.py
uses (the measured disagreement and the tolerance the GPU test derives from it are printed), the invariants of the fit
hold, the scenes hold what they claim, fuelmi_wptraj_plan answers at the way-point cap and refuses one past it, and
the library exports what the header declares."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

import goal_path_ref as gr
import waypoint_traj_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NEW_SYMBOLS = ("fuelmi_map_waypoint_trajs", "fuelmi_bspline_dev_load_waypoints", "fuelmi_wptraj_plan")


def _seg_num_safe(r, p):
    q = r["length"] / p["cfg"]["ctrl_pt_dist"]
    return abs(q - round(q)) > 1e-6


def test_forms_agree_on_the_parity_tours():
    measured, tol = wr.parity_tolerance()
    print("dense vs structured, largest disagreement on the parity tours: %s" % measured)
    print("tolerance of the GPU test (100 x): %s" % tol)
    # the dense inverses' own rounding at segments of 0.2 s and longer: far below a micrometre
    assert 0.0 < measured["samples"] < 1e-9 and 0.0 < measured["coef"] < 1e-9
    assert 0.0 < measured["length"] < 1e-9 and 0.0 < measured["derivs"] < 1e-9
    sizes = []
    for p in wr.parity_cases():
        a, b = wr.solve(p, "dense"), wr.solve(p, "structured")
        assert a["status"] == b["status"] == wr.OK and min(a["seg_times"]) >= 0.2
        for k in ("n_samples", "seg_num", "n_len"):
            assert a[k] == b[k], k
        for k in ("duration", "dt"):
            assert a[k] == b[k], k
        assert np.array_equal(a["seg_times"], b["seg_times"])
        assert a["n_samples"] == a["seg_num"] + 1 and a["dt"] == a["duration"] / a["seg_num"]
        assert _seg_num_safe(a, p) and _seg_num_safe(b, p)
        sizes.append(len(p["way"]))
    assert 3 in sizes and wr.MAX_WAY in sizes and 64 in sizes and 65 in sizes


def test_invariants_of_the_fit():
    measured, bound = wr.residual_bound()
    print("structured restatement, largest residual of each invariant on the short tours: %s" % measured)
    print("bound of the GPU test (100 x): %s" % bound)
    for p in wr.short_cases() + wr.parity_cases()[:9]:
        for form in ("structured", "dense"):
            r = wr.solve(p, form)
            assert r["status"] == wr.OK
            res = wr.joint_residuals(p["way"], p["vel"], p["acc"], r["seg_times"], r["coef"])
            short = min(r["seg_times"]) < 0.02
            # the dense inverses lose the short tours (cond(A) > 1e10); everywhere else both forms keep the invariants
            if form == "structured" or not short:
                assert all(v <= max(bound[k], 1e-9) for k, v in res.items()), (form, res)
    for p in wr.short_cases():
        t = wr.solve(p, "structured")["seg_times"]
        assert 0.9e-3 / 1.0 <= min(t) < 0.02


def test_statuses_and_edges_of_the_restatement():
    for p in wr.zero_cases():
        for form in ("dense", "structured"):
            r = wr.solve(p, form)
            assert r["status"] == wr.DEGENERATE and r["n_samples"] == 0 and r["duration"] == 0.0
    two = wr.problem(70, 2, 0.5, 1.0)
    assert wr.solve(two)["status"] == wr.FEW
    p = wr.parity_cases()[3]
    full = wr.solve(p)
    cut = wr.solve(p, max_samples=full["n_samples"] - 1)
    assert cut["status"] == wr.OVER and cut["n_samples"] == full["n_samples"]
    assert np.array_equal(cut["samples"], full["samples"][:-1])
    forced = wr.solve(p, seg_num=20)
    assert forced["n_samples"] == 21 and forced["dt"] == forced["duration"] / 20.0
    # the lookup past the last segment stays in the last segment (the sample at duration + rounding)
    last = wr.evaluate(full["coef"], list(full["seg_times"]), full["duration"] + 5e-5, 0)
    assert np.abs(np.array(last) - p["way"][-1]).max() < 1e-3


def test_forms_agree_on_the_batch_and_the_goal_path_tours():
    st = set()
    for p in wr.mixed_batch(300)[::12]:
        a, b = wr.solve(p, "dense"), wr.solve(p, "structured")
        st.add(a["status"])
        assert a["status"] == b["status"]
        if a["status"] == wr.OK:
            assert a["n_samples"] == b["n_samples"] and a["n_len"] == b["n_len"] and _seg_num_safe(a, p)
            d = wr.disagreement(a, b)
            assert max(d.values()) < 1e-9, d
    assert wr.OK in st
    assert {wr.solve(p, "structured")["status"] for p in wr.mixed_batch(300)} == {wr.OK, wr.FEW, wr.DEGENERATE}
    # way-points of the door scene's close and far problems, as the GPU test takes them from goal_paths
    om, pm, size, box, case = gr.door_scene()
    ref = gr.solve_case(pm, om, case, {})
    rng = np.random.default_rng(4)
    tours = [np.array(r["way"]).reshape(-1, 3) for r in ref if r["status"] in (gr.CLOSE, gr.FAR)]
    assert {r["status"] for r in ref} >= {gr.CLOSE, gr.FAR}
    vels, accs = rng.normal(scale=0.5, size=(len(tours), 3)), rng.normal(scale=0.3, size=(len(tours), 3))
    eligible = 0
    for w, v, a in zip(tours, vels, accs):
        p = dict(way=w, vel=v, acc=a, cfg=dict(wr.DEFAULTS))
        x, y = wr.solve(p, "dense"), wr.solve(p, "structured")
        assert x["status"] == y["status"] == (wr.OK if len(w) >= 3 else wr.FEW)  # ({p, p} is shortened to {p})
        if x["status"] == wr.OK and min(x["seg_times"]) >= 0.2:
            eligible += 1
            assert x["n_samples"] == y["n_samples"] and _seg_num_safe(x, p)
    assert eligible >= 4


def test_plan_call_at_the_way_point_cap():
    import fuel_amd
    from fuel_amd._lib import WptrajCfg
    L = fuel_amd.lib()
    out = (C.c_int * 3)()
    assert L.fuelmi_wptraj_plan(C.byref(WptrajCfg(2.0, 0.45, 8, 0, wr.MAX_WAY, 64)), out) == 0
    lanes, lds, cap = tuple(out)
    assert cap == wr.MAX_WAY == fuel_amd._lib.WPTRAJ_MAX_WAY and cap >= 256
    assert lanes % 64 == 0 and 0 < lds <= 160 * 1024
    assert L.fuelmi_wptraj_plan(C.byref(WptrajCfg(2.0, 0.45, 8, 0, wr.MAX_WAY + 1, 64)), out) == -5
    assert L.fuelmi_wptraj_plan(C.byref(WptrajCfg(2.0, 0.45, 8, 0, 0, 64)), out) == -1
    assert L.fuelmi_wptraj_plan(C.byref(WptrajCfg(2.0, 0.45, 8, 0, 16, 64)), out) == 0 and out[1] < lds
    assert fuel_amd.SDFMap.waypoint_traj_plan(wr.MAX_WAY) == (lanes, lds, cap)
    # refusals that need no device: one way-point past the cap, n_prob = 0
    cfg = WptrajCfg(2.0, 0.45, 8, 0, wr.MAX_WAY + 1, 64)
    assert L.fuelmi_map_waypoint_trajs(None, C.byref(cfg), 0, *([None] * 14)) == -5
    cfg = WptrajCfg(2.0, 0.45, 8, 0, 16, 64)
    assert L.fuelmi_map_waypoint_trajs(None, C.byref(cfg), 0, *([None] * 14)) == 0
    assert wr.MAX_SEG == fuel_amd._lib.WPTRAJ_MAX_SEG


def test_new_symbols_exported_and_declared():
    import fuel_amd
    header = open(os.path.join(ROOT, "include", "fuelmi.h")).read()
    L = fuel_amd.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert getattr(L, name) is not None
    for word in ("FUELMI_WPTRAJ_OK", "FUELMI_WPTRAJ_FEW", "FUELMI_WPTRAJ_DEGENERATE", "FUELMI_WPTRAJ_MAX_WAY",
                 "fuelmi_wptraj_cfg"):
        assert word in header, word
    exported = subprocess.run(["nm", "-D", "--defined-only", fuel_amd.LIB_PATH], check=True, capture_output=True,
                              text=True).stdout
    for name in NEW_SYMBOLS:
        assert re.search(r"\bT %s\b" % name, exported), name
    m = re.search(r"#define FUELMI_WPTRAJ_MAX_WAY (\d+)", header)
    assert m and int(m.group(1)) == wr.MAX_WAY
