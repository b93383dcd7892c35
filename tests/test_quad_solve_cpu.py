"""The restatement of the exact quadratic solve (tests/quad_solve_ref.py) checked against what exists outside it, and the
host side of the new calls: the gradient of the oracle's combineCost at the dense solution, the dense and the banded solve
against each other (the measured disagreement, which the GPU test's allowance is 100 x, is printed and recorded in
profiles/quad_solve_tolerance.json), the kernel's own text built for the host under sanitizers against the band form,
fuelmi_quad_plan, the exported symbols and every refusal, which the library makes before it touches a map."""
import json
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import quad_solve_cases as qc
import quad_solve_ref as qr
from quad_solve_cases import oracle_cost_grad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NEW_SYMBOLS = ("fuelmi_map_solve_quadratic", "fuelmi_bspline_dev_solve_quadratic", "fuelmi_quad_plan")


def test_oracle_gradient_vanishes_at_the_dense_solution():
    """2 (H q - g) through the oracle's combineCost, which knows nothing of H: at the dense solution what is left is the
    residual of a backward-stable solve, N eps |H| |q| -- ten orders below the gradient at the input, which is |H| times
    the decimetres the input lies from the minimiser.  1e-8 of the input's gradient leaves two orders to that."""
    from oracle import fuel_oracle as fo
    om = fo.OracleMap((10.0, 8.0, 4.0), *qr.BOX)
    for pr in qc.numeric_cases():
        r = qr.solve(pr, "dense")
        assert r["status"] == qr.OK, pr["tag"]
        c_in, g_in = oracle_cost_grad(om, pr, pr["ctrl"], r["pt_dist"])
        c, g = oracle_cost_grad(om, pr, r["ctrl"], r["pt_dist"])
        print("%-24s oracle |grad| at the input %.3e, at the dense solution %.3e; cost %.6g -> %.6g" %
              (pr["tag"], np.linalg.norm(g_in), np.linalg.norm(g), c_in, c))
        assert np.linalg.norm(g) <= 1e-8 * np.linalg.norm(g_in), pr["tag"]
        assert c <= c_in and abs(c - r["cost"]) <= 1e-12 * max(abs(c), 1.0), (pr["tag"], c, r["cost"])
        assert abs(fo.bspline_pt_dist(pr["ctrl"]) - r["pt_dist"]) <= 4 * 2.0 ** -52 * r["pt_dist"], pr["tag"]


def test_band_against_dense_and_the_recorded_table():
    table = json.load(open(qr.TOLERANCE_JSON))["cases"]
    for pr in qc.numeric_cases():
        d, b = qr.solve(pr, "dense"), qr.solve(pr, "band")
        dq, dc = qr.disagreement(pr)
        print("%-24s N %4d  band vs dense: ctrl %.3e cost %.3e (recorded %.3e, %.3e)" %
              (pr["tag"], len(pr["ctrl"]), dq, dc, table[pr["tag"]]["ctrl"], table[pr["tag"]]["cost"]))
        assert d["status"] == b["status"] == qr.OK and d["pt_dist"] == b["pt_dist"]
        # both are backward-stable solves of one system: they differ by its conditioning times a few eps, nowhere near 1e-7
        assert dq <= 1e-7 * max(np.abs(d["ctrl"]).max(), 1.0) and dc <= 1e-9 * max(d["cost"], 1.0), pr["tag"]
    assert sorted(table) == sorted(p["tag"] for p in qc.numeric_cases())


def test_degenerate_and_bounded_cases_of_the_restatement():
    for pr in qc.degenerate_cases():
        for form in ("dense", "band"):
            r = qr.solve(pr, form)
            assert r["status"] == qr.DEGENERATE and r["cost"] == 0.0 and np.array_equal(r["ctrl"], pr["ctrl"]), pr["tag"]
    assert qr.solve(qc.degenerate_cases()[1])["pt_dist"] == 0.0
    pr = qc.bounded_case()
    r = qr.solve(pr, "band")
    lo, hi = qr.shrunk_box(pr)
    assert r["status"] == qr.BOUNDED and np.array_equal(r["ctrl"], np.clip(pr["ctrl"], lo, hi))
    assert not np.array_equal(r["ctrl"], pr["ctrl"]) and r["cost"] == qr.combine_cost(pr, r["ctrl"], r["pt_dist"])
    free = qr.solve(dict(pr, bounds=False), "band")
    assert free["status"] == qr.OK and free["ctrl"][:, 0].max() > hi[0] and free["cost"] < r["cost"]
    inside = [p for p in qc.numeric_cases() if p["tag"] == "bounds_inside"][0]
    assert qr.solve(inside, "band")["status"] == qr.OK


def test_host_build_of_the_kernel():
    """tests/golden/check_quad_solve_host_build.py as a child process: k_quad_solve's own text, a thread per lane, under the
    address and undefined-behaviour sanitizers, every scene, bit-equal to the band form"""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "check_quad_solve_host_build.py")],
                       capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    assert p.stdout.splitlines()[-1].endswith("all identical, sanitizers silent"), p.stdout[-500:]


def test_plan_symbols_and_header():
    import fuel_amd
    hdr = open(os.path.join(ROOT, "include", "fuelmi.h")).read()
    L = fuel_amd.lib()
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % s, hdr) and hasattr(L, s) and s in fuel_amd._lib.SYMBOLS, s
    for maxc, dim in ((4, 3), (65, 3), (1024, 3), (64, 1), (1024, 1)):
        lanes, lds, cap = fuel_amd.quad_plan(max_ctrl=maxc, dim=dim)
        assert (lanes, cap) == (64, 1024) and lds == 8 * ((4 + 1 + 3 * dim) * maxc + 16), (maxc, dim, lds)
    assert fuel_amd.quad_plan(max_ctrl=1024)[1] <= 160 * 1024 < 8 * (14 * 2048 + 16)  # the next power of two does not fit
    for kw, rc in ((dict(max_ctrl=1025), -5), (dict(max_ctrl=3), -1), (dict(cost_function=0), -1),
                   (dict(cost_function=qr.GUIDE_PHASE | 4), -1), (dict(dim=2), -1), (dict(end_n=0), -1),
                   (dict(max_waypt=-1), -1)):
        with pytest.raises(fuel_amd.FuelmiError, match="error %d" % rc):
            fuel_amd.quad_plan(**kw)


@pytest.mark.parametrize("name,kw,rc,piece", qc.refusals(), ids=[r[0] for r in qc.refusals()])
def test_refusals_come_before_the_map(name, kw, rc, piece):
    """every refusal is made on the host before the map is looked at: a null map shows it"""
    import fuel_amd
    nomap = SimpleNamespace(L=fuel_amd.lib(), h=None)
    with pytest.raises(fuel_amd.FuelmiError) as e:
        fuel_amd.SDFMap.solve_quadratic(nomap, **kw)
    assert "error %d" % rc in str(e.value) and piece in str(e.value), str(e.value)


def test_no_problem_is_ok_and_a_good_call_reaches_the_map():
    import fuel_amd
    nomap = SimpleNamespace(L=fuel_amd.lib(), h=None)
    o = fuel_amd.SDFMap.solve_quadratic(nomap, [], [], dim=3)
    assert len(o["status"]) == 0
    with pytest.raises(fuel_amd.FuelmiError, match=r"invalid argument: m \("):
        fuel_amd.SDFMap.solve_quadratic(nomap, **qc.call_args([qc.numeric_cases()[3]]))
