"""Wall-clock of the exact quadratic solve on the device (fuelmi_map_solve_quadratic) on 1, 10 and 256 GUIDE_PHASE
problems of mixed point counts (12 .. 43 control points, the scenes' generator of tests/quad_solve_cases.py, the launch
file's weights), against the route that exists without it on the same problems: fuelmi_bspline_optimize with GUIDE_PHASE,
one call per point count (a batch shares its point count), at 2 evaluations (the reference's max_iteration_num1) and at
2000.  Each route is timed twice: through the Python method, which packs its arrays on every call, and as the bare C
call on arrays packed once.  The iterative batches are packed once for both.  The final costs of the three are recorded
beside the times.  Medians over repeats after a warm-up call; every call returns synchronised.  Writes one JSON object
(milliseconds).  Not part of bench.py.

    python scripts/quad_solve_timing.py [--reps 7] [--out profiles/quad_solve_timing.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fuel_amd  # noqa: E402
import quad_solve_cases as qc  # noqa: E402
import quad_solve_ref as qr  # noqa: E402

MAP_SIZE = (10.0, 8.0, 4.0)


def median_ms(fn, reps, gm):
    fn()  # warm: pinned blocks, the code object
    ts = []
    for _ in range(reps):
        gm.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), [round(t, 4) for t in ts]


def bare_call(gm, kw):
    """the C call SDFMap.solve_quadratic makes for kw, on the arrays that method packed once -> (callable, outputs)"""
    L, name, seen = gm.L, "fuelmi_map_solve_quadratic", []
    real = getattr(L, name)
    setattr(L, name, lambda *a: (seen.append(a), real(*a))[1])
    try:
        out = gm.solve_quadratic(**kw)
    finally:
        setattr(L, name, real)
    return (lambda: real(*seen[0])), out


def timed(gm, opt, n, reps):
    prs = [qc.guide_case(12 + (7 * k) % 32, seed=500 + k, tag="t%d" % k) for k in range(n)]
    kw = qc.call_args(prs)
    raw, first = bare_call(gm, kw)
    assert not first["status"].any()
    by_n = {}
    for k, p in enumerate(prs):
        by_n.setdefault(len(p["ctrl"]), []).append(k)
    batches = []
    for N, ids in by_n.items():
        g = np.stack([prs[k]["guide"] for k in ids])
        batches.append((ids, fuel_amd.BsplineBatchProblem(
            np.stack([prs[k]["ctrl"].reshape(-1) for k in ids]), N, fuel_amd.GUIDE_PHASE,
            [float(first["pt_dist"][k]) for k in ids], np.stack([prs[k]["start"] for k in ids]),
            np.stack([prs[k]["end"] for k in ids]), 3, 3, [prs[k]["dt"] for k in ids], guide_pts=g)))
    costs = {}

    def iterate(max_eval):
        c = np.zeros(n)
        for ids, bp in batches:
            c[ids] = opt.optimize(bp, max_eval=max_eval)[1]
        costs[max_eval] = c
    r = {"problems": n, "point_counts": sorted(by_n), "iterative_calls": len(batches)}
    r["exact_python_ms_median"], r["exact_python_ms_all"] = median_ms(lambda: gm.solve_quadratic(**kw), reps, gm)
    r["exact_c_call_ms_median"], r["exact_c_call_ms_all"] = median_ms(raw, reps, gm)
    for ev in (2, 2000):
        r["iterative_%d_ms_median" % ev], r["iterative_%d_ms_all" % ev] = median_ms(lambda: iterate(ev), reps, gm)
    r["cost_sum_exact"] = float(first["cost"].sum())
    r["cost_sum_iterative_2"], r["cost_sum_iterative_2000"] = float(costs[2].sum()), float(costs[2000].sum())
    r["largest_excess_of_exact_over_iterative_2000"] = float((first["cost"] - costs[2000]).max())
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    gm = fuel_amd.SDFMap(MAP_SIZE, *qr.BOX, device=0)
    opt = fuel_amd.BsplineOptimizer()
    opt.setEnvironment(gm)
    out = {"reps": args.reps, "kernel_plan_max_ctrl_43": list(fuel_amd.quad_plan(max_ctrl=43))}
    for n in (1, 10, 256):
        out["%d_problems" % n] = timed(gm, opt, n, args.reps)
    gm.close()
    txt = json.dumps(out, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
