"""Wall-clock of the yaw planner on the device (fuelmi_map_plan_yaws, fuelmi_bspline_dev_plan_yaws), on seeded curved
position splines of 32 control points (knot span 0.2 s) with the launch file's weights:
  (a) one planYawExplore problem;
  (b) 16 / 256 / 1024 problems in one call;
  (c) the device chain behind the timed device solve for 64 candidates x 32 control points (dev.plan_yaws reads the
      variables the solve left on the device), against the route that exists without it on the same inputs: the solved
      control points on the host, the way-points by the restatement tests/yaw_plan_ref.py (PYTHON: an interpreter, so
      its time says what an interpreter costs, not what the reference's C++ costs), then fuelmi_bspline_optimize with
      dimension 1, max_eval 2000 and the 5 ms cap.  Both times and both final costs are recorded.
Medians over repeats after a warm-up call; every call returns synchronised.  Writes one JSON object (milliseconds).
Not part of bench.py.

    python scripts/yaw_plan_timing.py [--reps 7] [--out profiles/yaw_plan_timing.json]"""
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
import yaw_plan_ref as yr  # noqa: E402

MAP_SIZE, BMIN, BMAX = (20.0, 20.0, 5.0), (-9.0, -9.0, 0.0), (9.0, 9.0, 4.0)


def median_ms(fn, reps, gm):
    fn()  # warm: pinned blocks, staging, the code object
    ts = []
    for _ in range(reps):
        gm.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), [round(t, 4) for t in ts]


def splines(n, n_ctrl, seed0):
    return [yr.curve(n_ctrl, seed0 + k, scale=0.25) for k in range(n)]


def timed_plans(gm, n, reps):
    rng = np.random.default_rng(n)
    pos = splines(min(n, 64), 32, 100) * ((n + 63) // 64)
    pos = pos[:n]
    start = np.stack([rng.uniform(-3, 3, n), rng.uniform(-0.3, 0.3, n), np.zeros(n)], axis=1)
    end = rng.uniform(-3, 3, n)
    call = lambda: gm.plan_yaws(pos, 0.2, start, end, relax_time=1.0, derivs=True)  # noqa: E731
    med, every = median_ms(call, reps, gm)
    out = call()
    return {"problems": n, "call_ms_median": med, "call_ms_all": every, "status": sorted(set(out["status"].tolist())),
            "n_waypt": sorted(set(out["n_waypt"].tolist()))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    gm = fuel_amd.SDFMap(MAP_SIZE, BMIN, BMAX, device=0)
    out = {"explore_one": timed_plans(gm, 1, args.reps)}
    for n in (16, 256, 1024):
        out["explore_%d_problems" % n] = timed_plans(gm, n, args.reps)
    out["kernel_plan"] = list(fuel_amd.SDFMap.yaw_plan(fuel_amd.host.yaw_cfg(max_ctrl=32)))

    # (c) 64 candidates x 32 control points behind the device solve
    C, N, dt = 64, 32, 0.2
    rng = np.random.default_rng(9)
    ctrl = np.array(splines(C, N, 300))
    x = np.concatenate([ctrl.reshape(C, 3 * N), np.full((C, 1), dt)], axis=1)
    ptd = np.array([np.linalg.norm(np.diff(c, axis=0), axis=1).sum() / N for c in ctrl])
    st, en = np.zeros((C, 3, 3)), np.zeros((C, 3, 3))
    st[:, 0], en[:, 0] = (ctrl[:, 0] + 4 * ctrl[:, 1] + ctrl[:, 2]) / 6.0, (ctrl[:, -1] + 4 * ctrl[:, -2] + ctrl[:, -3]) / 6.0
    cf = fuel_amd.SMOOTHNESS | fuel_amd.FEASIBILITY | fuel_amd.START | fuel_amd.END | fuel_amd.MINTIME
    opt = fuel_amd.BsplineOptimizer()
    opt.setEnvironment(gm)
    dev = opt.deviceProblem(fuel_amd.BsplineBatchProblem(x, N, cf, ptd, st, en, 1, 3, dt))
    start = np.stack([rng.uniform(-3, 3, C), rng.uniform(-0.3, 0.3, C), np.zeros(C)], axis=1)
    end = rng.uniform(-3, 3, C)
    xo, _, _ = dev.optimize(max_eval=100, max_time=5e-3)
    flags = fuel_amd.SMOOTHNESS | fuel_amd.START | fuel_amd.END | fuel_amd.WAYPOINTS
    host_ms, costs = [], {}

    def chain():
        r = dev.plan_yaws(start, end, relax_time=1.0)
        costs["chain"] = r["cost"]
        return r

    def present():
        t0 = time.perf_counter()
        fs = [yr.front(yr.problem(xo[c, :3 * N].reshape(N, 3), xo[c, -1], start[c], end[c], relax_time=1.0)) for c in range(C)]
        host_ms.append((time.perf_counter() - t0) * 1e3)
        by_nw = {}
        for c, f in enumerate(fs):
            by_nw.setdefault(len(f["waypts"]), []).append(c)
        cost = np.zeros(C)
        for nw, ids in by_nw.items():  # one fuelmi_bspline_optimize call per way-point count (a batch shares n_waypt)
            k = len(ids)
            s3, e3, wp = np.zeros((k, 3, 3)), np.zeros((k, 3, 3)), np.zeros((k, nw, 3))
            for j, c in enumerate(ids):
                s3[j, :, 0], e3[j, 0, 0], wp[j, :, 0] = fs[c]["start"], fs[c]["end_yaw"], fs[c]["waypts"]
            pb = fuel_amd.BsplineBatchProblem(np.array([fs[c]["q0"] for c in ids]), 15, flags,
                                              np.array([fs[c]["pt_dist"] for c in ids]), s3, e3, 2, 1,
                                              np.array([fs[c]["dt_yaw"] for c in ids]), None, None, wp if nw else None,
                                              np.array([fs[c]["idx"] for c in ids], dtype=np.int32) if nw else None)
            _, cs, _ = opt.optimize(pb, max_eval=2000, max_time=5e-3)
            cost[ids] = cs
        costs["present"] = cost

    c_med, c_all = median_ms(chain, args.reps, gm)
    p_med, p_all = median_ms(present, args.reps, gm)
    out["chain_64_candidates"] = {
        "candidates": C, "control_points": N,
        "dev_plan_yaws_ms_median": c_med, "dev_plan_yaws_ms_all": c_all,
        "host_waypoints_plus_iterative_solve_ms_median": p_med, "host_waypoints_plus_iterative_solve_ms_all": p_all,
        "of_which_host_restatement_python_ms_median": float(np.median(host_ms[1:])),
        "final_cost_chain_sum": float(costs["chain"].sum()), "final_cost_iterative_sum": float(costs["present"].sum()),
        "final_cost_largest_excess_of_iterative": float((costs["present"] - costs["chain"]).max()),
        "final_cost_largest_excess_of_chain": float((costs["chain"] - costs["present"]).max()),
        "note": "the host side of the present route is the Python restatement (an interpreter), not the reference's C++"}
    dev.close()
    gm.close()
    txt = json.dumps(out)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
