"""Wall-clock of the min-jerk initial trajectory through way-points on the device, on way-points that
fuelmi_map_goal_paths produces for the viewpoints of a G400 cycle's first search (the problem
scripts/goal_path_timing.py times):
  (a) fuelmi_map_waypoint_trajs for that one problem;
  (b) 16 and 256 problems in one call (the 16 goal paths of that script, repeated for 256);
  (c) way-points -> optimised control points for a batch of 16 candidates: load_waypoints + the timed device solve,
      against the present route on the same inputs: the restatement tests/waypoint_traj_ref.py on the host (dense
      formulation; PYTHON, so its time says what an interpreter costs, not what the reference's Eigen code costs),
      then loadSamples and the same solve.
Medians over repeats; every call returns synchronised.  Writes one JSON object (milliseconds).  Not part of bench.py.

    python scripts/waypoint_traj_timing.py [--reps 5] [--out profiles/waypoint_traj_timing.json]"""
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
import waypoint_traj_ref as wr  # noqa: E402
from goal_path_timing import cycle, farthest_reachable  # noqa: E402

CFG = dict(max_vel=2.0, ctrl_pt_dist=0.45, min_seg=8)


def median_ms(fn, reps, gm):
    fn()  # warm: pinned blocks, staging
    ts = []
    for _ in range(reps):
        gm.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), [round(t, 4) for t in ts]


def timed_trajs(gm, ways, reps):
    vel, acc = np.tile([0.6, -0.3, 0.1], (len(ways), 1)), np.tile([0.2, 0.1, 0.0], (len(ways), 1))
    kw = dict(CFG, max_way_points=64, max_samples=256, coef=False)
    med, every = median_ms(lambda: gm.waypoint_trajs(ways, vel, acc, **kw), reps, gm)
    out = gm.waypoint_trajs(ways, vel, acc, **kw)
    return {"call_ms_median": med, "call_ms_all": every, "problems": len(ways),
            "n_way": [len(w) for w in ways][:16], "n_samples": out["n_samples"].tolist()[:16],
            "status": sorted(set(out["status"].tolist()))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    gm, best = cycle("G400")
    n = len(best)
    g = farthest_reachable(gm, best, 10)
    one = gm.goal_paths(best[10:11], best[g:g + 1], max_path_points=8192, raw=False)
    s = np.arange(10, 26) % n
    many = gm.goal_paths(best[s], best[(s + n // 2) % n], max_path_points=8192, raw=False)
    ways16 = [w for w in many["way"] if len(w) >= 3]
    ways16 = (ways16 * 16)[:16]
    out = {"G400_one": timed_trajs(gm, one["way"], args.reps),
           "G400_16_problems": timed_trajs(gm, ways16, args.reps),
           "G400_256_problems": timed_trajs(gm, ways16 * 16, args.reps)}
    out["G400_one"]["goal_status"] = one["status"].tolist()

    # (c) the chain for 16 candidates of 20 control points
    gm.updateESDF3d()
    C, N = 16, 20
    seg = N - 3
    vel, acc = np.tile([0.6, -0.3, 0.1], (C, 1)), np.tile([0.2, 0.1, 0.0], (C, 1))
    opt = fuel_amd.BsplineOptimizer()
    opt.setEnvironment(gm)
    x0 = np.zeros((C, 3 * N + 1))
    x0[:, -1] = 1.0
    pb = fuel_amd.BsplineBatchProblem(x0, N, fuel_amd.NORMAL_PHASE | fuel_amd.MINTIME, np.ones(C), np.zeros((C, 3, 3)),
                                      np.zeros((C, 3, 3)), 1, 3, 1.0)
    dev = opt.deviceProblem(pb)

    def chain():
        dev.load_waypoints(ways16, vel, acc, max_way_points=64, **CFG)
        return dev.optimize(max_eval=100, max_time=5e-3)

    host_ms = []

    def present():
        t0 = time.perf_counter()
        rs = [wr.plan(ways16[c], vel[c], acc[c], seg_num=seg, form="dense", **CFG) for c in range(C)]
        host_ms.append((time.perf_counter() - t0) * 1e3)
        dev.loadSamples(np.array([r["dt"] for r in rs]), np.array([r["samples"] for r in rs]),
                        np.array([r["derivs"] for r in rs]))
        return dev.optimize(max_eval=100, max_time=5e-3)

    c_med, c_all = median_ms(chain, args.reps, gm)
    p_med, p_all = median_ms(present, args.reps, gm)
    l_med, l_all = median_ms(lambda: dev.load_waypoints(ways16, vel, acc, max_way_points=64, **CFG), args.reps, gm)
    out["G400_chain_16_candidates"] = {
        "candidates": C, "control_points": N,
        "load_waypoints_plus_solve_ms_median": c_med, "load_waypoints_plus_solve_ms_all": c_all,
        "load_waypoints_alone_ms_median": l_med, "load_waypoints_alone_ms_all": l_all,
        "host_restatement_plus_load_samples_plus_solve_ms_median": p_med,
        "host_restatement_plus_load_samples_plus_solve_ms_all": p_all,
        "of_which_host_restatement_python_ms_median": float(np.median(host_ms[1:])),
        "note": "the host side of the present route is the Python restatement, not the reference's Eigen code"}
    dev.close()
    gm.close()
    txt = json.dumps(out)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
