"""Wall-clock of the kinodynamic search of the mid-range goal branch on the device, on MID problems of a G400 cycle's
first search (viewpoint pairs whose shortened goal path is 1.5 m to 5 m long, found with fuelmi_map_goal_paths as
scripts/goal_path_timing.py sets the cycle up):
  (a) fuelmi_map_kino_paths for 1, 16 and 256 such problems in one call (the launch file's search/* values,
      allocate_num 100 000, so 256 problems hold 3.7 GB of workspace);
  (b) beside them, as the scale to read (a) against: goal_paths, load_waypoints (the close / far chain up to the fitted
      batch) and load_kino for batches of the same three sizes on the same tree.
The replay's share of the search kernel cannot be split by events (it is a phase inside one kernel); the pops and nodes
of every problem are recorded instead.  Medians over repeats; every call returns synchronised.  Writes one JSON object
(milliseconds).  Not part of bench.py.

    python scripts/kino_path_timing.py [--reps 5] [--out profiles/kino_path_timing.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import fuel_amd  # noqa: E402
from goal_path_timing import cycle  # noqa: E402
from waypoint_traj_timing import median_ms  # noqa: E402

VEL, ACC = (0.6, -0.3, 0.1), (0.2, 0.1, -0.05)


def mid_problems(gm, best, want):
    """(start, goal) viewpoint pairs of the cycle that planExploreMotion would hand to kinodynamicReplan"""
    n = len(best)
    starts, goals = [], []
    for shift in range(1, n):
        s = np.arange(n)
        out = gm.goal_paths(best[s], best[(s + shift) % n], max_path_points=8192, raw=False)
        for b in np.nonzero(out["status"] == fuel_amd.SDFMap.GOAL_MID)[0]:
            starts.append(best[b])
            goals.append(out["next_goal"][b])
        if len(starts) >= want:
            break
    return np.array(starts[:want]), np.array(goals[:want])


def timed_kino(gm, starts, goals, reps, **cfg):
    n = len(starts)
    vel, acc, gv = np.tile(VEL, (n, 1)), np.tile(ACC, (n, 1)), np.zeros((n, 3))
    run = lambda: gm.kino_paths(starts, vel, acc, goals, gv, nodes=False, allow_limit=True, **cfg)
    med, every = median_ms(run, reps, gm)
    out = run()
    return {"call_ms_median": med, "call_ms_all": every, "problems": n,
            "status_counts": {str(k): int((out["status"] == k).sum()) for k in sorted(set(out["status"].tolist()))},
            "pops": out["iter_num"].tolist()[:16], "nodes": out["use_node_num"].tolist()[:16],
            "pops_sum": int(out["iter_num"].sum()), "nodes_sum": int(out["use_node_num"].sum()),
            "answered_by_retry": int(out["which"].sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    gm, best = cycle("G400")
    starts, goals = mid_problems(gm, best, 16)
    if len(starts) == 0:
        raise SystemExit("the cycle has no MID problem")
    reps16 = (np.arange(16) % len(starts))
    s16, g16 = starts[reps16], goals[reps16]
    out = {"plan": fuel_amd.SDFMap.kino_plan(), "distinct_mid_problems": int(len(starts)),
           "G400_one": timed_kino(gm, s16[:1], g16[:1], args.reps),
           "G400_16_problems": timed_kino(gm, s16, g16, args.reps),
           "G400_256_problems": timed_kino(gm, np.tile(s16, (16, 1)), np.tile(g16, (16, 1)), args.reps)}
    # (b) the scale: the close / far chain (goal_paths, then load_waypoints into a device batch) and load_kino for
    # batches of the same three sizes, 20 control points per candidate
    gm.updateESDF3d()
    opt = fuel_amd.BsplineOptimizer()
    opt.setEnvironment(gm)
    N = 20
    for n in (1, 16, 256):
        s, g = np.tile(s16, (16, 1))[:n], np.tile(g16, (16, 1))[:n]
        gp_med, gp_all = median_ms(lambda: gm.goal_paths(s, g, max_path_points=8192, raw=False), args.reps, gm)
        ways = gm.goal_paths(s, g, max_path_points=8192, raw=False)["way"]
        vel, acc = np.tile(VEL, (n, 1)), np.tile(ACC, (n, 1))
        x0 = np.zeros((n, 3 * N + 1))
        x0[:, -1] = 1.0
        pb = fuel_amd.BsplineBatchProblem(x0, N, fuel_amd.NORMAL_PHASE | fuel_amd.MINTIME, np.ones(n), np.zeros((n, 3, 3)),
                                          np.zeros((n, 3, 3)), 1, 3, 1.0)
        dev = opt.deviceProblem(pb)
        lw_med, lw_all = median_ms(lambda: dev.load_waypoints(ways, vel, acc, max_way_points=64, max_vel=2.0,
                                                              ctrl_pt_dist=0.45, min_seg=8), args.reps, gm)
        lk_med, lk_all = median_ms(lambda: dev.load_kino(s, vel, acc, g, np.zeros((n, 3)), allow_limit=True), args.reps, gm)
        dev.close()
        out["G400_chain_%d" % n] = {"candidates": n, "control_points": N,
                                    "goal_paths_ms_median": gp_med, "goal_paths_ms_all": gp_all,
                                    "load_waypoints_ms_median": lw_med, "load_waypoints_ms_all": lw_all,
                                    "load_kino_ms_median": lk_med, "load_kino_ms_all": lk_all}
    gm.close()
    txt = json.dumps(out)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
