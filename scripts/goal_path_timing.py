"""Wall-clock of fuelmi_map_goal_paths on the viewpoints of a headline cycle's first search: one problem (from one
cluster's best viewpoint to the farthest one it reaches) and 16 problems with 16 distinct starts in one call on G400,
one problem on G800.  Each call is split by events on the map's stream into the lattice run and k_goal_shorten
(fuelmi_map_goal_path_times).  Medians over repeats; every call returns synchronised.  Writes one JSON object
(milliseconds, statuses, raw path lengths, fuelmi_map_path_stats).  Not part of bench.py.

    python scripts/goal_path_timing.py [--reps 5] [--out profiles/goal_path_timing.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import fuel_amd  # noqa: E402


def cycle(workload):
    map_size, box, occ, _, _ = bench.build_inputs(workload, seed=42)
    gm = fuel_amd.SDFMap(map_size, box[0], box[1], device=0)
    gm.uploadOccupancy(occ)
    nv = gm.nvox
    gm.setLocalBound((0, 0, 0), (nv[0] - 1, nv[1] - 1, nv[2] - 1))
    gm.clearAndInflateLocalMap()
    gf = fuel_amd.FrontierFinder(gm, cluster_min=100, cluster_size_xy=2.0, down_sample=3, split=True)
    gf.setViewpointConfig(gf.viewpointConfig())
    gm.setUpdatedBox(box[0], box[1])
    gf.searchFrontiers()
    na, _ = gf.computeFrontiersToVisit()
    best = np.array([gf.viewpoints(1, k)[0][0, :3] for k in range(na)])
    gf.close()
    return gm, best


def farthest_reachable(gm, best, s):
    """the cluster whose best viewpoint has the longest shortened path from cluster s's (a search that finds a goal)"""
    out = gm.goal_paths(np.repeat(best[s:s + 1], len(best), axis=0), best, max_path_points=8192, raw=False)
    ok = out["status"] != gm.GOAL_NO_PATH
    return int(np.argmax(np.where(ok, out["length"], -1.0)))


def timed(gm, starts, goals, reps):
    gm.goal_paths(starts, goals, max_path_points=8192)  # warm: the scratch allocations
    wall, lattice, shorten = [], [], []
    for _ in range(reps):
        gm.synchronize()
        t0 = time.perf_counter()
        out = gm.goal_paths(starts, goals, max_path_points=8192, raw=False)
        wall.append((time.perf_counter() - t0) * 1e3)
        a, b = gm.goal_path_times()
        lattice.append(a)
        shorten.append(b)
    full = gm.goal_paths(starts, goals, max_path_points=8192)
    return {"call_ms_median": float(np.median(wall)), "call_ms_all": [round(t, 3) for t in wall],
            "lattice_ms_median": float(np.median(lattice)), "lattice_ms_all": [round(t, 3) for t in lattice],
            "k_goal_shorten_ms_median": float(np.median(shorten)),
            "k_goal_shorten_ms_all": [round(t, 4) for t in shorten],
            "shorten_share_of_call": float(np.median(shorten) / np.median(wall)),
            "problems": len(starts), "status": out["status"].tolist(), "n_way": out["n_way"].tolist(),
            "raw_len": full["raw_len"].tolist(), "length": [round(float(v), 3) for v in out["length"]],
            "path_stats": gm.path_stats()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = {}
    for wl in ("G400", "G800"):
        gm, best = cycle(wl)
        n = len(best)
        g = farthest_reachable(gm, best, 10)
        out[wl + "_one"] = timed(gm, best[10:11], best[g:g + 1], args.reps)
        out[wl + "_one"]["viewpoint_clusters"] = n
        if wl == "G400":
            s = np.arange(10, 26) % n
            out["G400_16_problems"] = timed(gm, best[s], best[(s + n // 2) % n], args.reps)
        gm.close()
    txt = json.dumps(out)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
