"""Wall-clock of fuelmi_map_path_costs on the viewpoints of a headline cycle: the first cycle's full matrix (every
pair once, issued from the row's side), a typical later cycle (k new viewpoints x all), and the G800 map.
Prints one JSON object (milliseconds, pair counts, how many pairs took the lattice).  Not part of bench.py.

    python scripts/path_cost_timing.py [--new 12] [--reps 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import fuel_amd  # noqa: E402


def viewpoints(workload):
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
    vps = np.array([gf.viewpoints(1, k)[0][0, :3] for k in range(na)])
    gf.close()
    return gm, vps


def timed(gm, p1, p2, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        length, kind, _ = gm.path_costs(p1, p2, max_points=0)
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": float(np.median(ts)), "ms_all": [round(t, 2) for t in ts], "pairs": int(len(p1)),
            "sources": int(len(np.unique(p1, axis=0))), "line": int((kind == 0).sum()),
            "lattice": int((kind == 1).sum()), "no_path": int((kind == 2).sum()), "relaxation": gm.path_stats()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", type=int, default=12, help="new viewpoints of a typical cycle")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    out = {}
    for wl in ("G400", "G800"):
        gm, vps = viewpoints(wl)
        a, b = np.triu_indices(len(vps), 1)
        out[wl + "_first_cycle"] = timed(gm, vps[a], vps[b], args.reps)
        out[wl + "_first_cycle"]["viewpoints"] = int(len(vps))
        if wl == "G400":
            k = min(args.new, len(vps) - 1)
            new = np.arange(len(vps) - k, len(vps))
            # the facade issues old x new links from the new side: k sources, each to every other viewpoint
            p1 = np.concatenate([np.repeat(vps[i:i + 1], len(vps) - 1, axis=0) for i in new])
            p2 = np.concatenate([np.delete(vps, i, axis=0) for i in new])
            out["G400_typical_cycle"] = timed(gm, p1, p2, args.reps)
            out["G400_typical_cycle"]["new"] = int(k)
        gm.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
