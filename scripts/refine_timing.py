"""Wall-clock of fuelmi_map_refine_tours on the viewpoints of a headline cycle's first search: one problem at the
defaults (7 clusters x 15 viewpoints) with and without the refined-tour polyline, 16 problems in one call, and the
G800 map.  Beside each device figure, the host route for the same problem: SDFMap.path_costs for the same edges,
then computeCost and the layer pass in Python (tests/refine_ref.py).  Medians over repeats; every call returns
synchronised.  Writes one JSON object (milliseconds, edge counts, lattice edges, fuelmi_map_path_stats).  Not part of
bench.py.

    python scripts/refine_timing.py [--reps 5] [--out profiles/refine_timing.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
import fuel_amd  # noqa: E402
import refine_ref as rr  # noqa: E402

VM, YD, WDIR = 2.0, 60 * 3.1415926 / 180.0, 1.5  # algorithm.xml:95-99 at max_vel 2


def cycle(workload):
    map_size, box, occ, _, _ = bench.build_inputs(workload, seed=42)
    gm = fuel_amd.SDFMap(map_size, box[0], box[1], device=0)
    gm.uploadOccupancy(occ)
    nv = gm.nvox
    gm.setLocalBound((0, 0, 0), (nv[0] - 1, nv[1] - 1, nv[2] - 1))
    gm.clearAndInflateLocalMap()
    gf = fuel_amd.FrontierFinder(gm, cluster_min=100, cluster_size_xy=2.0, down_sample=3, split=True)
    cfg = gf.viewpointConfig()
    gf.setViewpointConfig(cfg)
    gm.setUpdatedBox(box[0], box[1])
    gf.searchFrontiers()
    na, _ = gf.computeFrontiersToVisit()
    views = {}
    for k in range(na):
        py, vis = gf.viewpoints(1, k)
        views[k] = [(py[i, :3], py[i, 3], int(vis[i])) for i in range(len(py))]
    gf.close()
    return gm, views, cfg.min_candidate_dist


def problem(views, s, ids, min_dist, vel=(0.5, -0.3, 0.1), yaw=0.3):
    """start at cluster s's best viewpoint; layers: the top 15 of each id, as getViewpointsInfo (max_decay 0.8)"""
    cur = views[s][0][0]
    P, Y = rr.viewpoints_info(cur, views, ids, 15, 0.8, min_dist)
    layers = [np.concatenate([np.array(p), np.array(y)[:, None]], axis=1) for p, y in zip(P, Y)]
    return (cur, np.array(vel), yaw, layers)


def host_route(gm, probs):
    """path_costs for every edge of every problem in one call, then computeCost + the layer pass per problem"""
    graphs = [rr.Graph(*p) for p in probs]
    pairs = [g.edge_pairs() for g in graphs]
    p1 = np.concatenate([[g.pts[u] for u, _ in e] for g, e in zip(graphs, pairs)])
    p2 = np.concatenate([[g.pts[v] for _, v in e] for g, e in zip(graphs, pairs)])
    length, kind, _ = gm.path_costs(p1, p2, max_points=0)
    k = 0
    out = []
    for g, e in zip(graphs, pairs):
        lengths = dict(zip(e, length[k:k + len(e)]))
        k += len(e)
        out.append(rr.layer_dp(g, g.costs(lengths, VM, YD, WDIR)))
    return out, kind


def timed(gm, probs, reps, tour_res=0.0):
    dev, host = [], []
    for _ in range(reps):
        gm.synchronize()
        t0 = time.perf_counter()
        ch, cost, _ = gm.refine_tours(probs, VM, YD, WDIR, tour_res=tour_res, max_tour_points=8192)
        dev.append((time.perf_counter() - t0) * 1e3)
    stats = gm.path_stats()
    for _ in range(reps):
        gm.synchronize()
        t0 = time.perf_counter()
        ref, kind = host_route(gm, probs)
        host.append((time.perf_counter() - t0) * 1e3)
    same = all(list(c) == (r[0] if r[0] is not None else [-1] * len(c)) for c, r in zip(ch, ref))
    return {"device_ms_median": float(np.median(dev)), "device_ms_all": [round(t, 2) for t in dev],
            "host_route_ms_median": float(np.median(host)), "host_route_ms_all": [round(t, 2) for t in host],
            "problems": len(probs), "layers": [len(p[3]) for p in probs][:4],
            "nodes_per_layer": [len(l) for l in probs[0][3]], "edges": int(len(kind)),
            "line": int((kind == 0).sum()), "lattice": int((kind == 1).sum()), "no_path": int((kind == 2).sum()),
            "choices_match_host_route": bool(same), "path_stats": stats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = {}
    for wl in ("G400", "G800"):
        gm, views, md = cycle(wl)
        ids = list(range(7))
        one = [problem(views, 10, ids, md)]
        out[wl + "_one"] = timed(gm, one, args.reps)
        if wl == "G400":
            out["G400_one_polyline"] = timed(gm, one, args.reps, tour_res=0.2)
            rng = np.random.default_rng(0)
            many = [problem(views, 10 + b, list(rng.choice(len(views), 7, replace=False)), md) for b in range(16)]
            out["G400_16_problems"] = timed(gm, many, args.reps)
        out[wl + "_one"]["viewpoint_clusters"] = len(views)
        gm.close()
    txt = json.dumps(out)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
