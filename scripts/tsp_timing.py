"""Wall-clock and tour cost of fuelmi_tsp_solve (fuel_amd.TourSolver) on the first-cycle cost matrices of the
headline workloads: G400 (295 nodes) and G800, built as the facade builds getFullCostMatrix with
frontier/device_path_cost (tests/tsp_ref.py cycle_matrix) and converted as findGlobalTour does (int(cost * 100)).
For a grid of restarts x kicks: tour cost and the median of five synchronised calls.  Then 16 typical-cycle problems
(sub-matrices of G400: the current state and 10 to 60 clusters) in one call against one call each, and the exact
method at d = 13, 16 and 17.  Writes one JSON object (milliseconds, int tour costs).  Not part of bench.py.

    python scripts/tsp_timing.py [--reps 5] [--sweep] [--out profiles/tsp_timing.json] [--dump DIR]
--dump writes the int matrices as <DIR>/tsp_<workload>.npy (for comparisons outside the project)."""
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
import tsp_ref as tr  # noqa: E402

DEFAULT = (fuel_amd._lib.TSP_DEFAULT_RESTARTS, fuel_amd._lib.TSP_DEFAULT_KICKS)
SWEEP = [(r, k) for r in (1, 16, 64, 256) for k in (0, 8, 32, 128)]


def timed(mats, reps, **cfg):
    ts = fuel_amd.TourSolver(device=0, **cfg)
    ms, res = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        res = ts.solve(mats)  # synchronous
        ms.append((time.perf_counter() - t0) * 1e3)
    ts.close()
    return float(np.median(ms)), [round(t, 3) for t in ms], res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--dump", default=None)
    args = ap.parse_args()
    out = {"default": {"restarts": DEFAULT[0], "kicks": DEFAULT[1]}}
    g400 = None
    for wl in ("G400", "G800"):
        c = fuel_amd.tour_matrix(tr.cycle_matrix(wl))
        if args.dump:
            np.save(os.path.join(args.dump, "tsp_%s.npy" % wl), c)
        if wl == "G400":
            g400 = c
        rows = []
        for r, k in (SWEEP if args.sweep else [DEFAULT]):
            med, all_ms, (o, v, m) = timed([c], args.reps, restarts=r, kicks=k)
            rows.append({"restarts": r, "kicks": k, "ms_median": med, "ms_all": all_ms, "tour_cost": int(v[0])})
            print(wl, rows[-1], flush=True)
        out[wl] = {"nodes": int(len(c)), "settings": rows}
    rng = np.random.default_rng(0)
    n = len(g400) - 1
    subs = []
    for b in range(16):
        ids = np.concatenate([[0], 1 + np.sort(rng.choice(n, int(rng.integers(10, 61)), replace=False))])
        subs.append(np.ascontiguousarray(g400[np.ix_(ids, ids)]))
    med, all_ms, (o, v, m) = timed(subs, args.reps)
    one = [timed([s], args.reps)[0] for s in subs]
    out["G400_16_typical"] = {"nodes": [int(len(s)) for s in subs], "ms_median": med, "ms_all": all_ms,
                              "one_call_each_ms_sum": float(np.sum(one)), "methods": [int(x) for x in m]}
    print("16 typical", out["G400_16_typical"], flush=True)
    for d, em in ((13, 12), (16, 15), (17, 16)):
        sub = np.ascontiguousarray(g400[:d, :d])
        med, all_ms, (o, v, m) = timed([sub], args.reps, exact_max=em)
        heur = timed([sub], 1, exact_max=3)[2][1][0]
        out["exact_d%d" % d] = {"exact_max": em, "ms_median": med, "ms_all": all_ms, "optimum": int(v[0]),
                                "method": int(m[0]), "heuristic_default_cost": int(heur)}
        print("exact", d, out["exact_d%d" % d], flush=True)
    txt = json.dumps(out)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
