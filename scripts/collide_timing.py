"""Time of the collision ranges and the guide points of guided replanning on the device
(fuelmi_map_collision_ranges, fuelmi_map_guide_points), on map `a` of tests/collide_cases.py:
  collision ranges   1, 8, 64 and 1 024 splines in one call: the `three_ranges` flight (12 s, 241 ticks, three ranges, 27
                     control points of degree 5), repeated to fill the batch
  guide points       1, 8 and 64 paths in one call: the `bend` path (four points) and the path at the cap (256 points),
                     alternating, degree 3
Per batch: the time on the map's stream between fuelmi_timer_begin and fuelmi_timer_end (input copy, the kernel, result
copy) and the wall-clock of the Python call around it, each call synchronised, medians of --reps.  Writes one JSON object
(milliseconds).  Not part of bench.py; no test asserts a time.  The reference's own time for the same flight on one core
is what `TIMING=1 python tests/golden/make_collide_golden.py` prints.

    python scripts/collide_timing.py [--reps 5] [--out profiles/collide_timing.json]"""
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
import collide_cases as cc  # noqa: E402


def timed(gm, run, reps):
    out = run()  # warm: the pool, the code object
    stream_ms, wall_ms = [], []
    for _ in range(reps):
        gm.synchronize()
        t0 = time.perf_counter()
        gm.timerBegin()
        run()
        stream_ms.append(gm.timerEnd())
        wall_ms.append((time.perf_counter() - t0) * 1e3)
    return out, {"stream_ms_median": float(np.median(stream_ms)), "stream_ms_all": [round(t, 4) for t in stream_ms],
                 "python_call_ms_median": float(np.median(wall_ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    m = cc.spec("a")
    gm = fuel_amd.SDFMap(m.map_size, device=0, **m.kw)
    gm.uploadOccupancy(m.occ)
    gm.setLocalBound((0, 0, 0), tuple(v - 1 for v in gm.nvox))
    gm.clearAndInflateLocalMap()
    gm.updateESDF3d()
    res = {"device": fuel_amd.device_name(0) if hasattr(fuel_amd, "device_name") else "", "reps": args.reps,
           "collision_ranges": {}, "guide_points": {}}
    sc = next(s for s in cc.collision_scenes() if s["tag"] == "three_ranges")
    for n in (1, 8, 64, 1024):
        out, t = timed(gm, lambda: gm.collision_ranges([sc["ctrl"]] * n, [sc["dt"]] * n, degree=sc["degree"],
                                                       clearance=sc["clearance"]), args.reps)
        t.update(splines=n, ticks_each=int(out["n_ticks"][0]), status_counts={str(k): int((out["status"] == k).sum())
                                                                                for k in sorted(set(out["status"].tolist()))})
        res["collision_ranges"]["%d_splines" % n] = t
    gs = {s["tag"]: s for s in cc.guide_scenes()}
    paths = [gs["bend_deg3"]["path"], gs["max_path_points"]["path"]]
    durs = [gs["bend_deg3"]["duration"], gs["max_path_points"]["duration"]]
    for n in (1, 8, 64):
        out, t = timed(gm, lambda: gm.guide_points([paths[i % 2] for i in range(n)], [durs[i % 2] for i in range(n)],
                                                   max_guide=200), args.reps)
        t.update(paths=n, n_guide=out["n_guide"][:2].tolist())
        res["guide_points"]["%d_paths" % n] = t
    gm.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
