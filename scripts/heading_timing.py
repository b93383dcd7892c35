"""Time of HeadingPlanner's yaw search on the device (fuelmi_map_yaw_paths): 1, 8 and 64 problems of searchPathOfYaw at the
reference's defaults in one call -- the `mid_defaults` scene of tests/heading_cases.py (128 x 128 x 32 map, far 4.5,
11 yaws, 7 layers, NON_UNIFORM), repeated to fill the batch -- and the same with the gains given (the search alone).
Per batch: the time on the map's stream between fuelmi_timer_begin and fuelmi_timer_end (the host's view setup, which
runs between the two records, input copy, the kernels, result copy) and the wall-clock of the Python call around it, each call synchronised,
medians of --reps.  Writes one JSON object (milliseconds).  Not part of bench.py; no test asserts a time.  The
reference's own time for one searchPathOfYaw of the same scene is what `TIMING=1 python
tests/golden/make_heading_golden.py` prints.

    python scripts/heading_timing.py [--reps 5] [--out profiles/heading_timing.json]"""
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
import heading_cases as hc  # noqa: E402


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
    sc = hc.mid_scene()
    m = hc.spec(sc["map"])
    gm = fuel_amd.SDFMap(m.map_size, m.box_min, m.box_max, device=0, **m.kw)
    gm.uploadOccupancy(m.log_odds())
    kw = dict(sc["cfg"], half_vert_num=sc["h"], yaw_diff=sc["yaw_diff"], max_yaw_rate=sc["max_yaw_rate"], w=sc["w"])
    res = {"reps": args.reps, "scene": sc["tag"], "plan": fuel_amd.yawpath_plan(), "yaw_paths": {}, "search_only": {}}
    for n in (1, 8, 64):
        out, t = timed(gm, lambda: gm.yaw_paths([sc["pts"]] * n, [sc["yaws"]] * n, [sc["dt"]] * n, ctrl=[sc["ctrl"]] * n, **kw),
                       args.reps)
        t.update(problems=n, rays_each=int(out["n_rays"][0].sum()), status_ok=int((out["status"] == 0).sum()))
        res["yaw_paths"]["%d_problems" % n] = t
        gains = out["gains"][0]
        _, t = timed(gm, lambda: gm.yaw_paths([sc["pts"]] * n, [sc["yaws"]] * n, [sc["dt"]] * n, gains_in=[gains] * n, **kw),
                     args.reps)
        t.update(problems=n)
        res["search_only"]["%d_problems" % n] = t
    gm.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
