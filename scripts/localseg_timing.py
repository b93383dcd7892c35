"""Time of the local segments of the global trajectory on the device (fuelmi_map_local_segments): 1, 8, 64 and 1 024
problems in one call, each the `exit_step_129` scene of tests/localseg_cases.py (getTrajInfoInSphere: 129 steps of 0.2 s
along a one-segment trajectory, then 29 points and the fit of 31 control points), all on ONE state, max_points = 64.
Per batch: the time on the map's stream between fuelmi_timer_begin and fuelmi_timer_end (input copy, the kernel, the fit,
result copy) and the wall-clock of the Python call around it, each call synchronised, medians of --reps.  Writes one JSON
object (milliseconds).  Not part of bench.py; no test asserts a time.  The reference's own time for the same problems on
one core is what `TIMING=1 python tests/golden/make_localseg_golden.py` prints.

    python scripts/localseg_timing.py [--reps 5] [--out profiles/localseg_timing.json]"""
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
import localseg_cases as lc  # noqa: E402


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
    gm = fuel_amd.SDFMap((4.0, 4.0, 2.0), device=0)
    sc = next(s for s in lc.scenes() if s["tag"] == "exit_step_129")
    state = [sc["state"].as_dict()]
    res = {"reps": args.reps, "scene": sc["tag"], "local_segments": {}}
    for n in (1, 8, 64, 1024):
        out, t = timed(gm, lambda: gm.local_segments(state, [lc.problem(sc)] * n, degree=sc["degree"], max_points=64),
                       args.reps)
        t.update(problems=n, steps_each=int(out["n_steps"][0]), points_each=int(out["n_points"][0]),
                 ctrl_each=int(out["n_ctrl"][0]), all_ok=bool(not out["status"].any()))
        res["local_segments"]["%d_problems" % n] = t
    gm.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
