"""Wall-clock of the trajectory safety check on the device (fuelmi_map_check_trajs, fuelmi_bspline_dev_check_trajs) on the
G400 cycle's map and candidate trajectories (bench.build_inputs: 40 x 40 x 10 m at 0.1 m, 32 control points, knot span
0.175 s), t_now = 0, the reference's step and radius:
  (a) 1 / 16 / 256 / 1024 problems per check_trajs call;
  (b) dev.check_trajs behind the timed device solve of 64 candidates (reads the variables the solve left on the device);
  (c) through the C++ facade, per trajectory (fuel_amd/facade/facade_trajcheck, a child process): the device call
      BsplineOptimizer::checkTrajCollision, and the route it replaces -- fuelmi_map_sync_host of the trajectory's box into
      the inflate mirror, then the reference's host loop through the facade's getters.
Medians of five synchronised calls after a warm-up call.  Writes one JSON object (milliseconds; (c) in microseconds).
No threshold: the numbers are recorded.  Not part of bench.py.

    python scripts/traj_check_timing.py [--reps 5] [--out profiles/traj_check_timing.json]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import fuel_amd  # noqa: E402

DT = 0.175


def median_ms(fn, reps, gm):
    fn()  # warm: the scratch allocation, the code object
    ts = []
    for _ in range(reps):
        gm.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), [round(t, 4) for t in ts]


def summary(o):
    return {"unsafe": int((o["safe"] == 0).sum()), "samples_median": float(np.median(o["n_samples"])),
            "samples_max": int(o["n_samples"].max()), "end_reasons": sorted(set(o["end_reason"].tolist()))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    map_size, box, occ, ctrl, _ = bench.build_inputs("G400", seed=42, n_traj=64)
    occ = np.ascontiguousarray(occ, dtype=np.float64).reshape(-1)
    gm = fuel_amd.SDFMap(map_size, box[0], box[1], device=0)
    gm.uploadOccupancy(occ)
    nv = gm.nvox
    gm.setLocalBound((0, 0, 0), (nv[0] - 1, nv[1] - 1, nv[2] - 1))
    gm.clearAndInflateLocalMap()
    gm.synchronize()
    out = {"map_voxels": list(nv), "control_points": int(ctrl.shape[1]), "knot_span": DT,
           "kernel_plan": list(fuel_amd.SDFMap.traj_check_plan(fuel_amd.host.traj_check_cfg(max_ctrl=int(ctrl.shape[1]))))}
    for n in (1, 16, 256, 1024):
        pos = (list(ctrl) * ((n + len(ctrl) - 1) // len(ctrl)))[:n]
        call = lambda: gm.check_trajs(pos, DT, 0.0)  # noqa: E731
        med, every = median_ms(call, args.reps, gm)
        out["check_%d_problems" % n] = dict(problems=n, call_ms_median=med, call_ms_all=every, **summary(call()))

    # (b) behind the device solve of the 64 candidates
    C, N = ctrl.shape[0], ctrl.shape[1]
    x, ptd, st, en = bench.bspline_problem(ctrl, DT)
    cf = fuel_amd.SMOOTHNESS | fuel_amd.FEASIBILITY | fuel_amd.START | fuel_amd.END | fuel_amd.MINTIME
    opt = fuel_amd.BsplineOptimizer()
    opt.setEnvironment(gm)
    dev = opt.deviceProblem(fuel_amd.BsplineBatchProblem(x, N, cf, ptd, st, en, 1, 3, DT))
    xo, _, _ = dev.optimize(max_eval=100, max_time=5e-3)
    chain = lambda: dev.check_trajs(np.zeros(C))  # noqa: E731
    med, every = median_ms(chain, args.reps, gm)
    got = chain()
    want = gm.check_trajs(list(xo[:, :3 * N].reshape(C, N, 3)), xo[:, -1], np.zeros(C))
    out["chain_64_candidates"] = dict(candidates=C, dev_check_trajs_ms_median=med, dev_check_trajs_ms_all=every,
                                      equals_host_array_route=all(got[k].tobytes() == want[k].tobytes() for k in
                                                                  ("status", "safe", "distance", "n_samples", "hit_index",
                                                                   "hit_t", "hit_pos", "end_reason", "duration")),
                                      **summary(got))
    dev.close()
    gm.close()

    # (c) the facade, and the route the call replaces
    exe = os.path.join(ROOT, "fuel_amd", "facade", "facade_trajcheck")
    org = [-map_size[0] / 2.0, -map_size[1] / 2.0, -1.0]
    with tempfile.TemporaryDirectory() as tmp:
        scen = os.path.join(tmp, "scen.bin")
        with open(scen, "wb") as f:
            np.array(list(map_size) + list(box[0]) + list(box[1]) + [0.1, org[2]], dtype=np.float64).tofile(f)
            occ.tofile(f)
            for c in ctrl[:16]:
                np.concatenate([[3, len(c), DT, 0.0], c.reshape(-1)]).tofile(f)
        p = subprocess.run([exe, scen, str(args.reps)], check=True, capture_output=True, text=True, timeout=600)
    res = json.loads(p.stdout[p.stdout.index("{"):])["problems"]
    out["facade_per_trajectory"] = {
        "trajectories": len(res),
        "device_call_us_median": float(np.median([r["device_us"] for r in res])),
        "sync_host_box_then_host_loop_us_median": float(np.median([r["sync_and_host_loop_us"] for r in res])),
        "box_voxels_median": float(np.median([r["box_voxels"] for r in res])),
        "device_call_us_all": [r["device_us"] for r in res],
        "sync_host_box_then_host_loop_us_all": [r["sync_and_host_loop_us"] for r in res],
        "answers_agree": all(r["safe"] == r["fresh_mirror_safe"] for r in res),
        "unsafe": sum(1 - r["safe"] for r in res)}
    txt = json.dumps(out)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
