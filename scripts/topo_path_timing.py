"""Time of the topological path search on the device (fuelmi_map_topo_paths) at the launch file's 2000 samples, for 1, 8
and 64 problems in one call:
  (a) the `two_pillars` scene of tests/topo_cases.py on its own 64 x 64 x 24 map (start and end of the scene);
  (b) on the G400 benchmark map (400 x 400 x 100 voxels, partly explored; full-box inflation and ESDF): eight problems
      between free voxel centres 1 m above the floor whose distance value is over 0.55 m, 3 m to 6 m apart, drawn with a
      fixed seed from the field read back (benchmark_problems).
Either with eight sample streams of different seeds; problems and streams are repeated to fill the larger batches.
Per batch: the time on the map's stream between fuelmi_timer_begin and fuelmi_timer_end (input copy, the kernel, result
copy) and the wall-clock of the Python call around it (which also builds the node and path lists), medians over repeats;
the statuses, and the counts and events of the first problems as the scale of the work done.  Writes one JSON object
(milliseconds).  Not part of bench.py.  The reference's own time for the recorded scenes is what
tests/golden/make_topo_golden.py prints.

    python scripts/topo_path_timing.py [--reps 5] [--out profiles/topo_path_timing.json]"""
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
import topo_cases as tc  # noqa: E402

SAMPLES = 2000
# topo_prm/* of plan_manage/launch/topo_algorithm.xml; the strides hold every node and the longest path the kernel keeps
CFG = dict(sample_inflate=(1.0, 3.5, 1.0), clearance=0.2, ratio_to_short=5.5, max_raw_path=300, max_raw_path2=25,
           reserve_num=6, max_path_points=256, max_nodes=SAMPLES + 2)


def benchmark_problems(dist, origin, res, n=8, seed=5):
    """n (start, end) pairs between centres of voxels of the plane 1 m above the floor with dist > 0.55, 3 m to 6 m apart"""
    iz = int((1.0 - origin[2]) / res)
    free = np.argwhere(dist[:, :, iz] > 0.55)
    rng = np.random.default_rng(seed)
    starts, ends = [], []
    while len(starts) < n:
        a, b = free[rng.integers(len(free), size=2)]
        if 3.0 <= np.linalg.norm((a - b) * res) <= 6.0:
            for lst, v in ((starts, a), (ends, b)):
                lst.append([(v[0] + 0.5) * res + origin[0], (v[1] + 0.5) * res + origin[1], (iz + 0.5) * res + origin[2]])
    return np.array(starts), np.array(ends)


def timed(gm, starts, ends, streams, reps):
    n = len(starts)
    run = lambda: gm.topo_paths(starts, ends, streams, allow_limit=True, **CFG)  # noqa: E731
    out = run()  # warm: the pool, the code object
    stream_ms, wall_ms = [], []
    for _ in range(reps):
        gm.synchronize()
        t0 = time.perf_counter()
        gm.timerBegin()
        run()
        stream_ms.append(gm.timerEnd())
        wall_ms.append((time.perf_counter() - t0) * 1e3)
    return {"problems": n, "stream_ms_median": float(np.median(stream_ms)), "stream_ms_all": [round(t, 4) for t in stream_ms],
            "python_call_ms_median": float(np.median(wall_ms)), "pool_bytes": gm.topo_pool_bytes(),
            "status_counts": {str(k): int((out["status"] == k).sum()) for k in sorted(set(out["status"].tolist()))},
            "counts": out["counts"][:8].tolist(), "events": out["events"][:8].tolist(), "n_nodes": out["n_nodes"][:8].tolist()}


def batches(gm, starts, ends, streams, reps):
    out = {}
    for n in (1, 8, 64):
        pick = np.arange(n) % len(starts)
        out["%d_problems" % n] = timed(gm, starts[pick], ends[pick], streams[np.arange(n) % len(streams)], reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    streams = np.stack([tc.sample_stream(100 + k, SAMPLES) for k in range(8)])
    out = {"samples": SAMPLES, "cfg": CFG, "plan": fuel_amd.SDFMap.topo_plan(max_sample_num=SAMPLES, **CFG)}

    sc = tc.scenes()["two_pillars"]
    gm = fuel_amd.SDFMap(tc.MAP_SIZE, device=0)
    gm.uploadOccupancy(tc.occupancy(sc["blocks"]))
    gm.setLocalBound((0, 0, 0), tuple(v - 1 for v in tc.NVOX))
    gm.clearAndInflateLocalMap()
    gm.updateESDF3d()
    p = sc["probs"][0]
    out["two_pillars"] = batches(gm, np.array([p["start"]]), np.array([p["end"]]), streams, args.reps)
    gm.close()

    map_size, box, occ, _, _ = bench.build_inputs("G400", seed=42, n_traj=1)
    gm = fuel_amd.SDFMap(map_size, box[0], box[1], device=0)
    gm.uploadOccupancy(occ)
    gm.setLocalBound((0, 0, 0), tuple(v - 1 for v in gm.nvox))
    gm.clearAndInflateLocalMap()
    gm.updateESDF3d()
    starts, ends = benchmark_problems(gm.syncHost(distance=True)["distance"].reshape(gm.nvox), gm.origin, gm.res)
    out["G400"] = dict(batches(gm, starts, ends, streams, args.reps), map_voxels=list(gm.nvox), starts=starts.tolist(),
                       ends=ends.tolist())
    gm.close()

    txt = json.dumps(out)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
