"""Wall-clock of the ordered cloud extraction on the device (fuelmi_map_extract_cloud) on the 400 x 400 x 100 map with
fuel_amd/synth's state (bench.build_inputs G400), beside the route it replaces on the same box in the same process:
syncHost(occupancy=True, box=...) followed by the numpy selection (tests/map_cloud_ref.py's vectorised restatement):
  OCCUPIED over the full box; OCCUPIED over a 100 x 100 x nz local box; the KNOWN count alone; UNKNOWN over the local box;
  the first two again on the 800 x 800 x 200 map (G800; --no-g800 leaves it out).
Each device call is split by events into count + scan, write, and copy (fuelmi_map_cloud_times).  Through the C++ facade
(fuel_amd/facade/facade_cloud, a child process, the 400 x 400 x 100 map after six fusions, every mirror off): the new calls
against fuelmi_map_sync_host into the occupancy mirror plus the restated loops of publishMapLocal / publishMapAll /
publishUnknown.  Medians of five synchronised calls after a warm-up call.  Writes one JSON object (milliseconds; the
facade's figures in microseconds).  No threshold: the numbers are recorded, also where the device route loses.  Not part
of bench.py.

    python scripts/map_cloud_timing.py [--reps 5] [--out profiles/map_cloud_timing.json] [--no-g800]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
import fuel_amd  # noqa: E402
import map_cloud_ref as mr  # noqa: E402


def median_ms(fn, reps, gm, after=None):
    fn()  # warm: the scratch allocation, the code object
    ts, extra = [], []
    for _ in range(reps):
        gm.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
        if after:
            extra.append(after())
    return float(np.median(ts)), [round(t, 4) for t in ts], extra


def one_map(workload, reps, cases):
    map_size, box, occ, _, _ = bench.build_inputs(workload, seed=42, n_traj=1)
    occ = np.ascontiguousarray(occ, dtype=np.float64).reshape(-1)
    gm = fuel_amd.SDFMap(map_size, box[0], box[1], device=0)
    gm.uploadOccupancy(occ)
    nv = gm.nvox
    P = mr.Params(gm.res, gm.origin, gm.info.min_occupancy_log, gm.info.clamp_min_log)
    full = ((0, 0, 0), (nv[0] - 1, nv[1] - 1, nv[2] - 1))
    c = (nv[0] // 2, nv[1] // 2)
    local = ((c[0] - 50, c[1] - 50, 0), (c[0] + 49, c[1] + 49, nv[2] - 1))
    boxes = {"full": full, "local_100x100": local}
    o3 = occ.reshape(nv)
    out = {"map_voxels": list(nv), "plan_full_box": fuel_amd.host.cloud_plan(nv, *full),
           "occupied_share": float((o3 > P.min_occupancy_log).mean()), "unknown_share": float((o3 < P.unknown_thr).mean())}
    infl = np.zeros((1, 1, 1), dtype=np.int8)  # (no INFLATED case here)
    for name, kind, bname, count_only in cases:
        lo, hi = boxes[bname]
        if count_only:
            dev = lambda: gm.count_voxels(kind, lo, hi)  # noqa: E731
            host = lambda: int(mr.select(P, gm.syncHost(occupancy=True, box=(lo, hi))["occupancy"].reshape(nv)[  # noqa: E731
                lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1], infl, kind).sum())
            same = dev() == host()
            n = dev()
        else:
            # cap = the count: one device call, as a publisher that keeps its buffer makes it
            n = gm.count_voxels(kind, lo, hi)
            dev = lambda: gm.extract_cloud(kind, lo, hi, cap=n)[0]  # noqa: E731
            host = lambda: mr.extract(P, gm.syncHost(occupancy=True, box=(lo, hi))["occupancy"].reshape(nv), infl, kind,  # noqa: E731
                                      lo, hi)
            same = dev().tobytes() == host().tobytes()
        med, every, split = median_ms(dev, reps, gm, after=gm.cloud_times)
        hmed, hevery, _ = median_ms(host, reps, gm)
        sp = np.median(np.array(split), axis=0)
        out[name] = dict(kind=mr.KIND_NAMES[kind], box=[list(lo), list(hi)], points=int(n), equal_to_host_route=bool(same),
                         device_call_ms_median=med, device_call_ms_all=every,
                         device_split_ms_median=dict(count_scan=float(sp[0]), write=float(sp[1]), copy=float(sp[2])),
                         sync_host_then_numpy_ms_median=hmed, sync_host_then_numpy_ms_all=hevery)
    gm.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-g800", action="store_true")
    args = ap.parse_args()
    out = {"G400": one_map("G400", args.reps, [("occupied_full", mr.OCCUPIED, "full", False),
                                               ("occupied_local", mr.OCCUPIED, "local_100x100", False),
                                               ("known_count_full", mr.KNOWN, "full", True),
                                               ("unknown_local", mr.UNKNOWN, "local_100x100", False)])}
    if not args.no_g800:
        out["G800"] = one_map("G800", args.reps, [("occupied_full", mr.OCCUPIED, "full", False),
                                                  ("occupied_local", mr.OCCUPIED, "local_100x100", False)])
    exe = os.path.join(ROOT, "fuel_amd", "facade", "facade_cloud")
    p = subprocess.run([exe, "40", "40", "10", str(args.reps)], check=True, capture_output=True, text=True, timeout=600)
    out["facade_400x400x100"] = json.loads(p.stdout[p.stdout.index("{"):])
    txt = json.dumps(out)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
