"""Wall-clock of the depth renderer on the device (fuelmi_render_depth, fuel_amd.DepthRenderer) at 640 x 480 with
camera.yaml's intrinsics.  The world is the truth voxels of the G400 benchmark map (bench.WORKLOADS, seed 42) as a 0.1 m
cloud of voxel centres; the poses are the first 16 of bench.streaming_frames' seeded camera path that look into open space.
  one frame and a batch of 16 frames, for both models, each split by events into cull + project, splat and convert
    (fuelmi_render_times); the host clock is around the synchronous call, frames left on the device (no host arrays);
  the same frames through HOST_NODE's sequential loop compiled as C++ on one core of the same box
    (scripts/depth_render_baseline.cpp): the baseline, the algorithm of the simulator's default-built node -- and whether
    its image equals the device's byte for byte;
  the closed loop: render one frame + fuelmi_map_input_depth on the renderer's device pointer, against the host route the
    repository had before: fuel_amd/synth builds the frame on the CPU and the fusion reads it from pageable memory;
  the splat's window pixels (an upper bound of its atomics: the plain read skips some) x 4 bytes over the splat time,
    beside the guide's ~1.3 TB/s for well-shaped global float atomic adds.
Medians of `reps` synchronised calls after a warm-up call; the device's clocks as rocm-smi shows them are noted.  No
threshold: the numbers are recorded, also where the device loses.  Not part of bench.py.

    python scripts/depth_render_timing.py [--reps 7] [--out profiles/depth_render_timing.json]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
import fuel_amd  # noqa: E402
from fuel_amd import _lib, synth  # noqa: E402
import depth_render_ref as rr  # noqa: E402

ROWS, COLS = 480, 640
N_PATH = 32  # frames asked of the seeded path (it skips poses that stare at a wall); the first 16 are used


def timed(fn, reps):
    fn()  # warm: scratch, code objects
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), [round(t, 4) for t in ts]


def baseline_lib(tmp):
    so = os.path.join(tmp, "libdepth_render_baseline.so")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-fPIC", "-ffp-contract=off", "-shared", "-o", so,
                           os.path.join(ROOT, "scripts", "depth_render_baseline.cpp")])
    L = C.CDLL(so)
    dp = C.POINTER(C.c_double)
    L.render_host_loop.restype = C.c_int
    L.render_host_loop.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p,
                                   C.c_int, dp, dp, C.c_void_p]
    return L


def clocks():
    try:
        p = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=60)
        return [ln.strip() for ln in p.stdout.splitlines() if "GPU[0]" in ln and ("sclk" in ln or "mclk" in ln)]
    except Exception as e:  # the figures stand without them
        return ["not available: %s" % e]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    map_size, n_obs, _ = bench.WORKLOADS["G400"]
    w = synth.World.for_map_size(map_size)
    truth = w.world(42, n_obs)
    idx = np.argwhere(truth.reshape(w.nvox) != 0)
    origin = np.array([w.g.origin[i] for i in range(3)])
    cloud = np.ascontiguousarray(((idx + 0.5) * w.g.res + origin).astype(np.float32))
    frames = bench.streaming_frames(map_size, n_obs, N_PATH, 42)[:16]
    assert len(frames) == 16
    tp = [fuel_amd.DepthRenderer.pose_transform(pos, q) for _, pos, q in frames]
    T = np.stack([t for t, _ in tp])
    P = np.stack([p for _, p in tp])
    cam = synth.CAM
    out = {"image": [ROWS, COLS], "cloud_points": int(len(cloud)), "reps": args.reps, "clocks_before": clocks(),
           "plan_16_poses": fuel_amd.DepthRenderer.plan_for(fuel_amd.DepthRenderer.config(
               ROWS, COLS, cam["fx"], cam["fy"], cam["cx"], cam["cy"], max_poses=16), len(cloud))}
    device_frames = {}
    for name, model in (("host_node", _lib.RENDER_HOST_NODE), ("cuda_node", _lib.RENDER_CUDA_NODE)):
        r = fuel_amd.DepthRenderer(ROWS, COLS, cam["fx"], cam["fy"], cam["cx"], cam["cy"], model=model, range=5.0, max_poses=16)
        r.set_cloud(cloud)
        res = {}
        for label, n in (("one_frame", 1), ("batch_16", 16)):
            split = []

            def call():
                r.render(T[:n], P[:n], metres=False, raw=False)
                split.append(r.times())
            med, every = timed(call, args.reps)
            sp = np.median(np.array(split[1:]), axis=0)
            _, _, stats = r.render(T[:n], P[:n], metres=False, raw=False)
            res[label] = dict(call_ms_median=med, call_ms_all=every,
                              split_ms_median=dict(cull_project=float(sp[0]), splat=float(sp[1]), convert=float(sp[2])),
                              points_kept=[int(v) for v in stats[:, 0]], pixels_with_return=[int(v) for v in stats[:, 2]])
        metres, raw, stats = r.render(T, P)
        device_frames[name] = metres
        # the splat's traffic, counted from the restatement's windows of frame 0
        d = rr.project(rr.Cam(ROWS, COLS, cam["fx"], cam["fy"], cam["cx"], cam["cy"], model, 5.0), cloud, T[0], P[0])
        k = d["why"] == rr.KEPT
        wpix = int(((d["x1"][k] - d["x0"][k] + 1) * (d["y1"][k] - d["y0"][k] + 1)).sum())
        splat_s = res["one_frame"]["split_ms_median"]["splat"] * 1e-3
        res["one_frame_window_pixels"] = wpix
        res["one_frame_window_bytes_per_s"] = wpix * 4 / splat_s if splat_s > 0 else None
        res["guide_float_atomic_bytes_per_s"] = 1.3e12
        res["windows_for_a_wave_share"] = float((d["size"][k] >= 17).mean()) if k.any() else 0.0
        if model == _lib.RENDER_HOST_NODE:
            # closed loop on the device: render + fusion through the device pointer
            map_kw = bench.build_inputs("G400", seed=42, n_traj=1)
            gm = fuel_amd.SDFMap(map_kw[0], map_kw[1][0], map_kw[1][1], device=0)
            cfg = gm.depthConfig()
            _, pos0, q0 = frames[0]

            def loop_dev():
                r.render(T[:1], P[:1], metres=False, raw=False)
                gm.inputDepthImageAt(r.frame_raw_ptr(0), ROWS, COLS, pos0, q0, cfg)
                gm.synchronize()
            pose0 = None
            n_try = 6 * N_PATH
            for kk in range(n_try):  # the pose behind frames[0], for synth's renderer
                pz = w.camera(truth, 7 + 42, kk, n_try, 0.7)
                if np.array_equal(pz[:3], pos0):
                    pose0 = pz
                    break

            def loop_host():
                img = w.depth_image(truth, pose0, COLS, ROWS)
                gm.inputDepthImage(img, pos0, q0, cfg)
                gm.synchronize()
            res["closed_loop_device_pointer_ms"] = timed(loop_dev, args.reps)
            res["closed_loop_synth_frame_pageable_ms"] = timed(loop_host, args.reps)
            res["synth_frame_alone_ms"] = timed(lambda: w.depth_image(truth, pose0, COLS, ROWS), args.reps)
            gm.close()
        r.close()
        out[name] = res
    # the baseline: one core, the sequential loop
    with tempfile.TemporaryDirectory() as tmp:
        L = baseline_lib(tmp)
        img = np.empty((ROWS, COLS), dtype=np.float32)
        dp = C.POINTER(C.c_double)

        def one(k):
            return L.render_host_loop(ROWS, COLS, cam["fx"], cam["fy"], cam["cx"], cam["cy"], 5.0, cloud.ctypes.data, len(cloud),
                                      T[k].ctypes.data_as(dp), P[k].ctypes.data_as(dp), img.ctypes.data)
        equal = []
        for k in range(16):
            one(k)
            equal.append(img.tobytes() == device_frames["host_node"][k].tobytes())
        out["cpu_one_core_loop"] = dict(one_frame_ms=timed(lambda: one(0), args.reps),
                                        batch_16_ms=timed(lambda: [one(k) for k in range(16)], max(3, args.reps // 2)),
                                        equal_to_device_frames=equal)
    out["clocks_after"] = clocks()
    txt = json.dumps(out)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
