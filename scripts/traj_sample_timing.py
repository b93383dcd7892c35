"""Wall-clock of trajectory sampling on the device (fuelmi_map_sample_trajs, fuelmi_bspline_dev_sample_trajs) on the G400
cycle's candidate trajectories (bench.build_inputs: 32 control points, knot span 0.175 s), a cubic yaw spline of 12
segments each:
  (a) one problem x one sample (STATE: one replan state);
  (b) 1024 problems x 1 sample (a fleet's replan states);
  (c) 1024 problems x 1024 samples (COMMAND tapes at 100 Hz with the flight record), through the host-array route and
      through the device chain behind the device solve (the position splines never leave the device);
  (d) through the C++ facade (fuel_amd/facade/facade_trajsample, a child process), per trajectory: replanState for one
      time and evaluateCommand for a tape of 1024 ticks, each beside the literal host NonUniformBspline loop it replaces,
      in the same process.
The C call alone is timed (arrays prepared beforehand), medians of five synchronised calls after a warm-up call.  Writes
one JSON object (milliseconds; (d) in microseconds).  No threshold: the numbers are recorded, the ones where the host wins
too.  Not part of bench.py.

    python scripts/traj_sample_timing.py [--reps 5] [--out profiles/traj_sample_timing.json]"""
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
import bench  # noqa: E402
import fuel_amd  # noqa: E402
from fuel_amd import _lib  # noqa: E402
from fuel_amd.host import _dp, _ip, traj_sample_cfg  # noqa: E402

DT, SEG = 0.175, 12


def median_ms(fn, reps, gm):
    fn()  # warm: the scratch allocation, the code object
    ts = []
    for _ in range(reps):
        gm.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), [round(t, 4) for t in ts]


class Call:
    """the arrays of one call, prepared once; host(gm) / chain(dev) make the C call alone"""

    def __init__(self, mode, pos, knot, n_t, record):
        n, N = pos.shape[0], pos.shape[1]
        self.n, self.n_t, self.keys = n, n_t, ("status", "pos", "vel", "acc", "jerk", "yaw", "yawdot", "yawddot", "duration")
        rng = np.random.default_rng(7)
        D = (N - 3) * knot
        self.cfg = traj_sample_cfg(mode=mode, max_ctrl=N, max_yaw_ctrl=SEG + 3, max_t=n_t)
        self.pos, self.knot = np.ascontiguousarray(pos), np.ascontiguousarray(knot)
        self.n_ctrl = np.full(n, N, dtype=np.int32)
        self.n_yaw = np.full(n, SEG + 3, dtype=np.int32)
        self.yaw = np.cumsum(rng.normal(scale=0.2, size=(n, SEG + 3)), axis=1)
        self.yaw_dt = np.ascontiguousarray(D / SEG)
        self.nt = np.full(n, n_t, dtype=np.int32)
        self.t = np.ascontiguousarray(np.broadcast_to(0.01 * np.arange(n_t), (n, n_t))) if n_t > 1 else rng.uniform(0.0, D.min(), (n, 1))
        self.flight = np.zeros((n, 8)) if record else None
        self.o = {"status": np.zeros((n, n_t), dtype=np.int32), "duration": np.zeros(n)}
        self.o.update({k: np.zeros((n, n_t, 3)) for k in ("pos", "vel", "acc", "jerk")})
        self.o.update({k: np.zeros((n, n_t)) for k in ("yaw", "yawdot", "yawddot")})

    def _tail(self):
        if self.flight is not None:
            self.flight[:] = 0.0
        o = self.o
        return (_ip(self.n_yaw), _dp(self.yaw), _dp(self.yaw_dt), None, _ip(self.nt), _dp(self.t), _ip(o["status"]),
                _dp(o["pos"]), _dp(o["vel"]), _dp(o["acc"]), _dp(o["jerk"]), _dp(o["yaw"]), _dp(o["yawdot"]),
                _dp(o["yawddot"]), _dp(o["duration"]), _dp(self.flight))

    def host(self, gm):
        _lib.check(gm.L.fuelmi_map_sample_trajs(gm.h, C.byref(self.cfg), self.n, _ip(self.n_ctrl), _dp(self.pos),
                                                _dp(self.knot), *self._tail()))

    def chain(self, dev):
        _lib.check(dev.L.fuelmi_bspline_dev_sample_trajs(dev.h, C.byref(self.cfg), *self._tail()))

    def snapshot(self):
        return {k: self.o[k].tobytes() for k in self.keys}, None if self.flight is None else self.flight.tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    map_size, box, occ, ctrl, _ = bench.build_inputs("G400", seed=42, n_traj=64)
    gm = fuel_amd.SDFMap(map_size, box[0], box[1], device=0)
    gm.synchronize()
    B, N = 1024, int(ctrl.shape[1])
    fleet = np.ascontiguousarray(np.tile(ctrl, (B // len(ctrl), 1, 1)))
    out = {"control_points": N, "knot_span": DT, "yaw_segments": SEG,
           "kernel_plan": list(fuel_amd.SDFMap.traj_sample_plan(traj_sample_cfg(max_ctrl=N, max_yaw_ctrl=SEG + 3)))}

    def host_case(name, mode, n, n_t, record):
        c = Call(mode, fleet[:n], np.full(n, DT), n_t, record)
        med, every = median_ms(lambda: c.host(gm), args.reps, gm)
        out[name] = dict(problems=n, samples_per_problem=n_t, call_ms_median=med, call_ms_all=every,
                         us_per_sample=1e3 * med / (n * n_t), result_mib=round(124.0 * n * n_t / 2 ** 20, 3))
        return c

    host_case("a_one_state", _lib.TRAJSMP_STATE, 1, 1, False)
    host_case("b_fleet_states_1024", _lib.TRAJSMP_STATE, B, 1, False)
    host_case("c_fleet_tapes_1024x1024_host_arrays", _lib.TRAJSMP_COMMAND, B, 1024, True)

    # (c) behind the device solve of the 1024 candidates
    x, ptd, st, en = bench.bspline_problem(fleet, DT)
    cf = fuel_amd.SMOOTHNESS | fuel_amd.FEASIBILITY | fuel_amd.START | fuel_amd.END | fuel_amd.MINTIME
    opt = fuel_amd.BsplineOptimizer()
    opt.setEnvironment(gm)
    dev = opt.deviceProblem(fuel_amd.BsplineBatchProblem(x, N, cf, ptd, st, en, 1, 3, DT))
    xo, _, _ = dev.optimize(max_eval=20)
    for name, mode, n_t, record in (("b_fleet_states_1024_device_chain", _lib.TRAJSMP_STATE, 1, False),
                                    ("c_fleet_tapes_1024x1024_device_chain", _lib.TRAJSMP_COMMAND, 1024, True)):
        c = Call(mode, np.ascontiguousarray(xo[:, :3 * N].reshape(B, N, 3)), np.ascontiguousarray(xo[:, -1]), n_t, record)
        med, every = median_ms(lambda: c.chain(dev), args.reps, gm)
        got = c.snapshot()
        c.host(gm)
        out[name] = dict(problems=B, samples_per_problem=n_t, call_ms_median=med, call_ms_all=every,
                         us_per_sample=1e3 * med / (B * n_t), equals_host_array_route=got == c.snapshot())
    dev.close()
    gm.close()

    # (d) the facade driver: its device call against its in-process host loop
    exe = os.path.join(ROOT, "fuel_amd", "facade", "facade_trajsample")
    org_z = -1.0
    rng = np.random.default_rng(11)
    with tempfile.TemporaryDirectory() as tmp:
        scen = os.path.join(tmp, "scen.bin")
        with open(scen, "wb") as f:
            np.array(list(map_size) + list(box[0]) + list(box[1]) + [0.1, org_z], dtype=np.float64).tofile(f)
            for mode, n_t in ((_lib.TRAJSMP_STATE, 1), (_lib.TRAJSMP_COMMAND, 1024)):
                for c in ctrl[:8]:
                    D = (N - 3) * DT
                    t = rng.uniform(0.0, D, 1) if n_t == 1 else 0.01 * np.arange(n_t)
                    yaw = np.cumsum(rng.normal(scale=0.2, size=SEG + 3))
                    np.concatenate([[mode, 3, N, DT, 3, SEG + 3, D / SEG, 0, 0.0, n_t], c.reshape(-1), yaw, t]).tofile(f)
        p = subprocess.run([exe, scen, str(args.reps)], check=True, capture_output=True, text=True, timeout=600)
    res = json.loads(p.stdout[p.stdout.index("{"):])["problems"]
    for name, n_t in (("d_facade_replan_state", 1), ("d_facade_command_tape_1024", 1024)):
        rows = [r for r in res if r["n_t"] == n_t]
        out[name] = {"trajectories": len(rows), "samples": n_t, "all_ok": all(r["ok"] == 1 for r in rows),
                     "device_route_us_median": float(np.median([r["device_us"] for r in rows])),
                     "host_loop_us_median": float(np.median([r["host_us"] for r in rows])),
                     "device_route_us_all": [r["device_us"] for r in rows], "host_loop_us_all": [r["host_us"] for r in rows]}
    txt = json.dumps(out)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
