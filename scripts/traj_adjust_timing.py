"""Wall-clock of trajectory time adjustment and metrics on the device (fuelmi_map_adjust_trajs) with every stage on
(LENGTHEN | REALLOC | RESAMPLE | SELECT, the reference's limits 2.0 / 2.0, three reallocation passes at most): 1, 64 and
1024 trajectories of 16 and of 64 control points (cubic, knot span 0.2 s, about 2.6 m/s: infeasible at the input, so the
reallocation runs), one group of SELECT per eight trajectories.  The C call alone is timed (arrays prepared beforehand),
medians of five synchronised calls after a warm-up call.

Beside it the same work through the reference's own NonUniformBspline on ONE CPU core: the golden driver
(tests/golden/traj_adjust_golden/driver.cpp, the reference's non_uniform_bspline.cpp built unmodified with -O2 by
tests/golden/make_traj_adjust_golden.py into build/traj_adjust_golden/) times the whole sequence per trajectory, from the
constructor on; the column is the mean of eight trajectories' medians times the number of trajectories (no ranking: a
sort of the jerks is nothing beside it).  Where neither the built driver nor the reference checkout is present the column
is null.  Writes one JSON object (milliseconds).  No threshold: the numbers are recorded.  Not part of bench.py.

    python scripts/traj_adjust_timing.py [--reps 5] [--out profiles/traj_adjust_timing.json]"""
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
for sub in ("tests", os.path.join("tests", "golden")):
    sys.path.insert(0, os.path.join(ROOT, sub))
import fuel_amd  # noqa: E402
from fuel_amd import _lib  # noqa: E402
from fuel_amd.host import _dp, _ip, traj_adjust_cfg  # noqa: E402

DT, SPEED = 0.2, 2.6
OPS = _lib.TRAJADJ_LENGTHEN | _lib.TRAJADJ_REALLOC | _lib.TRAJADJ_RESAMPLE | _lib.TRAJADJ_SELECT


def paths(n, n_ctrl, seed=11):
    rng = np.random.default_rng(seed)
    d = np.array([1.0, 0.4, 0.1]) / np.linalg.norm([1.0, 0.4, 0.1])
    return (np.array([0.5, -1.0, 1.0]) + np.arange(n_ctrl)[None, :, None] * (SPEED * DT) * d +
            rng.normal(scale=0.05, size=(n, n_ctrl, 3)))


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
    """the arrays of one call, prepared once"""

    def __init__(self, pos):
        n, N = pos.shape[0], pos.shape[1]
        self.n = n
        self.n_group = (n + 7) // 8
        self.cfg = traj_adjust_cfg(ops=OPS, max_ctrl=N, max_samples=N - 3 + 2, n_group=self.n_group)
        self.pos = np.ascontiguousarray(pos)
        self.n_ctrl = np.full(n, N, dtype=np.int32)
        self.knot = np.full(n, DT)
        self.group = (np.arange(n) // 8).astype(np.int32)
        self.info = np.zeros((n, _lib.TRAJADJ_NI), dtype=np.int32)
        self.met = np.zeros((n, _lib.TRAJADJ_NM))
        self.kout = np.zeros((n, N + 4))
        self.smp = np.zeros((n, N - 1, 3))
        self.best = np.zeros(self.n_group, dtype=np.int32)

    def host(self, gm):
        _lib.check(gm.L.fuelmi_map_adjust_trajs(gm.h, C.byref(self.cfg), self.n, _ip(self.n_ctrl), _dp(self.pos), _dp(self.knot),
                                                None, None, _ip(self.group), _ip(self.info), _dp(self.met), _dp(self.kout),
                                                _dp(self.smp), _ip(self.best)))


def reference_us(pos, reps):
    """microseconds of the reference's own class for each trajectory of pos (the golden driver), or None"""
    exe = os.path.join(ROOT, "build", "traj_adjust_golden", "driver")
    try:
        import make_traj_adjust_golden as mk
        if os.path.isdir(mk.REF):
            exe = mk.build("-O2")
    except Exception:
        mk = None
    if mk is None or not os.access(exe, os.X_OK):
        return None
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for b, ctrl in enumerate(pos):
            sc = dict(ctrl=ctrl, degree=3, dt=DT, knots=None, ops=OPS & 7, ratio_in=None, cfg={})
            base = os.path.join(tmp, "t%d" % b)
            mk.write_input(base + ".in", sc)
            p = subprocess.run(["taskset", "-c", "0", exe, base + ".in", base + ".out", str(max(reps, 5))], check=True,
                               capture_output=True, text=True)
            out.append(float(p.stdout.split()[0]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "traj_adjust_timing.json"))
    a = ap.parse_args()
    gm = fuel_amd.SDFMap((10.0, 10.0, 4.0), device=0)
    res = {"workload": "cubic splines, knot span %.1f s, %.1f m/s, all stages on, limits 2.0 / 2.0, 3 passes" % (DT, SPEED),
           "reps": a.reps, "rows": []}
    for n_ctrl in (16, 64):
        ref = reference_us(paths(8, n_ctrl), a.reps)
        for n in (1, 64, 1024):
            call = Call(paths(n, n_ctrl))
            med, runs = median_ms(lambda: call.host(gm), a.reps, gm)
            row = {"n_ctrl": n_ctrl, "n_traj": n, "device_ms": round(med, 4), "device_runs_ms": runs,
                   "iters_mean": float(call.info[:, 2].mean()), "status_ok": int((call.info[:, 0] == 0).sum()),
                   "reference_one_core_ms": None if ref is None else round(float(np.mean(ref)) * n / 1e3, 4),
                   "reference_us_per_traj": None if ref is None else [round(v, 1) for v in ref]}
            res["rows"].append(row)
            print(json.dumps(row))
    gm.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
