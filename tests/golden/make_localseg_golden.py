"""Records what the REFERENCE's own GlobalTrajData gives for the recorded scenes of tests/localseg_cases.py, as
tests/golden/localseg/<scene>.npz: the real getTrajInfoInSphere / getTrajInfoInDuration
(plan_manage/include/plan_manage/plan_container.hpp) over the real PolynomialTraj (poly_traj/polynomial_traj.h) and the
real NonUniformBspline (bspline/src/non_uniform_bspline.cpp): n_points, dt, duration, the four derivatives, the points.
seg_num is a local of getTrajInfoInSphere; the file holds the integer nearest duration / dt, which is that local for every
recorded scene (dt = duration / seg_num).  tests/test_local_segment_cpu.py compares the restatement
(tests/localseg_ref.py) with these files.

Needs the reference checkout (REF=<its fuel_planner directory>).  The sources are built with the driver
tests/golden/localseg_golden/driver.cpp against the Eigen / ROS stand-ins of compat/ and oracle/ref_build/shim_ros, the
facade's class headers and the stand-ins of tests/golden/collide_golden/.  The build goes to build/localseg_golden/
(git-ignored).  -O2 -ffp-contract=off: a release build for baseline x86-64.  The scenes the reference hangs or faults on
(DEGENERATE, NO_LOCAL) or where it reads past a vector (a polynomial time more than 1e-4 past the last segment) are not
recorded.  Prints the reference's own time inside the two functions, and with TIMING=1 its time for 1, 8, 64 and 1 024
problems (scripts/localseg_timing.py is the device's counterpart)."""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import localseg_cases as lc  # noqa: E402

REF = os.environ.get("REF", os.path.join(os.path.dirname(ROOT), "reference", "fuel_planner"))
OUT = os.path.join(ROOT, "build", "localseg_golden")


def build():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "driver")
    src = os.path.join(HERE, "localseg_golden")
    inc = [src, os.path.join(HERE, "collide_golden"), os.path.join(REF, "path_searching", "include"),
           os.path.join(ROOT, "fuel_amd", "facade"), os.path.join(REF, "active_perception", "include"),
           os.path.join(ROOT, "fuel_amd", "facade", "standin"), os.path.join(ROOT, "include"),
           os.path.join(ROOT, "oracle", "ref_build", "shim_ros"), os.path.join(ROOT, "compat")] + \
          [os.path.join(REF, p, "include") for p in ("plan_env", "bspline", "plan_manage", "exploration_manager", "traj_utils",
                                                      "poly_traj")]
    cmd = ["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-w", "-include", "ros/ros.h"]
    for d in inc:
        cmd += ["-I", d]
    cmd += [os.path.join(src, "driver.cpp"), os.path.join(REF, "bspline", "src", "non_uniform_bspline.cpp"),
            "-Wl,--unresolved-symbols=ignore-all", "-o", exe, "-lpthread"]
    subprocess.check_call(cmd)
    return exe


def hexes(a):
    return " ".join(float(v).hex() for v in np.asarray(a, dtype=np.float64).reshape(-1))


def state_record(st):
    n_local = 0 if st.local_ctrl is None else len(st.local_ctrl)
    return "S %d %d %s %d %s %s %s %s %s %s %s %s" % (
        st.degree, len(st.seg_times), float(st.global_duration).hex(), n_local, float(st.local_knot_span).hex(),
        float(st.local_ts).hex(), float(st.local_te).hex(), float(st.time_change).hex(), float(st.last_time_inc).hex(),
        hexes(st.seg_times), hexes(st.coef), hexes(st.local_ctrl) if n_local else "")


def problem_record(sc):
    return "P %d %s %s %s" % (sc["mode"], float(sc["start_t"]).hex(), float(sc["arg0"]).hex(), float(sc["arg1"]).hex())


def run_driver(exe, name, records):
    """the driver over the records (text lines) -> (its output lines, seconds inside the two functions)"""
    base = os.path.join(OUT, name)
    with open(base + ".in", "w") as f:
        f.write("\n".join(records) + "\n")
    p = subprocess.run([exe, base + ".in", base + ".out"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                       text=True)
    secs = [float(l.split()[2]) for l in p.stderr.splitlines() if l.startswith("getTrajInfo seconds")][0]
    return open(base + ".out").read().splitlines(), secs


def parse(line):
    tok = line.split()
    n = int(tok[0])
    v = [float.fromhex(t) for t in tok[1:]]
    assert len(v) == 2 + 12 + 3 * n
    dt, duration = v[0], v[1]
    return {"n_points": np.array(n), "dt": np.array(dt), "duration": np.array(duration),
            "seg_num": np.array(int(round(duration / dt))), "derivs": np.array(v[2:14]).reshape(4, 3),
            "points": np.array(v[14:]).reshape(-1, 3)}


if __name__ == "__main__":
    exe = build()
    os.makedirs(os.path.join(HERE, "localseg"), exist_ok=True)
    scs = lc.recorded_scenes()
    records = []
    for s in scs:
        records += [state_record(s["state"]), problem_record(s)]
    lines, secs = run_driver(exe, "scenes", records)
    assert len(lines) == len(scs)
    total = 0
    for s, line in zip(scs, lines):
        rec = parse(line)
        if s["mode"] == lc.DURATION:
            rec["seg_num"] = np.array(0)
        path = os.path.join(HERE, "localseg", s["tag"] + ".npz")
        np.savez_compressed(path, **rec)
        total += os.path.getsize(path)
    print("recorded %d files, %d bytes; the reference's two functions took %.6f s in all" % (len(scs), total, secs))
    if os.environ.get("TIMING"):
        sc = next(s for s in scs if s["tag"] == "exit_step_129")
        for n in (1, 8, 64, 1024):
            _, secs = run_driver(exe, "timing", [state_record(sc["state"])] + [problem_record(sc)] * n)
            print("reference, one core: %4d x exit_step_129 (129 steps, 29 points): %.6f s in getTrajInfoInSphere" % (n, secs))
