"""Records what the REFERENCE's NonUniformBspline (bspline/src/non_uniform_bspline.cpp, compiled unmodified) gives on GIVEN
knots for the scenes of tests/knots_cases.py, as one file tests/golden/knots/scenes.npz: per scene its control points,
knots and times, getTimeSum(), and evaluateDeBoorT of the spline and of getDerivative() applied one, two and three times at
those times.  tests/test_knots_cpu.py compares the restatement (tests/knots_ref.py) with it bit for bit.  Everything else
the three consumers do -- the first-hit walk, the flight record, the yaw way-points and solve -- does not look at knots and
is pinned by their own suites.

Needs the reference checkout (REF=... or /root/reference/fuel_planner).  The reference's file is built with the driver
tests/golden/knots_golden/driver.cpp against the Eigen / ROS stand-ins of compat/; the build goes to build/knots_golden/
(git-ignored).  -O2, x86-64 without contraction.  Every scene is recorded: a scene without its line is an error."""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import knots_cases as kc  # noqa: E402

REF = os.environ.get("REF", "/root/reference/fuel_planner")
OUT = os.path.join(ROOT, "build", "knots_golden")


def build(opt="-O2"):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "driver")
    subprocess.check_call(["g++", opt, "-std=c++14", "-w", "-I", os.path.join(ROOT, "compat"),
                           "-I", os.path.join(REF, "bspline", "include"),
                           os.path.join(HERE, "knots_golden", "driver.cpp"),
                           os.path.join(REF, "bspline", "src", "non_uniform_bspline.cpp"), "-o", exe])
    return exe


def hexes(a):
    return " ".join(float(v).hex() for v in np.asarray(a, dtype=np.float64).reshape(-1))


if __name__ == "__main__":
    exe = build()
    scenes = kc.scenes()
    path = os.path.join(OUT, "scenes.in")
    with open(path, "w") as f:
        f.write("%d\n" % len(scenes))
        for sc in scenes:
            f.write("%d %d %d\n%s\n%s\n%s\n" % (sc["degree"], len(sc["ctrl"]), len(sc["t"]), hexes(sc["ctrl"]), hexes(sc["u"]),
                                               hexes(sc["t"])))
    subprocess.run([exe, path, path[:-3] + ".out"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    lines = open(path[:-3] + ".out").read().splitlines()
    if len(lines) != len(scenes):
        sys.exit("recorded %d of %d scenes" % (len(lines), len(scenes)))
    rec = {"tags": np.array([sc["tag"] for sc in scenes])}
    for sc, line in zip(scenes, lines):
        vals = np.array([float.fromhex(t) for t in line.split()])
        if len(vals) != 1 + 12 * len(sc["t"]):
            sys.exit("scene %s: %d values for %d times" % (sc["tag"], len(vals), len(sc["t"])))
        tag = sc["tag"]
        rec[tag + "/ctrl"], rec[tag + "/u"], rec[tag + "/t"] = sc["ctrl"], sc["u"], sc["t"]
        rec[tag + "/degree"] = np.int32(sc["degree"])
        rec[tag + "/time_sum"] = np.float64(vals[0])
        rec[tag + "/levels"] = vals[1:].reshape(len(sc["t"]), 4, 3)
        print("recorded", tag)
    os.makedirs(os.path.join(HERE, "knots"), exist_ok=True)
    np.savez_compressed(os.path.join(HERE, "knots", "scenes.npz"), **rec)
