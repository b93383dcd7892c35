"""Records what the REFERENCE's NonUniformBspline (bspline/src/non_uniform_bspline.cpp, compiled unmodified) gives for the
scenes of tests/traj_adjust_cases.py, as tests/golden/traj_adjust/<scene>.npz: the scene and the reference's results.
tests/test_traj_adjust_cpu.py compares the restatement (tests/traj_adjust_ref.py) with these files bit for bit.

Needs the reference checkout (REF=... or /root/reference/fuel_planner).  The reference's file is built with the driver
tests/golden/traj_adjust_golden/driver.cpp against the Eigen / ROS stand-ins of compat/; the build goes to
build/traj_adjust_golden/ (git-ignored).  -O2, x86-64 without contraction.  The stand-in's norm() against real Eigen's is
the project's standing caveat.  getMeanAndMaxVel / Acc step by the literal 0.01 and
setPhysicalLimits sets limit_ratio 1.1, so a scene that changes stat_step or limit_ratio is not recorded; of a scene the
contract calls LONG only what the loops do not touch is recorded (the driver skips them as the device does)."""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import traj_adjust_cases as tc  # noqa: E402
import traj_adjust_ref as ar  # noqa: E402

REF = os.environ.get("REF", "/root/reference/fuel_planner")
OUT = os.path.join(ROOT, "build", "traj_adjust_golden")
INTS = ("feasible_in", "iters", "feasible", "feasible_out", "num_vel", "num_acc", "n_samples")


def build(opt="-O2"):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "driver")
    subprocess.check_call(["g++", opt, "-std=c++14", "-w", "-I", os.path.join(ROOT, "compat"),
                           "-I", os.path.join(REF, "bspline", "include"),
                           os.path.join(HERE, "traj_adjust_golden", "driver.cpp"),
                           os.path.join(REF, "bspline", "src", "non_uniform_bspline.cpp"), "-o", exe])
    return exe


def hexes(a):
    return " ".join(float(v).hex() for v in np.asarray(a, dtype=np.float64).reshape(-1))


def write_input(path, sc, loops=True):
    c = dict(ar.DEFAULTS)
    c.update(sc["cfg"])
    n, p = len(sc["ctrl"]), sc["degree"]
    with open(path, "w") as f:
        f.write("%d %d %d %d %d %d %d\n" % (p, n, sc["knots"] is not None, sc["ops"], sc["ratio_in"] is not None,
                                         c["realloc_iters"], 1 if loops else 0))
        f.write(hexes([sc["dt"] or 1.0, sc["ratio_in"] or 0.0, c["limit_vel"], c["limit_acc"], c["lengthen_cap"],
                       c["length_res"]]) + "\n")
        f.write(hexes(sc["ctrl"]) + "\n")
        if sc["knots"] is not None:
            f.write(hexes(sc["knots"]) + "\n")


def parse(line, sc):
    tok = line.split()
    n, p = len(sc["ctrl"]), sc["degree"]
    rec = {k: int(t) for k, t in zip(INTS, tok[:7])}
    vals = [float.fromhex(t) for t in tok[7:]]
    for k, v in zip(ar.METRICS, vals[:11]):
        rec[k] = v
    rec["knots_out"] = np.array(vals[11:11 + n + p + 1])
    rec["samples"] = np.array(vals[11 + n + p + 1:]).reshape(-1, 3)
    assert len(rec["samples"]) == rec["n_samples"]
    return rec


def recordable(sc):
    return not any(k in sc["cfg"] for k in ("stat_step", "limit_ratio"))


def run(exe, sc):
    base = os.path.join(OUT, sc["tag"])
    write_input(base + ".in", sc, loops=tc.restate(sc)["status"] != ar.LONG)
    subprocess.run([exe, base + ".in", base + ".out"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return parse(open(base + ".out").read(), sc)


if __name__ == "__main__":
    exe = build()
    os.makedirs(os.path.join(HERE, "traj_adjust"), exist_ok=True)
    for sc in tc.all_scenes():
        if not recordable(sc):
            continue
        rec = run(exe, sc)
        rec.update(ctrl=sc["ctrl"], degree=sc["degree"], ops=sc["ops"], dt=np.float64(sc["dt"] or 0.0),
                   knots=sc["knots"] if sc["knots"] is not None else np.zeros(0),
                   ratio_in=np.float64(sc["ratio_in"] if sc["ratio_in"] is not None else np.nan),
                   cfg_keys=np.array(sorted(sc["cfg"])), cfg_vals=np.array([float(sc["cfg"][k]) for k in sorted(sc["cfg"])]))
        np.savez_compressed(os.path.join(HERE, "traj_adjust", sc["tag"] + ".npz"), **rec)
        print("recorded", sc["tag"])
