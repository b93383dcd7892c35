"""Records what the REFERENCE's HeadingPlanner gives for the scenes of tests/heading_cases.py, as
tests/golden/heading/<scene>.npz: its own active_perception/src/heading_planner.cpp and plan_env/src/raycast.cpp, compiled
unmodified from where they lie, with -fno-access-control so that the driver (tests/golden/heading_golden/driver.cpp)
reaches the private calcInformationGain.
  gain scenes   per yaw the gain, the UNIFORM gain (n_visible) and the UNIFORM gain on the map with its obstacles made
                free (n_cand)
  path scenes   the gains per vertex, g_value_ of every vertex of the reference's Graph built as searchPathOfYaw builds it,
                the path (vertex ids and yaws), and -- without given gains -- what searchPathOfYaw itself returned
tests/test_heading_cpu.py compares the restatement (tests/heading_ref.py) with these files.

Needs the reference checkout (REF=<its fuel_planner directory>).  The sources are built against the Eigen / ROS / PCL
stand-ins of compat/, oracle/ref_build/shim_ros and tests/dropin/shim and the dense-array SDFMap of
tests/golden/heading_golden/.  The build goes to build/heading_golden/ (git-ignored).  -O2 -ffp-contract=off: a release
build for baseline x86-64.  Not recorded: the scenes with a subsampling factor other than the reference's constant 4, and
with cfg fields the reference has no parameter for.  With TIMING=1 it prints the reference's time for one searchPathOfYaw
at the defaults (scripts/heading_timing.py is the device's counterpart)."""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import heading_cases as hc  # noqa: E402
import heading_ref as hr  # noqa: E402

REF = os.environ.get("REF", os.path.join(os.path.dirname(ROOT), "reference", "fuel_planner"))
OUT = os.path.join(ROOT, "build", "heading_golden")
GOLDEN = os.path.join(HERE, "heading")


def recorded(sc):
    """the reference can be given this scene: factor 4 and the constructor's angles"""
    d = hr.DEFAULT_CFG
    return sc["cfg"]["factor"] == 4 and all(sc["cfg"][k] == d[k] for k in ("top_ang", "left_ang", "right_ang")) and \
        (sc["cfg"]["in_box"] or sc["cfg"]["weight_type"] == hr.UNIFORM)


def build():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "driver")
    src = os.path.join(HERE, "heading_golden")
    inc = [src, os.path.join(ROOT, "compat"), os.path.join(ROOT, "oracle", "ref_build", "shim_ros"),
           os.path.join(ROOT, "tests", "dropin", "shim"), os.path.join(REF, "active_perception", "include"),
           os.path.join(REF, "plan_env", "include")]
    cmd = ["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-fno-access-control", "-w", "-include", "Eigen/Eigen"]
    for d in inc:
        cmd += ["-I", d]
    cmd += [os.path.join(src, "driver.cpp"), os.path.join(REF, "active_perception", "src", "heading_planner.cpp"),
            os.path.join(REF, "plan_env", "src", "raycast.cpp"), "-o", exe, "-lpthread"]
    subprocess.check_call(cmd)
    return exe


def nums(a):
    """(C++ stream extraction does not read hexadecimal floats: repr's decimals round-trip)"""
    return " ".join(repr(float(v)) for v in np.asarray(a, dtype=np.float64).reshape(-1))


def ctrl_tokens(sc):
    c = sc["ctrl"] if sc["ctrl"] is not None else np.zeros((1, 3))
    return "%d %s" % (len(c), nums(c))


def gain_record(sc):
    c = sc["cfg"]
    return "G %d %d %s %s %s %s %d %s %s" % (c["weight_type"], 1 if c["in_box"] else 0, nums([c["far"]]), nums([c["lambda1"]]),
                                             nums([c["lambda2"]]), nums(sc["pos"]), len(sc["yaws"]), nums(sc["yaws"]),
                                             ctrl_tokens(sc))


def path_record(sc):
    c, L, nv = sc["cfg"], len(sc["yaws"]), 2 * sc["h"] + 1
    given = sc["gains_in"] is not None
    rec = "P %d %s %s %s %d %s %s %s %d %d %s %s %s %s" % (
        sc["h"], nums([sc["yaw_diff"]]), nums([sc["max_yaw_rate"]]), nums([sc["w"]]), c["weight_type"], nums([c["far"]]),
        nums([c["lambda1"]]), nums([c["lambda2"]]), 1 if given else 0, L, nums([sc["dt"]]), nums(sc["pts"]), nums(sc["yaws"]),
        ctrl_tokens(sc))
    if given:
        rec += " " + nums(np.asarray(sc["gains_in"])[:L, :nv])
    return rec


def run_driver(exe, name, records):
    """the driver on map `name` over the records -> (its output lines, seconds inside searchPathOfYaw, problems timed)"""
    m = hc.spec(name)
    base = os.path.join(OUT, name)
    np.where(m.unk, 0, np.where(m.occ, 2, 1)).astype(np.int8).tofile(base + ".state")
    with open(base + ".in", "w") as f:
        f.write("%d %d %d %s %r %s %s\n" % (m.nvox + (" ".join(repr(float(v)) for v in m.origin), hc.RES,
                                                     " ".join(repr(float(v)) for v in m.box_min),
                                                     " ".join(repr(float(v)) for v in m.box_max))))
        f.write("\n".join(records) + "\n")
    p = subprocess.run([exe, base + ".in", base + ".state", base + ".out"], check=True, stdout=subprocess.DEVNULL,
                       stderr=subprocess.PIPE, text=True)
    t = [l.split() for l in p.stderr.splitlines() if l.startswith("searchPathOfYaw seconds")][0]
    return open(base + ".out").read().splitlines(), float(t[2]), int(t[4])


def parse(line):
    tok = line.split()
    f = float.fromhex
    if tok[0] == "G":
        k = int(tok[1])
        v = np.array([f(t) for t in tok[2:2 + 3 * k]]).reshape(3, k)
        assert len(tok) == 2 + 3 * k
        return dict(gain=v[0], n_visible=v[1].astype(np.int64), n_cand=v[2].astype(np.int64))
    L, nv = int(tok[1]), int(tok[2])
    at = 3
    gains = np.array([f(t) for t in tok[at:at + L * nv]]).reshape(L, nv)
    at += L * nv
    n = int(tok[at])
    g = np.array([f(t) for t in tok[at + 1:at + 1 + n]])
    at += 1 + n
    k = int(tok[at])
    ids = np.array([int(t) for t in tok[at + 1:at + 1 + k]], dtype=np.int64)
    yaws = np.array([f(t) for t in tok[at + 1 + k:at + 1 + 2 * k]])
    at += 1 + 2 * k
    k2 = int(tok[at])
    own = np.array([f(t) for t in tok[at + 1:at + 1 + k2]])
    assert at + 1 + k2 == len(tok)
    return dict(gains=gains, g_value=g, path_ids=ids, path=yaws, search_path_of_yaw=own)


if __name__ == "__main__":
    exe = build()
    os.makedirs(GOLDEN, exist_ok=True)
    scenes = [s for s in hc.all_scenes() if recorded(s)]
    total = 0
    for name in sorted({s["map"] for s in scenes}):
        scs = [s for s in scenes if s["map"] == name]
        lines, secs, timed = run_driver(exe, name, [gain_record(s) if s["kind"] == "gain" else path_record(s) for s in scs])
        assert len(lines) == len(scs)
        for s, line in zip(scs, lines):
            path = os.path.join(GOLDEN, s["tag"] + ".npz")
            np.savez_compressed(path, **parse(line))
            total += os.path.getsize(path)
        print("map %s: %d scenes, the reference's searchPathOfYaw took %.6f s for %d problems" % (name, len(scs), secs, timed))
    skipped = [s["tag"] for s in hc.all_scenes() if not recorded(s)]
    print("recorded %d files, %d bytes; not recorded: %s" % (len(scenes), total, ", ".join(skipped)))
    if os.environ.get("TIMING"):
        sc = hc.mid_scene()
        for n in (1, 8):
            _, secs, timed = run_driver(exe, "mid", [path_record(sc)] * n)
            print("reference: %d x searchPathOfYaw at the defaults (far 4.5, 11 yaws, 7 layers): %.6f s" % (timed, secs))
