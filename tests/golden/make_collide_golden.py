"""Records what the REFERENCE's own functions give for the scenes of tests/collide_cases.py, as
tests/golden/collide/<scene>.npz and tests/golden/collide/guide_<scene>.npz:
  collision scenes   FastPlannerManager::findCollisionRange (plan_manage/src/planner_manager.cpp, compiled unmodified with
                     -fno-access-control to reach the private function) over the real NonUniformBspline
                     (bspline/src/non_uniform_bspline.cpp): the ticks (its calls of evaluateCoarseEDT), colli_start,
                     colli_end, start_pts, end_pts.  t_s and t_e are locals of the function and are not recorded.
  guide scenes       the real TopologyPRM::pathLength / pathToGuidePts (path_searching/src/topo_prm.cpp) and the real
                     GlobalTrajData::getTrajInfoInDuration (plan_container.hpp) round the integer rules of :553-577,
                     which the driver restates: seg_num, dt, n_pts, n_ctrl, the guide points.
tests/test_collide_range_cpu.py compares the restatement (tests/collide_ref.py) with these files.

Needs the reference checkout (REF=<its fuel_planner directory>).  The sources are built with the driver
tests/golden/collide_golden/driver.cpp against the Eigen / ROS stand-ins of compat/ and oracle/ref_build/shim_ros, the
facade's class headers, and the stand-ins of tests/golden/collide_golden/; the distance field is a dense array behind
EDTEnvironment::evaluateCoarseEDT, which the driver defines.  Symbols of the classes the driver never calls stay
unresolved.  The build goes to build/collide_golden/ (git-ignored).  -O2 -ffp-contract=off: a release build for baseline
x86-64.  The scenes whose behaviour is undefined in the reference (no segment for a point, a non-finite control point)
are left out.  Prints the reference's own time inside findCollisionRange, and with TIMING=1 its time for 1, 8, 64 and
1 024 splines (scripts/collide_timing.py is the device's counterpart)."""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import collide_cases as cc  # noqa: E402

REF = os.environ.get("REF", os.path.join(os.path.dirname(ROOT), "reference", "fuel_planner"))
OUT = os.path.join(ROOT, "build", "collide_golden")
NOT_RECORDED = ("no_segment", "one_point")


def build():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "driver")
    src = os.path.join(HERE, "collide_golden")
    inc = [src, os.path.join(REF, "path_searching", "include"), os.path.join(ROOT, "fuel_amd", "facade"),
           os.path.join(REF, "active_perception", "include"), os.path.join(ROOT, "fuel_amd", "facade", "standin"),
           os.path.join(ROOT, "include"), os.path.join(ROOT, "oracle", "ref_build", "shim_ros"), os.path.join(ROOT, "compat")] + \
          [os.path.join(REF, p, "include") for p in ("plan_env", "bspline", "plan_manage", "exploration_manager", "traj_utils",
                                                      "poly_traj")]
    cmd = ["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-fno-access-control", "-w", "-include", "ros/ros.h"]
    for d in inc:
        cmd += ["-I", d]
    cmd += [os.path.join(src, "driver.cpp"), os.path.join(REF, "plan_manage", "src", "planner_manager.cpp"),
            os.path.join(REF, "bspline", "src", "non_uniform_bspline.cpp"),
            os.path.join(REF, "path_searching", "src", "topo_prm.cpp"), "-Wl,--unresolved-symbols=ignore-all", "-o", exe,
            "-lpthread"]
    subprocess.check_call(cmd)
    return exe


def hexes(a):
    return " ".join(float(v).hex() for v in np.asarray(a, dtype=np.float64).reshape(-1))


def run_driver(exe, name, m, records):
    """the driver on map spec m over the records (text lines) -> (its output lines, seconds inside findCollisionRange)"""
    base = os.path.join(OUT, name)
    m.dist.astype(np.float64).tofile(base + ".field")
    with open(base + ".in", "w") as f:
        f.write("%d %d %d %s %r\n" % (m.nvox + (" ".join(repr(float(v)) for v in m.origin), m.res)))
        f.write("\n".join(records) + "\n")
    p = subprocess.run([exe, base + ".in", base + ".field", base + ".out"], check=True, stdout=subprocess.DEVNULL,
                       stderr=subprocess.PIPE, text=True)
    secs = [float(l.split()[2]) for l in p.stderr.splitlines() if l.startswith("findCollisionRange seconds")][0]
    return open(base + ".out").read().splitlines(), secs


def range_record(sc):
    return "R %d %d %r %r %s" % (sc["degree"], len(sc["ctrl"]), sc["dt"], sc["clearance"], hexes(sc["ctrl"]))


def guide_record(sc):
    return "G %d %d %r %r %s" % (sc["degree"], len(sc["path"]), sc["duration"], sc["ctrl_pt_dist"], hexes(sc["path"]))


def parse(line):
    tok = line.split()
    at = [1]

    def pts():
        n = int(tok[at[0]])
        v = np.array([float.fromhex(t) for t in tok[at[0] + 1:at[0] + 1 + 3 * n]], dtype=np.float64).reshape(-1, 3)
        at[0] += 1 + 3 * n
        return v
    if tok[0] == "R":
        rec = {"n_ticks": np.array(int(tok[1]))}
        at[0] = 2
        for key in ("colli_start", "colli_end", "start_pts", "end_pts"):
            rec[key] = pts()
    else:
        rec = {"seg_num": np.array(int(tok[1])), "dt": np.array(float.fromhex(tok[2])), "n_pts": np.array(int(tok[3])),
               "n_ctrl": np.array(int(tok[4]))}
        at[0] = 5
        rec["guide_pts"] = pts()
    assert at[0] == len(tok)
    return rec


if __name__ == "__main__":
    exe = build()
    os.makedirs(os.path.join(HERE, "collide"), exist_ok=True)
    scenes = cc.collision_scenes()
    guides = [s for s in cc.guide_scenes() if s["tag"] not in NOT_RECORDED]
    total = 0
    for name in sorted(cc.MAPS):
        scs = [s for s in scenes if s["map"] == name]
        gs = guides if name == "b" else []
        lines, secs = run_driver(exe, name, cc.spec(name), [range_record(s) for s in scs] + [guide_record(s) for s in gs])
        assert len(lines) == len(scs) + len(gs)
        for s, line in zip(scs + gs, lines):
            rec = parse(line)
            path = os.path.join(HERE, "collide", ("guide_" if "path" in s else "") + s["tag"] + ".npz")
            np.savez_compressed(path, **rec)
            total += os.path.getsize(path)
        print("map %s: %d collision scenes, the reference's findCollisionRange took %.6f s in all" % (name, len(scs), secs))
    print("recorded %d files, %d bytes" % (len(scenes) + len(guides), total))
    if os.environ.get("TIMING"):
        sc = next(s for s in scenes if s["tag"] == "three_ranges")
        for n in (1, 8, 64, 1024):
            _, secs = run_driver(exe, "timing", cc.spec("a"), [range_record(sc)] * n)
            print("reference, one core: %4d x three_ranges (12 s, 241 ticks): %.6f s in findCollisionRange" % (n, secs))
