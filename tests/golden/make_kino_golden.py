"""Records what the REFERENCE's KinodynamicAstar (path_searching/src/kinodynamic_astar.cpp, compiled unmodified) gives
for the scenes of tests/kino_ref.py, as tests/golden/kino/<scene>.npz: the map planes, the parameters, the problems and,
per problem, the reference's results.  tests/test_kino_path_cpu.py compares the restatement with these files.

Needs the reference checkout (REF=... or /root/reference/fuel_planner).  The reference's file is built with the driver
tests/golden/kino_golden/driver.cpp against the Eigen / ROS stand-ins of compat/, tests/dropin/shim and a dense-array
stand-in for the five SDFMap members it uses (tests/golden/kino_golden/plan_env/); the build goes to build/kino_golden/
(git-ignored).  -O2: the reference's pow(tau, 2) is then the product the compiler folds it into, as in a release build.
Scenes that change what the reference holds constant (kino_ref.NOT_IN_REFERENCE: res / time_res / time_res_init of
search(), seg_num and the 8 of getSamples) are not recorded.  Arguments: the scenes to record; none records all."""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kino_ref as kr  # noqa: E402

REF = os.environ.get("REF", "/root/reference/fuel_planner")
OUT = os.path.join(ROOT, "build", "kino_golden")
CFG_KEYS = ("max_tau", "init_max_tau", "max_vel", "max_acc", "w_time", "horizon", "resolution", "lambda_heu",
            "allocate_num", "check_num", "optimistic")


def build():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "driver")
    src = os.path.join(HERE, "kino_golden")
    cmd = ["g++", "-O2", "-std=c++14", "-w", "-I", src, "-I", os.path.join(ROOT, "tests", "dropin", "shim"),
           "-I", os.path.join(ROOT, "oracle", "ref_build", "shim_ros"), "-I", os.path.join(ROOT, "compat"),
           "-I", os.path.join(REF, "path_searching", "include"), os.path.join(src, "driver.cpp"),
           os.path.join(REF, "path_searching", "src", "kinodynamic_astar.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    return exe


def run(exe, name, sc):
    km = kr.scene_map(sc)
    cfg = dict(kr.DEFAULTS)
    cfg.update(sc.get("cfg", {}))
    base = os.path.join(OUT, name)
    km.infl.astype(np.int8).tofile(base + ".infl")
    km.unk.astype(np.uint8).tofile(base + ".unk")
    rep = lambda v: " ".join(repr(float(x)) for x in v)
    with open(base + ".in", "w") as f:
        f.write("%d %d %d\n" % tuple(km.nvox))
        for v in (km.origin, km.map_size, km.box_mind, km.box_maxd, [kr.MAP_RES], [cfg[k] for k in CFG_KEYS], [cfg["ts"]]):
            f.write(rep(v) + "\n")
        f.write("%d\n" % len(sc["probs"]))
        for p in sc["probs"]:
            f.write(" ".join(rep(p[k]) for k in ("start", "vel", "acc", "goal", "goal_vel")) + "\n")
    subprocess.run([exe, base + ".in", base + ".infl", base + ".unk", base + ".out"], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    rec = {"infl_bits": np.packbits(km.infl), "unk_bits": np.packbits(km.unk), "nvox": km.nvox, "origin": km.origin,
           "map_size": km.map_size, "box_mind": km.box_mind, "box_maxd": km.box_maxd,
           "cfg_keys": np.array(sorted(cfg)), "cfg_vals": np.array([float(cfg[k]) for k in sorted(cfg)]),
           "probs": np.array([[p[k] for k in ("start", "vel", "acc", "goal", "goal_vel")] for p in sc["probs"]], dtype=np.float64)}
    for b, line in enumerate(open(base + ".out").read().splitlines()):
        tok = line.split()
        at = [0]

        def ints(n):
            v = [int(t) for t in tok[at[0]:at[0] + n]]
            at[0] += n
            return v

        def dbl(n):
            v = [float.fromhex(t) for t in tok[at[0]:at[0] + n]]
            at[0] += n
            return np.array(v, dtype=np.float64)
        head = ints(4)
        rec["head%d" % b] = np.array(head)
        if head[0] == kr.NO_PATH:
            continue
        n = ints(1)[0]
        idx, st, inp, dur = [], [], [], []
        for _ in range(n):
            idx.append(ints(3)), st.append(dbl(6)), inp.append(dbl(3)), dur.append(dbl(1)[0])
        rec["index%d" % b], rec["state%d" % b] = np.array(idx), np.array(st)
        rec["input%d" % b], rec["duration%d" % b] = np.array(inp), np.array(dur)
        rec["shot%d" % b] = np.array(ints(1))
        rec["t_shot%d" % b], rec["coef%d" % b], rec["ts%d" % b] = dbl(1), dbl(12).reshape(3, 4), dbl(1)
        k = ints(1)[0]
        rec["samples%d" % b], rec["derivs%d" % b] = dbl(3 * k).reshape(k, 3), dbl(12).reshape(4, 3)
        assert at[0] == len(tok)
    os.makedirs(os.path.join(HERE, "kino"), exist_ok=True)
    np.savez_compressed(os.path.join(HERE, "kino", name + ".npz"), **rec)


if __name__ == "__main__":
    exe = build()
    for name, sc in kr.scenes().items():
        if not kr.has_fixture(sc) or (sys.argv[1:] and name not in sys.argv[1:]):
            continue
        run(exe, name, sc)
        print("recorded", name)
