"""Records what the REFERENCE's TopologyPRM (path_searching/src/topo_prm.cpp with plan_env/src/raycast.cpp, compiled
unmodified) gives for the scenes of tests/topo_cases.py, as tests/golden/topo/<scene>.npz: the source voxels, the
parameters, the problems, the sample stream its engine gave and, per problem, the reference's graph and path sets.
tests/test_topo_path_cpu.py compares the restatement (tests/topo_ref.py) with these files.

Needs the reference checkout (REF=<its fuel_planner directory>).  The two files are built with the driver
tests/golden/topo_golden/driver.cpp against the Eigen / ROS stand-ins of compat/ and a dense-array stand-in for the
SDFMap / EDTEnvironment members they use (tests/golden/topo_golden/plan_env/); the build goes to build/topo_golden/
(git-ignored).  -O2 -ffp-contract=off: a release build for baseline x86-64.  The scenes of topo_cases.NOT_RECORDED are
left out.  Prints the reference's own time per scene, and with TIMING=<samples> the time of the `two_pillars` problem at
that many samples (scripts/topo_path_timing.py is its device counterpart)."""
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import topo_cases as tc  # noqa: E402

REF = os.environ.get("REF", os.path.join(os.path.dirname(ROOT), "reference", "fuel_planner"))
OUT = os.path.join(ROOT, "build", "topo_golden")
CFG_KEYS = ("clearance", "ratio_to_short", "max_sample_num", "max_raw_path", "max_raw_path2", "reserve_num")


def build():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "driver")
    src = os.path.join(HERE, "topo_golden")
    cmd = ["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-w", "-I", src, "-I", os.path.join(ROOT, "compat"),
           "-I", os.path.join(REF, "path_searching", "include"), "-I", os.path.join(REF, "plan_env", "include"),
           os.path.join(src, "driver.cpp"), os.path.join(REF, "path_searching", "src", "topo_prm.cpp"),
           os.path.join(REF, "plan_env", "src", "raycast.cpp"), "-o", exe, "-lpthread"]
    subprocess.check_call(cmd)
    return exe


def write_input(base, sc, probs=None):
    """the driver's input file base.in for the scene (tests/golden/check_topo_host_build.py reads the same file)"""
    cfg = sc["cfg"]
    probs = sc["probs"] if probs is None else probs
    rep = lambda v: " ".join(repr(float(x)) for x in v)
    with open(base + ".in", "w") as f:
        f.write("%d %d %d\n%s\n%r\n" % (tc.NVOX + (rep(tc.ORIGIN), tc.RES)))
        f.write(rep(cfg["sample_inflate"]) + " " + rep([cfg[k] for k in CFG_KEYS]) + "\n")
        f.write("%d %d\n" % (sc["seed"], len(probs)))
        for p in probs:
            f.write(rep(p["start"]) + " " + rep(p["end"]) + " %d " % len(p["start_pts"]) +
                    rep(np.array(p["start_pts"]).reshape(-1)) + " %d " % len(p["end_pts"]) +
                    rep(np.array(p["end_pts"]).reshape(-1)) + "\n")


def run_driver(exe, name, sc, probs=None):
    """-> (the output's lines, the driver's seconds inside findTopoPaths)"""
    base = os.path.join(OUT, name)
    tc.field_of(sc["blocks"]).astype(np.float64).tofile(base + ".field")
    write_input(base, sc, probs)
    p = subprocess.run([exe, base + ".in", base + ".field", base + ".out"], check=True, stdout=subprocess.DEVNULL,
                       stderr=subprocess.PIPE, text=True)
    secs = [float(l.split()[2]) for l in p.stderr.splitlines() if l.startswith("findTopoPaths seconds")][0]
    return open(base + ".out").read().splitlines(), secs


def record(exe, name, sc):
    lines, secs = run_driver(exe, name, sc)
    cfg = sc["cfg"]
    rec = {"source_bits": np.packbits(tc.sources(sc["blocks"])), "nvox": np.array(tc.NVOX), "origin": np.array(tc.ORIGIN),
           "res": np.array(tc.RES), "sample_inflate": np.array(cfg["sample_inflate"], dtype=np.float64),
           "cfg_keys": np.array(CFG_KEYS), "cfg_vals": np.array([float(cfg[k]) for k in CFG_KEYS]),
           "seed": np.array(sc["seed"]), "n_prob": np.array(len(sc["probs"]))}
    tok = lines[0].split()
    rec["samples"] = np.array([float.fromhex(t) for t in tok[1:]]).reshape(-1, 3)
    assert 3 * len(rec["samples"]) == int(tok[0])
    for b, (line, p) in enumerate(zip(lines[1:], sc["probs"])):
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
        rec["start%d" % b], rec["end%d" % b] = np.array(p["start"], dtype=np.float64), np.array(p["end"], dtype=np.float64)
        rec["start_pts%d" % b] = np.array(p["start_pts"], dtype=np.float64).reshape(-1, 3)
        rec["end_pts%d" % b] = np.array(p["end_pts"], dtype=np.float64).reshape(-1, 3)
        ids, kinds, pos, nbs = [], [], [], []
        for _ in range(ints(1)[0]):
            i, k = ints(2)
            ids.append(i), kinds.append(k), pos.append(dbl(3))
            nbs.append(ints(ints(1)[0]))
        rec["node_id%d" % b], rec["node_type%d" % b] = np.array(ids), np.array(kinds)
        rec["node_pos%d" % b] = np.array(pos).reshape(-1, 3)
        rec["nb_off%d" % b] = np.cumsum([0] + [len(v) for v in nbs])
        rec["nb_ids%d" % b] = np.array([i for v in nbs for i in v], dtype=np.int64)
        for key in ("raw", "filt", "sel"):
            lens = []
            pts = []
            for _ in range(ints(1)[0]):
                n = ints(1)[0]
                lens.append(n), pts.append(dbl(3 * n))
            rec[key + "_len%d" % b] = np.array(lens, dtype=np.int64)
            rec[key + "_pts%d" % b] = np.concatenate(pts + [np.zeros(0)]).reshape(-1, 3)
        rec["sel_length%d" % b] = dbl(len(rec["sel_len%d" % b]))
        assert at[0] == len(tok)
    os.makedirs(os.path.join(HERE, "topo"), exist_ok=True)
    path = os.path.join(HERE, "topo", name + ".npz")
    np.savez_compressed(path, **rec)
    return secs, os.path.getsize(path)


if __name__ == "__main__":
    exe = build()
    scenes = tc.scenes()
    for name, sc in scenes.items():
        if name in tc.NOT_RECORDED:
            continue
        secs, size = record(exe, name, sc)
        print("recorded %-20s %6d bytes, the reference's findTopoPaths took %.4f s" % (name, size, secs))
    if os.environ.get("TIMING"):
        n_s = int(os.environ["TIMING"])
        sc = dict(scenes["two_pillars"])
        sc["cfg"] = dict(sc["cfg"], max_sample_num=n_s)
        for n_prob in (1, 8, 64):
            _, secs = run_driver(exe, "timing", sc, probs=sc["probs"] * n_prob)
            print("reference, one core: %2d x two_pillars at %d samples: %.4f s in findTopoPaths" % (n_prob, n_s, secs))
