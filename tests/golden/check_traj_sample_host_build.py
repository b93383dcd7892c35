"""Builds k_traj_sample's own text for the host (tests/golden/traj_sample_golden/host_kernel.cpp on
tests/golden/host_lanes.h: a thread per lane, guard zones round the LDS block) with the address and the
undefined-behaviour sanitizers, runs it once on every scene of tests/traj_sample_cases.py -- grouped into launches by
mode and degrees, so that problems of different sizes share workgroups -- plus a launch laid out like a device batch
with a bad knot span among good neighbours, and compares every output with the restatement (tests/traj_sample_ref.py)
bit for bit.  Everything stays under build/traj_sample_golden/; the cut, the build and the run are
tests/golden/host_build.py's."""
import os
import sys

import numpy as np

import host_build as hb
from host_build import bits, hexes

sys.path.insert(0, os.path.join(hb.ROOT, "tests"))

import traj_sample_cases as tc  # noqa: E402
import traj_sample_ref as sr  # noqa: E402


def build():
    text = hb.lds_from_host(hb.cut("traj_sample.hip", "namespace {", "size_t ts_lds("))
    return hb.compile("traj_sample", text + hb.cut("traj_sample.hip", "size_t ts_lds(", "int trajsmp_cfg_check("))


def batch_scenes():
    """a launch laid out like a device batch (every problem the stride's number of points, no n_ctrl array): knot spans
    0, not a number and infinite among good neighbours; the carried record of a bad problem must come back untouched"""
    out = []
    for b, dt in enumerate((0.2, 0.0, 0.21, float("nan"), float("inf"), 0.19, -0.1)):
        sc = tc.scene("batch_%d" % b, sr.COMMAND, 3, tc.wiggle(16, 300 + b), dt, tc.tape(70 if b != 2 else 3, 0.05, -0.1))
        sc["flight0"] = [float(v) for v in np.arange(8.0) + 8 * b]
        out.append(sc)
    return out


def main():
    exe = build()
    launches = [(k, g, False) for k, g in tc.groups(tc.quick_scenes()).items()]
    launches.append(((sr.COMMAND, 3, 3), tc.big_scenes(), False))
    launches.append(((sr.COMMAND, 3, 0), batch_scenes(), True))
    path = os.path.join(hb.out_dir("traj_sample"), "scenes.in")
    order = []
    with open(path, "w") as f:
        f.write("%d\n" % len(launches))
        for (mode, degree, py), grp, batch in launches:
            maxc = max(len(sc["ctrl"]) for sc in grp) + (0 if batch or len(grp[0]["ctrl"]) == sr.MAX_CTRL else 1)
            maxy = max([len(sc["yaw"]["ctrl"]) for sc in grp if sc["yaw"]] + [0])
            maxt = max(len(sc["t"]) for sc in grp) + 3
            stop = any(sc["t_stop"] is not None for sc in grp)
            command = mode == sr.COMMAND
            f.write("%d %d %d %d %d %d %d %d %d %d %d\n" % (mode, degree, py or 3, maxc, maxy, maxt, len(grp), 1 if maxy else 0,
                                                         1 if stop else 0, 1 if command else 0, 1 if batch else 0))
            for sc in grp:
                y = sc["yaw"]
                f.write("%d %s %s\n" % (len(sc["ctrl"]), float(sc["dt"]).hex(), hexes(sc["ctrl"])))
                f.write("%d %s %s\n" % (len(y["ctrl"]) if y else 0, float(y["dt"] if y else 1.0).hex(), hexes(y["ctrl"]) if y else ""))
                f.write("%s %s\n" % (float(sc["t_stop"] if sc["t_stop"] is not None else 1e300).hex(), hexes(sc.get("flight0", [0.0] * 8))))
                f.write("%d %s\n" % (len(sc["t"]), hexes(sc["t"])))
                order.append((sc, maxt))
    lines = hb.run(exe, [path]).splitlines()
    assert len(lines) == sum(1 + maxt for _, maxt in order), (len(lines), len(order))
    bad = at = 0
    for sc, maxt in order:
        y = sc["yaw"]
        r = sr.sample(sc["mode"], sc["ctrl"], sc["degree"], sc["dt"], sc["t"], y["ctrl"] if y else None, y["degree"] if y else 3,
                      y["dt"] if y else None, sc["t_stop"])
        fl = sc.get("flight0", [0.0] * 8)
        if sc["mode"] == sr.COMMAND and r["duration"] != 0.0:
            fl = sr.record_windowed(fl, sc["t"], r, tc.WIN)
        want = ["P " + " ".join(bits(v) for v in [r["duration"]] + list(fl))]
        for k in range(maxt):
            if k < len(sc["t"]):
                vals = r["pos"][k] + r["vel"][k] + r["acc"][k] + r["jerk"][k] + [r["yaw"][k], r["yawdot"][k], r["yawddot"][k]]
                want.append("%d %s" % (r["status"][k], " ".join(bits(v) for v in vals)))
            else:
                want.append("0 " + " ".join([bits(0.0)] * 15))
        got = lines[at:at + 1 + maxt]
        at += 1 + maxt
        if got != want:
            first = next(i for i in range(len(want)) if got[i] != want[i])
            print(sc["tag"], "DIFFERS at line", first, "\n  host build:  ", got[first], "\n  restatement: ", want[first])
            bad += 1
    sizes = sorted(len(g) for _, g, _ in launches)
    print("%d scenes in %d launches (problems per launch: %s): %s" %
          (len(order), len(launches), sizes, "all identical, sanitizers silent" if not bad else "%d DIFFER" % bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
