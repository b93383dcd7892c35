"""Builds k_traj_check's own text for the host (tests/golden/traj_check_golden/host_kernel.cpp on
tests/golden/host_lanes.h: a thread per lane, guard zones round the LDS block) with the address and the
undefined-behaviour sanitizers, runs it once on every scene of tests/traj_check_cases.py -- grouped into launches by map
and configuration, so that problems of different sizes share workgroups -- and compares every output with the restatement
(tests/traj_check_ref.py) bit for bit.  Everything stays under build/traj_check_golden/; the cut, the build and the run are
tests/golden/host_build.py's.  `--long` adds the two 2^20-sample scenes."""
import os
import sys

import numpy as np

import host_build as hb
from host_build import bits

sys.path.insert(0, os.path.join(hb.ROOT, "tests"))

import traj_check_cases as tc  # noqa: E402


def build():
    text = hb.lds_from_host(hb.cut("traj_check.hip", "namespace {", "size_t tc_lds("))
    return hb.compile("traj_check", text + hb.cut("traj_check.hip", "size_t tc_lds(", "int trajchk_cfg_check("))


def main():
    exe = build()
    scenes = tc.quick_scenes() + (tc.long_scenes() if "--long" in sys.argv else [])
    names = sorted(tc.MAPS)
    groups = {}
    for sc in scenes:
        groups.setdefault((names.index(sc["map"]), sc["degree"], sc["step"], sc["max_radius"]), []).append(sc)
    path = os.path.join(hb.out_dir("traj_check"), "scenes.in")
    order = []
    with open(path, "w") as f:
        f.write("%d\n" % len(names))
        for name in names:
            m = tc.spec(name)
            adr = np.nonzero(m.infl3.reshape(-1))[0]
            f.write("%d %d %d %s %s %s %s\n%d %s\n" % (m.nvox + tuple(float(v).hex() for v in m.origin) + (float(m.res_inv).hex(),)
                                                        + (len(adr), " ".join(str(a) for a in adr))))
        f.write("%d\n" % len(groups))
        for (mi, degree, step, radius), grp in groups.items():
            maxc = max(len(sc["ctrl"]) for sc in grp) + 1
            f.write("%d %d %d %d %s %s\n" % (mi, len(grp), degree, maxc, float(step).hex(), float(radius).hex()))
            for sc in grp:
                f.write("%d %s %s %s\n" % (len(sc["ctrl"]), float(sc["dt"]).hex(), float(sc["t_now"]).hex(),
                                           " ".join(float(v).hex() for v in sc["ctrl"].reshape(-1))))
                order.append(sc)
    lines = hb.run(exe, [path]).splitlines()
    assert len(lines) == len(order), (len(lines), len(order))
    bad = 0
    for sc, line in zip(order, lines):
        r = tc.restate(sc, "first_hit", width=8192 if sc["tag"].startswith("cap") else 64)
        want = "%d %d %d %d %d %s" % (r["status"], r["safe"], r["n_samples"], r["hit_index"], r["end_reason"],
                                      " ".join(bits(v) for v in [r["distance"], r["hit_t"], r["duration"]] + r["hit_pos"]))
        if want != line:
            print(sc["tag"], "DIFFERS\n  host build:  ", line, "\n  restatement: ", want)
            bad += 1
    sizes = sorted(len(g) for g in groups.values())
    print("%d scenes in %d launches (problems per launch: %s): %s" %
          (len(order), len(groups), sizes, "all identical, sanitizers silent" if not bad else "%d DIFFER" % bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
