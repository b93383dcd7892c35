"""Builds k_kino_path's own text for the host (tests/golden/kino_golden/host_kernel.cpp on tests/golden/host_lanes.h: a
thread per lane, glibc's libm, the undefined-behaviour sanitizer) and compares what it writes for every recorded scene with
what the reference's KinodynamicAstar wrote: the two output files must be identical byte for byte (every double is
printed as a hexadecimal float), except the close-goal problem the manager refuses before the search.  Run
tests/golden/make_kino_golden.py first: it leaves the inputs and the reference's outputs under build/kino_golden/.
The cut, the build and the run are tests/golden/host_build.py's."""
import glob
import os
import sys

import host_build as hb


def build():
    return hb.compile("kino", hb.cut("kino_path.hip", "namespace {", "bool pos_fin(", keep_start=False), sanitizers="undefined")


def main():
    exe = build()
    ins = sorted(glob.glob(os.path.join(hb.out_dir("kino"), "*.in")))
    if not ins:
        raise SystemExit("no inputs under build/kino_golden/: run tests/golden/make_kino_golden.py first")
    bad = 0
    for path in ins:
        base = path[:-3]
        name = os.path.basename(base)
        if hb.run(exe, [path, base + ".infl", base + ".unk", base + ".host"], fatal=False) is None:
            print(name, "FAILED")
            bad += 1
            continue
        ref, got = open(base + ".out").read().splitlines(), open(base + ".host").read().splitlines()
        same = [a == b for a, b in zip(ref, got)]
        refused = [not s and b.split()[0] == "5" for s, b in zip(same, got)]  # FUELMI_KINO_CLOSE_GOAL
        ok = len(ref) == len(got) and all(s or r for s, r in zip(same, refused))
        print(name, "identical" if ok else "DIFFERS", "(%d refused as close goals)" % sum(refused) if any(refused) else "")
        bad += not ok
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
