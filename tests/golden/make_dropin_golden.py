"""Rewrites tests/golden/dropin_caller_imports.txt: every fast_planner::{SDFMap,EDTEnvironment,FrontierFinder,
BsplineOptimizer}:: symbol the reference's own callers of the hot path (tests/dropin/Makefile: the exploration manager,
the planner manager, both A* searches, ViewNode) leave undefined when compiled against fuel_amd/facade/ -- one
"<mangled>\\t<demangled>" line each.  Needs the reference checkout (tests/dropin/Makefile REF=...);
tests/test_dropin_link_cpu.py checks that libfuelmi_facade.so defines all of them."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CLASSES = r"fast_planner::(SDFMap|EDTEnvironment|FrontierFinder|BsplineOptimizer)::"


def _nm(args):
    return subprocess.run(["nm"] + args, capture_output=True, text=True, check=True).stdout.splitlines()


def main():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "fuel_amd", "facade"), "-s"])
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "dropin"), "-s"] + sys.argv[1:])
    out = os.path.join(ROOT, "build", "dropin")
    need = set()
    for o in sorted(f for f in os.listdir(out) if f.endswith(".o")):
        mangled = [l.split()[-1] for l in _nm(["-u", os.path.join(out, o)])]
        demangled = [l.split(None, 1)[-1] for l in _nm(["-u", "-C", os.path.join(out, o)])]
        need.update((m, d) for m, d in zip(mangled, demangled) if re.search(CLASSES, d))
    with open(os.path.join(ROOT, "tests", "golden", "dropin_caller_imports.txt"), "w") as f:
        f.writelines("%s\t%s\n" % md for md in sorted(need))
    print("wrote tests/golden/dropin_caller_imports.txt (%d symbols)" % len(need))


if __name__ == "__main__":
    main()
