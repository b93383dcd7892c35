"""Rewrites tests/golden/dropin_lkh_imports.txt: the symbols of the TSP solver package (lkh_tsp_solver) that the
reference's exploration manager leaves undefined when the drop-in build (tests/dropin/Makefile) compiles it -- one
"<mangled>\\t<demangled>" line each.  Needs the reference checkout; tests/test_tsp_cpu.py checks that
libfuelmi_lkh.so defines all of them."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _nm(args):
    return subprocess.run(["nm"] + args, capture_output=True, text=True, check=True).stdout.splitlines()


def lkh_imports(obj):
    mangled = [l.split()[-1] for l in _nm(["-u", obj])]
    demangled = [l.split(None, 1)[-1] for l in _nm(["-u", "-C", obj])]
    return sorted((m, d) for m, d in zip(mangled, demangled) if "TSPLKH" in d or "lkh" in d.lower())


def main():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "fuel_amd", "facade"), "-s"])
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "dropin"), "-s"] + sys.argv[1:])
    need = lkh_imports(os.path.join(ROOT, "build", "dropin", "fast_exploration_manager.o"))
    with open(os.path.join(ROOT, "tests", "golden", "dropin_lkh_imports.txt"), "w") as f:
        f.writelines("%s\t%s\n" % md for md in need)
    print("wrote tests/golden/dropin_lkh_imports.txt (%d symbols)" % len(need))


if __name__ == "__main__":
    main()
