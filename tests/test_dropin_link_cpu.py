"""Drop-in link proof (north_star: "exploration_manager / plan_manage link against the new library
unchanged").  The reference's own callers of the hot path -- fast_exploration_manager.cpp:88-293,
planner_manager.cpp:96-118,124-316, astar2.cpp:97-109, kinodynamic_astar.cpp:172-177, graph_node.cpp:38 -- compiled
unmodified against fuel_amd/facade/ (tests/dropin/Makefile) leave the SDFMap / EDTEnvironment / FrontierFinder /
BsplineOptimizer symbols listed in tests/golden/dropin_caller_imports.txt undefined (tests/golden/make_dropin_golden.py
writes that list where the reference checkout is present); every one of them must be defined by the facade library.
CPU only."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dropin_caller_imports.txt")
CLASSES = r"fast_planner::(SDFMap|EDTEnvironment|FrontierFinder|BsplineOptimizer)::"


def _nm(args):
    return subprocess.run(["nm"] + args, capture_output=True, text=True, check=True).stdout.splitlines()


def test_no_unresolved_hot_path_symbol():
    """every fast_planner::{SDFMap,EDTEnvironment,FrontierFinder,BsplineOptimizer}:: symbol the callers leave
    undefined is exported by libfuelmi_facade.so (mangled names compared: same signatures, not just same names)"""
    subprocess.run(["make", "-C", os.path.join(ROOT, "fuel_amd", "facade"), "-s"], check=True)
    need = [tuple(l.rstrip("\n").split("\t", 1)) for l in open(GOLDEN) if l.strip()]
    assert all(re.search(CLASSES, d) for _, d in need)
    assert len(need) >= 30, "the callers reference the hot-path classes: %d symbols found" % len(need)
    have = {l.split()[-1] for l in _nm(["-D", "--defined-only", os.path.join(ROOT, "fuel_amd", "libfuelmi_facade.so")])}
    missing = sorted(d for m, d in need if m not in have)
    assert not missing, "unresolved against libfuelmi_facade.so:\n" + "\n".join(missing)
