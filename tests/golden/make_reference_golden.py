"""Rewrites tests/golden/reference/*.npz: the REAL reference's observations that the modules of MODULES compare the
oracle with (tests/reference_tape.py).  Needs oracle/_ref (built by __graft_entry__.build() where the reference checkout
is present); runs the modules once with FUELMI_RECORD_REFERENCE=1.  With module names as arguments only those are run
and only their files are rewritten."""
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
MODULES = ("test_oracle_vs_reference_cpu.py", "test_fusion_edges_cpu.py", "test_frontier_split_cpu.py")


def main():
    sys.path.insert(0, ROOT)
    from oracle.ref_build import ref
    if not (ref.available() and ref.mapros_available()):
        sys.exit("oracle/_ref is not built: run __graft_entry__.build() where the reference checkout is present")
    only = [a for a in sys.argv[1:] if a in MODULES]
    if len(only) != len(sys.argv) - 1:
        sys.exit("unknown module; known: %s" % ", ".join(MODULES))
    if not only:
        shutil.rmtree(os.path.join(ROOT, "tests", "golden", "reference"), ignore_errors=True)
    env = dict(os.environ, FUELMI_RECORD_REFERENCE="1")
    subprocess.check_call([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider"] +
                          [os.path.join(ROOT, "tests", m) for m in (only or MODULES)], cwd=ROOT, env=env)


if __name__ == "__main__":
    main()
