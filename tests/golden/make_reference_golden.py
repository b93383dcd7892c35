"""Rewrites tests/golden/reference/*.npz: the REAL reference's observations that tests/test_oracle_vs_reference_cpu.py
compares the oracle with (tests/reference_tape.py).  Needs oracle/_ref (built by __graft_entry__.build() where the
reference checkout is present); runs that module once with FUELMI_RECORD_REFERENCE=1."""
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    sys.path.insert(0, ROOT)
    from oracle.ref_build import ref
    if not (ref.available() and ref.mapros_available()):
        sys.exit("oracle/_ref is not built: run __graft_entry__.build() where the reference checkout is present")
    shutil.rmtree(os.path.join(ROOT, "tests", "golden", "reference"), ignore_errors=True)
    env = dict(os.environ, FUELMI_RECORD_REFERENCE="1")
    subprocess.check_call([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider",
                           os.path.join(ROOT, "tests", "test_oracle_vs_reference_cpu.py")], cwd=ROOT, env=env)


if __name__ == "__main__":
    main()
