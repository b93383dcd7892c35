"""Builds k_kino_path's own text for the host (tests/golden/kino_golden/host_kernel.cpp: a thread per lane, a barrier for
__syncthreads, glibc's libm, the undefined-behaviour sanitizer) and compares what it writes for every recorded scene with
what the reference's KinodynamicAstar wrote: the two output files must be identical byte for byte (every double is
printed as a hexadecimal float), except the close-goal problem the manager refuses before the search.  Run
tests/golden/make_kino_golden.py first: it leaves the inputs and the reference's outputs under build/kino_golden/.
Needs g++ with C++20 and the HIP headers (ROCM_PATH, default /opt/rocm) for the shared declarations; no GPU."""
import glob
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(ROOT, "build", "kino_golden")


def build():
    src = open(os.path.join(ROOT, "fuel_amd", "csrc", "kino_path.hip")).read()
    text = src[src.index("namespace {") + len("namespace {"):src.index("bool pos_fin(")]
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "kernel.inc"), "w") as f:
        f.write(text)
    exe = os.path.join(OUT, "host_kernel")
    subprocess.check_call(["g++", "-O1", "-std=c++20", "-ffp-contract=off", "-fsanitize=undefined", "-w",
                           "-I", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"),
                           "-I", os.path.join(ROOT, "fuel_amd", "csrc"), "-I", OUT,
                           os.path.join(HERE, "kino_golden", "host_kernel.cpp"), "-o", exe, "-lpthread"])
    return exe


def main():
    exe = build()
    ins = sorted(glob.glob(os.path.join(OUT, "*.in")))
    if not ins:
        raise SystemExit("no inputs under build/kino_golden/: run tests/golden/make_kino_golden.py first")
    bad = 0
    for path in ins:
        base = path[:-3]
        name = os.path.basename(base)
        p = subprocess.run([exe, path, base + ".infl", base + ".unk", base + ".host"], capture_output=True, text=True)
        if p.returncode or p.stderr.strip():
            print(name, "FAILED", p.returncode, p.stderr[-500:])
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
