"""What the check_*_host_build.py scripts share: a kernel's own text cut out of its .hip into
build/<name>_golden/kernel.inc, the driver tests/golden/<name>_golden/host_kernel.cpp (on tests/golden/host_lanes.h)
compiled round it by g++ with sanitizers as a stand-alone program, its run, and the bits of a double as the drivers print
them.  Needs g++ with C++20 and the HIP headers (ROCM_PATH, default /opt/rocm) for the shared declarations; no GPU."""
import os
import struct
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "fuel_amd", "csrc")
SMEM_DECL = "extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];"


def out_dir(name):
    d = os.path.join(ROOT, "build", name + "_golden")
    os.makedirs(d, exist_ok=True)
    return d


def cut(path, start, end, keep_start=True):
    """the text of fuel_amd/csrc/<path> from the first `start` (with it, or behind it) up to the first `end`"""
    src = open(os.path.join(CSRC, path)).read()
    a = src.index(start)
    return src[a if keep_start else a + len(start):src.index(end)]


def lds_from_host(text):
    """the one line of a kernel that differs in a host build: the address of its LDS block"""
    assert text.count(SMEM_DECL) == 1
    return text.replace(SMEM_DECL, "unsigned char* smem_raw = g_lds;")


def compile(name, text, sanitizers="address,undefined"):
    """kernel.inc = text; the driver built round it -> the program's path"""
    out = out_dir(name)
    with open(os.path.join(out, "kernel.inc"), "w") as f:
        f.write(text)
    exe = os.path.join(out, "host_kernel")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++20", "-ffp-contract=off", "-fsanitize=" + sanitizers,
                           "-fno-sanitize-recover=undefined", "-w",
                           "-I", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"),
                           "-I", CSRC, "-I", HERE, "-I", out,
                           os.path.join(HERE, name + "_golden", "host_kernel.cpp"), "-o", exe, "-lpthread"])
    return exe


def run(exe, args, fatal=True):
    """the program's stdout; a return code or anything on stderr (a sanitizer's report) is a failure: the script ends
    (fatal) or None comes back"""
    p = subprocess.run([exe] + list(args), capture_output=True, text=True)
    if p.returncode or p.stderr.strip():
        print("FAILED", p.returncode, p.stdout[-300:], p.stderr[-3000:])
        if fatal:
            sys.exit(1)
        return None
    return p.stdout


def bits(v, one_nan=False):
    """a double as the drivers print it.  one_nan: a generated NaN is one NaN (its sign is the processor's choice)"""
    v = float(v)
    return "%016x" % (0x7ff8000000000000 if one_nan and v != v else struct.unpack("<Q", struct.pack("<d", v))[0])


def from_bits(token):
    return struct.unpack("<d", struct.pack("<Q", int(token, 16)))[0]


def hexes(a):
    return " ".join(float(v).hex() for v in np.asarray(a, dtype=np.float64).reshape(-1))
