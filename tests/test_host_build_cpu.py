"""The host builds of kernel text (tests/golden/check_*_host_build.py): each script cuts a kernel's own text out of its
.hip, builds it with g++ under sanitizers as a stand-alone program (tests/golden/host_lanes.h: a thread per lane) and
compares what it computes with the restatement or the reference's recorded output, bit for bit.  This test runs each
script as a child process and asks for exit status 0 and the script's own verdict, so that a driver that no longer
compiles, a sanitizer report, a guard hit or a differing bit fails the suite.  No GPU.  A check whose inputs this machine
cannot make is skipped with the reason, never passed."""
import glob
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
REF = os.environ.get("REF", "/root/reference/fuel_planner")  # (make_kino_golden.py's)


def script(name, *args):
    return subprocess.run([sys.executable, os.path.join(GOLDEN, name)] + list(args), capture_output=True, text=True, cwd=ROOT)


def check(name, *args):
    p = script("check_%s_host_build.py" % name, *args)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    return p.stdout.splitlines()


@pytest.mark.parametrize("name", ["traj_check", "traj_sample", "traj_adjust"])
def test_spline_kernels_host_build(name):
    assert check(name)[-1].endswith("all identical, sanitizers silent")


def test_result_block_host_build():
    """the result-block descriptor of the staged batch calls (csrc/block_layout.h): no kernel text, host memory only"""
    assert check("result_block")[-1].endswith("all passed, sanitizers silent")


def test_map_cloud_host_build():
    import fuel_amd._lib as fl
    if not os.path.exists(fl.LIB_PATH):
        pytest.skip("the map_cloud scenes are made through the built library; %s is not built" % fl.LIB_PATH)
    assert check("map_cloud")[-1].endswith("all identical, sanitizers silent")


def test_inflate_host_build():
    """the inflation kernels and their launch ranges on planes of exactly the allocated size, every scene of
    tests/inflate_cases.py through the fused kernel and the factored pair, against the oracle"""
    assert check("inflate")[-1].endswith("all identical, sanitizers silent")


def test_kino_host_build():
    if not glob.glob(os.path.join(ROOT, "build", "kino_golden", "*.in")):
        if not os.path.isdir(REF):
            pytest.skip("the kino inputs and the reference's outputs under build/kino_golden/ are made by "
                        "tests/golden/make_kino_golden.py from the reference checkout, which is not at %s" % REF)
        p = script("make_kino_golden.py")
        assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    lines = check("kino")
    assert lines and all(ln.split()[1] == "identical" for ln in lines), lines
