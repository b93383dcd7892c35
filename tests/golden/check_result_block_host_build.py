"""Builds tests/golden/result_block_golden/host_kernel.cpp -- ResultBlock and BlockLayout of fuel_amd/csrc/block_layout.h
on host memory only, no kernel text and no HIP -- with the address and the undefined-behaviour sanitizers as a stand-alone
program and runs it: sizing against binding at alignments 16 and 256, the three kinds of entry, the scatter between guard
bytes, element counts 0 and 1, a block embedded in a larger BlockLayout, the overflow of the entry table.  The build and
the run are tests/golden/host_build.py's; everything stays under build/result_block_golden/."""
import sys

import host_build as hb


def main():
    exe = hb.compile("result_block", "")
    out = hb.run(exe, [])
    print(out, end="")
    sys.exit(0 if out.splitlines()[-1].endswith("all passed, sanitizers silent") else 1)


if __name__ == "__main__":
    main()
