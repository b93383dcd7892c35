"""Builds the inflation kernels' own text for the host (tests/golden/inflate_golden/host_kernel.cpp on
tests/golden/host_lanes.h: a thread per lane) as a stand-alone program with the address and the undefined-behaviour
sanitizers: k_box_and, k_inflate_yz, k_inflate_x, k_inflate_fused and the launch ranges cut out of map_core.hip,
box_mask_word and bit_range out of fuelmi_internal.h.  Every bit-plane is a heap block of exactly W + 2 * margin_words + 2
words, the fused kernel's LDS a guarded block of exactly lds_f bytes, so a window load that leaves a plane by one word --
which no device run can see -- is reported.  Runs every scene of tests/inflate_cases.py through the fused kernel (step 2
only) and through the factored pair (every step), the scratch planes pre-filled as stale words would be, and compares the
inflated plane after every call with the oracle's, bit for bit.  The planes are packed here from the scenes' log-odds with
the comparison of k_state_planes, which is not under test.  Everything stays under build/inflate_golden/; the cut, the
build and the run are tests/golden/host_build.py's."""
import os
import struct
import sys

import numpy as np

import host_build as hb

sys.path.insert(0, os.path.join(hb.ROOT, "tests"))
sys.path.insert(0, hb.ROOT)

import inflate_cases as ic  # noqa: E402


def build():
    helpers = hb.cut("fuelmi_internal.h", "__device__ __forceinline__ u64 bit_range", "#endif  // __HIPCC__")
    kernels = hb.lds_from_host(hb.cut("map_core.hip", "// S[w] = occupied[w] & box(w)", "// virtual ceiling"))
    ranges = hb.cut("map_core.hip", "// ---- the launch ranges of the inflation", "// ---- end of the launch ranges")
    for name in ("k_box_and", "k_inflate_yz", "k_inflate_x", "k_inflate_fused"):
        assert kernels.count(name + "(") == 1, name
    assert "box_mask_word" in helpers and "inflate_plan(" in ranges and "inflate_margin_words(" in ranges
    return hb.compile("inflate", helpers + kernels + ranges)


def pack(bits):
    b = np.packbits(np.asarray(bits, dtype=bool), bitorder="little")
    w = (len(bits) + 63) // 64
    return b.tobytes() + bytes(8 * w - len(b))


def main():
    exe = build()
    jobs = []  # (scene, pin of the run, [kernel per call], [plane per call])
    blob = []
    for sc in ic.SCENES:
        occ, planes, (l_min, l_max, l_occ) = ic.expected(sc)
        pre = np.zeros(sc.N, dtype=bool)
        pre[list(sc.pre)] = True
        for pin in sc.pins[1:]:  # (AUTO is one of the two on every map of the table)
            jobs.append((sc, pin, [sc.kernel_of(pin, c) for c in sc.calls], planes))
            blob.append(struct.pack("<5i", *sc.dims, sc.step, len(sc.calls)) + pack(occ > l_occ) + pack(pre))
            for c in sc.calls:
                blob.append(struct.pack("<7i", *c[0], *c[1], sc.kernel_of(pin, c)))
    p_in, p_out = (os.path.join(hb.out_dir("inflate"), n) for n in ("jobs.bin", "out.bin"))
    with open(p_in, "wb") as f:
        f.write(struct.pack("<i", len(jobs)) + b"".join(blob))
    hb.run(exe, [p_in, p_out])
    raw = open(p_out, "rb").read()
    at, bad, calls, ran = 0, 0, 0, set()
    for sc, pin, kernels, planes in jobs:
        for i, (k, want) in enumerate(zip(kernels, planes)):
            got_k, = struct.unpack_from("<i", raw, at)
            got = raw[at + 4:at + 4 + 8 * sc.W]
            at += 4 + 8 * sc.W
            calls += 1
            ran.add((got_k, sc.step if sc.step == 2 else 0))
            if got_k != k or got != pack(want == 1):
                print(sc.name, "pin", pin, "call", i, "DIFFERS" if got_k == k else "ran kernel %d, not %d" % (got_k, k))
                bad += 1
    assert at == len(raw)
    assert ran == {(ic.FUSED, 2), (ic.FACTORED, 2), (ic.FACTORED, 0)}, ran
    print("%d calls of %d runs of %d scenes: %s" % (calls, len(jobs), len(ic.SCENES),
                                                    "all identical, sanitizers silent" if not bad else "%d DIFFER" % bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
