"""Builds the cloud kernels' own text for the host (tests/golden/map_cloud_golden/host_kernel.cpp on
tests/golden/host_lanes.h: a thread per lane, every array a heap block of its exact size, one margin word
behind each plane) as a stand-alone program with the address and the undefined-behaviour sanitizers, runs it once on every
scene of tests/map_cloud_cases.py with every kind -- plus the cap scenes, whose buffers must keep their fill behind the
points, and map E's full box, whose scan takes two rounds -- and compares counts and points with the restatement
(tests/map_cloud_ref.py) bit for bit.  The planes are packed here from the scenes' log-odds with the comparisons of
k_state_planes, which is not under test.  Everything stays under build/map_cloud_golden/; the cut, the build and
the run are tests/golden/host_build.py's.  `--quick` leaves map E out."""
import os
import struct
import sys

import numpy as np

import host_build as hb

sys.path.insert(0, os.path.join(hb.ROOT, "tests"))
sys.path.insert(0, hb.ROOT)

import map_cloud_cases as mc  # noqa: E402
import map_cloud_ref as mr  # noqa: E402

FILL = b"\xA5\xA5\xA5\xA5"


def build():
    return hb.compile("map_cloud", hb.cut("map_cloud.hip", "namespace {", "// the geometry of a box:"))


def pack(bits3):
    b = np.packbits(bits3.reshape(-1), bitorder="little")
    w = (bits3.size + 63) // 64
    return b.tobytes() + bytes(8 * w - len(b))


def main():
    exe = build()
    states, blobs, jobs = {}, [], []  # (map, state) -> index; the planes file; (state index, scene, kind, cap, occ, infl, P)

    def state_of(m, name, occ, infl):
        if (m.name, name) not in states:
            states[(m.name, name)] = len(blobs)
            blobs.append(struct.pack("<3i4d", *m.nvox, m.res, *m.origin)
                         + pack(occ > m.P.min_occupancy_log) + pack(occ < m.P.unknown_thr) + pack(infl == 1))
        return states[(m.name, name)]

    for sc in mc.scenes():
        m = mc.spec(sc["map"])
        occ, infl = m.state(sc["state"])
        si = state_of(m, sc["state"], occ, infl)
        for kind in mr.KINDS:
            caps = [1 << 40]
            if sc["tag"] == mc.CAP_SCENE:
                n = len(mc.restate(sc, kind))
                caps += [f(n) for _, f in mc.CAPS]
            for cap in caps:
                jobs.append((si, sc, kind, cap, m, occ, infl))
    if "--quick" not in sys.argv:
        e = mc.map_e()
        occ = mc.e_state(e)
        infl = np.zeros(e.nvox, dtype=np.int8)
        si = state_of(e, "e", occ, infl)
        sc = mc.scene("map_e", "e", "e", *mc.full_box(e.nvox))
        jobs.append((si, sc, mr.OCCUPIED, 1 << 40, e, occ, infl))
        jobs.append((si, sc, mr.KNOWN, 1000, e, occ, infl))
    p_planes, p_scenes, p_out = (os.path.join(hb.out_dir("map_cloud"), n) for n in ("planes.bin", "scenes.txt", "out.bin"))
    with open(p_planes, "wb") as f:
        f.write(struct.pack("<i", len(blobs)) + b"".join(blobs))
    with open(p_scenes, "w") as f:
        f.write("%d\n" % len(jobs))
        for si, sc, kind, cap, *_ in jobs:
            f.write("%d %d %d %d %d %d %d %d %s %s %d\n" % ((si, kind) + sc["lo"] + sc["hi"]
                                                            + (float(sc["z_low"]).hex(), float(sc["z_high"]).hex(), cap)))
    hb.run(exe, [p_planes, p_scenes, p_out])
    raw = open(p_out, "rb").read()
    at, bad = 0, 0
    for si, sc, kind, cap, m, occ, infl in jobs:
        total, nw = struct.unpack_from("<2i", raw, at)
        buf = raw[at + 8:at + 8 + 12 * nw]
        at += 8 + 12 * nw
        # the device holds the planes: KNOWN is the complement of the unknown plane
        want = mr.extract(m.P, occ, infl, kind, sc["lo"], sc["hi"], sc["z_low"], sc["z_high"], known_as="plane")
        k = min(len(want), nw)
        ok = total == len(want) and buf[:12 * k] == want[:k].tobytes() and buf[12 * k:] == FILL * (3 * (nw - k))
        if not ok:
            print(sc["tag"], mr.KIND_NAMES[kind], "cap", cap, "DIFFERS: total", total, "want", len(want))
            bad += 1
    assert at == len(raw)
    print("%d launches of %d map states: %s" % (len(jobs), len(blobs),
                                                "all identical, sanitizers silent" if not bad else "%d DIFFER" % bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
