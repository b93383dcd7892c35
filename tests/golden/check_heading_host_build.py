"""Builds k_info_gain's and k_yaw_path's own text and the host's view setup for the host
(tests/golden/heading_golden/host_kernel.cpp on tests/golden/host_lanes.h: a thread per lane, guard zones round the LDS
block) with the address and the undefined-behaviour sanitizers as a stand-alone program, runs it on every scene of
tests/heading_cases.py -- the gain scenes grouped into launches by map and configuration, every path scene, the scene at
the reference's defaults -- and compares every output with the restatement (tests/heading_ref.py, sums in the device's
order) bit for bit: on the host the kernel's exp is the C library's, like the restatement's.  Everything stays under
build/heading_golden/; the cut, the build and the run are tests/golden/host_build.py's.  Nothing is loaded into Python and
nothing runs on a GPU."""
import os
import sys

import numpy as np

import host_build as hb

sys.path.insert(0, os.path.join(hb.ROOT, "tests"))

import heading_cases as hc  # noqa: E402
import heading_ref as hr  # noqa: E402

CFG_KEYS = ("weight_type", "in_box", "factor", "far", "top_ang", "left_ang", "right_ang", "lambda1", "lambda2")


def build():
    return hb.compile("heading", hb.lds_from_host(hb.cut("info_gain.hip", "namespace {", "bool fin3(")))


def plane(a):
    """a bool [nx, ny, nz] array as the 64-bit words of a bit plane over the linear voxel address"""
    bits = np.packbits(a.reshape(-1), bitorder="little")
    bits = np.concatenate([bits, np.zeros((-len(bits)) % 8, dtype=np.uint8)])
    return bits.view("<u8")


def cfg_tokens(c, max_yaw, max_ctrl):
    return "%d %d %d %d %d %s" % (c["weight_type"], 1 if c["in_box"] else 0, c["factor"], max_yaw, max_ctrl,
                                  " ".join(float(c[k]).hex() for k in CFG_KEYS[3:]))


def main():
    exe = build()
    out = hb.out_dir("heading")
    scenes = hc.all_scenes()
    names = sorted({s["map"] for s in scenes})
    ggroups = {}
    for sc in scenes:
        if sc["kind"] == "gain":
            ggroups.setdefault((names.index(sc["map"]),) + tuple(sc["cfg"][k] for k in CFG_KEYS), []).append(sc)
    paths = [s for s in scenes if s["kind"] == "path"]
    path = os.path.join(out, "scenes.in")
    want = []
    with open(path, "w") as f:
        f.write("%d\n" % len(names))
        for name in names:
            m = hc.spec(name)
            r = m.ref()
            fu, fo = os.path.join(out, name + ".unk"), os.path.join(out, name + ".occ")
            plane(m.unk).tofile(fu), plane(m.occ).tofile(fo)
            f.write("%d %d %d %s %s %s %s %s %s %s\n" % (m.nvox + (hb.hexes(m.origin), float(r.res_inv).hex(), float(r.res).hex(),
                                                               hb.hexes(m.box_min), hb.hexes(m.box_max),
                                                               " ".join(str(v) for v in r.box_min + r.box_max), fu + " " + fo)))
        for key, grp in ggroups.items():
            c = grp[0]["cfg"]
            my = max(len(s["yaws"]) for s in grp) + 1
            ctrls = [s["ctrl"] for s in grp] if c["weight_type"] == hr.NON_UNIFORM else []
            mc = max([len(x) for x in ctrls] + [1]) + 1
            f.write("G %d %d %s\n" % (key[0], len(grp), cfg_tokens(c, my, mc)))
            for b, sc in enumerate(grp):
                f.write("%s %d %s %d\n" % (hb.hexes(sc["pos"]), len(sc["yaws"]), hb.hexes(sc["yaws"]), b if ctrls else 0))
                r = hc.restate(sc)
                tok = [0, r["n_rays"]]
                for v in range(my):
                    tok += [r["n_cand"][v], r["n_visible"][v], hb.bits(r["gain"][v])] if v < len(sc["yaws"]) else [0, 0, hb.bits(0.0)]
                want.append((sc["tag"], " ".join(str(t) for t in tok)))
            f.write("%d\n" % len(ctrls))
            for x in ctrls:
                f.write("%d %s\n" % (len(x), hb.hexes(x)))
        for sc in paths:
            c, L, nv = sc["cfg"], len(sc["yaws"]), 2 * sc["h"] + 1
            ml = L + 1
            mc = (len(sc["ctrl"]) if sc["ctrl"] is not None else 0) + 1
            given = sc["gains_in"] is not None
            f.write("P %d 1 %d %d %s %s %s %d %s\n" % (names.index(sc["map"]), sc["h"], ml, float(sc["yaw_diff"]).hex(),
                                                     float(sc["max_yaw_rate"]).hex(), float(sc["w"]).hex(), 1 if given else 0,
                                                     cfg_tokens(c, nv, mc)))
            f.write("%d %s %s %s\n" % (L, float(sc["dt"]).hex(), hb.hexes(sc["pts"]), hb.hexes(sc["yaws"])))
            f.write("%d %s\n" % (mc - 1, hb.hexes(sc["ctrl"]) if sc["ctrl"] is not None else ""))
            if given:
                g = np.zeros((ml, nv))
                g[:L] = sc["gains_in"][:L]
                f.write(hb.hexes(g) + "\n")
            r = hc.restate(sc)
            tok = [0]
            for i in range(L):
                tok += [r["n_rays"][i], r["path_vertex"][i], hb.bits(r["path"][i])]
            for i in range(L):
                for j in range(nv):
                    inner = 0 < i < L - 1
                    gain = (float(sc["gains_in"][i][j]) if given else r["gains"][i][j]) if (inner or given) else 0.0
                    gv = r["g_value"][i][j] if j < len(r["g_value"][i]) else 0.0
                    tok += [hb.bits(gain), hb.bits(gv)]
            want.append((sc["tag"], " ".join(str(t) for t in tok)))
    lines = hb.run(exe, [path]).splitlines()
    assert len(lines) == len(want), (len(lines), len(want))
    bad = 0
    for (tag, exp), line in zip(want, lines):
        if line.strip() != exp:
            print(tag, "DIFFERS\n  host build:  ", line[:600], "\n  restatement: ", exp[:600])
            bad += 1
    print("%d groups and problems in %d + %d launches: %s" % (len(want), len(ggroups), len(paths),
                                                             "all identical, sanitizers silent" if not bad else "%d DIFFER" % bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
