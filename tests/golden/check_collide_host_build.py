"""Builds k_collide_range's and k_guide_points' own text for the host (tests/golden/collide_golden/host_kernel.cpp on
tests/golden/host_lanes.h: a thread per lane, guard zones round the LDS block) with the address and the undefined-behaviour
sanitizers as a stand-alone program, runs it on every scene of tests/collide_cases.py -- the collision scenes grouped into
launches by map and configuration, on the f32 rounding of the scene's field, so that problems of different sizes share
workgroups; the limit scenes and the non-finite control point among good neighbours; the guide scenes grouped by
configuration -- and compares every output with the restatement (tests/collide_ref.py, `cut` mode) bit for bit.  Everything
stays under build/collide_golden/; the cut, the build and the run are tests/golden/host_build.py's."""
import os
import sys

import numpy as np

import host_build as hb

sys.path.insert(0, os.path.join(hb.ROOT, "tests"))

import collide_cases as cc  # noqa: E402


def build():
    text = hb.lds_from_host(hb.cut("collide_range.hip", "namespace {", "size_t cr_lds("))
    return hb.compile("collide", text + hb.cut("collide_range.hip", "size_t cr_lds(", "int colrange_cfg_check("))


def one_nan(tokens):
    """the driver's bit patterns with every NaN made the one NaN hb.bits(one_nan=True) prints"""
    return [hb.bits(hb.from_bits(t), one_nan=True) if len(t) == 16 else t for t in tokens]


def rows(points, cap):
    return [hb.bits(v, one_nan=True) for p in list(points)[:cap] for v in p]


def main():
    exe = build()
    out = hb.out_dir("collide")
    names = sorted(cc.MAPS)
    over_ev, over_pts = cc.limit_scenes()
    scenes = cc.collision_scenes()
    good = [s for s in scenes if s["tag"] in ("enter_64", "leave_64")]
    extra = [dict(s, max_events=over_ev["max_events"]) for s in scenes if s["tag"] in ("enter_64_deg5", "leave_64_deg5")] + \
        [over_ev] + [dict(s, max_pts=over_pts["max_pts"]) for s in good] + [over_pts] + [cc.nonfinite_scene()]
    groups = {}
    for sc in scenes + extra:
        groups.setdefault((names.index(sc["map"]), sc["degree"], sc["max_events"], sc["max_pts"], sc["clearance"]), []).append(sc)
    ggroups = {}
    for sc in cc.guide_scenes():
        ggroups.setdefault((sc["degree"], sc["max_guide"], sc["ctrl_pt_dist"]), []).append(sc)
    path = os.path.join(out, "scenes.in")
    want = []
    with open(path, "w") as f:
        f.write("%d\n" % len(names))
        for name in names:
            m = cc.spec(name)
            fp = os.path.join(out, name + ".f32")
            m.f32().tofile(fp)
            f.write("%d %d %d %s %s %s %s %s %s\n" % (m.nvox + tuple(float(v).hex() for v in m.origin) +
                                                    (float(m.res_inv).hex(), float(m.res).hex(), fp)))
        for (mi, degree, ev, mp, clearance), grp in groups.items():
            maxc = max(len(sc["ctrl"]) for sc in grp) + 1
            f.write("R %d %d %d %d %d %d %s\n" % (mi, len(grp), degree, maxc, ev, mp, float(clearance).hex()))
            field = cc.spec(names[mi]).field("cut")
            for sc in grp:
                f.write("%d %s %s\n" % (len(sc["ctrl"]), float(sc["dt"]).hex(), hb.hexes(sc["ctrl"])))
                r = cc.restate(sc, field=field)
                tok = [r[k] for k in ("status", "n_ticks", "n_start_events", "n_end_events", "n_start_pts", "n_end_pts")] + \
                    [hb.bits(r["t_s"]), hb.bits(r["t_e"])] + rows([r["first_start"]], 1) + rows([r["last_end"]], 1) + \
                    rows(r["colli_start"], ev) + rows(r["colli_end"], ev) + rows(r["start_pts"], mp) + rows(r["end_pts"], mp)
                want.append((sc["tag"], " ".join(str(t) for t in tok)))
        for (degree, mg, dist), grp in ggroups.items():
            mpp = max(len(sc["path"]) for sc in grp)
            f.write("G %d %d %d %d %s\n" % (len(grp), mpp, degree, mg, float(dist).hex()))
            for sc in grp:
                f.write("%d %s %s\n" % (len(sc["path"]), float(sc["duration"]).hex(), hb.hexes(sc["path"])))
                r = cc.grestate(sc)
                tok = [r[k] for k in ("status", "seg_num", "n_pts", "n_ctrl", "n_guide")] + [hb.bits(r["dt"])] + \
                    rows(r["guide_pts"], mg)
                want.append(("guide " + sc["tag"], " ".join(str(t) for t in tok)))
    lines = hb.run(exe, [path]).splitlines()
    assert len(lines) == len(want), (len(lines), len(want))
    bad = 0
    for (tag, exp), line in zip(want, lines):
        got = " ".join(one_nan(line.split()))
        if got != exp:
            print(tag, "DIFFERS\n  host build:  ", got[:600], "\n  restatement: ", exp[:600])
            bad += 1
    print("%d problems in %d + %d launches: %s" % (len(want), len(groups), len(ggroups),
                                                    "all identical, sanitizers silent" if not bad else "%d DIFFER" % bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
