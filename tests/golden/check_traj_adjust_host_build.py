"""Builds k_traj_adjust's and k_traj_select's own text for the host (tests/golden/traj_adjust_golden/host_kernel.cpp on
tests/golden/host_lanes.h: a thread per lane, guard zones round the LDS block) with the address and the
undefined-behaviour sanitizers as a stand-alone program, runs it once on every scene of
tests/traj_adjust_cases.py -- grouped into launches by degree, stages and configuration, so that problems of different
sizes share workgroups, each launch with SELECT over three groups -- plus a launch laid out like a device batch with bad
knot spans among good neighbours, and compares every output with the restatement (tests/traj_adjust_ref.py) bit for bit.
Everything stays under build/traj_adjust_golden/; the cut, the build and the run are tests/golden/host_build.py's.  With
an argument (a substring of scene tags) only those scenes run.

The restatement takes norm() as the Eigen stand-in of compat/ does; against real Eigen's that is the project's standing
caveat."""
import os
import sys

import host_build as hb

sys.path.insert(0, os.path.join(hb.ROOT, "tests"))

import traj_adjust_cases as tc  # noqa: E402
import traj_adjust_ref as ar  # noqa: E402


def build():
    return hb.compile("traj_adjust", hb.lds_from_host(hb.cut("traj_adjust.hip", "namespace {", "int trajadj_cfg_check(")))


def bits(v):
    return hb.bits(v, one_nan=True)


hexes = hb.hexes


def batch_scenes():
    """a launch laid out like a device batch (every problem the stride's number of points, no n_ctrl array): knot spans
    0, not a number, infinite and negative among good neighbours"""
    return [tc.scene("batch_%d" % b, 3, tc.path(16, 300 + b), dt, ops=tc.ALL)
            for b, dt in enumerate((0.2, 0.0, 0.21, float("nan"), float("inf"), 0.19, -0.1))]


def main():
    exe = build()
    pick = sys.argv[1] if len(sys.argv) > 1 else ""
    scenes = [s for s in tc.all_scenes() if pick in s["tag"]]
    big = {s["tag"] for s in tc.big_scenes()}
    launches = [(g, False) for g in tc.groups([s for s in scenes if s["tag"] not in big]).values()]
    if any(s["tag"] in big for s in scenes):
        launches.append(([s for s in scenes if s["tag"] in big], False))
    if not pick:
        launches.append((batch_scenes(), True))
    path = os.path.join(hb.out_dir("traj_adjust"), "scenes.in")
    plan = []
    with open(path, "w") as f:
        f.write("%d\n" % len(launches))
        for grp, batch in launches:
            s0 = grp[0]
            c = dict(ar.DEFAULTS)
            c.update(s0["cfg"])
            p = s0["degree"]
            maxc = max(len(s["ctrl"]) for s in grp) + (0 if batch or len(grp[0]["ctrl"]) == ar.MAX_CTRL else 1)
            maxs = maxc - p + 2 if s0["ops"] & ar.RESAMPLE else 0
            group = [b % 3 for b in range(len(grp))]
            f.write("%d %d %d %d %d %d %d %d %d %d\n" % (s0["ops"] | ar.SELECT, p, maxc, maxs, c["realloc_iters"], 3, len(grp),
                                                       s0["knots"] is not None, s0["ratio_in"] is not None, batch))
            f.write(hexes([c[k] for k in ("limit_vel", "limit_acc", "limit_ratio", "lengthen_cap", "length_res", "stat_step")]) + "\n")
            for b, s in enumerate(grp):
                f.write("%d %d %s %s\n" % (len(s["ctrl"]), group[b], hexes([s["dt"] if s["dt"] is not None else 1.0,
                                                                           s["ratio_in"] if s["ratio_in"] is not None else 0.0]),
                                           hexes(s["ctrl"])))
                if s["knots"] is not None:
                    f.write(hexes(s["knots"]) + "\n")
            plan.append((grp, group, maxc + p + 1, maxs))
    lines = hb.run(exe, [path]).splitlines()
    assert len(lines) == sum(4 * len(g) + 1 for g, _, _, _ in plan), (len(lines), len(plan))
    bad = at = count = 0
    for grp, group, ks, maxs in plan:
        res = []
        for s in grp:
            r = ar.adjust(s["ctrl"], s["degree"], s["dt"], s["knots"], s["ops"], s["ratio_in"], maxs if maxs else None, **s["cfg"])
            res.append(r)
            info, met, ko, smp = tc.want_arrays(r, len(s["ctrl"]), s["degree"], ks, maxs)
            want = [" ".join(str(int(v)) for v in info), " ".join(bits(v) for v in met), " ".join(bits(v) for v in ko),
                    " ".join(bits(v) for v in smp.reshape(-1))]
            got = [" ".join(bits(hb.from_bits(t)) for t in ln.split()) if i else ln
                   for i, ln in enumerate(lines[at:at + 4])]
            at += 4
            count += 1
            if got != want:
                first = next(i for i in range(4) if got[i] != want[i])
                print(s["tag"], "DIFFERS at line", first, "\n  host build:  ", got[first][:400], "\n  restatement: ", want[first][:400])
                bad += 1
        want_best = "B " + " ".join(str(v) for v in ar.select(group, res, 3))
        if lines[at] != want_best:
            print(grp[0]["tag"], "best DIFFERS", lines[at], want_best)
            bad += 1
        at += 1
    sizes = sorted(len(g) for g, _, _, _ in plan)
    print("%d scenes in %d launches (problems per launch: %s): %s" %
          (count, len(plan), sizes, "all identical, sanitizers silent" if not bad else "%d DIFFER" % bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
