"""Builds k_quad_solve's own text for the host (tests/golden/quad_solve_golden/host_kernel.cpp on
tests/golden/host_lanes.h: a thread per lane, guard zones round the LDS block) with the address and the
undefined-behaviour sanitizers, runs it once on every scene of tests/quad_solve_cases.py -- grouped into launches by
configuration, so that problems of different sizes share a launch -- and compares status, cost, pt_dist and every control
point with the band form of the restatement (tests/quad_solve_ref.py) bit for bit.  Everything stays under
build/quad_solve_golden/; the cut, the build and the run are tests/golden/host_build.py's."""
import os
import sys

import host_build as hb
from host_build import bits

sys.path.insert(0, os.path.join(hb.ROOT, "tests"))

import quad_solve_cases as qc  # noqa: E402
import quad_solve_ref as qr  # noqa: E402


def build():
    text = hb.lds_from_host(hb.cut("quad_solve.hip", "namespace {", "size_t qs_lds("))
    return hb.compile("quad_solve", text + hb.cut("quad_solve.hip", "size_t qs_lds(", "bool fin_lt("))


def hx(a):
    return " ".join(float(v).hex() for v in a)


def main():
    exe = build()
    groups = {}
    for pr in qc.all_cases():
        w = pr["weights"]
        key = (pr["mask"], pr["dim"], pr["end_n"], pr["bounds"], qr.order_of(pr), pr["box"]) + \
            tuple(w[k] for k in ("ld_smooth", "ld_start", "ld_end", "ld_guide", "ld_waypt"))
        groups.setdefault(key, []).append(pr)
    path = os.path.join(hb.out_dir("quad_solve"), "scenes.in")
    order = []
    with open(path, "w") as f:
        f.write("%d\n" % len(groups))
        for key, grp in groups.items():
            mask, dim, end_n, bounds, o, box = key[:6]
            maxc = max(len(p["ctrl"]) for p in grp) + 1
            maxw = max(len(p["widx"]) for p in grp)
            lo, hi = qr.shrunk_box(grp[0])
            f.write("%d %d %d %d %d %d %d %d\n%s\n%s %s\n" % (mask, dim, maxc, end_n, maxw, int(bounds), o, len(grp),
                                                          hx(key[6:]), hx(lo), hx(hi)))
            for p in grp:
                nw = len(p["widx"]) if mask & qr.WAYPOINTS else 0
                f.write("%d %s %d\n%s\n%s\n%s\n%s\n%s\n%s\n" % (
                    len(p["ctrl"]), float(p["dt"]).hex(), nw, hx(p["ctrl"].reshape(-1)), hx(p["start"].reshape(-1)),
                    hx(p["end"].reshape(-1)), hx(p["guide"].reshape(-1)[:qr.n_guide(p) * dim]) if mask & qr.GUIDE
                    else hx([0.0] * (qr.n_guide(p) * dim)), " ".join(str(i) for i in p["widx"][:nw]),
                    hx(p["waypts"].reshape(-1)[:nw * dim])))
                order.append(p)
    lines = hb.run(exe, [path]).splitlines()
    assert len(lines) == len(order), (len(lines), len(order))
    bad = 0
    for p, line in zip(order, lines):
        r = qr.solve(p, "band")
        want = "%d 0 %s %s %s" % (r["status"], bits(r["cost"]), bits(r["pt_dist"]),
                                  " ".join(bits(v) for v in r["ctrl"].reshape(-1)))
        if want != line:
            print(p["tag"], "DIFFERS\n  host build:  ", line[:200], "\n  restatement: ", want[:200])
            bad += 1
    sizes = sorted(len(g) for g in groups.values())
    print("%d scenes in %d launches (problems per launch: %s): %s" %
          (len(order), len(groups), sizes, "all identical, sanitizers silent" if not bad else "%d DIFFER" % bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
