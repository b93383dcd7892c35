"""Builds the own text of the three kernels that take given knots -- k_traj_check, k_traj_sample, k_yaw_plan -- for the
host (tests/golden/knots_golden/host_kernel.cpp on tests/golden/host_lanes.h: a thread per lane, guard zones round the
LDS block) as a stand-alone program with the address and the undefined-behaviour sanitizers, runs every scene of
tests/knots_cases.py through SplineSrc's knot pointer -- in launches by degree, so that problems of different sizes share
workgroups -- and two scenes with bad knots through the kernels' own check, and compares with the restatement
(tests/knots_ref.py): the safety check and the samples bit for bit; of the yaw plan the duration, the segments and the
way-point count bit for bit and what follows atan2 within knots_ref.yaw_tolerance (the host's atan2 is not the
restatement's to the bit by contract, like the device's).  Everything stays under build/knots_golden/."""
import os
import sys

import numpy as np

import host_build as hb
from host_build import bits, from_bits, hexes

sys.path.insert(0, os.path.join(hb.ROOT, "tests"))

import knots_cases as kc  # noqa: E402
import knots_ref as kr  # noqa: E402
import traj_check_cases as tc  # noqa: E402
import traj_sample_ref as ts  # noqa: E402
import yaw_plan_ref as yr  # noqa: E402

MAX_SEG = 40


def build():
    text = ""
    for path, lds, host in (("traj_check.hip", "size_t tc_lds(", "int trajchk_cfg_check("),
                            ("traj_sample.hip", "size_t ts_lds(", "int trajsmp_cfg_check("),
                            ("yaw_plan.hip", "size_t yp_lds(", "bool fin_nonneg(")):
        text += hb.lds_from_host(hb.cut(path, "namespace {", lds, keep_start=False)) + hb.cut(path, lds, host)
    return hb.compile("knots", text)


def main():
    exe = build()
    groups = kc.by_degree()
    groups[3] = groups[3][:2] + kc.bad_scenes() + groups[3][2:]  # bad knots between good neighbours
    m = tc.spec(kc.MAP)
    adr = np.nonzero(m.infl3.reshape(-1))[0]
    path = os.path.join(hb.out_dir("knots"), "scenes.in")
    order = []
    pr0 = kc.yaw_problem(kc.scenes()[0], yr.EXPLORE)
    w = pr0["weights"]
    with open(path, "w") as f:
        f.write("%d %d %d %s %s\n%d %s\n" % (m.nvox + (hexes(m.origin), float(m.res_inv).hex(), len(adr), " ".join(str(a) for a in adr))))
        f.write("%d\n" % len(groups))
        for p, grp in sorted(groups.items()):
            maxc, max_t = max(len(sc["ctrl"]) for sc in grp), max(len(sc["t"]) for sc in grp)
            f.write("%d %d %d %d\n" % (p, maxc, len(grp), max_t))
            for sc in grp:
                f.write("%d %s %s %s %d %s %s %s\n" % (len(sc["ctrl"]), " ".join("nan" if v != v else float(v).hex() for v in sc["u"]),
                                                      hexes(sc["ctrl"]), float(sc["t_now"]).hex(), len(sc["t"]), hexes(sc["t"]),
                                                      hexes(pr0["start"]), float(pr0["end"]).hex()))
                order.append((sc, max_t))
            f.write("%s %s\n" % (float(grp[0]["step"]).hex(), float(grp[0]["max_radius"]).hex()))
            f.write("%d %d %d %s\n" % (pr0["seg_num"], 1 if pr0["lookfwd"] else 0, MAX_SEG,
                                       hexes([pr0["relax_time"], pr0["forward_t"], pr0["dt_target"], pr0["end_back"],
                                              w["ld_smooth"], w["ld_start"], w["ld_end"], w["ld_waypt"]])))
    lines = hb.run(exe, [path]).splitlines()
    grid = m.grid()
    bad = 0
    tol_cases = [(kc.yaw_problem(sc, mode), sc["u"]) for sc in kc.scenes() for mode in (yr.EXPLORE, yr.FOLLOW)]
    tol = kr.yaw_tolerance(tol_cases)[1]
    worst = {k: 0.0 for k in tol}
    it = iter(lines)
    pos = 0
    for p, grp in sorted(groups.items()):
        max_t = max(len(sc["t"]) for sc in grp)
        for sc in grp:  # C
            r = kr.check(grid, sc["ctrl"], p, sc["u"], sc["t_now"], sc["step"], sc["max_radius"])
            want = "C %d %d %d %d %d %s" % (r["status"], r["safe"], r["n_samples"], r["hit_index"], r["end_reason"],
                                            " ".join(bits(v) for v in [r["distance"], r["hit_t"], r["duration"]] + r["hit_pos"]))
            line = next(it)
            if want != line:
                print(sc["tag"], "check DIFFERS\n  host build:  ", line, "\n  restatement: ", want)
                bad += 1
        for sc in grp:  # S
            r = kr.sample(ts.COMMAND, sc["ctrl"], p, sc["u"], sc["t"])
            ok = kr.knots_ok(sc["u"])
            fl = ts.record_windowed([0.0] * 8, sc["t"], r) if ok else [0.0] * 8
            want = ["S " + " ".join(bits(v) for v in [r["duration"]] + fl)]
            for k in range(max_t):
                if k < len(sc["t"]):
                    vals = r["pos"][k] + r["vel"][k] + r["acc"][k] + r["jerk"][k] + [0.0, 0.0, 0.0]
                    want.append("%d %s" % (r["status"][k], " ".join(bits(v) for v in vals)))
                else:
                    want.append("0 " + " ".join(bits(0.0) for _ in range(15)))
            got = [next(it) for _ in range(1 + max_t)]
            if want != got:
                k = [a != b for a, b in zip(want, got)].index(True)
                print(sc["tag"], "sample DIFFERS at line", k, "\n  host build:  ", got[k], "\n  restatement: ", want[k])
                bad += 1
        for mode in (yr.EXPLORE, yr.FOLLOW):  # Y, W, Q
            for sc in grp:
                pr = kc.yaw_problem(sc, mode)
                r = kr.yaw_solve(pr, sc["u"], "banded")
                head, wl, ql = next(it).split(), next(it).split()[1:], next(it).split()[1:]
                nw, N = r["n_waypt"], (r["seg_num"] + 3 if not r.get("bad_knots") else 0)
                exact = (head[:5] == ["Y", str(mode), str(r["status"]), str(r["seg_num"]), str(nw)]
                         and head[5] == bits(r["duration"]) and head[6] == bits(r["dt_yaw"]))
                wp = np.array([from_bits(v) for v in wl])
                q = np.array([from_bits(v) for v in ql])
                d = {"waypts": max([abs(from_bits(head[7]) - r["end_yaw"])] + list(np.abs(wp[:nw] - np.array(r["waypts"])))),
                     "yaw_ctrl": float(np.abs(q[:N] - r["yaw_ctrl"]).max()) if N else 0.0,
                     "cost": abs(from_bits(head[8]) - r["cost"])}
                for k in d:
                    worst[k] = max(worst[k], d[k])
                if not exact or any(d[k] > tol[k] for k in d) or wp[nw:].any() or q[N:].any():
                    print(sc["tag"], "yaw mode", mode, "DIFFERS", head, d, tol)
                    bad += 1
    assert next(it, None) is None
    print("%d problems in %d launches through three kernels: %s; yaw behind atan2: largest differences %s, tolerances %s" %
          (len(order), len(groups), "all identical, sanitizers silent" if not bad else "%d DIFFER" % bad, worst, tol))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
