"""Builds k_local_segment's own text for the host (tests/golden/localseg_golden/host_kernel.cpp on
tests/golden/host_lanes.h: a thread per lane, guard zones round the LDS block) with the address and the undefined-behaviour
sanitizers as a stand-alone program, runs it on every scene of tests/localseg_cases.py -- grouped into launches by degree
and max_points, so that problems of different sizes and the defined failures share workgroups with good neighbours; once
more with all problems of a launch on shared, interleaved states in reversed order; and once laid out like the batch
loader (a required point count) -- and compares every output with the restatement (tests/localseg_ref.py, product form)
bit for bit.  Everything stays under build/localseg_golden/; the cut, the build and the run are
tests/golden/host_build.py's."""
import os
import sys

import host_build as hb

sys.path.insert(0, os.path.join(hb.ROOT, "tests"))

import localseg_cases as lc  # noqa: E402


def build():
    text = hb.lds_from_host(hb.cut("local_segment.hip", "namespace {", "size_t ls_lds("))
    return hb.compile("localseg", text + hb.cut("local_segment.hip", "size_t ls_lds(", "int localseg_cfg_check("))


def state_record(st, max_seg, max_ctrl):
    n_local = 0 if st.local_ctrl is None else len(st.local_ctrl)
    assert len(st.seg_times) <= max_seg and n_local <= max_ctrl
    return "%d %s %d %s %s %s %s %s %s %s %s" % (
        len(st.seg_times), float(st.global_duration).hex(), n_local, float(st.local_knot_span).hex(),
        float(st.local_ts).hex(), float(st.local_te).hex(), float(st.time_change).hex(), float(st.last_time_inc).hex(),
        hb.hexes(st.seg_times), hb.hexes(st.coef), hb.hexes(st.local_ctrl) if n_local else "")


def expected(r, max_points):
    fit_k = r["n_points"] if r["status"] == 0 else 0
    tok = [r["status"], r["n_steps"], r["seg_num"], r["n_points"], r["n_ctrl"], fit_k] + \
        [hb.bits(r[k]) for k in ("segment_len", "duration", "dt")] + [hb.bits(v) for row in r["derivs"] for v in row]
    rows = [v for p in r["points"] for v in p]
    return " ".join(str(t) for t in tok + [hb.bits(v) for v in rows + [0.0] * (3 * max_points - len(rows))])


def launches():
    """(header fields, states, problems as (state, scene), need_points)"""
    out = []
    for (degree, mp), scs in lc.groups(lc.scenes()).items():
        states = [s["state"] for s in scs]
        out.append((degree, mp, states, list(enumerate(scs)), 0))
        # the states once each, the problems reversed: several problems on one state, interleaved
        uniq = []
        for st in states:
            if not any(st is u for u in uniq):
                uniq.append(st)
        idx = [next(i for i, u in enumerate(uniq) if u is s["state"]) for s in scs]
        out.append((degree, mp, uniq, list(zip(idx, scs))[::-1], 0))
    loader = [s for s in lc.scenes() if s["degree"] == 3 and s["max_points"] == 200]
    out.append((3, 9, [s["state"] for s in loader], list(enumerate(loader)), 9))  # the batch loader: 9 points or MISFIT
    return out


def main():
    exe = build()
    path = os.path.join(hb.out_dir("localseg"), "scenes.in")
    want = []
    with open(path, "w") as f:
        for degree, mp, states, probs, need in launches():
            ms = max(len(st.seg_times) for st in states) + 1
            mc = max([len(st.local_ctrl) for st in states if st.local_ctrl is not None] + [degree + 1]) + 1
            f.write("L %d %d %d %d %d %d %d\n" % (len(states), len(probs), degree, ms, mc, mp, need))
            for st in states:
                f.write(state_record(st, ms, mc) + "\n")
            for i, sc in probs:
                f.write("%d %d %s %s %s\n" % (i, sc["mode"], float(sc["start_t"]).hex(), float(sc["arg0"]).hex(),
                                              float(sc["arg1"]).hex()))
                r = lc.lr.solve(sc["state"], sc["mode"], sc["start_t"], sc["arg0"], sc["arg1"], max_points=mp,
                                need_points=need)
                want.append((sc["tag"], expected(r, mp)))
    lines = hb.run(exe, [path]).splitlines()
    assert len(lines) == len(want), (len(lines), len(want))
    bad = 0
    for (tag, exp), line in zip(want, lines):
        if line.strip() != exp:
            print(tag, "DIFFERS\n  host build:  ", line[:700], "\n  restatement: ", exp[:700])
            bad += 1
    print("%d problems in %d launches: %s" % (len(want), len(launches()),
                                              "all identical, sanitizers silent" if not bad else "%d DIFFER" % bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
