"""Builds k_topo_path's own text for the host (tests/golden/topo_golden/host_kernel.cpp on tests/golden/host_lanes.h: a
thread per lane, the address and undefined-behaviour sanitizers, every array a heap block of its exact size) and compares
what it writes for every scene of tests/topo_cases.py, scenes() and edge_scenes() -- on the f32 rounding of the scene's field, and on that field moved
by +2 ulp -- with the restatement (tests/topo_ref.py) in `cut` mode on the same field: every output and counter bit for
bit.  The scenes `overflow` and `rows_one_less` run with their own max_path_points: the rows are cut, nothing is written
past them; `forest10` runs again (+0 ulp) with max_nodes one under its graph and with max_nodes = 2, where the graph's
rows stop and the neighbour ids stop at their 4 max_nodes slots.  A scene whose problems have streams of their own hands
the driver one stream per problem.
The cut, the build and the run are tests/golden/host_build.py's."""
import os
import sys

import numpy as np

import host_build as hb

sys.path.insert(0, os.path.join(hb.ROOT, "tests"))
sys.path.insert(0, hb.HERE)
import make_topo_golden as mg  # noqa: E402
import topo_cases as tc  # noqa: E402


def build():
    return hb.compile("topo", hb.cut("topo_path.hip", "namespace {", "// the workspace of n problems", keep_start=False))


def expected(r, mpp, maxn):
    """a result of the restatement as host_kernel prints it"""
    tok = [r["status"]] + list(r["counts"]) + list(r["events"]) + [len(r["nodes"])]
    flat = [i for n in r["nodes"] for i in n[3]]
    off = np.minimum(np.cumsum([0] + [len(n[3]) for n in r["nodes"]]), 4 * maxn)  # nb_off stops where nb_ids does
    for at, (ident, kind, pos, _) in enumerate(r["nodes"][:maxn]):
        nb = flat[off[at]:off[at + 1]]
        tok += [ident, kind] + [hb.bits(v) for v in pos] + [len(nb)] + list(nb)
    errored = r["status"] in (2, -1)
    for key in ("raw", "filt", "sel"):
        paths = [] if errored else r[key]
        tok.append(len(paths))
        for p in paths:
            tok.append(len(p))
            tok += [hb.bits(v) for q in p[:mpp] for v in q]
    if not errored:
        tok += [hb.bits(v) for v in r["sel_length"]]
    return " ".join(str(t) for t in tok)


def main():
    exe = build()
    bad = 0
    runs = [(name, name, sc, (0, 2)) for name, sc in list(tc.scenes().items()) + list(tc.edge_scenes().items())]
    runs += [("forest10 max_nodes %d" % n, "forest10", dict(tc.scenes()["forest10"], max_nodes=n), (0,)) for n in tc.FOREST10_MAX_NODES]
    restated = {}
    for label, name, sc, ulps in runs:
        if "max_nodes" in sc:
            sc = dict(sc, cfg=dict(sc["cfg"], max_nodes=sc["max_nodes"]))
        for ulp in ulps:
            base = os.path.join(hb.out_dir("topo"), name)
            d32 = tc.f32_field(sc["blocks"], ulp)
            d32.tofile(base + ".f32")
            np.concatenate([np.asarray(tc.samples_of(sc, p), dtype=np.float64).reshape(-1) for p in sc["probs"]]).tofile(base + ".smp")
            mg.write_input(base, sc)  # the driver's input file
            cfg = sc["cfg"]
            got = hb.run(exe, [base + ".in", base + ".f32", base + ".smp", str(cfg["max_path_points"]), str(cfg["max_nodes"])], fatal=False)
            if (name, ulp) not in restated:  # (max_nodes is the caller's business: the restatement's lists are complete)
                restated[name, ulp] = tc.run_ref(sc, "cut", tc.as_field_array(d32))
            want = restated[name, ulp]
            if got is None:
                print(label, ulp, "FAILED")
                bad += 1
                continue
            lines = got.splitlines()
            ok = len(lines) == len(want)
            for line, r in zip(lines, want):
                over = any(len(p) > cfg["max_path_points"] for k in ("raw", "filt", "sel") for p in r[k]) or \
                    len(r["nodes"]) > cfg["max_nodes"]
                if over and r["status"] in (0, 1):
                    r = dict(r, status=-1)
                    exp = expected(dict(r, status=0), cfg["max_path_points"], cfg["max_nodes"]).split()
                    exp[0] = "-1"
                    exp = " ".join(exp)
                else:
                    exp = expected(r, cfg["max_path_points"], cfg["max_nodes"])
                ok = ok and line.strip() == exp
            print("%-20s %+d ulp %s" % (label, ulp, "identical" if ok else "DIFFERS"))
            if not ok:
                print("  got ", lines[0][:400] if lines else "")
                print("  want", exp[:400])
            bad += not ok
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
