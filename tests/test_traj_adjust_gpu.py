"""fuelmi_map_adjust_trajs / fuelmi_bspline_dev_adjust_trajs on the device against the restatement
(tests/traj_adjust_ref.py) on the scenes of tests/traj_adjust_cases.py.

Every output is compared BIT FOR BIT, as bytes, the zero padding included: only + - * /, comparisons and a correctly
rounded f64 square root are involved, compiled without FMA contraction, so there is no tolerance to choose (one scene's
jerk is not a number on purpose: which NaN a processor generates is its own choice, so a NaN equals a NaN, see _bits).  Then the
one call against two chained calls, SELECT, batch independence and the workgroup packing, the device chain behind
_dev_optimize (with a bad MINTIME variable among good neighbours), the scratch pools growing between calls and the
facade driver in a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import traj_adjust_cases as tc
import traj_adjust_ref as ar
import traj_check_cases as tcc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

QUICK = tc.quick_scenes()
BY = {s["tag"]: s for s in QUICK}


def _bits(a):
    """the bytes of f64 values; IEEE 754 leaves the sign and the payload of a generated NaN to the processor (x86
    produces the negative quiet NaN for inf - inf; the restatement runs there, the kernel on the device), so every NaN is
    taken as the same one.  Nothing else is touched."""
    a = np.array(a, dtype=np.float64)
    a[np.isnan(a)] = np.nan
    return np.ascontiguousarray(a).tobytes()


@pytest.fixture(scope="module")
def gm():
    import fuel_amd
    m = tcc.spec("a")
    g = fuel_amd.SDFMap(m.map_size, device=0, **m.kw)
    yield g
    g.close()


def run(gm, scs, group=None, n_group=None, **kw):
    """one call for scenes that share a key"""
    s0 = scs[0]
    assert all(tc.key(s) == tc.key(s0) for s in scs)
    ops = s0["ops"] | (ar.SELECT if group is not None else 0)
    knots = [s["knots"] for s in scs] if s0["knots"] is not None else None
    spans = [s["dt"] for s in scs] if s0["knots"] is None else None
    ratio = [s["ratio_in"] for s in scs] if s0["ratio_in"] is not None else None
    cfg = dict(s0["cfg"], degree=s0["degree"])
    cfg.update(kw)
    return gm.adjust_trajs([s["ctrl"] for s in scs], spans, knots_in=knots, ratio_in=ratio, group=group, n_group=n_group, ops=ops, **cfg)


def assert_same(out, b, sc, r=None):
    """problem b of a call against the restatement of scene sc: every entry of every array, the zeros of the padding too"""
    max_samples = out["samples"].shape[1] if out["samples"] is not None else 0
    r = r if r is not None else tc.restate(sc, max_samples if out["samples"] is not None else None)
    n, p = len(sc["ctrl"]), sc["degree"]
    info, met, ko, smp = tc.want_arrays(r, n, p, out["knots_out"].shape[1], max_samples)
    assert out["info"][b].tobytes() == info.tobytes(), (sc["tag"], out["info"][b], info)
    assert _bits(out["metrics"][b]) == _bits(met), (sc["tag"], dict(zip(ar.METRICS, zip(out["metrics"][b], met))))
    assert _bits(out["knots_out"][b]) == _bits(ko), (sc["tag"], np.abs(out["knots_out"][b] - ko).max())
    if out["samples"] is not None:
        assert _bits(out["samples"][b]) == _bits(smp), (sc["tag"], np.abs(out["samples"][b] - smp).max())


# ---- 1. every scene, grouped into calls by degree, stages and configuration ----------------------------------------------------
def test_every_scene(gm):
    seen = 0
    for key, scs in tc.groups(QUICK).items():
        out = run(gm, scs)
        assert out["knots_out"].shape == (len(scs), max(len(s["ctrl"]) for s in scs) + scs[0]["degree"] + 1)
        for b, sc in enumerate(scs):
            assert_same(out, b, sc)
            seen += 1
    assert seen == len(QUICK) >= 45


def test_scenes_say_what_they_are_drawn_for(gm):
    """the outputs a user reads, by name: feasible at the input, the statuses, the sample counts"""
    out = run(gm, [BY["feasible"]])
    assert (out["status"][0], out["feasible_in"][0], out["iters"][0], out["feasible_out"][0]) == (ar.OK, 1, 0, 1)
    assert _bits(out["knots_out"][0]) == _bits(ar.knots(12, 3, 0.25))
    out = run(gm, [BY["long_valid"], BY["long_long"], BY["long_valid_again"]])  # one workgroup
    assert out["status"].tolist() == [ar.OK, ar.LONG, ar.OK]
    assert out["length"][1] == 0.0 and out["num_vel"][1] == 0 and not out["samples"][1].any() and out["jerk"][1] > 0.0
    assert out["knots_out"][1].any() and out["length"][0] > 0.0
    assert out["info"][0].tobytes() == out["info"][2].tobytes() and _bits(out["samples"][0]) == _bits(out["samples"][2])
    assert run(gm, [BY["resample_plus1"]])["n_samples"][0] == 7 and run(gm, [BY["resample_plus2"]])["n_samples"][0] == 8
    assert run(gm, [BY["resample_plus2"]])["samples"].shape[1] == 8  # seg_num + 2 at the smallest stride accepted
    assert (run(gm, [BY["cap_binds_it3"]])["iters"][0], run(gm, [BY["cap_binds_it1"]])["iters"][0]) == (3, 1)
    assert run(gm, [BY["vel_at_limit"]])["feasible_in"][0] == 1 and run(gm, [BY["vel_ulp_above"]])["feasible_in"][0] == 0


def test_largest_stride_with_small_neighbours(gm):
    """max_ctrl = 1024: the largest LDS block, one problem per workgroup; problems of p + 1 points beside it"""
    big = tc.big_scenes()
    assert len(big[0]["ctrl"]) == ar.MAX_CTRL and len(big[1]["ctrl"]) == 4
    out = run(gm, big)
    assert out["knots_out"].shape[1] == ar.MAX_CTRL + 4
    for b, sc in enumerate(big):
        assert_same(out, b, sc)
    out = run(gm, big[::-1])
    for b, sc in enumerate(big[::-1]):
        assert_same(out, b, sc)


# ---- 2. LENGTHEN then REALLOC in one call against two chained calls through knots_in ------------------------------------------
def test_one_call_equals_two_chained_calls(gm):
    sc = BY["chain_both"]
    both = run(gm, [sc])
    first = run(gm, [dict(sc, ops=ar.LENGTHEN)])
    second = run(gm, [dict(sc, ops=ar.REALLOC, dt=None, knots=first["knots_out"][0])])
    assert _bits(first["knots_out"]) != _bits(ar.knots(16, 3, 0.2)) and _bits(second["knots_out"]) != _bits(first["knots_out"])
    assert _bits(second["knots_out"]) == _bits(both["knots_out"])
    assert _bits(second["metrics"][0][2:9]) == _bits(both["metrics"][0][2:9])  # duration_out .. max_acc
    assert second["info"][0][2:].tobytes() == both["info"][0][2:].tobytes()
    assert second["duration_in"][0] == first["duration_out"][0]
    assert_same(both, 0, sc)


# ---- 3. SELECT -----------------------------------------------------------------------------------------------------------------
def test_select(gm):
    a, b, nan, lng = BY["finite_jerk_a"], BY["finite_jerk_b"], BY["nan_jerk"], BY["long_long"]
    scs = [b, a, nan, a, b, nan, a]
    group = [0, 0, 0, 1, 1, 2, 1]  # group 0: a unique minimum beside a jerk that is not a number; 1: an exact tie; 2: only that
    out = run(gm, scs, group=group, n_group=5)
    res = [tc.restate(s) for s in scs]
    assert res[0]["jerk"] > res[1]["jerk"] and np.isnan(res[2]["jerk"])
    assert out["best"].tolist() == ar.select(group, res, 5) == [1, 3, -1, -1, -1]
    assert np.isnan(out["jerk"][2]) and out["jerk"][3] == out["jerk"][6]
    for i, sc in enumerate(scs):
        assert_same(out, i, sc)
    # a group whose every member is LONG has no candidate; the tie at the other end of the batch
    scs = [BY["long_long"], BY["long_valid"], BY["long_long"], BY["long_valid_again"]]
    out = run(gm, scs, group=[0, 1, 0, 1], n_group=2)
    assert out["best"].tolist() == [-1, 1] == ar.select([0, 1, 0, 1], [tc.restate(s, out["samples"].shape[1]) for s in scs], 2)
    many = [a, b] * 70 + [a]  # more problems than lanes: the tie is met by different lanes
    out = run(gm, many, group=[0] * 141, n_group=1)
    assert out["best"].tolist() == [0]
    out = run(gm, many[1:], group=[1] * 139 + [0], n_group=2)
    assert out["best"].tolist() == [139, 1]


# ---- 4. batch independence and the packing -------------------------------------------------------------------------------------
def test_packing_and_batch_independence(gm):
    main = max(tc.groups(QUICK).values(), key=len)
    assert len(main) >= 8 and {len(s["ctrl"]) for s in main} >= {4, 7, 8, 59, 60, 61, 124}
    alone = [run(gm, [sc]) for sc in main]
    for sc, o in zip(main, alone):
        assert_same(o, 0, sc)
    for n in (1, 2, 3, 4, 5, 7):  # no multiple of any number of problems per workgroup above 1
        out = run(gm, main[:n])
        for b in range(n):
            assert_same(out, b, main[b])
    probe = BY["lanes_n61"]
    one = alone[main.index(probe)]
    n, ns = len(probe["ctrl"]) + 4, one["samples"].shape[1]
    rest = [s for s in main if s is not probe]
    for place in (0, 3, len(rest)):
        batch = rest[:place] + [probe] + rest[place:]
        out = run(gm, batch, max_ctrl=130, max_samples=140)  # wider strides: the same bits
        assert out["info"][place].tobytes() == one["info"][0].tobytes() and _bits(out["metrics"][place]) == _bits(one["metrics"][0])
        assert _bits(out["knots_out"][place][:n]) == _bits(one["knots_out"][0]) and not out["knots_out"][place][n:].any()
        assert _bits(out["samples"][place][:ns]) == _bits(one["samples"][0]) and not out["samples"][place][ns:].any()
        for b, s in enumerate(batch):
            assert_same(out, b, s)
    empty = gm.adjust_trajs([], [])
    assert empty["info"].shape == (0, ar.NI)


# ---- 5. the device chain -------------------------------------------------------------------------------------------------------
def _chain(gm, mintime, spoil=()):
    import fuel_amd
    C, N, dt = 8, 16, 0.2
    ctrl = np.stack([tcc.wiggle((0.3, tcc.HIT_Y, tcc.HIT_Z) if c % 2 == 0 else (-1.4, tcc.FREE_Y, 0.3), N, seed=40 + c, amp=0.03)
                     for c in range(C)])
    x, ptd, st, en = helpers.bspline_inputs(ctrl, dt, mintime)
    for c, v in spoil:
        x[c, -1] = v
    cf = fuel_amd.SMOOTHNESS | fuel_amd.FEASIBILITY | fuel_amd.START | fuel_amd.END | (fuel_amd.MINTIME if mintime else 0)
    opt = fuel_amd.BsplineOptimizer()
    opt.setEnvironment(gm)
    return opt.deviceProblem(fuel_amd.BsplineBatchProblem(x, N, cf, ptd, st, en, 3, 3, dt)), C, N, dt


ALL_OPS = ar.LENGTHEN | ar.REALLOC | ar.RESAMPLE | ar.SELECT
LIMITS = dict(limit_vel=0.8, limit_acc=0.6)  # the candidates are slow: limits they break


def test_device_chain(gm):
    import fuel_amd
    dev, C, N, dt = _chain(gm, True)
    group = [0, 0, 0, 1, 1, 1, 1, 2]
    kw = dict(ops=ALL_OPS, group=group, n_group=4, **LIMITS)
    with pytest.raises(fuel_amd.FuelmiError, match="error -1"):  # not optimised yet
        dev.adjust_trajs(**kw)
    xo, co, ev = dev.optimize(max_eval=40)
    got = dev.adjust_trajs(**kw)
    pos = xo[:, :3 * N].reshape(C, N, 3)
    knot = xo[:, -1]
    assert np.abs(knot - dt).max() > 0.0  # the knot span really comes from the variables
    want = gm.adjust_trajs(list(pos), knot, **kw)
    for k in ("info", "metrics", "knots_out", "samples", "best"):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert got["iters"].max() >= 1 and (got["status"] == ar.OK).all()
    res = []
    for c in range(C):  # and both equal the restatement on the x_out the solve returned
        r = ar.adjust(pos[c], 3, float(knot[c]), ops=ALL_OPS, max_samples=got["samples"].shape[1], **LIMITS)
        assert_same(got, c, dict(tag="candidate %d" % c, ctrl=pos[c], degree=3), r)
        res.append(r)
    assert got["best"].tolist() == ar.select(group, res, 4) and got["best"][3] == -1 and (got["best"][:3] >= 0).all()
    # given knots replace the span: the second call continues from the first call's knots
    again = dev.adjust_trajs(knots_in=list(got["knots_out"]), ops=ar.REALLOC, **LIMITS)
    host = gm.adjust_trajs(list(pos), knots_in=list(got["knots_out"]), ops=ar.REALLOC, **LIMITS)
    assert _bits(again["duration_in"]) == _bits(got["duration_out"])
    for k in ("info", "metrics", "knots_out"):
        assert again[k].tobytes() == host[k].tobytes(), k
    with pytest.raises(fuel_amd.FuelmiError, match="error -1"):  # the batch's degree is 3
        dev.adjust_trajs(degree=4)
    dev.close()


def test_bad_spline_among_good_neighbours(gm):
    """a MINTIME variable that is 0 / not a number reaches the device through the batch's own variables; the host never
    sees it.  The kernel does not index by it: BADSPLINE, zeros; the neighbours are complete; a group of bad ones is -1"""
    import fuel_amd
    dev, C, N, dt = _chain(gm, True, spoil=((1, 0.0), (4, float("nan"))))
    xo, co, ev = dev.optimize(max_eval=1)
    knot = xo[:, -1]
    bad = ~(np.isfinite(knot) & (knot > 0.0))
    assert bad[1] and bad[4] and bad.sum() == 2, knot
    group = np.array([0, 1, 0, 0, 1, 2, 2, 2])  # group 1: every member is BADSPLINE
    kw = dict(ops=ALL_OPS, n_group=3, **LIMITS)
    got = dev.adjust_trajs(group=group, **kw)
    pos = xo[:, :3 * N].reshape(C, N, 3)
    with pytest.raises(fuel_amd.FuelmiError, match="error -1"):  # the host route refuses what it can see
        gm.adjust_trajs(list(pos), knot, group=group, **kw)
    good = np.flatnonzero(~bad)
    want = gm.adjust_trajs(list(pos[good]), knot[good], group=group[good], **kw)
    for k in ("info", "metrics", "knots_out", "samples"):
        assert got[k][good].tobytes() == want[k].tobytes(), k
    assert got["best"][1] == -1 and got["best"][0] == good[want["best"][0]] and got["best"][2] == good[want["best"][2]]
    for c in np.flatnonzero(bad):
        r = ar.adjust(pos[c], 3, float(knot[c]), ops=ALL_OPS)
        assert r["status"] == ar.BADSPLINE
        assert_same(got, c, dict(tag="bad %d" % c, ctrl=pos[c], degree=3), r)
        assert got["status"][c] == ar.BADSPLINE and not got["info"][c][1:].any() and not got["metrics"][c].any()
        assert not got["knots_out"][c].any() and not got["samples"][c].any()
    dev.close()


# ---- 6. the scratch pools growing between calls --------------------------------------------------------------------------------
def test_scratch_growth(gm):
    """a small call, a larger one that outgrows the pool, the small one again: on a fresh map and on a fresh batch"""
    import fuel_amd
    m = tcc.spec("a")
    g2 = fuel_amd.SDFMap(m.map_size, device=0, **m.kw)
    main = max(tc.groups(QUICK).values(), key=len)
    small, large = [main[0]], main[:5] + [BY["lanes_n124"]]
    rounds = [run(g2, small), run(g2, large, max_ctrl=600, max_samples=700), run(g2, small)]
    assert_same(rounds[0], 0, small[0])
    for b, sc in enumerate(large):
        assert_same(rounds[1], b, sc)
    for k in ("info", "metrics", "knots_out", "samples"):
        assert rounds[2][k].tobytes() == rounds[0][k].tobytes(), k
    dev, C, N, dt = _chain(g2, True)
    dev.optimize(max_eval=5)
    r0 = dev.adjust_trajs(ops=0)
    r1 = dev.adjust_trajs(ops=ALL_OPS, group=[0] * C, max_samples=2000, **LIMITS)
    r2 = dev.adjust_trajs(ops=0)
    assert r1["samples"].shape == (C, 2000, 3) and r1["best"][0] >= 0
    for k in ("info", "metrics", "knots_out"):
        assert r2[k].tobytes() == r0[k].tobytes(), k
    dev.close()
    g2.close()


# ---- 7. the facade -------------------------------------------------------------------------------------------------------------
def test_facade_driver(gm, tmp_path):
    """facade_trajadjust in a child process: adjustTime / trajectoryMetrics / selectBestTraj against the restatement"""
    m = tcc.spec("a")
    tags = ("all_p3_n8", "all_p4_n11", "all_p5_n14", "lanes_n61", "feasible", "vel_last", "cap_binds_it1", "acc_i1", "acc_i2",
            "vel_flips_acc", "lengthen_above", "chain_both", "given_knots_offset", "window_0.645", "margin", "resample_plus2",
            "nan_jerk", "finite_jerk_a", "finite_jerk_b", "finite_jerk_a")
    scs = [BY[t] for t in tags]
    scen = str(tmp_path / "scen.bin")
    with open(scen, "wb") as f:
        np.array(list(m.map_size) + list(m.origin) + list(m.origin + np.array(m.map_size)) + [m.res, m.kw["ground_height"]],
                 dtype=np.float64).tofile(f)
        np.array([len(scs)], dtype=np.float64).tofile(f)
        for s in scs:
            c = dict(ar.DEFAULTS)
            c.update(s["cfg"])
            u = s["knots"] if s["knots"] is not None else []
            np.concatenate([[s["degree"], len(s["ctrl"]), s["ops"], len(u), s["dt"] or 0.0, 0 if s["ratio_in"] is None else 1,
                             s["ratio_in"] or 0.0, c["limit_vel"], c["limit_acc"], c["limit_ratio"], c["lengthen_cap"],
                             c["realloc_iters"], c["length_res"], c["stat_step"]], s["ctrl"].reshape(-1), u]).astype(np.float64).tofile(f)
    exe = os.path.join(ROOT, "fuel_amd", "facade", "facade_trajadjust")
    p = subprocess.run([exe, scen], check=True, capture_output=True, text=True, timeout=300)
    doc = json.loads(p.stdout[p.stdout.index("{"):])
    res = doc["problems"]
    assert len(res) == len(scs)
    for got, s in zip(res, scs):
        assert got["ok"] == 1, s["tag"]
        n, p_ = len(s["ctrl"]), s["degree"]
        r = tc.restate(s, n - p_ + 2 if s["ops"] & ar.RESAMPLE else None)
        assert got["info"] == [r[k] for k in ar.INFO], (s["tag"], got["info"])
        assert _bits([float.fromhex(v) for v in got["metrics"]]) == _bits([r[k] for k in ar.METRICS]), s["tag"]
        assert _bits([float.fromhex(v) for v in got["knots"]]) == _bits(r["knots_out"]), s["tag"]
        assert _bits([float.fromhex(v) for v in got["samples"]]) == _bits(np.array(r["samples"]).reshape(-1)), s["tag"]
    # selectBestTraj over the last four: a jerk that is not a number, a unique minimum, the tie of the two a's
    last = [tc.restate(s) for s in scs[-4:]]
    assert doc["best"] == ar.select([0] * 4, last, 1)[0] == 1
    assert doc["best_of_none"] == -1
