"""fuelmi_map_sample_trajs / fuelmi_bspline_dev_sample_trajs on the device against the restatement
(tests/traj_sample_ref.py) on the scenes of tests/traj_sample_cases.py.

Every output is compared BIT FOR BIT, as bytes: only + - * / and a correctly rounded f64 square root are involved,
compiled without FMA contraction, so there is no tolerance to choose.  Then the workgroup packing (3 problems per
workgroup), batch independence, the record carried over a split tape, the device chain behind _dev_optimize (with a bad
MINTIME variable among good neighbours) and the facade driver in a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import traj_check_cases as tcc
import traj_sample_cases as tc
import traj_sample_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

VEC = ("pos", "vel", "acc", "jerk")
SCL = ("yaw", "yawdot", "yawddot")
QUICK = tc.quick_scenes()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


@pytest.fixture(scope="module")
def gm():
    import fuel_amd
    m = tcc.spec("a")
    g = fuel_amd.SDFMap(m.map_size, device=0, **m.kw)
    yield g
    g.close()


def run(gm, scs, flight="zeros", **kw):
    """one call for scenes that share mode and degrees; COMMAND scenes start a record from zeros"""
    s0 = scs[0]
    py = max([s["yaw"]["degree"] for s in scs if s["yaw"]] + [0])
    assert all((s["mode"], s["degree"]) == (s0["mode"], s0["degree"]) and (not s["yaw"] or s["yaw"]["degree"] == py) for s in scs)
    yaw = [s["yaw"]["ctrl"] if s["yaw"] else None for s in scs] if py else None
    ydt = [s["yaw"]["dt"] if s["yaw"] else 1.0 for s in scs] if py else None
    stop = None
    if any(s["t_stop"] is not None for s in scs):  # (a t_stop far above D is no t_stop)
        stop = [s["t_stop"] if s["t_stop"] is not None else 1e300 for s in scs]
    if isinstance(flight, str):
        flight = np.zeros((len(scs), 8)) if s0["mode"] == sr.COMMAND else None
    return gm.sampleTrajs([s["ctrl"] for s in scs], [s["dt"] for s in scs], [s["t"] for s in scs], yaw_ctrl=yaw, yaw_dt=ydt,
                          t_stop=stop, flight=flight, mode=s0["mode"], degree=s0["degree"], yaw_degree=py or 3, **kw)


def assert_same(out, b, sc, r=None, flight=True):
    """problem b of a call against the restatement of scene sc: every entry of every array, the zeros past n_t too"""
    r = r if r is not None else tc.restate(sc)
    n_t, max_t = len(sc["t"]), out["status"].shape[1]
    assert out["n_t"][b] == n_t
    want = np.zeros(max_t, dtype=np.int32)
    want[:n_t] = r["status"]
    assert out["status"][b].tobytes() == want.tobytes(), (sc["tag"], out["status"][b], want)
    for k in VEC:
        w = np.zeros((max_t, 3))
        w[:n_t] = np.array(r[k]).reshape(n_t, 3)
        assert _bits(out[k][b]) == _bits(w), (sc["tag"], k, np.abs(out[k][b] - w).max())
    for k in SCL:
        w = np.zeros(max_t)
        w[:n_t] = r[k]
        assert _bits(out[k][b]) == _bits(w), (sc["tag"], k, np.abs(out[k][b] - w).max())
    assert _bits(out["duration"][b]) == _bits(r["duration"]), sc["tag"]
    if flight and r.get("flight") is not None:
        assert _bits(out["flight"][b]) == _bits(r["flight"]), (sc["tag"], out["flight"][b], r["flight"])


# ---- 1. every scene, grouped into calls by mode and degrees -----------------------------------------------------------------
def test_every_scene(gm):
    seen = 0
    for key, scs in tc.groups(QUICK).items():
        out = run(gm, scs)
        assert out["status"].shape == (len(scs), max(len(s["t"]) for s in scs))
        for b, sc in enumerate(scs):
            assert_same(out, b, sc)
            seen += 1
    assert seen == len(QUICK) >= 70


def test_largest_stride_with_a_small_neighbour(gm):
    """max_ctrl = max_yaw_ctrl = 1024: the largest knot blocks, a problem of p + 1 points in the same workgroup"""
    big = tc.big_scenes()
    assert len(big) == tc.PACK and len(big[0]["ctrl"]) == sr.MAX_CTRL and len(big[1]["ctrl"]) == 4
    out = run(gm, big)
    for b, sc in enumerate(big):
        assert_same(out, b, sc)
    out = run(gm, big[::-1], max_yaw_ctrl=sr.MAX_CTRL)
    for b, sc in enumerate(big[::-1]):
        assert_same(out, b, sc)


# ---- 2. the packing: 1, PACK and PACK + 1 problems, every scene alone, a problem at several places ----------------------------
def test_packing_and_batch_independence(gm):
    main = max((g for k, g in tc.groups(QUICK).items() if k[0] == sr.COMMAND), key=len)
    main = [s for s in main if len(s["t"])]  # (a call without a sample launches nothing and writes nothing: below)
    assert len(main) >= 3 * tc.PACK
    alone = [run(gm, [sc]) for sc in main]
    for sc, o in zip(main, alone):
        assert_same(o, 0, sc)
    for n in (1, tc.PACK, tc.PACK + 1):
        out = run(gm, main[:n])
        for b in range(n):
            assert_same(out, b, main[b])
    probe = [s for s in main if s["tag"].startswith(("cmd_p3_n40", "tape_p3_nt65"))]
    assert len(probe) == 2
    for sc in probe:
        rest = [s for s in main if s is not sc]
        for place in (0, 1, tc.PACK - 1, tc.PACK, 2 * tc.PACK + 1, len(rest)):
            batch = rest[:place] + [sc] + rest[place:]
            out = run(gm, batch, max_ctrl=64, max_yaw_ctrl=48, max_t=200)  # wider strides: the same bits
            one = alone[main.index(sc)]
            n_t = len(sc["t"])
            for k in ("status",) + VEC + SCL:
                assert out[k][place][:n_t].tobytes() == one[k][0][:n_t].tobytes(), (sc["tag"], place, k)
                assert not out[k][place][n_t:].any()
            assert _bits(out["flight"][place]) == _bits(one["flight"][0]) and out["duration"][place] == one["duration"][0]
            for b, s in enumerate(batch):
                assert_same(out, b, s)
    # nothing to do is no launch: empty arrays, and a call whose problems all have n_t = 0
    assert gm.sampleTrajs([], [], [])["status"].shape == (0, 0)
    none = [s for s in QUICK if len(s["t"]) == 0]
    assert len(none) == 3 and not run(gm, none[:1])["duration"].any()


# ---- 3. the record carried from call to call ---------------------------------------------------------------------------------
def test_record_carried_over_a_split_tape(gm):
    by = {s["tag"]: s for s in QUICK}
    scs = [by["record_slow"], by["record_invalid_mid"], by["record_past_end"], by["tape_p3_nt129"]]
    whole = run(gm, scs)
    for cut in (1, 40, tc.WIN, tc.WIN + 1):
        first = [dict(s, t=s["t"][:cut]) for s in scs]
        second = [dict(s, t=s["t"][cut:]) for s in scs]
        a = run(gm, first)
        b = run(gm, second, flight=a["flight"])
        assert _bits(b["flight"]) == _bits(whole["flight"]), cut
        for i, s in enumerate(scs):
            assert _bits(b["flight"][i]) == _bits(tc.restate(s)["flight"]), (s["tag"], cut)
            for k in VEC:
                assert _bits(np.concatenate([a[k][i][:cut], b[k][i][:len(s["t"]) - cut]])) == _bits(whole[k][i][:len(s["t"])])
    # without a record the same samples; a record is COMMAND's alone
    import fuel_amd
    bare = run(gm, scs, flight=None)
    assert bare["flight"] is None and all(_bits(bare[k]) == _bits(whole[k]) for k in VEC + SCL)
    with pytest.raises(fuel_amd.FuelmiError, match="error -1"):
        run(gm, [s for s in QUICK if s["mode"] == sr.STATE][:2], flight=np.zeros((2, 8)))


# ---- 4. the device chain -----------------------------------------------------------------------------------------------------
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
    return opt.deviceProblem(fuel_amd.BsplineBatchProblem(x, N, cf, ptd, st, en, 3, 3, dt)), C, N, dt, ctrl


@pytest.mark.parametrize("mintime", [True, False])
def test_device_chain(gm, mintime):
    import fuel_amd
    dev, C, N, dt, ctrl = _chain(gm, mintime)
    rng = np.random.default_rng(5)
    t = [np.sort(rng.uniform(-0.2, 3.2, (1, 63, 64, 65, 129, 0, 7, 30)[c])) for c in range(C)]
    yaw = [tc.yaw_wiggle(15, 60 + c) if c % 3 else None for c in range(C)]
    stop = rng.uniform(1.0, 4.0, C)
    kw = dict(yaw_ctrl=yaw, yaw_dt=np.full(C, 0.21), t_stop=stop, flight=np.zeros((C, 8)))
    with pytest.raises(fuel_amd.FuelmiError, match="error -1"):  # not optimised yet
        dev.sample_trajs(t, **kw)
    xo, co, ev = dev.optimize(max_eval=40)
    got = dev.sample_trajs(t, **kw)
    pos = xo[:, :3 * N].reshape(C, N, 3)
    knot = xo[:, -1] if mintime else np.full(C, dt)
    if mintime:
        assert np.abs(knot - dt).max() > 0.0  # the knot span really comes from the variables
    want = gm.sampleTrajs(list(pos), knot, t, **kw)
    for k in ("status",) + VEC + SCL + ("duration", "flight"):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert {sr.IN, sr.PAST, sr.INVALID} <= set(got["status"].reshape(-1).tolist())
    for c in range(C):  # and both equal the restatement on the x_out the solve returned
        r = sr.sample(sr.COMMAND, pos[c], 3, float(knot[c]), t[c], yaw[c], 3, 0.21, float(stop[c]))
        r["flight"] = sr.record_windowed([0.0] * 8, t[c], r)
        assert_same(got, c, dict(tag="candidate %d" % c, t=t[c]), r)
    # STATE through the same chain: a fleet's replan states, one time each
    t_r = [np.array([v]) for v in rng.uniform(0.0, 2.0, C)]
    gs = dev.sample_trajs(t_r, yaw_ctrl=yaw, yaw_dt=np.full(C, 0.21), mode=sr.STATE)
    ws = gm.sampleTrajs(list(pos), knot, t_r, yaw_ctrl=yaw, yaw_dt=np.full(C, 0.21), mode=sr.STATE)
    for k in ("status",) + VEC + SCL + ("duration",):
        assert gs[k].tobytes() == ws[k].tobytes(), k
    with pytest.raises(fuel_amd.FuelmiError, match="error -1"):  # the batch's degree is 3
        dev.sample_trajs(t, degree=4)
    # a reload invalidates what the last solve left
    dev.loadSamples(np.full(C, dt), np.ascontiguousarray(ctrl[:, :N - 2]), np.zeros((C, 4, 3)))
    with pytest.raises(fuel_amd.FuelmiError, match="error -1"):
        dev.sample_trajs(t)
    dev.optimize(max_eval=5)
    assert dev.sample_trajs(t)["duration"].all()
    dev.close()


def test_bad_spline_among_good_neighbours(gm):
    """a MINTIME variable that is 0 / not a number reaches the device through the batch's own variables; the host never
    sees it.  The kernel does not index by it: BADSPLINE, zeros, the record untouched; the neighbours are complete."""
    import fuel_amd
    dev, C, N, dt, _ = _chain(gm, True, spoil=((1, 0.0), (4, float("nan"))))
    xo, co, ev = dev.optimize(max_eval=1)
    knot = xo[:, -1]
    bad = ~(np.isfinite(knot) & (knot > 0.0))
    assert bad[1] and bad[4] and bad.sum() == 2, knot
    t = [tc.tape(70 if c != 2 else 3, 0.05, -0.1) for c in range(C)]
    carried = np.arange(8.0 * C).reshape(C, 8)
    got = dev.sample_trajs(t, flight=carried)
    pos = xo[:, :3 * N].reshape(C, N, 3)
    with pytest.raises(fuel_amd.FuelmiError, match="error -1"):  # the host route refuses what it can see
        gm.sampleTrajs(list(pos), knot, t)
    good = np.flatnonzero(~bad)
    want = gm.sampleTrajs(list(pos[good]), knot[good], [t[c] for c in good], flight=carried[good])
    for k in ("status",) + VEC + SCL + ("duration", "flight"):
        assert got[k][good].tobytes() == want[k].tobytes(), k
    for c in np.flatnonzero(bad):
        r = sr.sample(sr.COMMAND, pos[c], 3, float(knot[c]), t[c])
        assert set(r["status"]) == {sr.BADSPLINE}
        assert_same(got, c, dict(tag="bad %d" % c, t=t[c]), r)
        assert (got["status"][c] == sr.BADSPLINE).all() and got["duration"][c] == 0.0
        assert _bits(got["flight"][c]) == _bits(carried[c])
    dev.close()


def test_device_chain_refuses_other_batches(gm):
    import fuel_amd
    rng = np.random.default_rng(3)
    opt = fuel_amd.BsplineOptimizer()
    opt.setEnvironment(gm)
    N = 15
    x = rng.normal(size=(2, N))
    st, en = np.zeros((2, 3, 3)), np.zeros((2, 3, 3))
    flags = fuel_amd.SMOOTHNESS | fuel_amd.START | fuel_amd.END
    dev = opt.deviceProblem(fuel_amd.BsplineBatchProblem(x, N, flags, np.array([0.3, 0.3]), st, en, 2, 1, 0.3))
    dev.optimize(max_eval=5)
    with pytest.raises(fuel_amd.FuelmiError, match="error -1"):  # dim 1
        dev.sample_trajs([np.zeros(1), np.zeros(1)])
    dev.close()


# ---- 5. the facade -------------------------------------------------------------------------------------------------------------
def test_facade_driver(gm, tmp_path):
    """facade_trajsample in a child process: evaluateCommand / replanState against SDFMap.sampleTrajs and the
    restatement, and its own in-process host loop against both"""
    m = tcc.spec("a")
    scs = [s for s in QUICK if s["tag"].startswith(("cmd_", "stop_", "state_p", "record_", "tape_p4")) and len(s["t"])]
    assert len(scs) >= 40 and {s["degree"] for s in scs} == {3, 4, 5} and {s["mode"] for s in scs} == {sr.COMMAND, sr.STATE}
    scen = str(tmp_path / "scen.bin")
    with open(scen, "wb") as f:
        np.array(list(m.map_size) + list(m.origin) + list(m.origin + np.array(m.map_size)) + [m.res, m.kw["ground_height"]],
                 dtype=np.float64).tofile(f)
        for s in scs:
            y = s["yaw"]
            np.concatenate([[s["mode"], s["degree"], len(s["ctrl"]), s["dt"], y["degree"] if y else 3, len(y["ctrl"]) if y else 0,
                             y["dt"] if y else 1.0, 0 if s["t_stop"] is None else 1, s["t_stop"] or 0.0, len(s["t"])],
                            s["ctrl"].reshape(-1), y["ctrl"] if y else [], s["t"]]).astype(np.float64).tofile(f)
    exe = os.path.join(ROOT, "fuel_amd", "facade", "facade_trajsample")
    p = subprocess.run([exe, scen], check=True, capture_output=True, text=True, timeout=300)
    res = json.loads(p.stdout[p.stdout.index("{"):])["problems"]
    assert len(res) == len(scs)
    for got, s in zip(res, scs):
        assert got["ok"] == 1, s["tag"]
        r = tc.restate(s)
        n_t = len(s["t"])
        cols = np.concatenate([np.array(r[k], dtype=np.float64).reshape(n_t, -1) for k in VEC + SCL], axis=1)
        if s["mode"] == sr.STATE:
            cols[:, 9:12] = 0.0  # the FSM's six: replanState returns no jerk
        for route in ("device", "host"):
            assert got[route]["status"] == list(r["status"]), (s["tag"], route)
            v = np.array(got[route]["values"], dtype=np.float64).reshape(n_t, 16)
            if s["mode"] == sr.STATE and route == "host":
                v[:, 9:12] = 0.0
            assert _bits(v[:, :15]) == _bits(cols), (s["tag"], route, np.abs(v[:, :15] - cols).max())
            if s["mode"] == sr.COMMAND and n_t:
                assert _bits(got[route]["flight"]) == _bits(r["flight"]), (s["tag"], route)
    o = run(gm, [scs[0]])
    assert_same(o, 0, scs[0])
