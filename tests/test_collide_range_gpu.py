"""fuelmi_map_collision_ranges / fuelmi_map_guide_points on the device against the restatement (tests/collide_ref.py) on
the scenes of tests/collide_cases.py.

The field is built through the map's own calls (occupancy upload, inflation, updateESDF3d), read back, and first checked
to lie within 2 ulp (f32) of res * sqrt(k) of the scene.  Every output is then compared BIT FOR BIT with the restatement in
`cut` mode on the device's own field: the two calls are + - * /, floor, ceil and a correctly rounded f64 square root,
compiled without FMA contraction, so there is no tolerance to measure.  (A NaN the arithmetic generates compares as one
NaN: its sign is the processor's choice.)  Then the recordings of the reference's own code, the workgroup packing (4
problems per workgroup), batch independence and reversal, the limits and the defined failures among good neighbours, the
guide points fed to the guide cost, and the chain collision ranges -> topological search on a tests/topo_cases.py scene."""
import os
import sys

import numpy as np
import pytest

import collide_cases as cc
import collide_ref as cr
import topo_cases as tcs
import topo_ref as tpr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "collide")
PACK = 4  # problems per workgroup (collide_range.hip CR_WAVES)
SCENES = cc.collision_scenes()
GUIDES = cc.guide_scenes()
ARRAYS = (("colli_start", "n_start_events", "max_events"), ("colli_end", "n_end_events", "max_events"),
          ("start_pts", "n_start_pts", "max_pts"), ("end_pts", "n_end_pts", "max_pts"))
_REF = {}


def _bits(a):
    a = np.ascontiguousarray(a, dtype=np.float64).copy()
    a[np.isnan(a)] = np.nan
    return a.tobytes()


def device_map(map_size, kw, occ, src, k, res):
    """(the device map, its distance field [nx, ny, nz] as read back)"""
    import fuel_amd
    gm = fuel_amd.SDFMap(map_size, device=0, **kw)
    assert gm.nvox == k.shape
    gm.uploadOccupancy(occ)
    gm.setLocalBound((0, 0, 0), tuple(v - 1 for v in gm.nvox))
    gm.clearAndInflateLocalMap()
    gm.updateESDF3d()
    h = gm.syncHost(inflate=True, distance=True)
    assert np.array_equal(h["inflate"].reshape(gm.nvox) == 1, src)
    dist = h["distance"].reshape(gm.nvox)
    want = res * np.sqrt(k.astype(np.float64))
    assert np.array_equal(dist.astype(np.float32).astype(np.float64), dist)  # the mirror holds the device's f32 values
    assert np.all(np.abs(dist - want) <= 2 * np.spacing(want.astype(np.float32)).astype(np.float64))
    return gm, dist


@pytest.fixture(scope="module")
def maps():
    """name -> (device map, the restatement's field in `cut` mode on the distances read back from that map)"""
    out = {}
    for name in sorted(cc.MAPS):
        m = cc.spec(name)
        gm, dist = device_map(m.map_size, m.kw, m.occ, m.src, m.k, m.res)
        assert np.array_equal(gm.origin, m.origin) and gm.info.resolution_inv == m.res_inv
        out[name] = (gm, cr.Field(m.origin, m.res, dist, "cut", gm.info.resolution_inv))
    yield out
    for gm, _ in out.values():
        gm.close()


def ref(sc, field):
    if sc["tag"] not in _REF:
        _REF[sc["tag"]] = cc.restate(sc, field=field)
    return _REF[sc["tag"]]


def run(gm, scs, **kw):
    """one call for scenes that share their map and configuration"""
    s0 = scs[0]
    key = ("map", "degree", "clearance", "max_events", "max_pts")
    assert all(tuple(s[k] for k in key) == tuple(s0[k] for k in key) for s in scs)
    return gm.collision_ranges([s["ctrl"] for s in scs], [s["dt"] for s in scs], degree=s0["degree"],
                               clearance=s0["clearance"], max_events=s0["max_events"], max_pts=s0["max_pts"], **kw)


def assert_same(out, b, r, sc):
    tag = sc["tag"]
    for k in cr.INT_KEYS:
        assert out[k][b] == r[k], (tag, k, out[k][b], r[k])
    for k in cr.DBL_KEYS:
        assert _bits(out[k][b]) == _bits(r[k]), (tag, k, out[k][b], r[k])
    for key, cnt, cap in ARRAYS:
        rows = np.array(r[key], dtype=np.float64).reshape(-1, 3)[:sc[cap]]
        assert _bits(out[key][b][:len(rows)]) == _bits(rows), (tag, key)
        assert not out[key][b][len(rows):].any(), (tag, key)  # rows that are not written are zero


def groups(scenes):
    g = {}
    for sc in scenes:
        g.setdefault((sc["map"], sc["degree"], sc["clearance"], sc["max_events"], sc["max_pts"]), []).append(sc)
    return g


# ---- 1. every scene, grouped into calls by map and configuration ---------------------------------------------------------
def test_every_scene(maps):
    seen = 0
    for key, scs in groups(SCENES).items():
        gm, field = maps[key[0]]
        out = run(gm, scs)
        assert not out["limit"]
        for b, sc in enumerate(scs):
            r = ref(sc, field)
            for k, v in sc["expect"].items():
                assert r[k] == v, (sc["tag"], k, r[k], v)
            assert_same(out, b, r, sc)
            seen += 1
    assert seen == len(SCENES) >= 29


def test_against_the_recorded_reference(maps):
    """the device against what the reference's own findCollisionRange computed on its f64 field"""
    missing = [s["tag"] for s in SCENES if not os.path.exists(os.path.join(GOLDEN, s["tag"] + ".npz"))]
    if missing:
        pytest.skip("tests/golden/collide has no recording of %s" % ", ".join(missing[:4]))
    for key, scs in groups(SCENES).items():
        gm, _ = maps[key[0]]
        out = run(gm, scs)
        for b, sc in enumerate(scs):
            z = np.load(os.path.join(GOLDEN, sc["tag"] + ".npz"))
            assert out["n_ticks"][b] == int(z["n_ticks"]), sc["tag"]
            for key_, cnt, cap in ARRAYS:
                rows = z[key_].reshape(-1, 3)
                assert out[cnt][b] == len(rows) and _bits(out[key_][b][:len(rows)]) == _bits(rows), (sc["tag"], key_)


# ---- 2. the packing: 1, 4 and 5 problems, every scene alone, the batch reversed ---------------------------------------------
def test_packing_reversal_and_batch_independence(maps):
    gm, field = maps["a"]
    main = max(groups(SCENES).values(), key=len)
    assert len(main) >= 2 * PACK + 1 and main[0]["map"] == "a"
    alone = [run(gm, [sc]) for sc in main]
    for sc, o in zip(main, alone):
        assert_same(o, 0, ref(sc, field), sc)
    for n in (1, PACK, PACK + 1):
        out = run(gm, main[:n])
        for b in range(n):
            assert_same(out, b, ref(main[b], field), main[b])
    fwd, rev = run(gm, main), run(gm, main[::-1])
    keys = cr.INT_KEYS + cr.DBL_KEYS + tuple(a[0] for a in ARRAYS)
    for b in range(len(main)):
        for k in keys:
            assert _bits(np.float64(fwd[k][b])) == _bits(np.float64(rev[k][len(main) - 1 - b])), (main[b]["tag"], k)
            assert _bits(np.float64(fwd[k][b])) == _bits(np.float64(alone[b][k][0])), (main[b]["tag"], k)
    # a wider stride of the control points: the same bits
    wide = run(gm, main[:PACK + 1], max_ctrl=64)
    for b in range(PACK + 1):
        assert_same(wide, b, ref(main[b], field), main[b])
    assert gm.collision_ranges([], [])["status"].shape == (0,)  # n_prob = 0


# ---- 3. the limits and the defined failures among good neighbours -----------------------------------------------------------
def test_limits_and_nonfinite_among_neighbours(maps):
    import fuel_amd
    gm, field = maps["a"]
    over_ev, over_pts = cc.limit_scenes()
    good = [s for s in SCENES if s["tag"] in ("enter_63", "leave_64")]
    for over in (over_ev, over_pts):
        others = [s for s in SCENES if s["degree"] == over["degree"] and s["tag"].startswith(("enter_64", "leave_64"))]
        assert len(others) == 2
        cfgd = [dict(s, max_events=over["max_events"], max_pts=over["max_pts"], tag=s["tag"] + "/" + over["tag"])
                for s in others]
        batch = cfgd[:1] + [over] + cfgd[1:]
        with pytest.raises(fuel_amd.FuelmiError, match="error -5"):
            run(gm, batch)
        out = run(gm, batch, allow_limit=True)
        assert out["limit"]
        for b, sc in enumerate(batch):
            r = cc.restate(sc, field=field)
            assert_same(out, b, r, sc)
        assert out["status"][batch.index(over)] == -1
        for k, v in over["expect"].items():
            assert out[k][batch.index(over)] == v, (over["tag"], k)
    nan = cc.nonfinite_scene()
    inf_dt = dict(good[0], tag="inf_dt", dt=float("inf"))
    batch = [good[0], nan, good[1], inf_dt, good[0]]
    out = run(gm, batch)
    assert not out["limit"] and out["status"].tolist() == [cr.OK, cr.NONFINITE, cr.OK, cr.NONFINITE, cr.OK]
    for b, sc in enumerate(batch):
        assert_same(out, b, cc.restate(sc, field=field), sc)


def test_follows_the_field_not_a_mirror():
    """the call runs behind the ESDF update on the map's stream: the answer changes with the field"""
    m = cc.spec("a")
    gm, _ = device_map(m.map_size, m.kw, m.occ, m.src, m.k, m.res)
    sc = next(s for s in SCENES if s["tag"] == "enter_64")
    assert run(gm, [sc])["n_start_events"][0] == 1
    gm.uploadOccupancy(np.full(m.nvox, tcs.L_FREE))
    gm.setLocalBound((0, 0, 0), tuple(v - 1 for v in gm.nvox))
    gm.clearAndInflateLocalMap()
    gm.updateESDF3d()
    after = run(gm, [sc])
    assert after["status"][0] == cr.NO_COLLISION and after["n_ticks"][0] == 141
    gm.close()


# ---- 4. guide points ---------------------------------------------------------------------------------------------------------
def grun(gm, scs, **kw):
    s0 = scs[0]
    key = ("ctrl_pt_dist", "degree", "max_guide")
    assert all(tuple(s[k] for k in key) == tuple(s0[k] for k in key) for s in scs)
    return gm.guide_points([s["path"] for s in scs], [s["duration"] for s in scs], ctrl_pt_dist=s0["ctrl_pt_dist"],
                           degree=s0["degree"], max_guide=s0["max_guide"], **kw)


def gassert_same(out, b, r, sc):
    for k in cr.G_INT_KEYS:
        assert out[k][b] == r[k], (sc["tag"], k, out[k][b], r[k])
    assert _bits(out["dt"][b]) == _bits(r["dt"]), sc["tag"]
    rows = np.array(r["guide_pts"], dtype=np.float64).reshape(-1, 3)[:sc["max_guide"]]
    assert _bits(out["guide_pts"][b][:len(rows)]) == _bits(rows), sc["tag"]
    assert not out["guide_pts"][b][len(rows):].any(), sc["tag"]


def test_every_guide_scene(maps):
    gm, _ = maps["b"]
    g = {}
    for sc in GUIDES:
        g.setdefault((sc["ctrl_pt_dist"], sc["degree"], sc["max_guide"]), []).append(sc)
    seen = 0
    for scs in g.values():
        out = grun(gm, scs, allow_limit=True)
        assert out["limit"] == any(s["expect"].get("status") == cr.OVER for s in scs)
        for b, sc in enumerate(scs):
            r = cc.grestate(sc)
            for k, v in sc["expect"].items():
                assert r[k] == v, (sc["tag"], k)
            gassert_same(out, b, r, sc)
            alone = grun(gm, [sc], allow_limit=True)
            gassert_same(alone, 0, r, sc)
            seen += 1
    assert seen == len(GUIDES)
    # UNDEFINED between good neighbours, and the batch reversed
    main = max(g.values(), key=len)
    assert any(s["expect"].get("status") == cr.G_UNDEFINED for s in main) and len(main) > PACK
    fwd, rev = grun(gm, main), grun(gm, main[::-1])
    assert not fwd["limit"]
    for b, sc in enumerate(main):
        gassert_same(rev, len(main) - 1 - b, cc.grestate(sc), sc)
    # a wider stride of the path points
    wide = grun(gm, main[:3], max_path_points=cc.MAX_PATH_POINTS)
    for b in range(3):
        gassert_same(wide, b, cc.grestate(main[b]), main[b])
    assert gm.guide_points([], [])["status"].shape == (0,)
    # the recordings of the reference's own pathLength / pathToGuidePts / getTrajInfoInDuration
    rec = [s for s in GUIDES if os.path.exists(os.path.join(GOLDEN, "guide_" + s["tag"] + ".npz"))]
    for sc in rec:
        z = np.load(os.path.join(GOLDEN, "guide_" + sc["tag"] + ".npz"))
        o = grun(gm, [sc], allow_limit=True)
        assert (o["seg_num"][0], o["n_pts"][0], o["n_ctrl"][0]) == (int(z["seg_num"]), int(z["n_pts"]), int(z["n_ctrl"]))
        rows = z["guide_pts"].reshape(-1, 3)[:sc["max_guide"]]
        assert _bits(o["dt"][0]) == _bits(z["dt"]) and _bits(o["guide_pts"][0][:len(rows)]) == _bits(rows), sc["tag"]


@pytest.mark.parametrize("degree", [3, 4])
def test_guide_points_feed_the_guide_cost(maps, degree):
    """the rows go unchanged into fuelmi_bspline_problem.guide_pts of one fuelmi_bspline_cost_grad call with
    FUELMI_COST_GUIDE: accepted, and the cost of the one computed from the restatement's points"""
    import fuel_amd
    gm, _ = maps["a"]
    sc = next(s for s in GUIDES if s["tag"] == "bend_deg%d" % degree)
    out = grun(gm, [sc])
    r = cc.grestate(sc)
    N, ng = int(out["n_ctrl"][0]), int(out["n_guide"][0])
    assert ng == N - 2 * degree == r["n_guide"] > 0
    rng = np.random.default_rng(5)
    x = rng.uniform(-1.0, 1.0, size=(1, 3 * N))
    opt = fuel_amd.BsplineOptimizer(bspline_degree=degree)
    opt.setEnvironment(gm)
    costs = []
    for guide in (out["guide_pts"][0][:ng], np.array(r["guide_pts"])):
        pb = fuel_amd.BsplineBatchProblem(x, N, fuel_amd.GUIDE, 0.3, np.zeros((1, 3, 3)), np.zeros((1, 3, 3)), 3, 3,
                                          float(out["dt"][0]), None, guide.reshape(1, ng, 3))
        cost, grad = opt.combineCost(pb)
        assert np.isfinite(cost).all() and cost[0] > 0.0 and np.abs(grad).max() > 0.0
        costs.append(cost[0])
    assert _bits(costs[0]) == _bits(costs[1])
    # by hand: ld_guide * sum |q_i - guide_(i - order)|^2 over the inner control points (bspline_optimizer.cpp calcGuideCost)
    q = x.reshape(N, 3)[degree:N - degree]
    want = fuel_amd.host.DEFAULT_BSPLINE["ld_guide"] * float(((q - np.array(r["guide_pts"])) ** 2).sum())
    assert abs(costs[0] - want) <= 1e-12 * want


# ---- 5. the chain: collision ranges -> topological search ---------------------------------------------------------------------
def test_chain_into_the_topological_search():
    """start_pts / end_pts / first_start / last_end of collision_ranges go unchanged into topo_paths and give the paths the
    restatement chain gives"""
    sc = tcs.scenes()["pillar"]
    k = tcs.squared_distance(tcs.sources(sc["blocks"]))
    gm, dist = device_map(tcs.MAP_SIZE, {}, tcs.occupancy(sc["blocks"]), tcs.sources(sc["blocks"]), k, tcs.RES)
    ctrl = cc.flight((-2.5, 0.0, 0.0), (1, 0, 0), 0.02, 12.5)
    clearance = sc["cfg"]["clearance"]
    col = gm.collision_ranges([ctrl], [0.5], clearance=clearance)
    want = cr.collision_ranges(cr.Field(tcs.ORIGIN, tcs.RES, dist, "cut", gm.info.resolution_inv), ctrl, 3, 0.5, clearance, 8, 64)
    cs = dict(tag="chain", max_events=8, max_pts=64)
    assert_same(col, 0, want, cs)
    assert col["status"][0] == cr.OK and col["n_start_pts"][0] >= 2 and col["n_end_pts"][0] >= 2
    nsp, nep = int(col["n_start_pts"][0]), int(col["n_end_pts"][0])
    cfg = {key: v for key, v in sc["cfg"].items() if key != "max_sample_num"}
    got = gm.topo_paths(col["first_start"], col["last_end"], [sc["samples"]], [col["start_pts"][0][:nsp]],
                        [col["end_pts"][0][:nep]], **cfg)
    r = tpr.find_topo_paths(tpr.Field(tcs.ORIGIN, tcs.RES, dist, "cut"), sc["cfg"], want["first_start"], want["last_end"],
                            sc["samples"], want["start_pts"], want["end_pts"])
    assert got["status"][0] == r["status"] == tpr.OK and list(got["counts"][0]) == list(r["counts"])
    assert len(got["sel"][0]) == len(r["sel"]) >= 1
    for a, b in zip(got["sel"][0], r["sel"]):
        assert _bits(a) == _bits(b)
        # (the five shortcut iterations behind the merge keep the merged path's two ends)
        assert _bits(a[0]) == _bits(col["start_pts"][0][0]) and _bits(a[-1]) == _bits(col["end_pts"][0][nep - 1])
    # ... and on into the guide points of every select path
    dur = 12.5
    gp = gm.guide_points(got["sel"][0], [dur] * len(got["sel"][0]))
    for b, path in enumerate(r["sel"]):
        w = cr.guide_points(path, dur, 0.5, 3, 64)
        gassert_same(gp, b, w, dict(tag="chain guide", max_guide=64))
        assert gp["status"][b] == cr.G_OK and gp["n_guide"][b] == gp["n_ctrl"][b] - 6
    gm.close()


# ---- 6. the tick cap -----------------------------------------------------------------------------------------------------------
def test_tick_cap(maps):
    """2^20 ticks are walked, one more is status -1.  Two slow flights in free space (every tick safe) whose t_mp lies on
    either side of the accumulated time of tick 2^20; numpy's cumulative sum adds one element at a time, as the loop does"""
    import traj_check_ref as tr
    gm, field = maps["a"]
    acc = np.cumsum(np.concatenate([[0.0], np.full(cr.CAP, cr.TICK)]))  # acc[k] = tc of tick k
    n, p = 1024, 3
    ctrl = cc.flight((-2.9, cc.LINE_MID, cc.Z_LINE), (1, 0, 0), 0.3 / cr.CAP, 0.5 * (n - p), p)  # (millimetres in all)
    assert len(ctrl) == n

    def t_mp(dt):
        return tr.knots(n, p, dt)[n]
    fits = (acc[cr.CAP - 1] + 0.02) / (n - p)   # the last tick that passes is 2^20 - 1
    over = (acc[cr.CAP] + 0.02) / (n - p)       # tick 2^20 would pass too
    assert acc[cr.CAP - 1] <= t_mp(fits) + 1e-4 < acc[cr.CAP] <= t_mp(over) + 1e-4
    good = next(s for s in SCENES if s["tag"] == "enter_64")
    out = gm.collision_ranges([good["ctrl"], ctrl, ctrl, good["ctrl"]], [good["dt"], fits, over, good["dt"]], allow_limit=True)
    assert out["limit"] and out["status"].tolist() == [cr.OK, cr.NO_COLLISION, -1, cr.OK]
    assert out["n_ticks"][1] == out["n_ticks"][2] == cr.CAP and not out["n_start_events"][1:3].any()
    assert not out["n_start_pts"][1:3].any() and not out["n_end_pts"][1:3].any()
    for b in (0, 3):
        assert_same(out, b, ref(good, field), good)
