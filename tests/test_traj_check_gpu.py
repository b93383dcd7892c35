"""fuelmi_map_check_trajs / fuelmi_bspline_dev_check_trajs on the device against the restatement
(tests/traj_check_ref.py) on the scenes of tests/traj_check_cases.py.

Every output is compared BIT FOR BIT: the step is + - * /, floor and a correctly rounded f64 square root, compiled without
FMA contraction, so there is no tolerance to measure.  The inflated plane the restatement reads is the one read back from
the device (it is also compared with the scenes' numpy inflation, which the CPU test pins to the oracle).  Then the
workgroup packing (4 problems per workgroup), batch independence, the defined results among good neighbours, the device
chain behind _dev_optimize and the facade with its inflate mirror switched off."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import traj_check_cases as tc
import traj_check_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

INT_KEYS = ("status", "safe", "n_samples", "hit_index", "end_reason")
DBL_KEYS = ("distance", "hit_t", "duration", "hit_pos")
PACK = 4  # problems per workgroup (traj_check.hip TC_WAVES)
_REF = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def make_map(name):
    import fuel_amd
    m = tc.spec(name)
    gm = fuel_amd.SDFMap(m.map_size, device=0, **m.kw)
    assert gm.nvox == m.nvox and np.array_equal(gm.origin, m.origin) and gm.info.resolution_inv == m.res_inv
    gm.uploadOccupancy(m.occ3.reshape(-1))
    gm.setLocalBound(*helpers.full_box(gm.nvox))
    gm.clearAndInflateLocalMap()
    return gm


@pytest.fixture(scope="module")
def maps():
    """name -> (device map, the restatement's grid on the plane read back from that map)"""
    out = {}
    for name in sorted(tc.MAPS):
        gm = make_map(name)
        infl = gm.syncHost(inflate=True)["inflate"].reshape(gm.nvox)
        assert np.array_equal(infl, tc.spec(name).infl3), name
        out[name] = (gm, tc.spec(name).grid(infl))
    yield out
    for gm, _ in out.values():
        gm.close()


def ref(sc, grid):
    """the restatement of one scene on the device's plane, computed once"""
    if id(sc) not in _REF:
        _REF[id(sc)] = (sc, tc.restate(sc, "first_hit", grid=grid, width=8192 if sc["step"] < tr.STEP else 64))
    return _REF[id(sc)][1]


def run(gm, scs, **kw):
    """one call for scenes that share their map and configuration"""
    s0 = scs[0]
    assert all((s["map"], s["degree"], s["step"], s["max_radius"]) == (s0["map"], s0["degree"], s0["step"], s0["max_radius"])
               for s in scs)
    return gm.check_trajs([s["ctrl"] for s in scs], [s["dt"] for s in scs], [s["t_now"] for s in scs], degree=s0["degree"],
                          step=s0["step"], max_radius=s0["max_radius"], **kw)


def assert_same(out, b, r, tag=""):
    for k in INT_KEYS:
        assert out[k][b] == r[k], (tag, k, out[k][b], r[k])
    for k in DBL_KEYS:
        assert _bits(out[k][b]) == _bits(r[k]), (tag, k, out[k][b], r[k])


def groups(scenes):
    g = {}
    for sc in scenes:
        g.setdefault((sc["map"], sc["degree"], sc["step"], sc["max_radius"]), []).append(sc)
    return g


QUICK = tc.quick_scenes()


# ---- 1. every scene, grouped into calls by map and configuration ----------------------------------------------------------
def test_every_scene(maps):
    seen = 0
    for (name, _, _, _), scs in groups(QUICK).items():
        gm, grid = maps[name]
        out = run(gm, scs)
        assert not out["limit"]
        for b, sc in enumerate(scs):
            r = ref(sc, grid)
            for k, v in sc["expect"].items():
                assert r[k] == v, (sc["tag"], k, r[k], v)
            assert_same(out, b, r, sc["tag"])
            seen += 1
    assert seen == len(QUICK) >= 39


# ---- 2. the packing: 1, 4 and 5 problems, and every scene alone --------------------------------------------------------------
def test_packing_and_batch_independence(maps):
    gm, grid = maps["a"]
    main = max(groups(QUICK).values(), key=len)
    assert len(main) >= 3 * PACK and main[0]["map"] == "a"
    alone = [run(gm, [sc]) for sc in main]
    for sc, o in zip(main, alone):
        assert_same(o, 0, ref(sc, grid), sc["tag"])
    for n in (1, PACK, PACK + 1):
        out = run(gm, main[:n])
        for b in range(n):
            assert_same(out, b, ref(main[b], grid), main[b]["tag"])
    # the same problem at several places of a mixed batch, a wider stride of the control points: the same bits
    probe = [s for s in main if s["tag"] in ("hit_65", "voxel_boundary")]
    assert len(probe) == 2
    for sc in probe:
        rest = [s for s in main if s is not sc]
        for place in (0, 1, PACK - 1, PACK, 2 * PACK + 1, len(rest)):
            batch = rest[:place] + [sc] + rest[place:]
            out = run(gm, batch, max_ctrl=64)
            for k in INT_KEYS + DBL_KEYS:
                assert _bits(np.float64(out[k][place])) == _bits(np.float64(alone[main.index(sc)][k][0])), (sc["tag"], place, k)
            for b, s in enumerate(batch):
                assert_same(out, b, ref(s, grid), s["tag"])
    assert run(gm, main[:1])["hit_pos"].shape == (1, 3)
    assert gm.check_trajs([], [], [])["status"].shape == (0,)  # n_prob = 0


# ---- 3. the defined results among good neighbours ----------------------------------------------------------------------------
def test_nonfinite_and_cap_among_neighbours(maps):
    import fuel_amd
    gm, grid = maps["a"]
    cap, exact = tc.long_scenes()
    kw = dict(step=tc.CAP_STEP)
    good_hit = tc.scene("fine_hit", "a", tc.line((tc.BAND_X - 0.205, tc.HIT_Y, tc.HIT_Z), (1, 0, 0), 12), tc.DT, **kw)
    good_safe = tc.scene("fine_safe", "a", tc.wiggle((-1.2, -1.5, 0.05), 9, seed=4), 0.1, **kw)
    bad = tc.scene("fine_nonfinite", "a", tc.wiggle((-1.2, -1.5, 0.05), 12, seed=3), 1e308, **kw)
    batch = [good_hit, bad, cap, good_safe, exact, good_hit]
    with pytest.raises(fuel_amd.FuelmiError, match="error -5"):
        run(gm, batch)
    out = run(gm, batch, allow_limit=True)
    assert out["limit"]
    for b, sc in enumerate(batch):
        assert_same(out, b, ref(sc, grid), sc["tag"])
    assert out["status"].tolist() == [tr.OK, tr.NONFINITE, tr.OVER, tr.OK, tr.OK, tr.OK]
    assert out["safe"].tolist() == [0, 0, 0, 1, 1, 0] and out["n_samples"][0] > 5 * 64
    assert out["end_reason"].tolist() == [tr.END_HIT, tr.END_NONFINITE, tr.END_CAP, tr.END_DURATION, tr.END_DURATION, tr.END_HIT]
    assert out["n_samples"][2] == out["n_samples"][4] == tr.CAP
    # without the capped problem the same batch is no limit
    out = run(gm, [good_hit, bad, good_safe, exact])
    assert not out["limit"] and out["status"].tolist() == [tr.OK, tr.NONFINITE, tr.OK, tr.OK]


# ---- 4. the device chain -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mintime", [True, False])
def test_device_chain(maps, mintime):
    import fuel_amd
    gm, grid = maps["a"]
    C, N, dt = 8, 16, 0.2
    rng = np.random.default_rng(23)
    ctrl = np.stack([tc.wiggle((0.3, tc.HIT_Y, tc.HIT_Z) if c % 2 == 0 else (-1.4, tc.FREE_Y, 0.3), N, seed=40 + c, amp=0.03)
                     for c in range(C)])
    x, ptd, st, en = helpers.bspline_inputs(ctrl, dt, mintime)
    cf = fuel_amd.SMOOTHNESS | fuel_amd.FEASIBILITY | fuel_amd.START | fuel_amd.END | (fuel_amd.MINTIME if mintime else 0)
    opt = fuel_amd.BsplineOptimizer()
    opt.setEnvironment(gm)
    dev = opt.deviceProblem(fuel_amd.BsplineBatchProblem(x, N, cf, ptd, st, en, 3, 3, dt))
    t_now = rng.uniform(0.0, 0.4, C)
    with pytest.raises(fuel_amd.FuelmiError, match="error -1"):  # not optimised yet
        dev.check_trajs(t_now)
    xo, co, ev = dev.optimize(max_eval=40)
    got = dev.check_trajs(t_now)
    pos = xo[:, :3 * N].reshape(C, N, 3)
    knot = xo[:, -1] if mintime else np.full(C, dt)
    if mintime:
        assert np.abs(knot - dt).max() > 0.0  # the knot span really comes from the variables
    want = gm.check_trajs(list(pos), knot, t_now)
    for k in INT_KEYS + DBL_KEYS:
        assert _bits(np.asarray(got[k], dtype=np.float64)) == _bits(np.asarray(want[k], dtype=np.float64)), k
    assert not got["status"].any() and set(got["safe"].tolist()) == {0, 1}, got["safe"]
    for c in range(C):  # and both equal the restatement on the x_out the solve returned
        assert_same(got, c, tr.check_first_hit(grid, pos[c], 3, float(knot[c]), float(t_now[c])), "candidate %d" % c)
    with pytest.raises(fuel_amd.FuelmiError, match="error -1"):  # the batch's degree is 3
        dev.check_trajs(t_now, degree=4)
    # a reload invalidates what the last solve left
    dev.loadSamples(np.full(C, dt), np.ascontiguousarray(ctrl[:, :N - 2]), np.zeros((C, 4, 3)))
    with pytest.raises(fuel_amd.FuelmiError, match="error -1"):
        dev.check_trajs(t_now)
    dev.optimize(max_eval=5)
    assert not dev.check_trajs(t_now)["status"].any()
    dev.close()


def test_device_chain_refuses_other_batches(maps):
    import fuel_amd
    gm, _ = maps["a"]
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
        dev.check_trajs(np.zeros(2))
    dev.close()


# ---- 5. the check follows the plane, not a mirror ------------------------------------------------------------------------------
def test_follows_the_inflation_queued_before_it():
    """fuelmi_map_check_trajs runs behind the inflation on the map's stream: the answer changes with the plane, no host
    mirror is refreshed in between"""
    gm = make_map("a")
    m = tc.spec("a")
    sc = tc.hit_scene(65)
    before = run(gm, [sc])
    assert before["safe"][0] == 0
    occ = m.occ3.copy()
    occ[30, 20, 10] = tc.UNKNOWN  # the first obstacle goes
    gm.uploadOccupancy(occ.reshape(-1))
    gm.setLocalBound(*helpers.full_box(gm.nvox))
    gm.clearAndInflateLocalMap()
    after = run(gm, [sc])
    assert after["safe"][0] == 1 and after["distance"][0] == -1.0 and after["end_reason"][0] == tr.END_DURATION
    gm.close()


# ---- 6. the facade -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b"])
def test_facade_check_traj_collision(maps, tmp_path, name):
    """facade_trajcheck: BsplineOptimizer::checkTrajCollision with the inflate mirror switched off, in a child process,
    against SDFMap.check_trajs; the reference's host loop on the mirror nobody refreshed sees no obstacle at all"""
    gm, grid = maps[name]
    m = tc.spec(name)
    scs = [s for s in QUICK if s["map"] == name and s["step"] == tr.STEP and s["max_radius"] == tr.MAX_RADIUS]
    scs = [s for s in scs if s["tag"] != "nonfinite"]  # (every degree: the facade takes it per call)
    assert len(scs) >= 6 and (name == "b" or {s["degree"] for s in scs} == {3, 4, 5})
    scen = str(tmp_path / "scen.bin")
    with open(scen, "wb") as f:
        np.array(list(m.map_size) + list(m.origin) + list(m.origin + np.array(m.map_size)) + [m.res, m.kw["ground_height"]],
                 dtype=np.float64).tofile(f)
        m.occ3.reshape(-1).tofile(f)
        for s in scs:
            np.concatenate([[s["degree"], len(s["ctrl"]), s["dt"], s["t_now"]], s["ctrl"].reshape(-1)]).tofile(f)
    exe = os.path.join(ROOT, "fuel_amd", "facade", "facade_trajcheck")
    p = subprocess.run([exe, scen], check=True, capture_output=True, text=True, timeout=300)
    res = json.loads(p.stdout[p.stdout.index("{"):])["problems"]
    assert len(res) == len(scs)
    unsafe = 0
    for got, s in zip(res, scs):
        o = gm.check_trajs([s["ctrl"]], [s["dt"]], [s["t_now"]], degree=s["degree"])
        assert_same(o, 0, ref(s, grid), s["tag"])
        assert got["safe"] == o["safe"][0], s["tag"]
        # distance is written only when the result is unsafe (the driver hands in -7)
        assert got["distance"] == (o["distance"][0] if not o["safe"][0] else -7.0), s["tag"]
        assert got["stale_mirror_safe"] == 1, s["tag"]
        unsafe += 1 - got["safe"]
    assert unsafe >= (3 if name == "a" else 0) and len(res) - unsafe >= 3
