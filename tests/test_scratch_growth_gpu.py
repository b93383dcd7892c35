"""The device scratch of the batched planner calls when it grows between calls on one live map or batch: a small
problem set, a larger one that outgrows the pool, the small one again.  Every round is held to what the call's own GPU
test asserts against its CPU reference (those tests' helpers, imported), and the third round repeats the first bit for
bit.  Five problems cross the four-problems-per-workgroup edge of the wave-per-problem kernels.

The scratch of fuelmi_bspline_dev_check_trajs depends on the batch's candidate count alone, so on one batch it grows
only once, from nothing; its three rounds differ in t_now."""
import numpy as np
import pytest

import goal_path_ref as gr
import helpers
import kino_ref as kr
import map_cloud_cases as mc
import map_cloud_ref as mr
import traj_check_cases as tcc
import traj_check_ref as tr
import traj_sample_cases as tsc
import traj_sample_ref as sr
import waypoint_traj_ref as wr
import test_goal_path_gpu as t_goal
import test_kino_path_gpu as t_kino
import test_map_cloud_gpu as t_cloud
import test_path_cost_gpu as t_path
import test_refine_gpu as t_refine
import test_traj_check_gpu as t_chk
import test_traj_sample_gpu as t_smp
import test_waypoint_traj_gpu as t_wp

pytestmark = pytest.mark.gpu

ROUNDS = (1, 5, 1)  # problems per round


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def _same(a, b):
    """two results of one call, every bit: arrays, lists of arrays, tuples and dicts of them"""
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is b
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the seven map calls -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def door():
    """the wall-and-door map: two starts west of the wall, goals on both sides"""
    om, pm, size, box, case = gr.door_scene()
    gm = t_goal._device_twin(om, size, box)
    yield gm, om, pm, case
    gm.close()


def _refine_problems(case, n):
    """n problems of two layers from the door scene's goals; zero velocity: no direction term, every cost exact"""
    goals = case["goals"]
    layer = lambda i: np.concatenate([goals[i:i + 3], np.array([[0.3], [-0.4], [1.0]])], axis=1)  # noqa: E731
    return [(case["starts"][43 * (b % 2)], np.zeros(3), 0.1 * b, [layer(6 * b), layer(6 * b + 3)]) for b in range(n)]


def _assert_refine(gm, probs):
    ch, c, tours = t_refine._refine(gm, probs)
    assert tours is None
    for b, (pos, vel, yaw, layers) in enumerate(probs):
        _, _, rch, rc, _ = t_refine._restated(gm, pos, vel, yaw, layers)
        t_refine._assert_same(ch[b], c[b], rch, rc)
    return ch, c


def test_path_costs_then_refine(door):
    gm, om, pm, case = door
    _assert_refine(gm, _refine_problems(case, 1))  # the refine pool exists before the path pool grows
    pick = [0, 1, 2, 47, 44]                       # both starts: the larger round searches two lattices
    lattices, seen, kinds = {}, [], set()
    for n in ROUNDS:
        p1, p2 = case["starts"][pick[:n]], case["goals"][pick[:n]]
        length, kind, paths = gm.path_costs(p1, p2, max_points=512)
        t_path._compare(pm, om, p1, p2, length, kind, paths, lattices)
        kinds |= set(kind.tolist())
        seen.append((length, kind, paths))
        if n == max(ROUNDS):  # the refine scratch after the path scratch has grown
            _assert_refine(gm, _refine_problems(case, 2))
    assert 1 in kinds  # the lattice search ran
    assert _same(seen[0], seen[2])


def test_refine_tours(door):
    gm, om, pm, case = door
    seen = [_assert_refine(gm, _refine_problems(case, n)) for n in ROUNDS]
    assert _same(seen[0], seen[2])


def test_goal_paths(door):
    gm, om, pm, case = door
    pick = [1, 0, 2, 43, 44]
    sources, seen = {}, []
    for n in ROUNDS:
        sub = dict(starts=case["starts"][pick[:n]], goals=case["goals"][pick[:n]], cfg={})
        out, ref = t_goal._assert_case(gm, pm, om, sub, sources, tag="round of %d" % n)
        seen.append(out)
    assert len(sources) == 2 and seen[1]["raw_len"].max() > 2
    assert _same(seen[0], seen[2])


def test_kino_paths():
    sc = kr.scenes()["open"]
    gm = t_kino._device_map(sc)
    probs = kr.batch65()[:max(ROUNDS)]
    ref = kr.problem_results("open", probs)
    seen = []
    try:
        for n in ROUNDS:
            out = t_kino._run(gm, probs[:n], t_kino._cfg(sc))
            assert len(out["status"]) == n and not out["limit"]
            for b in range(n):
                r, robust, worst = ref[b]
                assert robust, b
                t_kino._assert_problem(out, b, r, worst, "round of %d" % n)
            seen.append(out)
    finally:
        gm.close()
        t_kino._maps.clear()
    assert _same(seen[0], seen[2])


@pytest.fixture(scope="module")
def map_a():
    """map "a" of the trajectory checks: (device map, the restatement's grid on the plane read back from it)"""
    gm = t_chk.make_map("a")
    infl = gm.syncHost(inflate=True)["inflate"].reshape(gm.nvox)
    assert np.array_equal(infl, tcc.spec("a").infl3)
    yield gm, tcc.spec("a").grid(infl)
    gm.close()


def test_check_trajs(map_a):
    gm, grid = map_a
    main = max(t_chk.groups(t_chk.QUICK).values(), key=len)
    assert len(main) >= max(ROUNDS) and main[0]["map"] == "a"
    seen = []
    for n in ROUNDS:
        out = t_chk.run(gm, main[:n])
        assert not out["limit"]
        for b in range(n):
            t_chk.assert_same(out, b, t_chk.ref(main[b], grid), main[b]["tag"])
        seen.append(out)
    assert _same(seen[0], seen[2])


def test_sample_trajs(map_a):
    gm, _ = map_a
    main = max((g for k, g in tsc.groups(t_smp.QUICK).items() if k[0] == sr.COMMAND), key=len)
    main = sorted((s for s in main if len(s["t"])), key=lambda s: len(s["t"]))
    scs = [main[0]] + main[-(max(ROUNDS) - 1):]  # the shortest tape first: the larger round also has the longer rows
    assert len(scs[0]["t"]) < len(scs[-1]["t"])
    seen = []
    for n in ROUNDS:
        out = t_smp.run(gm, scs[:n])
        assert out["status"].shape == (n, max(len(s["t"]) for s in scs[:n]))
        for b in range(n):
            t_smp.assert_same(out, b, scs[b])
        seen.append(out)
    assert _same(seen[0], seen[2])


def test_extract_cloud():
    m = mc.MapSpec("growth", (32, 32, 16), 0.1, -1.0)
    gm = t_cloud.new_map(m)
    try:
        o, i = t_cloud.load_state(gm, m, (mc.st_random(m), None))
        small, whole = ((3, 4, 2), (10, 11, 7)), mc.full_box(m.nvox)  # 8 x 8 x 6 voxels, then all 16384
        seen = []
        for lo, hi in (small, whole, small):
            seen.append([t_cloud.check(gm, o, i, kind, lo, hi, tag="growth") for kind in mr.KINDS])
        assert max(len(c) for c in seen[0]) < max(len(c) for c in seen[1])
        assert _same(seen[0], seen[2])
    finally:
        gm.close()


# ---- the four batch calls ------------------------------------------------------------------------------------------------
C_BATCH, N_CTRL, DT = 5, 16, 0.2


@pytest.fixture(scope="module")
def solved(map_a):
    """a batch of five candidates on map "a" after one solve: (batch, control points, knot spans) of what it left"""
    import fuel_amd
    gm, _ = map_a
    ctrl = np.stack([tcc.wiggle((0.3, tcc.HIT_Y, tcc.HIT_Z) if c % 2 == 0 else (-1.4, tcc.FREE_Y, 0.3), N_CTRL, seed=40 + c,
                                amp=0.03) for c in range(C_BATCH)])
    x, ptd, st, en = helpers.bspline_inputs(ctrl, DT, True)
    cf = fuel_amd.SMOOTHNESS | fuel_amd.FEASIBILITY | fuel_amd.START | fuel_amd.END | fuel_amd.MINTIME
    opt = fuel_amd.BsplineOptimizer()
    opt.setEnvironment(gm)
    dev = opt.deviceProblem(fuel_amd.BsplineBatchProblem(x, N_CTRL, cf, ptd, st, en, 3, 3, DT))
    xo, _, _ = dev.optimize(max_eval=40)
    yield dev, xo[:, :3 * N_CTRL].reshape(C_BATCH, N_CTRL, 3), xo[:, -1].copy()
    dev.close()


def test_batch_plan_yaws(map_a, solved):
    gm, _ = map_a
    dev, pos, knot = solved
    rng = np.random.default_rng(17)
    start = np.stack([rng.uniform(-3, 3, C_BATCH), rng.uniform(-0.3, 0.3, C_BATCH), rng.uniform(-0.2, 0.2, C_BATCH)], axis=1)
    end = rng.uniform(-3, 3, C_BATCH)
    small, large = dict(relax_time=0.5, derivs=False), dict(relax_time=0.5, derivs=True, max_seg=48)
    seen = []
    for kw in (small, large, small):
        got = dev.plan_yaws(start, end, **kw)
        want = gm.plan_yaws(list(pos), knot, start, end, **kw)
        assert not got["status"].any()
        assert (got["yawdot_ctrl"] is not None) == kw["derivs"]
        assert _same(got, want)
        seen.append(got)
    assert seen[1]["yaw_ctrl"].shape[1] > seen[0]["yaw_ctrl"].shape[1]
    assert _same(seen[0], seen[2])


def test_batch_check_trajs(map_a, solved):
    gm, grid = map_a
    dev, pos, knot = solved
    rng = np.random.default_rng(23)
    first = rng.uniform(0.0, 0.4, C_BATCH)
    seen = []
    for t_now in (first, first + 0.3, first):
        got = dev.check_trajs(t_now)
        want = gm.check_trajs(list(pos), knot, t_now)
        for k in t_chk.INT_KEYS + t_chk.DBL_KEYS:
            assert _bits(got[k]) == _bits(want[k]), k
        for c in range(C_BATCH):
            t_chk.assert_same(got, c, tr.check_first_hit(grid, pos[c], 3, float(knot[c]), float(t_now[c])), "candidate %d" % c)
        seen.append(got)
    assert not seen[0]["status"].any() and set(seen[0]["safe"].tolist()) == {0, 1}
    assert _same(seen[0], seen[2])


def test_batch_sample_trajs(map_a, solved):
    gm, _ = map_a
    dev, pos, knot = solved
    rng = np.random.default_rng(5)
    long_t = [np.sort(rng.uniform(-0.2, 3.2, n)) for n in (1, 63, 64, 65, 129)]
    short_t = [t[:1] for t in long_t]
    yaw = [tsc.yaw_wiggle(15, 60 + c) if c % 3 else None for c in range(C_BATCH)]
    stop = rng.uniform(1.0, 4.0, C_BATCH)
    seen = []
    for t in (short_t, long_t, short_t):
        kw = dict(yaw_ctrl=yaw, yaw_dt=np.full(C_BATCH, 0.21), t_stop=stop, flight=np.zeros((C_BATCH, 8)))
        got = dev.sample_trajs(t, **kw)
        want = gm.sampleTrajs(list(pos), knot, t, **kw)
        for k in ("status",) + t_smp.VEC + t_smp.SCL + ("duration", "flight"):
            assert got[k].tobytes() == want[k].tobytes(), k
        for c in range(C_BATCH):
            r = sr.sample(sr.COMMAND, pos[c], 3, float(knot[c]), t[c], yaw[c], 3, 0.21, float(stop[c]))
            r["flight"] = sr.record_windowed([0.0] * 8, t[c], r)
            t_smp.assert_same(got, c, dict(tag="candidate %d" % c, t=t[c]), r)
        seen.append(got)
    assert seen[1]["status"].shape[1] == 129 and seen[0]["status"].shape[1] == 1
    assert _same(seen[0], seen[2])


def test_batch_load_waypoints():
    """the chain of tests/test_waypoint_traj_gpu.py: the load equals loadSamples of the host call's samples, by the cost,
    the gradient and a solve of both batches; the staging grows with max_way_points"""
    import fuel_amd
    gm = fuel_amd.SDFMap(t_wp.MAP_SIZE, t_wp.BMIN, t_wp.BMAX, device=0)
    try:
        gm.setLocalBound(*helpers.full_box(gm.nvox))
        gm.clearAndInflateLocalMap()
        gm.updateESDF3d()
        N = 14
        seg = N - 3
        few = [t_wp._in_box(wr.problem(300 + i, n, 0.3, 0.9)) for i, n in enumerate((3, 4, 3, 4, 3))]
        many = [t_wp._in_box(wr.problem(300 + i, n, 0.3, 0.9)) for i, n in enumerate((3, 4, 5, 8, 11))]
        dev = t_wp._batch(gm, C_BATCH, N)
        seen = []
        for ps, maxw in ((few, 4), (many, 40), (few, 4)):
            ways, vels, accs = [p["way"] for p in ps], [p["vel"] for p in ps], [p["acc"] for p in ps]
            status, duration = dev.load_waypoints(ways, vels, accs, max_way_points=maxw, **wr.DEFAULTS)
            assert not status.any()
            chain = t_wp._state(dev)
            host = gm.waypoint_trajs(ways, vels, accs, seg_num=seg, max_samples=seg + 1, **wr.DEFAULTS)
            assert host["n_samples"].tolist() == [seg + 1] * C_BATCH and _bits(host["duration"]) == _bits(duration)
            dev2 = t_wp._batch(gm, C_BATCH, N)
            dev2.loadSamples(host["dt"], np.array(host["samples"]), host["derivs"])
            assert t_wp._state(dev2) == chain
            dev2.close()
            seen.append((status, duration, chain))
        dev.close()
        assert _same(seen[0][:2], seen[2][:2]) and seen[0][2] == seen[2][2]
    finally:
        gm.close()
