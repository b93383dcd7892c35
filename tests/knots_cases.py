"""The scenes of the given-knots path (spline_stage_knots in fuel_amd/csrc/spline_internal.h and the three kernels that
call it): a position spline on map "a" of tests/traj_check_cases.py plus a knot vector, and what each of the three
consumers is asked about it -- t_now of the safety check, the sample times, the yaw problem.  Every scene feeds all three.
tests/test_knots_cpu.py pins them to the reference's own class (tests/golden/knots/scenes.npz) and runs them through the
host build of the kernels; tests/test_knots_gpu.py runs them on the device.  Nothing here needs a GPU.

A scene is a dict: tag, degree, ctrl [n, 3], u [n + degree + 1], t_now, t (sample times), dyadic (its knots are multiples
of 2^-12, so u[k] - u[p] and t + u[p] are exact and a time drawn on a knot lands on it)."""
import math

import numpy as np

import traj_adjust_cases as tac
import traj_adjust_ref as ar
import traj_check_cases as tc
import traj_check_ref as tr
import yaw_plan_ref as yr

MAP = "a"
CHECK_WAVES, SAMPLE_WAVES = 4, 3  # problems per workgroup: traj_check.hip TC_WAVES, traj_sample.hip TS_WAVES
GRAIN = 4096.0                    # dyadic knots: multiples of 2^-12
X0, SPAN = -1.7, 3.2              # the flights run along +x on the first obstacle's line of map a, inside the map


def flight(n, seed, x0=X0, span=SPAN):
    """n control points along +x through the band the voxel (30, 20, 10) inflates, a seeded lateral wiggle"""
    return tc.wiggle((x0, tc.HIT_Y, tc.HIT_Z), n, seed, spacing=span / max(n - 1, 1), amp=0.04)


def dyadic(u):
    u = np.round(np.asarray(u, dtype=np.float64) * GRAIN) / GRAIN
    assert np.all(np.diff(u) > 0.0)
    return u


def uneven(n, p, seed, duration=4.0, ratio=50.0, shift=0.0):
    """n + p + 1 dyadic knots whose spans spread over a factor `ratio`, u[0] = shift"""
    rng = np.random.default_rng(seed)
    mean = duration / (n - p)
    h = 0.5 * math.log(ratio)
    spans = mean * np.exp(rng.uniform(-h, h, size=n + p))
    spans[rng.integers(0, n + p)] = mean * math.exp(h)  # both ends of the spread are there
    spans[rng.integers(0, n + p)] = mean * math.exp(-h)
    return dyadic(shift + np.concatenate([[0.0], np.cumsum(spans)]))


def times(u, p, n, seed, dyadic_knots):
    """below 0, 0, on every inner knot, one ulp inside the end, the end, past it, and seeded times between"""
    u = [float(v) for v in u]
    D = u[n] - u[p]
    rng = np.random.default_rng(seed)
    on = [u[k] - u[p] for k in range(p + 1, n)]
    if dyadic_knots:
        assert all(t + u[p] == u[k] for t, k in zip(on, range(p + 1, n)))
    t = [-0.3, 0.0] + on + [math.nextafter(D, 0.0), D, D + 0.5] + list(rng.uniform(0.0, D, size=5))
    return np.array(t, dtype=np.float64)


def scene(tag, degree, ctrl, u, t_now=0.0, seed=0, dyadic_knots=True):
    ctrl = np.ascontiguousarray(ctrl, dtype=np.float64).reshape(-1, 3)
    u = np.ascontiguousarray(u, dtype=np.float64)
    n = len(ctrl)
    assert len(u) == n + degree + 1 and n >= degree + 1
    return dict(tag=tag, degree=int(degree), ctrl=ctrl, u=u, t_now=float(t_now), t=times(u, degree, n, seed, dyadic_knots),
                dyadic=dyadic_knots, map=MAP, step=tr.STEP, max_radius=tr.MAX_RADIUS)


_SCENES = []


def scenes():
    if _SCENES:
        return _SCENES
    out = []
    seed = 100
    # one span: n_ctrl = degree + 1, degrees 3, 4, 5
    for p in (3, 4, 5):
        seed += 1
        out.append(scene("one_span_p%d" % p, p, flight(p + 1, seed, x0=0.4, span=0.6), uneven(p + 1, p, seed, 2.0, 8.0), seed=seed))
    # the lane-strided copy across wave widths: n + p + 1 = 63, 64, 65, 129 knots
    for n in (59, 60, 61, 125):
        seed += 1
        out.append(scene("lanes_%d" % (n + 4), 3, flight(n, seed), uneven(n, 3, seed, 5.0, 20.0), seed=seed))
    # a shifted vector: u[p] != 0 on either side
    out.append(scene("shift_plus", 3, flight(10, 120), uneven(10, 3, 120, 3.0, 10.0, shift=7.375), seed=120))
    out.append(scene("shift_minus", 4, flight(13, 121), uneven(13, 4, 121, 3.0, 10.0, shift=-5.125), seed=121))
    # strongly uneven spans, ratio 50; a cubic's jerk spline has degree 0 (the knot search alone)
    out.append(scene("ratio50_cubic", 3, flight(12, 122), uneven(12, 3, 122, 4.0, 50.0), seed=122))
    out.append(scene("ratio50_p4", 4, flight(20, 123), uneven(20, 4, 123, 4.0, 50.0), seed=123))
    # the largest problem of degree 5 fills its knot block: n + p + 1 = max_ctrl + 6 in a call of the degree-5 scenes
    out.append(scene("full_block_p5", 5, flight(30, 124), uneven(30, 5, 124, 5.0, 50.0, shift=0.25), seed=124))
    # t_now of the safety check: on a moved knot, below 0, past the end
    base = dict(degree=3, ctrl=flight(16, 125), u=uneven(16, 3, 125, 4.0, 30.0, shift=1.5))
    ub = base["u"]
    for name, t_now in (("on_knot", float(ub[8] - ub[3])), ("below_0", -0.25), ("past_end", float(ub[16] - ub[3]) + 1.0)):
        out.append(scene("t_now_" + name, 3, base["ctrl"], ub, t_now=t_now, seed=125))
    # real knots_out of a LENGTHEN run and of a REALLOC run (tests/traj_adjust_cases.py); not dyadic
    by_tag = {sc["tag"]: sc for sc in tac.quick_scenes()}
    for tag, ops in (("lengthen_above", ar.LENGTHEN), ("cap_binds_it3", ar.REALLOC), ("acc_i2_p5", ar.REALLOC)):
        sc = by_tag[tag]
        r = ar.adjust(sc["ctrl"], sc["degree"], sc["dt"], None, ops, sc["ratio_in"], None, **sc["cfg"])
        moved = np.array(r["knots_out"])
        assert not np.array_equal(moved, np.array(ar.knots(len(sc["ctrl"]), sc["degree"], sc["dt"]))), tag
        # the adjustment scenes fly at 2.6 m/s from (0.5, -1, 1): moved onto map a's obstacle line, the same shape
        ctrl = (sc["ctrl"] - sc["ctrl"][0]) * 0.5 + np.array([-0.9, tc.HIT_Y, tc.HIT_Z])
        out.append(scene("adjusted_" + tag, sc["degree"], ctrl, moved, seed=126, dyadic_knots=False))
    _SCENES.extend(out)
    return _SCENES


def bad_scenes():
    """knots only the device-side check can meet (the host route refuses them): a NaN, two equal neighbours"""
    sc = scenes()[7]
    u1, u2 = sc["u"].copy(), sc["u"].copy()
    u1[5] = float("nan")
    u2[9] = u2[8]
    return [dict(sc, tag="bad_nan", u=u1), dict(sc, tag="bad_equal", u=u2)]


def by_degree(scs=None):
    """the scenes in launches by degree: problems of different n_ctrl side by side, the first scene again at the end (its
    place must not matter), and as many more copies of it as make the batch no multiple of either kernel's waves per
    workgroup"""
    g = {}
    for sc in (scs if scs is not None else scenes()):
        g.setdefault(sc["degree"], []).append(sc)
    for p, grp in g.items():
        grp.append(dict(grp[0], tag=grp[0]["tag"] + "_again"))
        while len(grp) % CHECK_WAVES == 0 or len(grp) % SAMPLE_WAVES == 0:
            grp.append(dict(grp[0], tag=grp[0]["tag"] + "_again%d" % len(grp)))
    return g


def yaw_problem(sc, mode):
    """the yaw problem of a scene (the dt of the problem record is not read: the knots are the scene's)"""
    return yr.problem(sc["ctrl"], 1.0, (0.3, 0.1, 0.0), 1.2, mode=mode, degree=sc["degree"], relax_time=0.5, tag=sc["tag"])


def uniform_cases():
    """uniform splines for the tie between the two paths: (degree, ctrl, dt)"""
    return [(3, flight(4, 201, x0=0.4, span=0.6), 0.5), (3, flight(61, 202), 0.07), (3, flight(125, 203), 0.04),
            (4, flight(17, 204), 0.3), (5, flight(6, 205, x0=0.4, span=0.6), 0.45), (5, flight(30, 206), 0.13),
            (3, flight(12, 207), 0.31)]
