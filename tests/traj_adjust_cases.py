"""The scenes of the trajectory-adjustment tests (tests/test_traj_adjust_cpu.py, tests/test_traj_adjust_gpu.py, the golden
recorder and the host build): the smallest shapes at which the kernel can still go wrong.  A scene is a dict: tag,
degree, ctrl [n, 3], dt (or None) / knots (or None), ops, ratio_in (or None), cfg (the fields of the configuration that
differ from the reference's values).  Scenes with the same key() share a call."""
import math

import numpy as np

import traj_adjust_ref as ar

WIN = 64  # samples per window and knots per round of the lanes (traj_adjust.hip TA_WIN)
ALL = ar.LENGTHEN | ar.REALLOC | ar.RESAMPLE
_REF = {}
FREE_ACC = dict(limit_acc=1e3)  # scenes about the velocity pass alone
FREE_VEL = dict(limit_vel=1e3)  # ... and about the acceleration pass alone


def path(n, seed, speed=2.6, dt=0.2, amp=0.05, start=(0.5, -1.0, 1.0)):
    """a forward-moving path with noise: n control points speed * dt apart"""
    rng = np.random.default_rng(seed)
    d = np.array([1.0, 0.4, 0.1]) / np.linalg.norm([1.0, 0.4, 0.1])
    return np.array(start) + np.arange(n)[:, None] * (speed * dt) * d + rng.normal(scale=amp, size=(n, 3))


def line(n, speed, dt):
    """a straight constant-speed line along x: every velocity row is (speed, 0, 0), every acceleration row 0"""
    return np.array([1.0, 2.0, 0.5]) + np.arange(n)[:, None] * (speed * dt) * np.array([1.0, 0.0, 0.0])


def scene(tag, degree, ctrl, dt=None, knots=None, ops=ALL, ratio_in=None, **cfg):
    return dict(tag=tag, degree=degree, ctrl=np.ascontiguousarray(ctrl, dtype=np.float64), dt=None if dt is None else float(dt),
                knots=None if knots is None else np.ascontiguousarray(knots, dtype=np.float64), ops=ops, ratio_in=ratio_in,
                cfg=cfg)


def key(sc):
    return (sc["degree"], sc["ops"], sc["knots"] is not None, sc["ratio_in"] is not None, tuple(sorted(sc["cfg"].items())))


def groups(scenes):
    g = {}
    for sc in scenes:
        g.setdefault(key(sc), []).append(sc)
    return g


def restate(sc, max_samples=None):
    """adjust() of a scene, computed once"""
    k = (id(sc), max_samples)
    if k not in _REF:
        _REF[k] = (sc, ar.adjust(sc["ctrl"], sc["degree"], sc["dt"], sc["knots"], sc["ops"], sc["ratio_in"], max_samples,
                                  **sc["cfg"]))
    return _REF[k][1]


def spline_of(sc):
    """the scene's spline on its input knots, with its limits"""
    c = dict(ar.DEFAULTS)
    c.update(sc["cfg"])
    u = sc["knots"] if sc["knots"] is not None else ar.knots(len(sc["ctrl"]), sc["degree"], sc["dt"])
    return ar.Spline(sc["ctrl"], sc["degree"], u, c["limit_vel"], c["limit_acc"], c["limit_ratio"])


def violations(sc):
    """the rows checkFeasibility finds infeasible on the input knots: (velocity rows, acceleration rows)"""
    s = spline_of(sc)
    rows = len(s.ctrl)
    return ([i for i in range(rows - 1) if s._over(s._vel(i), s.limit_vel)],
            [i for i in range(rows - 2) if s._over(s._acc(i), s.limit_acc)])


def _solve_first_step(target, lo=0.5, hi=4.0):
    """x with 3.0 * x / 3.0 == target bit for bit: the first velocity row of a cubic with knot span 1 whose first two
    points are x apart (u[4] - u[1] is exactly 3)"""
    x = target
    for _ in range(64):
        v = 3.0 * x / 3.0
        if v == target:
            return x
        x = math.nextafter(x, math.inf if v < target else -math.inf)
    raise AssertionError("no such step")


def edge_line(target, n=8):
    """a cubic with knot span 1 along x: first velocity row exactly `target`, every other row 1.0"""
    x = _solve_first_step(target)
    c = np.zeros((n, 3))
    c[1:, 0] = x + np.arange(n - 1) * 1.0
    return c


def bump(n, at, height, speed=1.0, dt=0.2):
    """a constant-speed line with control point `at` lifted in z: acceleration rows at - 2 .. at leave 0"""
    c = line(n, speed, dt)
    c[at, 2] += height
    return c


def quick_scenes():
    out = []
    seed = 0
    # n_ctrl at the minimum and at lengthenTime's first moved knot (3p - 2 is still a no-op, 3p - 1 moves), all ops
    for p, sizes in ((3, (4, 7, 8)), (4, (5, 10, 11)), (5, (6, 13, 14))):
        for n in sizes:
            seed += 1
            out.append(scene("all_p%d_n%d" % (p, n), p, path(n, seed), 0.2))
    # lane edges: 63 / 64 / 65 knots, two rounds
    for n in (59, 60, 61, 124):
        seed += 1
        out.append(scene("lanes_n%d" % n, 3, path(n, seed, amp=0.03), 0.2))
    # feasible at the input: no pass runs, the knots come back as built
    out.append(scene("feasible", 3, path(12, 40, speed=0.8, amp=0.01), 0.25, ops=ar.REALLOC | ar.RESAMPLE))
    # one velocity violation on the first interval, one on the last (it moves the last knot)
    c = line(9, 1.0, 0.2)
    c[0, 0] -= 0.35
    out.append(scene("vel_first", 3, c, 0.2, **FREE_ACC))
    c = line(9, 1.0, 0.2)
    c[-1, 0] += 0.35
    out.append(scene("vel_last", 3, c, 0.2, **FREE_ACC))
    # an axis exactly at limit + 1e-4 (not infeasible), and one ulp above
    lim = 2.0 + 1e-4
    out.append(scene("vel_at_limit", 3, edge_line(lim), 1.0, ops=ar.REALLOC, **FREE_ACC))
    out.append(scene("vel_ulp_above", 3, edge_line(math.nextafter(lim, math.inf)), 1.0, ops=ar.REALLOC, **FREE_ACC))
    # a violation so large that limit_ratio binds; still infeasible after 3 passes, and with 1 pass
    out.append(scene("cap_binds_it3", 3, path(10, 50, speed=6.5), 0.2))
    out.append(scene("cap_binds_it1", 3, path(10, 50, speed=6.5), 0.2, realloc_iters=1))
    # acceleration violations at i = 0, 1, 2, 3: the branch for i == 1 || i == 2 and both neighbours
    for i in range(4):
        out.append(scene("acc_i%d" % i, 3, bump(10, i + 1, 0.12), 0.2, **FREE_VEL))
    out.append(scene("acc_i1_p4", 4, bump(12, 2, 0.12), 0.2, **FREE_VEL))
    out.append(scene("acc_i2_p5", 5, bump(14, 3, 0.12), 0.2, **FREE_VEL))
    # a velocity violation whose knot move makes a later acceleration test flip: every velocity row is 5 % over, row 5 of
    # the acceleration is 2 % over on the input knots and under once the velocity pass has stretched them
    c = line(12, 2.1, 0.2)
    c[6, 2] += 0.0408
    out.append(scene("vel_flips_acc", 3, c, 0.2, ops=ar.REALLOC))
    # LENGTHEN with a given ratio below 1, exactly 1 and above the cap
    for name, r in (("below", 0.9), ("one", 1.0), ("above", 1.5)):
        out.append(scene("lengthen_%s" % name, 3, path(11, 60), 0.2, ops=ar.LENGTHEN, ratio_in=r))
    out.append(scene("lengthen_small_n", 3, path(7, 61), 0.2, ops=ar.LENGTHEN, ratio_in=1.5))
    # LENGTHEN then REALLOC in one call (the GPU test chains two calls through knots_in against it)
    out.append(scene("chain_both", 3, path(16, 70), 0.2, ops=ar.LENGTHEN | ar.REALLOC))
    # given knots with u[p] != 0, not uniform: the absolute parameter of the mean / max walks
    u = np.array(ar.knots(14, 3, 0.2)) + 0.37
    u[6:] += 0.013 * np.arange(1, len(u) - 5) ** 1.3
    out.append(scene("given_knots_offset", 3, path(14, 80), knots=u))
    u4 = np.array(ar.knots(12, 4, 0.15)) - 1.9
    u4[5:] += 0.02 * np.arange(1, len(u4) - 4) ** 1.5
    out.append(scene("given_knots_p4", 4, path(12, 81, dt=0.15), knots=u4))
    # durations at the edges of a 64-sample window: getLength takes 62 .. 65 steps, the mean / max walks 63 .. 66 samples
    for dur in (0.625, 0.635, 0.645, 0.655):
        out.append(scene("window_%g" % dur, 3, path(8, 90, speed=1.0, dt=dur / 5), dur / 5, ops=0))
    # the last accumulated t lands inside getLength's 1e-4 margin
    out.append(scene("margin", 3, path(8, 91, speed=1.0, dt=0.14), (0.7 - 5e-5) / 5, ops=0))
    # RESAMPLE: seg_num + 1 samples, and seg_num + 2 (the step must be below the 1e-4 margin; the longest problem of the
    # call has seg_num + 2 = max_samples at the smallest stride the call accepts)
    out.append(scene("resample_plus1", 3, path(9, 92), 0.2, ops=ar.RESAMPLE))
    out.append(scene("resample_plus2", 3, path(9, 93, speed=1.0, dt=8e-5, amp=1e-6), 8e-5, ops=ar.RESAMPLE, **dict(FREE_ACC, **FREE_VEL)))
    # a LONG problem and a valid one in one workgroup (getLength at 1e-5: 120 000 steps against 30 000)
    out.append(scene("long_valid", 3, path(8, 94, speed=1.0, dt=0.06), 0.06, length_res=1e-5))
    out.append(scene("long_long", 3, path(10, 95, speed=1.0), 0.2, length_res=1e-5))
    out.append(scene("long_valid_again", 3, path(8, 94, speed=1.0, dt=0.06), 0.06, length_res=1e-5))
    # a jerk that is not a number (the second derivative overflows to infinities of one sign) beside finite ones
    c = np.zeros((8, 3))
    c[:, 0] = 1e4 * np.arange(8) ** 3
    out.append(scene("nan_jerk", 3, c, 1e-160, ops=0))
    out.append(scene("finite_jerk_a", 3, path(8, 96), 0.2, ops=0))
    out.append(scene("finite_jerk_b", 3, path(8, 97), 0.2, ops=0))
    return out


def big_scenes():
    """max_ctrl = 1024 with small neighbours (one call, stride 1024)"""
    n = ar.MAX_CTRL
    big = scene("big_n1024", 3, path(n, 901, speed=2.3, dt=0.05, amp=0.002), 0.05)
    small = scene("big_neighbour_n4", 3, path(4, 903), 0.3)
    return [big, small, dict(small, tag="big_neighbour_again")]


def all_scenes():
    return quick_scenes() + big_scenes()


def want_arrays(r, n, p, kstride, max_samples):
    """the restatement of one problem laid out as the call lays a problem out: info, metrics, knots_out, samples"""
    info = np.array([r[k] for k in ar.INFO], dtype=np.int32)
    met = np.zeros(ar.NM)
    met[:len(ar.METRICS)] = [r[k] for k in ar.METRICS]
    ko = np.zeros(kstride)
    if r["status"] != ar.BADSPLINE:
        ko[:n + p + 1] = r["knots_out"]
    smp = np.zeros((max_samples, 3))
    if r["n_samples"]:
        smp[:r["n_samples"]] = np.array(r["samples"]).reshape(-1, 3)
    return info, met, ko, smp
