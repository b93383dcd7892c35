"""The scenes of the exact quadratic solve, shared by the restatement's own checks (test_quad_solve_cpu.py), the host build
of the kernel's text (tests/golden/check_quad_solve_host_build.py) and the device test (test_quad_solve_gpu.py).  Every
size is the smallest at which the kernel takes another path: the start and end blocks overlapping (N = 4, 5), the first
guide row at every degree (N = 2 order, 2 order + 1), the rows wrapping round the wave (N = 63, 64, 65), the cap (1024)."""
import numpy as np

import quad_solve_ref as qr

LO = np.array(qr.BOX[0]) + 0.5
HI = np.array(qr.BOX[1]) - 0.5


def curve(n, seed, dim=3):
    """n control points of a bent path inside the box, a little noise on them"""
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 1.0, n)[:, None]
    a, b = LO + (HI - LO) * rng.random(3), LO + (HI - LO) * rng.random(3)
    bend = (rng.random(3) - 0.5) * np.array([1.5, 1.5, 0.4])
    c = a + (b - a) * t + bend * np.sin(np.pi * t) + rng.normal(scale=0.02, size=(n, 3))
    c = np.clip(c, LO - 0.2, HI + 0.2)
    return c if dim == 3 else np.cumsum(rng.normal(scale=0.2, size=(n, 1)), axis=0)


def states(ctrl, seed):
    """start (position, velocity, acceleration) near the first points, end near the last"""
    rng = np.random.default_rng(1000 + seed)
    dim = ctrl.shape[1]
    st = np.stack([ctrl[:3].mean(axis=0), rng.normal(scale=0.3, size=dim), rng.normal(scale=0.2, size=dim)])
    en = np.stack([ctrl[-3:].mean(axis=0), rng.normal(scale=0.1, size=dim), rng.normal(scale=0.1, size=dim)])
    return st, en


def guide_for(ctrl, degree, seed):
    """the points of a geometric path beside the control points: one per control point order .. N - order - 1"""
    n = len(ctrl) - 2 * degree
    if n <= 0:
        return None
    rng = np.random.default_rng(2000 + seed)
    return np.clip(ctrl[degree:len(ctrl) - degree] + rng.normal(scale=0.15, size=(n, ctrl.shape[1])), LO - 0.3, HI + 0.3)


def guide_case(n, degree=3, seed=0, tag=None, **kw):
    ctrl = curve(n, seed + 7 * n)
    st, en = states(ctrl, seed + n)
    return qr.problem(ctrl, 0.3 + 0.01 * (n % 7), qr.GUIDE_PHASE | kw.pop("extra_mask", 0), st, en, kw.pop("end_n", 3),
                      guide_for(ctrl, degree, seed + n), weights=dict(bspline_degree=degree),
                      tag=tag or "n%d_d%d" % (n, degree), **kw)


def waypoint_case(n, mask, widx, seed, tag):
    ctrl = curve(n, seed)
    st, en = states(ctrl, seed)
    rng = np.random.default_rng(3000 + seed)
    wp = [(ctrl[i] + 4 * ctrl[i + 1] + ctrl[i + 2]) / 6.0 + rng.normal(scale=0.1, size=3) for i in widx]
    return qr.problem(ctrl, 0.25, mask, st, en, 3, guide_for(ctrl, 3, seed) if mask & qr.GUIDE else None, wp, widx, tag=tag)


def yaw_case(n=15, seed=5):
    """dimension 1 with the yaw objective, two end entries as planYawExplore passes them"""
    ctrl = curve(n, seed, dim=1)
    st, en = states(ctrl, seed)
    widx = list(range(1, n - 5))
    rng = np.random.default_rng(4000 + seed)
    wp = [[(ctrl[i, 0] + 4 * ctrl[i + 1, 0] + ctrl[i + 2, 0]) / 6.0 + rng.normal(scale=0.05)] for i in widx]
    return qr.problem(ctrl, 0.2, qr.YAW_MASK, st, en, 2, None, wp, widx, tag="yaw_dim1")


_CASES = {}


def _once(name, make):
    if name not in _CASES:
        _CASES[name] = make()
    return _CASES[name]


def numeric_cases():
    """the cases that have a minimiser: compared with the dense form"""
    def make():
        cs = [guide_case(4), guide_case(5), guide_case(6), guide_case(7), guide_case(8, 4), guide_case(9, 4),
              guide_case(10, 5), guide_case(11, 5), guide_case(63), guide_case(64), guide_case(65),
              guide_case(qr_cap(), tag="n_cap")]
        cs += [guide_case(12, end_n=e, seed=e, tag="end_n%d" % e) for e in (1, 2, 3)]
        cs.append(waypoint_case(10, qr.SMOOTHNESS | qr.WAYPOINTS, [0, 7, 4, 4], 11, "waypoints_edges_repeat"))
        cs.append(waypoint_case(20, qr.GUIDE_PHASE | qr.WAYPOINTS, [0, 17, 9, 9], 12, "guide_waypoints"))
        cs.append(yaw_case())
        cs.append(guide_case(14, seed=3, bounds=True, tag="bounds_inside"))
        return cs
    return _once("numeric", make)


def qr_cap():
    return 1024  # FUELMI_QUAD_MAX_CTRL


def ragged_batch():
    """problems of one configuration (GUIDE_PHASE | WAYPOINTS, degree 3, three end entries) and every size above, for one
    call"""
    def make():
        out = [guide_case(n, seed=40, extra_mask=qr.WAYPOINTS, tag="ragged_n%d" % n) for n in (65, 4, 1024, 5, 63, 6, 64, 7, 12)]
        out.insert(3, waypoint_case(20, qr.GUIDE_PHASE | qr.WAYPOINTS, [0, 17, 9, 9], 41, "ragged_waypoints"))
        return out
    return _once("ragged", make)


def degenerate_cases():
    def make():
        c = curve(12, 21)
        st, en = states(c, 21)
        flat = np.tile(np.array([[0.5, -0.25, 1.0]]), (9, 1))
        return [qr.problem(c, 0.3, qr.SMOOTHNESS, tag="smoothness_alone"),
                qr.problem(flat, 0.3, qr.GUIDE_PHASE, *states(flat, 22), 3, guide_for(flat, 3, 22), tag="all_points_equal")]
    return _once("degenerate", make)


def bounded_case():
    """a guide path beyond the shrunk box pulls the minimiser out of it: q0 comes back"""
    def make():
        c = curve(14, 31)
        st, en = states(c, 31)
        g = guide_for(c, 3, 31).copy()
        g[:, 0] += 6.0
        c[2, 1] = qr.BOX[1][1] + 0.4  # (one input point outside the shrunk box: q0 is the clamped one)
        return qr.problem(c, 0.3, qr.GUIDE_PHASE, st, en, 3, g, bounds=True, tag="bounded")
    return _once("bounded", make)


def all_cases():
    return numeric_cases() + ragged_batch() + degenerate_cases() + [bounded_case()]


# ---- the call --------------------------------------------------------------------------------------------------------
def call_args(prs, **over):
    """the arguments of SDFMap.solve_quadratic for problems of one configuration (the first one's)"""
    p0 = prs[0]
    dim, m = p0["dim"], p0["mask"]
    kw = dict(ctrl=[p["ctrl"] for p in prs], knot_span=[p["dt"] for p in prs], cost_function=m,
              start_state=np.stack([p["start"] for p in prs]), end_state=np.stack([p["end"] for p in prs]),
              end_n=p0["end_n"], guide_pts=[p["guide"][:qr.n_guide(p)] for p in prs] if m & qr.GUIDE else None,
              waypoints=[p["waypts"] for p in prs] if m & qr.WAYPOINTS else None,
              waypt_idx=[np.array(p["widx"], dtype=np.int32) for p in prs] if m & qr.WAYPOINTS else None,
              weights=dict(p0["weights"]), bounds=p0["bounds"], dim=dim)
    kw.update(over)
    return kw


def refusals():
    """(name, arguments, return code, a piece of the library's message): every refusal the host makes before a launch"""
    base = guide_case(12, seed=50, tag="refusal_base")
    wp = waypoint_case(10, qr.SMOOTHNESS | qr.WAYPOINTS, [0, 7, 4], 51, "refusal_waypoints")
    EINVAL, ELIMIT = -1, -5

    def with_ctrl(fn, p=base):
        c = p["ctrl"].copy()
        fn(c)
        return call_args([dict(p, ctrl=c)])
    out = [("mask_empty", call_args([base], cost_function=0), EINVAL, "cost_function != 0"),
           ("mask_distance", call_args([base], cost_function=qr.GUIDE_PHASE | 2), EINVAL, "cost_function"),
           ("mask_mintime", call_args([base], cost_function=qr.GUIDE_PHASE | 256), EINVAL, "cost_function"),
           ("dim_2", call_args([base], ctrl=[base["ctrl"][:, :2]], dim=2, start_state=None, end_state=None,
                               guide_pts=None), EINVAL, "dim == 1"),
           ("n_ctrl_3", call_args([dict(base, ctrl=base["ctrl"][:3])], max_ctrl=8), EINVAL, "N >= 4"),
           ("n_ctrl_degree", call_args([dict(base, ctrl=base["ctrl"][:5])], weights=dict(base["weights"], bspline_degree=5),
                                       max_ctrl=8), EINVAL, "N >= order + 1"),
           ("n_ctrl_over", call_args([base], max_ctrl=11), EINVAL, "N <= cfg->max_ctrl"),
           ("end_n_0", call_args([base], end_n=0), EINVAL, "end_n"),
           ("end_n_4", call_args([base], end_n=4), EINVAL, "end_n"),
           ("waypt_idx_low", call_args([dict(wp, widx=[0, -1, 4])]), EINVAL, "i >= 0"),
           ("waypt_idx_high", call_args([dict(wp, widx=[0, 8, 4])]), EINVAL, "i <= N - 3"),
           ("ctrl_nan", with_ctrl(lambda c: c.__setitem__((5, 1), np.nan)), EINVAL, "fin_lt(P[k]"),
           ("ctrl_inf", with_ctrl(lambda c: c.__setitem__((0, 0), np.inf)), EINVAL, "fin_lt(P[k]"),
           ("ctrl_1e7", with_ctrl(lambda c: c.__setitem__((11, 2), 1e7)), EINVAL, "fin_lt(P[k]"),
           ("start_nan", call_args([dict(base, start=base["start"] * np.nan)]), EINVAL, "start_state"),
           ("guide_1e7", call_args([dict(base, guide=base["guide"] - 1e7)]), EINVAL, "guide_pts"),
           ("waypoint_nan", call_args([dict(wp, waypts=wp["waypts"] * np.nan)]), EINVAL, "waypoints"),
           ("knot_zero", call_args([base], knot_span=[0.0]), EINVAL, "knot_span"),
           ("knot_negative", call_args([base], knot_span=[-0.3]), EINVAL, "knot_span"),
           ("knot_nan", call_args([base], knot_span=[np.nan]), EINVAL, "knot_span"),
           ("max_ctrl_over_cap", call_args([base], max_ctrl=qr_cap() + 1), ELIMIT, "exceeds 1024")]
    return out


# ---- the oracle ------------------------------------------------------------------------------------------------------
def pad3(a):
    a = np.asarray(a, dtype=np.float64)
    a = a.reshape(len(a), a.size // max(len(a), 1))
    return np.concatenate([a, np.zeros((len(a), 3 - a.shape[1]))], axis=1)


def oracle_cost_grad(om, pr, q, ptd):
    """combineCost of the oracle at q [N, dim] for a problem of the restatement -> (cost, gradient [N * dim])"""
    from oracle import fuel_oracle as fo
    w = {k: v for k, v in pr["weights"].items()}
    return fo.bspline_cost_grad(om, np.asarray(q, dtype=np.float64).reshape(-1), len(q), pr["mask"], ptd, pad3(pr["start"]),
                                pad3(pr["end"]), pr["end_n"], pr["dim"], pr["dt"],
                                guide_pts=pad3(pr["guide"]) if len(pr["guide"]) else None,
                                waypoints=pad3(pr["waypts"]) if len(pr["widx"]) else None,
                                waypt_idx=pr["widx"] if len(pr["widx"]) else None, **w)
