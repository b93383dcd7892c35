"""The three consumers of a finished trajectory on GIVEN knots (setKnot), restated on the host in f64: thin functions over
tests/traj_sample_ref.py's Spline(ctrl, p, u), tests/traj_check_ref.py and tests/yaw_plan_ref.py with the uniform spline
replaced by one on the caller's knot vector.  Where a restated loop of those modules builds its uniform knots inside, the
loop is restated here on `u`, statement for statement, and the module is left as it is.

  check()       FastPlannerManager::checkTrajCollision (plan_manage/src/planner_manager.cpp:96-118): traj_check_ref's
                check_literal with `u` in place of knots(n, p, dt).
  sample()      traj_server's cmdCallback / the FSM's replan state: traj_sample_ref's sample() with Spline(ctrl, p, u) in
                place of Spline.uniform; the yaw spline stays uniform, as the reference builds every one.
  yaw_solve()   planYawExplore / planYaw: yaw_plan_ref's front() with `u`, then its solve, cost and derivative points.
  evaluate()    getTimeSum and evaluateDeBoorT of the spline and of getDerivative applied one, two and three times: what
                tests/golden/knots/scenes.npz records from the reference's own class.

Defined where the reference is not (include/fuelmi.h): knots that are not finite and strictly increasing make the
problem a bad spline of each consumer -- the reference asks nothing of them and divides by their differences."""
import math

import numpy as np

import traj_check_ref as tr
import traj_sample_ref as ts
import yaw_plan_ref as yr


def knots_ok(u):
    u = [float(v) for v in u]
    return all(math.isfinite(v) for v in u) and all(a < b for a, b in zip(u[:-1], u[1:]))


def uniform(n_ctrl, p, dt):
    """setUniformBspline's accumulated knots, explicitly"""
    return tr.knots(n_ctrl, p, float(dt))


def evaluate(ctrl, p, u, times):
    """(getTimeSum, [len(times)][4][3]: the spline and its first three derivative splines at every time)"""
    fam = ts.Spline(ctrl, p, u).family(3)
    return fam[0].duration(), [[s.at(float(t)) for s in fam] for t in times]


# ---- the safety check ---------------------------------------------------------------------------------------------------
def check(grid, ctrl, p, u, t_now, step=tr.STEP, max_radius=tr.MAX_RADIUS, cap=tr.CAP):
    ctrl = np.asarray(ctrl, dtype=np.float64).reshape(-1, 3)
    n = len(ctrl)
    if not knots_ok(u):
        return tr._result(tr.NONFINITE, 0, 0.0, 0, 0, 0.0, None, tr.END_NONFINITE, 0.0)
    u = [float(v) for v in u]
    assert len(u) == n + p + 1
    duration = u[n] - u[p]
    cur_pt = tr.deboor(u, p, ctrl, t_now)
    if tr.bad_point(cur_pt):
        return tr._result(tr.NONFINITE, 0, 0.0, 0, 0, t_now, None, tr.END_NONFINITE, duration)
    radius = 0.0
    fut_t = step
    k = 0
    while radius < max_radius and t_now + fut_t < duration:
        if k == cap:
            return tr._result(tr.OVER, 0, radius, cap, 0, 0.0, None, tr.END_CAP, duration)
        k += 1
        fut_pt = tr.deboor(u, p, ctrl, t_now + fut_t)
        if tr.bad_point(fut_pt):
            return tr._result(tr.NONFINITE, 0, 0.0, k, k, t_now + fut_t, None, tr.END_NONFINITE, duration)
        if grid.inflate_occupancy(fut_pt) == 1:
            return tr._result(tr.OK, 0, radius, k, k, t_now + fut_t, fut_pt, tr.END_HIT, duration)
        radius = tr._norm(fut_pt, cur_pt)
        fut_t += step
    reason = tr.END_RADIUS if not radius < max_radius else tr.END_DURATION
    return tr._result(tr.OK, 1, -1.0, k, 0, 0.0, None, reason, duration)


# ---- sampling -----------------------------------------------------------------------------------------------------------
def sample(mode, ctrl, p, u, t, yaw_ctrl=None, yaw_p=3, yaw_dt=None, t_stop=None):
    ctrl = [list(map(float, row)) for row in ctrl]
    n_t = len(t)
    zero3 = [0.0, 0.0, 0.0]
    out = dict(status=[], pos=[], vel=[], acc=[], jerk=[], yaw=[], yawdot=[], yawddot=[], duration=0.0)
    if not knots_ok(u):
        out.update(status=[ts.BADSPLINE] * n_t, yaw=[0.0] * n_t, yawdot=[0.0] * n_t, yawddot=[0.0] * n_t)
        for k in ("pos", "vel", "acc", "jerk"):
            out[k] = [list(zero3) for _ in range(n_t)]
        return out
    traj = ts.Spline(ctrl, p, u).family(3)
    ytraj = None
    if yaw_ctrl is not None and len(yaw_ctrl) > 0:
        ytraj = ts.Spline.uniform([[float(v)] for v in yaw_ctrl], yaw_p, yaw_dt).family(2)
    D = traj[0].duration()
    T = D if t_stop is None else min(float(t_stop), D)
    out["duration"] = D
    for tk in t:
        tk = float(tk)
        te, status = tk, ts.IN
        if mode == ts.COMMAND:
            if tk < T and tk >= 0.0:
                status = ts.IN
            elif tk >= T:
                status, te = ts.PAST, T
            else:
                status = ts.INVALID
        if status == ts.INVALID:
            vals = [list(zero3) for _ in range(4)]
            yv = [0.0, 0.0, 0.0]
        else:
            vals = [s.at(te) for s in traj]
            yv = [s.at(te)[0] for s in ytraj] if ytraj else [0.0, 0.0, 0.0]
            if status == ts.PAST:
                vals[1:] = [list(zero3) for _ in range(3)]
                yv[1:] = [0.0, 0.0]
        out["status"].append(status)
        for key, v in zip(("pos", "vel", "acc", "jerk"), vals):
            out[key].append(v)
        for key, v in zip(("yaw", "yawdot", "yawddot"), yv):
            out[key].append(v)
    return out


# ---- the yaw trajectory -------------------------------------------------------------------------------------------------
def yaw_front(pr, u):
    """yaw_plan_ref.front() on the knots u"""
    ctrl, p = pr["ctrl"], pr["degree"]
    n = len(ctrl)
    u = [float(v) for v in u]
    assert len(u) == n + p + 1
    duration = u[n] - u[p]
    follow = pr["mode"] == yr.FOLLOW
    out = dict(duration=duration, status=yr.OK)
    if follow:
        seg = int(math.ceil(duration / pr["dt_target"]))
        if seg > pr["max_seg"]:
            out.update(status=yr.OVER, seg_num=seg, dt_yaw=duration / seg)
            return out
    else:
        seg = pr["seg_num"]
    dt_yaw = duration / seg
    s = list(pr["start"])
    if not follow:
        while s[0] < -yr.PI:
            s[0] += 2 * yr.PI
        while s[0] > yr.PI:
            s[0] -= 2 * yr.PI
    last_yaw = s[0]
    idx, wps, diffs, norms = [], [], [], []
    if follow:
        rng_i = range(0, seg)
    elif pr["lookfwd"]:
        relax_num = int(min(pr["relax_time"] / dt_yaw, float(seg)))
        rng_i = range(1, seg - relax_num)
    else:
        rng_i = range(0)
    for i in rng_i:
        tc = i * dt_yaw
        tf = min(duration, tc + pr["forward_t"])
        pc = yr.deboor(u, p, ctrl, tc)
        pf = yr.deboor(u, p, ctrl, tf)
        x, y, z = pf[0] - pc[0], pf[1] - pc[1], pf[2] - pc[2]
        nrm = math.sqrt(x * x + y * y + z * z)
        norms.append(nrm)
        if nrm > 1e-6:
            w, ad = yr.calc_next_yaw(last_yaw, math.atan2(y, x))
            diffs.append(ad)
        else:
            w = wps[-1] if wps else last_yaw
        last_yaw = w
        wps.append(w)
        idx.append(i)
    if follow:
        du, dp, dq = yr.derivative(u, p, ctrl)
        v = yr.deboor(du, dp, dq, duration - pr["end_back"])
        e = math.atan2(v[1], v[0])
    else:
        e = pr["end"]
    e, ad = yr.calc_next_yaw(last_yaw, e)
    diffs.append(ad)
    N = seg + 3
    q = [0.0] * N
    m02, m12 = (1 / 3.0) * dt_yaw * dt_yaw, -(1 / 6.0) * dt_yaw * dt_yaw
    M = [[1.0, -dt_yaw, m02], [1.0, 0.0, m12], [1.0, dt_yaw, m02]]
    for r in range(3):
        q[r] = M[r][0] * s[0] + M[r][1] * s[1] + M[r][2] * s[2]
    for r in range(3):
        q[seg + r] = M[r][0] * e + M[r][1] * 0.0 + M[r][2] * 0.0
    pd = 0.0
    for i in range(N - 1):
        pd += abs(q[i + 1] - q[i])
    pd /= float(N)
    out.update(seg_num=seg, dt_yaw=dt_yaw, start=s, waypts=wps, idx=idx, end_yaw=e, q0=q, pt_dist=pd,
               end_n=3 if follow else 2, degree_yaw=p if follow else 3,
               margins=(min(abs(a - yr.PI) for a in diffs), norms))
    return out


def yaw_solve(pr, u, form="dense"):
    """yaw_plan_ref.solve() behind yaw_front(); bad knots: DEGENERATE with every output 0"""
    if not knots_ok(u):
        return dict(status=yr.DEGENERATE, duration=0.0, seg_num=0, dt_yaw=0.0, n_waypt=0, waypts=[], end_yaw=0.0, cost=0.0,
                    yaw_ctrl=np.zeros(0), bad_knots=True)
    f = yaw_front(pr, u)
    if f["status"] == yr.OVER:
        return f
    w = pr["weights"]
    pd = f["pt_dist"]
    q = None
    if pd != 0.0 and math.isfinite(pd):
        q = yr.solve_banded(f, w) if form == "banded" else yr.solve_dense(f, w)
    if q is None or not np.all(np.isfinite(q)):
        f.update(status=yr.DEGENERATE, yaw_ctrl=np.array(f["q0"]), cost=0.0)
    else:
        f.update(yaw_ctrl=np.asarray(q), cost=yr.cost(f, w, q))
    f["yawdot_ctrl"], f["yawddot_ctrl"] = yr.derivative_ctrl(f["yaw_ctrl"], f["degree_yaw"], f["dt_yaw"])
    f["n_waypt"] = len(f["waypts"])
    return f


def yaw_parity_ok(pr, u):
    """yaw_plan_ref.parity_ok on the knots u: one ulp of atan2 flips no branch"""
    f = yaw_front(pr, u)
    near_pi, norms = f["margins"]
    return near_pi > 1e-6 and all(nm > 1e-5 or nm < 1e-7 for nm in norms)


def yaw_tolerance(cases):
    """yaw_plan_ref.tolerance_for's recipe over cases = [(problem, knots)]: (measured, 100 x measured) per quantity; the
    larger of the dense-versus-banded disagreement and the change of the dense solution when every way-point moves by 6
    ulp of max(pi, |w|), the bound of the device's atan2.  Nothing is taken from the code under test.  (The inputs of
    atan2 are bit-equal; what follows it -- way-points, the solve, the cost -- cannot be, as in tests/test_yaw_plan_gpu.py.)"""
    worst = {"waypts": 0.0, "yaw_ctrl": 0.0, "cost": 0.0}
    rng = np.random.default_rng(2024)
    for pr, u in cases:
        a, b = yaw_solve(pr, u, "dense"), yaw_solve(pr, u, "banded")
        worst["yaw_ctrl"] = max(worst["yaw_ctrl"], float(np.abs(a["yaw_ctrl"] - b["yaw_ctrl"]).max()))
        worst["cost"] = max(worst["cost"], abs(a["cost"] - b["cost"]))
        w2 = yr._perturbed(a, rng)
        q2 = yr.solve_dense(a, pr["weights"], w2)
        if w2:
            worst["waypts"] = max(worst["waypts"], max(abs(x - y) for x, y in zip(w2, a["waypts"])))
        worst["yaw_ctrl"] = max(worst["yaw_ctrl"], float(np.abs(q2 - a["yaw_ctrl"]).max()))
        worst["cost"] = max(worst["cost"], abs(yr.cost(a, pr["weights"], q2, w2) - a["cost"]))
    return worst, {k: 100.0 * v for k, v in worst.items()}
