"""FastPlannerManager::planYawExplore (plan_manage/src/planner_manager.cpp:774-865) and ::planYaw (:695-772) restated
on the host in f64: the knots of setUniformBspline (bspline/src/non_uniform_bspline.cpp:25-31, accumulated), the literal
evaluateDeBoor (:51-71) and getDerivative (:77-106), calcNextYaw (:867-885), the look-ahead way-points, states2pts,
optimize()'s pt_dist_ (bspline_opt/src/bspline_optimizer.cpp:136-140) and the objective SMOOTHNESS | START | END |
WAYPOINTS of order 3 in one dimension (:255-282, 355-457, 571-630).

That objective is a convex quadratic, a sum of c (a . q - b)^2 over linear forms a of at most four neighbouring control
points.  Two formulations of its minimiser stand side by side:

  dense   the reference's form: every cost term contributes c a a^T to a dense N x N Hessian and c b a to the right-hand
          side, solved by numpy.linalg.solve (partial-pivot LU).
  banded  what the device computes: each row gathers its four diagonals (half-bandwidth 3) and its right-hand side, a
          banded Cholesky factorisation, two substitutions.

The reference itself hands the objective to NLopt for at most 2000 evaluations (algorithm.xml:185): its iterate is not
restated, the minimiser it moves towards is.  Everything before the solve is shared and literal.  When the first
way-point stalls the reference reads waypts.back() of an empty vector; this project defines that way-point as last_yaw.
planner_manager.cpp is not part of oracle/_ref, so calcNextYaw and the way-point loop are pinned by reading, by the
exact-pi and +-2 pi edge cases, and the spline evaluation by the real NonUniformBspline (tests/test_yaw_plan_cpu.py).
"""
import math

import numpy as np

EXPLORE, FOLLOW = 0, 1
OK, DEGENERATE, OVER = 0, 1, -1
WEIGHTS = dict(ld_smooth=20.0, ld_start=100.0, ld_end=0.5, ld_waypt=0.3)  # exploration_manager/launch/algorithm.xml
PI = math.pi  # M_PI


def knots(n_ctrl, p, dt):
    """setUniformBspline: u[i] = double(i - p) * dt for i <= p, then u[i] = u[i-1] + dt; m + 1 = n_ctrl + p + 1 knots"""
    u = []
    for i in range(n_ctrl + p + 1):
        u.append(float(i - p) * dt if i <= p else u[i - 1] + dt)
    return u


def deboor(u, p, ctrl, t):
    """evaluateDeBoorT(t) of the spline (ctrl [n][3], degree p, knots u)"""
    n = len(ctrl)
    v = t + u[p]
    ub = min(max(u[p], v), u[n])
    k = p
    while u[k + 1] < ub:
        k += 1
    d = [[float(c) for c in ctrl[k - p + i]] for i in range(p + 1)]
    for r in range(1, p + 1):
        for i in range(p, r - 1, -1):
            alpha = (ub - u[i + k - p]) / (u[i + 1 + k - r] - u[i + k - p])
            d[i] = [(1 - alpha) * d[i - 1][c] + alpha * d[i][c] for c in range(3)]
    return d[p]


def derivative(u, p, ctrl):
    """getDerivative: control points p (P[i+1] - P[i]) / (u[i+p+1] - u[i+1]), knots u[1 .. m-1], degree p - 1"""
    q = []
    for i in range(len(ctrl) - 1):
        den = u[i + p + 1] - u[i + 1]
        q.append([float(p) * (float(ctrl[i + 1][c]) - float(ctrl[i][c])) / den for c in range(3)])
    return u[1:-1], p - 1, q


def calc_next_yaw(last_yaw, yaw):
    """calcNextYaw; also returns |diff| for the parity condition"""
    round_last = last_yaw
    while round_last < -PI:
        round_last += 2 * PI
    while round_last > PI:
        round_last -= 2 * PI
    diff = yaw - round_last
    if abs(diff) <= PI:
        yaw = last_yaw + diff
    elif diff > PI:
        yaw = last_yaw + diff - 2 * PI
    elif diff < -PI:
        yaw = last_yaw + diff + 2 * PI
    return yaw, abs(diff)


def problem(ctrl, dt, start, end=0.0, mode=EXPLORE, degree=3, seg_num=12, lookfwd=True, relax_time=1.0, forward_t=2.0,
            dt_target=0.3, end_back=0.1, max_seg=None, weights=None, tag=""):
    return dict(ctrl=np.ascontiguousarray(ctrl, dtype=np.float64).reshape(-1, 3), dt=float(dt),
                start=[float(s) for s in start], end=float(end), mode=mode, degree=degree, seg_num=seg_num,
                lookfwd=lookfwd, relax_time=float(relax_time), forward_t=float(forward_t), dt_target=float(dt_target),
                end_back=float(end_back), max_seg=max_seg if max_seg is not None else (seg_num if mode == EXPLORE else 256),
                weights=dict(WEIGHTS, **(weights or {})), tag=tag)


def front(pr):
    """everything before the solve: duration, seg_num, dt_yaw, way-points, end yaw, initial control points, pt_dist.
    margins: (smallest | |diff| - pi | of a calcNextYaw call, the pd norms) for the parity condition"""
    ctrl, p, dt = pr["ctrl"], pr["degree"], pr["dt"]
    n = len(ctrl)
    u = knots(n, p, dt)
    duration = u[n] - u[p]
    follow = pr["mode"] == FOLLOW
    out = dict(duration=duration, status=OK)
    if follow:
        seg = int(math.ceil(duration / pr["dt_target"]))
        if seg > pr["max_seg"]:
            out.update(status=OVER, seg_num=seg, dt_yaw=duration / seg)
            return out
    else:
        seg = pr["seg_num"]
    dt_yaw = duration / seg
    s = list(pr["start"])
    if not follow:
        while s[0] < -PI:
            s[0] += 2 * PI
        while s[0] > PI:
            s[0] -= 2 * PI
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
        pc = deboor(u, p, ctrl, tc)
        pf = deboor(u, p, ctrl, tf)
        x, y, z = pf[0] - pc[0], pf[1] - pc[1], pf[2] - pc[2]
        nrm = math.sqrt(x * x + y * y + z * z)
        norms.append(nrm)
        if nrm > 1e-6:
            w, ad = calc_next_yaw(last_yaw, math.atan2(y, x))
            diffs.append(ad)
        else:
            w = wps[-1] if wps else last_yaw  # the reference: waypts.back(), undefined for the first one
        last_yaw = w
        wps.append(w)
        idx.append(i)
    if follow:
        du, dp, dq = derivative(u, p, ctrl)
        v = deboor(du, dp, dq, duration - pr["end_back"])
        e = math.atan2(v[1], v[0])
    else:
        e = pr["end"]
    e, ad = calc_next_yaw(last_yaw, e)
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
               margins=(min(abs(a - PI) for a in diffs), norms))
    return out


_J = (-1.0, 3.0, -3.0, 1.0)
_P = (1.0 / 6.0, 4.0 / 6.0, 1.0 / 6.0)


def _terms(f, w):
    """the cost terms as (weight c, first index, coefficients a, target b)"""
    N, dt, pd = f["seg_num"] + 3, f["dt_yaw"], f["pt_dist"]
    V = (-1.0 / (2 * dt), 0.0 / (2 * dt), 1.0 / (2 * dt))
    A = (1.0 / (dt * dt), -2.0 / (dt * dt), 1.0 / (dt * dt))
    s, e = f["start"], f["end_yaw"]
    T = [(w["ld_smooth"], i, tuple(j / pd for j in _J), 0.0) for i in range(N - 3)]
    T += [(10.0 * w["ld_start"], 0, _P, s[0]), (w["ld_start"], 0, V, s[1]), (w["ld_start"], 0, A, s[2])]
    T += [(w["ld_end"], N - 3, _P, e), (w["ld_end"], N - 3, V, 0.0)]
    if f["end_n"] == 3:
        T.append((w["ld_end"], N - 3, A, 0.0))
    T += [(w["ld_waypt"], i, _P, wp) for i, wp in zip(f["idx"], f["waypts"])]
    return T


def hessian_dense(f, w, waypts=None):
    """(H, g) of the normal equations from the cost terms, dense"""
    if waypts is not None:
        f = dict(f, waypts=list(waypts))
    N = f["seg_num"] + 3
    H, g = np.zeros((N, N)), np.zeros(N)
    for c, i0, a, b in _terms(f, w):
        a = np.asarray(a)
        k = len(a)
        H[i0:i0 + k, i0:i0 + k] += c * np.outer(a, a)
        g[i0:i0 + k] += c * b * a
    return H, g


def solve_dense(f, w, waypts=None):
    H, g = hessian_dense(f, w, waypts)
    return np.linalg.solve(H, g)


def solve_banded(f, w):
    """the device's order: rows gathered, banded Cholesky (half-bandwidth 3), two substitutions; None: a bad pivot"""
    N, dt, pd = f["seg_num"] + 3, f["dt_yaw"], f["pt_dist"]
    idx, wps = f["idx"], f["waypts"]
    i0, nw = (idx[0], len(idx)) if idx else (0, 0)
    cs, cp, cv, ce, cw = w["ld_smooth"], 10.0 * w["ld_start"], w["ld_start"], w["ld_end"], w["ld_waypt"]
    s, e, end3 = f["start"], f["end_yaw"], f["end_n"] == 3
    Pk = lambda k: 4.0 / 6.0 if k == 1 else 1.0 / 6.0  # noqa: E731
    Vk = lambda k: (-1.0 if k == 0 else 0.0 if k == 1 else 1.0) / (2 * dt)  # noqa: E731
    Ak = lambda k: (-2.0 if k == 1 else 1.0) / (dt * dt)  # noqa: E731
    band = [[0.0] * 4 for _ in range(N)]
    g = [0.0] * N
    for r in range(N):
        for d in range(4):
            c = r - d
            if c < 0:
                continue
            sj = 0.0
            for i in range(max(0, r - 3), min(c, N - 4) + 1):
                sj += (_J[r - i] / pd) * (_J[c - i] / pd)
            hd = cs * sj
            if r <= 2:
                hd += cp * (Pk(r) * Pk(c)) + cv * (Vk(r) * Vk(c)) + cv * (Ak(r) * Ak(c))
            if c >= N - 3:
                rr, cc = r - (N - 3), c - (N - 3)
                t = Pk(rr) * Pk(cc) + Vk(rr) * Vk(cc)
                if end3:
                    t += Ak(rr) * Ak(cc)
                hd += ce * t
            sw = 0.0
            for i in range(max(i0, r - 2), min(c, i0 + nw - 1) + 1):
                sw += Pk(r - i) * Pk(c - i)
            hd += cw * sw
            band[r][d] = hd
        gr = 0.0
        if r <= 2:
            gr += cp * (s[0] * Pk(r)) + cv * (s[1] * Vk(r)) + cv * (s[2] * Ak(r))
        if r >= N - 3:
            gr += ce * (e * Pk(r - (N - 3)))
        sw = 0.0
        for i in range(max(i0, r - 2), min(r, i0 + nw - 1) + 1):
            sw += wps[i - i0] * Pk(r - i)
        gr += cw * sw
        g[r] = gr
    hb = 3
    for j in range(N):
        sj = band[j][0]
        for d in range(1, min(hb, j) + 1):
            sj -= band[j][d] * band[j][d]
        if not (sj > 0.0) or not math.isfinite(sj):
            return None
        ljj = math.sqrt(sj)
        band[j][0] = ljj
        for i in range(j + 1, min(j + hb, N - 1) + 1):
            t = band[i][i - j]
            for k in range(max(0, i - hb), j):
                t -= band[i][i - k] * band[j][j - k]
            band[i][i - j] = t / ljj
    for j in range(N):
        sj = g[j]
        for d in range(1, min(hb, j) + 1):
            sj -= band[j][d] * g[j - d]
        g[j] = sj / band[j][0]
    for j in range(N - 1, -1, -1):
        sj = g[j]
        for d in range(1, hb + 1):
            if j + d < N:
                sj -= band[j + d][d] * g[j + d]
        g[j] = sj / band[j][0]
    return np.array(g)


def cost(f, w, q, waypts=None):
    """combineCost's value at q, the reference's order of operations"""
    q = [float(v) for v in q]
    N, dt, pd = len(q), f["dt_yaw"], f["pt_dist"]
    wps = f["waypts"] if waypts is None else waypts
    fs = 0.0
    for i in range(N - 3):
        ji = (q[i + 3] - 3 * q[i + 2] + 3 * q[i + 1] - q[i]) / pd
        fs += ji * ji
    s = f["start"]
    f0 = 0.0
    dq = 1 / 6.0 * (q[0] + 4 * q[1] + q[2]) - s[0]
    f0 += 10.0 * (dq * dq)
    dq = 1 / (2 * dt) * (q[2] - q[0]) - s[1]
    f0 += dq * dq
    dq = 1 / (dt * dt) * (q[0] - 2 * q[1] + q[2]) - s[2]
    f0 += dq * dq
    q3, q2, q1 = q[N - 3], q[N - 2], q[N - 1]
    fe = 0.0
    dq = 1 / 6.0 * (q1 + 4 * q2 + q3) - f["end_yaw"]
    fe += dq * dq
    dq = 1 / (2 * dt) * (q1 - q3) - 0.0
    fe += dq * dq
    if f["end_n"] == 3:
        dq = 1 / (dt * dt) * (q1 - 2 * q2 + q3) - 0.0
        fe += dq * dq
    fw = 0.0
    for i, wp in zip(f["idx"], wps):
        dq = 1 / 6.0 * (q[i] + 4 * q[i + 1] + q[i + 2]) - wp
        fw += dq * dq
    c = 0.0
    c += w["ld_smooth"] * fs
    c += w["ld_start"] * f0
    c += w["ld_end"] * fe
    c += w["ld_waypt"] * fw
    return c


def derivative_ctrl(q, p, dt):
    """getDerivativeControlPoints once and twice on setUniformBspline(q, p, dt)"""
    q = [float(v) for v in q]
    u = knots(len(q), p, dt)
    d1 = [float(p) * (q[i + 1] - q[i]) / (u[i + p + 1] - u[i + 1]) for i in range(len(q) - 1)]
    u1 = u[1:-1]
    d2 = [float(p - 1) * (d1[i + 1] - d1[i]) / (u1[i + p] - u1[i + 1]) for i in range(len(d1) - 1)]
    return np.array(d1), np.array(d2)


def solve(pr, form="dense"):
    """the whole step for one problem: the C-ABI's outputs as a dict"""
    f = front(pr)
    if f["status"] == OVER:
        return f
    w = pr["weights"]
    pd = f["pt_dist"]
    q = None
    if pd != 0.0 and math.isfinite(pd):
        q = solve_banded(f, w) if form == "banded" else solve_dense(f, w)
    if q is None or not np.all(np.isfinite(q)):
        f.update(status=DEGENERATE, yaw_ctrl=np.array(f["q0"]), cost=0.0)
    else:
        f.update(yaw_ctrl=np.asarray(q), cost=cost(f, w, q))
    f["yawdot_ctrl"], f["yawddot_ctrl"] = derivative_ctrl(f["yaw_ctrl"], f["degree_yaw"], f["dt_yaw"])
    f["n_waypt"] = len(f["waypts"])
    return f


# ---- cases ----------------------------------------------------------------------------------------------------------
def curve(n_ctrl, seed, scale=1.0, turn=1.3):
    """a curved path of n_ctrl control points: a helix arc with seeded wobble, step `scale` metres"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.0, 2 * PI)
    k = np.arange(n_ctrl)
    th = a + turn * k / max(n_ctrl - 1, 1) * (1.0 if seed % 2 else -1.0)
    r = scale * n_ctrl / 2.0
    pts = np.stack([r * np.cos(th), r * np.sin(th), 1.0 + 0.05 * k], axis=1)
    return pts + rng.uniform(-0.1, 0.1, size=pts.shape) * scale


def parity_ok(pr):
    """no calcNextYaw difference within 1e-6 of pi, no pd norm within a factor 10 of 1e-6: one ulp of atan2 flips nothing"""
    f = front(pr)
    near_pi, norms = f["margins"]
    return near_pi > 1e-6 and all(nm > 1e-5 or nm < 1e-7 for nm in norms)


def parity_cases():
    """curved degree-3 splines, n_ctrl in {4, 11, 35}, durations on both sides of forward_t (tf clamped / not)"""
    spec = [  # n_ctrl, knot span, start (yaw, rate, acc), end yaw, relax_time, seed
        (4, 0.9, (0.3, 0.1, 0.0), 1.2, 0.0, 1),      # duration 0.9 < forward_t: every tf clamped
        (4, 3.5, (-2.0, 0.0, 0.2), -0.4, 1.0, 2),    # 3.5 s: tf clamped late only
        (11, 0.11, (0.5, -0.2, 0.1), 2.5, 0.2, 3),   # 0.88 s
        (11, 0.4, (3.0, 0.3, 0.0), -2.9, 1.0, 4),    # 3.2 s
        (11, 1.3, (-1.0, 0.0, 0.0), 0.7, 2.0, 5),    # 10.4 s: tf never clamped before the relax
        (35, 0.05, (1.5, 0.5, -0.3), 0.1, 0.5, 6),   # 1.6 s
        (35, 0.2, (-3.0, -0.1, 0.0), 3.1, 1.0, 7),   # 6.4 s
        (35, 0.6, (0.0, 0.2, 0.1), -1.7, 3.0, 8),    # 19.2 s
    ]
    out = []
    for n, dt, st, en, relax, seed in spec:
        out.append(problem(curve(n, seed), dt, st, en, relax_time=relax, tag="n%d_dt%g" % (n, dt)))
    return out


def follow_cases():
    """planYaw: one wave and more of way-points, position degrees 3..5"""
    return [problem(curve(11, 11), 0.35, (0.4, 0.1, 0.0), mode=FOLLOW, tag="follow_n11"),
            problem(curve(35, 12), 0.61, (-1.0, 0.0, 0.1), mode=FOLLOW, tag="follow_65"),  # 19.52 s: 66 way-points
            problem(curve(14, 13), 0.3, (2.0, 0.0, 0.0), mode=FOLLOW, degree=4, tag="follow_p4"),
            problem(curve(16, 14), 0.25, (-2.5, 0.2, 0.0), mode=FOLLOW, degree=5, tag="follow_p5")]


def edge_cases():
    """the named edge cases of the GPU tests (not all satisfy parity_ok: some sit on a branch on purpose)"""
    k = np.arange(11, dtype=np.float64)
    line_mx = np.stack([-0.5 * k, 0.0 * k, 1.0 + 0.0 * k], axis=1)
    climb = np.stack([0.0 * k + 1.0, 0.0 * k - 2.0, 0.3 * k], axis=1)
    th = 3.4 * PI * np.arange(35) / 34.0
    spiral = np.stack([3.0 * np.cos(th), 3.0 * np.sin(th), 1.0 + 0.0 * th], axis=1)
    stall_late = curve(11, 21)
    stall_late[6:] = stall_late[6]
    same = np.tile(np.array([[1.0, 2.0, 1.0]]), (11, 1))
    return {
        "spiral": problem(spiral, 0.2, (1.6, 0.0, 0.0), 1.0, relax_time=0.0),
        "start_7": problem(curve(11, 22), 0.4, (7.0, 0.1, 0.0), 0.5),
        "start_m7": problem(curve(11, 23), 0.4, (-7.0, 0.1, 0.0), 0.5),
        "end_plus": problem(line_mx, 0.4, (3.0, 0.0, 0.0), -3.0, relax_time=0.0),    # last_yaw = pi, end -3: +2 pi
        "end_minus": problem(-line_mx + [0, 0, 2], 0.4, (0.1, 0.0, 0.0), 3.5, lookfwd=False),
        "line_mx": problem(line_mx, 0.4, (0.0, 0.0, 0.0), 3.0, relax_time=0.0),
        "stall_late": problem(stall_late, 0.4, (0.2, 0.0, 0.0), 1.0, relax_time=0.0),
        "stall_all": problem(same, 0.4, (0.7, 0.1, 0.0), 1.0, relax_time=0.0),
        "climb": problem(climb, 0.4, (2.0, 0.0, 0.0), 2.5, relax_time=0.0),
        "degenerate": problem(curve(11, 24), 0.4, (0.0, 0.0, 0.0), 0.0, lookfwd=False),
    }


def _perturbed(f, rng):
    return [wv + sgn * 6.0 * 2.0 ** -52 * max(PI, abs(wv)) for wv, sgn in zip(f["waypts"], rng.choice([-1.0, 1.0], len(f["waypts"])))]


_TOL = {}


def tolerance_for(name, cases):
    """the recipe of parity_tolerance() over `cases`, cached under `name`"""
    if name not in _TOL:
        worst = {"waypts": 0.0, "yaw_ctrl": 0.0, "cost": 0.0}
        rng = np.random.default_rng(2024)
        for pr in cases:
            a, b = solve(pr, "dense"), solve(pr, "banded")
            worst["yaw_ctrl"] = max(worst["yaw_ctrl"], float(np.abs(a["yaw_ctrl"] - b["yaw_ctrl"]).max()))
            worst["cost"] = max(worst["cost"], abs(a["cost"] - b["cost"]))
            w2 = _perturbed(a, rng)
            q2 = solve_dense(a, pr["weights"], w2)
            if w2:
                worst["waypts"] = max(worst["waypts"], max(abs(x - y) for x, y in zip(w2, a["waypts"])))
            worst["yaw_ctrl"] = max(worst["yaw_ctrl"], float(np.abs(q2 - a["yaw_ctrl"]).max()))
            worst["cost"] = max(worst["cost"], abs(cost(a, pr["weights"], q2, w2) - a["cost"]))
        _TOL[name] = (worst, {k: 100.0 * v for k, v in worst.items()})
    return _TOL[name]


def parity_tolerance():
    """(measured, tolerance = 100 x measured) per quantity over parity_cases().  measured = the larger of (i) the
    dense-versus-banded disagreement and (ii) the change of the dense solution when every way-point moves by 6 ulp of
    max(pi, |w|) (the OpenCL bound of atan2 the device maths library keeps) with seeded random signs; the de Boor inputs
    of atan2 are bit-equal by construction.  Nothing is taken from the code under test."""
    return tolerance_for("explore", parity_cases())


def follow_tolerance():
    """the same recipe over follow_cases(): planYaw's problems are larger (up to 69 unknowns) and have three end entries,
    so they get a tolerance of their own instead of widening parity_tolerance()"""
    return tolerance_for("follow", follow_cases())
