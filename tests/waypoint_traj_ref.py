"""The first half of FastPlannerManager::planExploreTraj (plan_manage/src/planner_manager.cpp:266-297) restated on the
host: segment times from the way-points, PolynomialTraj::waypointsTraj (poly_traj/src/polynomial_traj.cpp:5-175),
getTotalTime, getLength, seg_num, the sample loop and the four boundary derivatives.

Two formulations of the min-jerk fit stand side by side:

  coef_dense       the reference's literal loops and dense 6S x 6S matrices: A, Ct, Q, R = C A^-T Q A^-1 Ct, the blocks of
                   R, Rpp.inverse(), A.inverse(); numpy.linalg.inv where Eigen's inverse() stands (both partial-pivot LU,
                   so close but not bit-identical) and `**` where pow stands.
  coef_structured  what the device computes: A and Q are block diagonal and A_k^-1 is known in closed form, so
                   M_k = A_k^-T Q_k A_k^-1 is an integer matrix times powers of 1 / T_k; Rpp is gathered from the M_k
                   (symmetric, order 2S - 2, half-bandwidth 3), factored by a banded Cholesky with the three axes as
                   right-hand sides, and each segment's coefficients follow from its six boundary values.

Everything around the fit (times, the two accumulated sampling loops, the segment lookup) is shared and literal.
The lookup `while (times[idx] + 1e-4 < ts) ts -= times[idx++]` clamps idx to the last segment: the reference reads
past the end of its vectors there, the clamp is this project's defined result.
"""
import math

import numpy as np

OK, FEW, DEGENERATE, OVER = 0, 1, 2, -1
MAX_SEG = 1 << 20  # cap of int(length / ctrl_pt_dist) and of a forced seg_num (include/fuelmi.h)


def seg_times(way, max_vel):
    """times[k] = |p[k+1] - p[k]| / (max_vel * 0.5), the norm summed left to right (:276-278)"""
    out = []
    for k in range(len(way) - 1):
        x = float(way[k + 1][0]) - float(way[k][0])
        y = float(way[k + 1][1]) - float(way[k][1])
        z = float(way[k + 1][2]) - float(way[k][2])
        out.append(math.sqrt(x * x + y * y + z * z) / (max_vel * 0.5))
    return out


def total_time(times):
    s = 0.0
    for t in times:
        s += t
    return s


def _factorial(x):
    fac = 1
    for i in range(x, 0, -1):
        fac = fac * i
    return fac


def coef_dense(way, vel, acc, times):
    """waypointsTraj with end velocity = end acceleration = 0 -> coef [S][3][6] (p0 + p1 t + ... + p5 t^5)"""
    pos = np.asarray(way, dtype=np.float64)
    S = len(times)
    D = np.zeros((3, 6 * S))
    for k in range(S):
        for a in range(3):
            D[a, k * 6] = pos[k, a]
            D[a, k * 6 + 1] = pos[k + 1, a]
            if k == 0:
                D[a, k * 6 + 2] = vel[a]
                D[a, k * 6 + 4] = acc[a]
            elif k == S - 1:
                D[a, k * 6 + 3] = 0.0
                D[a, k * 6 + 5] = 0.0
    A = np.zeros((6 * S, 6 * S))
    for k in range(S):
        Ab = np.zeros((6, 6))
        for i in range(3):
            Ab[2 * i, i] = _factorial(i)
            for j in range(i, 6):
                Ab[2 * i + 1, j] = _factorial(j) // _factorial(j - i) * times[k] ** (j - i)
        A[k * 6:k * 6 + 6, k * 6:k * 6 + 6] = Ab
    num_f, num_p, num_d = 2 * S + 4, 2 * S - 2, 6 * S
    Ct = np.zeros((num_d, num_f + num_p))
    Ct[0, 0] = 1
    Ct[2, 1] = 1
    Ct[4, 2] = 1
    Ct[1, 3] = 1
    Ct[3, 2 * S + 4] = 1
    Ct[5, 2 * S + 5] = 1
    Ct[6 * (S - 1) + 0, 2 * S + 0] = 1
    Ct[6 * (S - 1) + 1, 2 * S + 1] = 1
    Ct[6 * (S - 1) + 2, 4 * S + 0] = 1
    Ct[6 * (S - 1) + 3, 2 * S + 2] = 1
    Ct[6 * (S - 1) + 4, 4 * S + 1] = 1
    Ct[6 * (S - 1) + 5, 2 * S + 3] = 1
    for j in range(2, S):
        Ct[6 * (j - 1) + 0, 2 + 2 * (j - 1) + 0] = 1
        Ct[6 * (j - 1) + 1, 2 + 2 * (j - 1) + 1] = 1
        Ct[6 * (j - 1) + 2, 2 * S + 4 + 2 * (j - 2) + 0] = 1
        Ct[6 * (j - 1) + 3, 2 * S + 4 + 2 * (j - 1) + 0] = 1
        Ct[6 * (j - 1) + 4, 2 * S + 4 + 2 * (j - 2) + 1] = 1
        Ct[6 * (j - 1) + 5, 2 * S + 4 + 2 * (j - 1) + 1] = 1
    Cm = Ct.T.copy()
    D1 = [Cm @ D[a] for a in range(3)]
    Q = np.zeros((6 * S, 6 * S))
    for k in range(S):
        for i in range(3, 6):
            for j in range(3, 6):
                Q[k * 6 + i, k * 6 + j] = i * (i - 1) * (i - 2) * j * (j - 1) * (j - 2) // (i + j - 5) * \
                    times[k] ** (i + j - 5)
    Ainv = np.linalg.inv(A)
    R = Cm @ np.linalg.inv(A.T) @ Q @ Ainv @ Ct
    Rfp = R[:num_f, num_f:]
    Rpp = R[num_f:, num_f:]
    G = np.linalg.inv(Rpp) @ Rfp.T
    back = Ainv @ Ct
    coef = np.zeros((S, 3, 6))
    for a in range(3):
        D1[a][num_f:] = -G @ D1[a][:num_f]
        P = back @ D1[a]
        for k in range(S):
            coef[k, a] = P[6 * k:6 * k + 6]
    return coef


def free_system(way, vel, acc, times):
    """Rpp in band storage (band[r][d] = Rpp(r, r - d), d = 0..3) and -Rfp^T d_f [2S - 2][3], gathered from the closed
    form of M_k; unknown 2 (w - 1) is the velocity, 2 (w - 1) + 1 the acceleration of way-point w = 1 .. S - 1"""
    S = len(times)
    n = 2 * S - 2
    band = [[0.0] * 4 for _ in range(n)]
    rhs = [[0.0] * 3 for _ in range(n)]
    for w in range(1, S):
        ta, tb = times[w - 1], times[w]
        a1 = 1.0 / ta
        a2 = a1 * a1
        a3 = a2 * a1
        a4 = a3 * a1
        b1 = 1.0 / tb
        b2 = b1 * b1
        b3 = b2 * b1
        b4 = b3 * b1
        r0, r1 = 2 * (w - 1), 2 * (w - 1) + 1
        band[r0][0] = 192.0 * a3 + 192.0 * b3
        band[r1][0] = 9.0 * a1 + 9.0 * b1
        band[r1][1] = -36.0 * a2 + 36.0 * b2
        if w > 1:
            band[r0][1] = 24.0 * a2    # v_w  with a_{w-1}
            band[r0][2] = 168.0 * a3   # v_w  with v_{w-1}
            band[r1][2] = -3.0 * a1    # a_w  with a_{w-1}
            band[r1][3] = -24.0 * a2   # a_w  with v_{w-1}
        for ax in range(3):
            da = float(way[w - 1][ax]) - float(way[w][ax])
            db = float(way[w][ax]) - float(way[w + 1][ax])
            sv = 360.0 * a4 * da + 360.0 * b4 * db
            sa = -60.0 * a3 * da + 60.0 * b3 * db
            if w == 1:
                sv = sv + (168.0 * a3 * float(vel[ax]) + 24.0 * a2 * float(acc[ax]))
                sa = sa + (-24.0 * a2 * float(vel[ax]) - 3.0 * a1 * float(acc[ax]))
            rhs[r0][ax] = -sv
            rhs[r1][ax] = -sa
    return band, rhs


def band_cholesky_solve(band, rhs, hb=3):
    """in place: band holds L afterwards, rhs the solution (the loops of k_bspline_fit at half-bandwidth 3)"""
    n = len(band)
    for j in range(n):
        s = band[j][0]
        for d in range(1, min(hb, j) + 1):
            s -= band[j][d] * band[j][d]
        ljj = math.sqrt(s)
        band[j][0] = ljj
        for i in range(j + 1, min(j + hb, n - 1) + 1):
            t = band[i][i - j]
            for k in range(max(0, i - hb), j):
                t -= band[i][i - k] * band[j][j - k]
            band[i][i - j] = t / ljj
    for ax in range(3):
        for j in range(n):
            s = rhs[j][ax]
            for d in range(1, min(hb, j) + 1):
                s -= band[j][d] * rhs[j - d][ax]
            rhs[j][ax] = s / band[j][0]
        for j in range(n - 1, -1, -1):
            s = rhs[j][ax]
            for d in range(1, hb + 1):
                if j + d < n:
                    s -= band[j + d][d] * rhs[j + d][ax]
            rhs[j][ax] = s / band[j][0]


def segment_coef(p0, p1, v0, v1, a0, a1, T):
    """p = A^-1 d of one segment and one axis, A^-1 in closed form"""
    i1 = 1.0 / T
    i2 = i1 * i1
    i3 = i2 * i1
    i4 = i3 * i1
    i5 = i4 * i1
    d = p1 - p0
    return [p0, v0, 0.5 * a0,
            (10.0 * d) * i3 + (-6.0 * v0 - 4.0 * v1) * i2 + (-1.5 * a0 + 0.5 * a1) * i1,
            (-15.0 * d) * i4 + (8.0 * v0 + 7.0 * v1) * i3 + (1.5 * a0 - a1) * i2,
            (6.0 * d) * i5 + (-3.0 * v0 - 3.0 * v1) * i4 + (-0.5 * a0 + 0.5 * a1) * i3]


def coef_structured(way, vel, acc, times):
    S = len(times)
    band, sol = free_system(way, vel, acc, times)
    band_cholesky_solve(band, sol)
    coef = np.zeros((S, 3, 6))
    for k in range(S):
        for ax in range(3):
            v0 = float(vel[ax]) if k == 0 else sol[2 * (k - 1)][ax]
            a0 = float(acc[ax]) if k == 0 else sol[2 * (k - 1) + 1][ax]
            v1 = 0.0 if k == S - 1 else sol[2 * k][ax]
            a1 = 0.0 if k == S - 1 else sol[2 * k + 1][ax]
            coef[k, ax] = segment_coef(float(way[k][ax]), float(way[k + 1][ax]), v0, v1, a0, a1, times[k])
    return coef


def evaluate(coef, times, t, k, literal_pow=True):
    """PolynomialTraj::evaluate(t, k): the segment lookup (idx clamped to the last segment), then tv . c with
    tv[i] = i (i-1) .. (i-k+1) t^(i-k), summed from i = 0"""
    idx, ts = 0, t
    last = len(times) - 1
    while idx < last and times[idx] + 1e-4 < ts:
        ts -= times[idx]
        idx += 1
    out = [0.0, 0.0, 0.0]
    pw = 1.0
    for i in range(k, 6):
        c = 1
        for q in range(i, i - k, -1):
            c *= q
        tv = c * (ts ** (i - k) if literal_pow else pw)
        pw = pw * ts
        for a in range(3):
            out[a] += tv * coef[idx][a][i]
    return out


def get_length(coef, times, duration, literal_pow=True):
    """getLength (getSamplePoints at the accumulated eval_t, then the norms left to right) -> (length, samples)"""
    pts = []
    eval_t = 0.0
    while eval_t < duration:
        pts.append(evaluate(coef, times, eval_t, 0, literal_pow))
        eval_t += 0.01
    length = 0.0
    for i in range(1, len(pts)):
        x, y, z = pts[i][0] - pts[i - 1][0], pts[i][1] - pts[i - 1][1], pts[i][2] - pts[i - 1][2]
        length += math.sqrt(x * x + y * y + z * z)
    return length, len(pts)


def plan(way, vel, acc, max_vel, ctrl_pt_dist, min_seg=8, seg_num=0, max_samples=None, form="dense"):
    """One problem of fuelmi_map_waypoint_trajs -> dict with the call's per-problem outputs (and n_len, the number of
    length samples).  form: "dense" (the yardstick) or "structured" (the device's formulation)."""
    way = np.asarray(way, dtype=np.float64).reshape(-1, 3)
    n = len(way)
    zero = {"status": OK, "duration": 0.0, "length": 0.0, "seg_num": 0, "dt": 0.0, "n_samples": 0, "n_len": 0,
            "samples": np.zeros((0, 3)), "derivs": np.zeros((4, 3)), "seg_times": np.zeros(max(n - 1, 0)),
            "coef": np.zeros((max(n - 1, 0), 3, 6))}
    if n < 3:
        zero["status"] = FEW
        return zero
    times = seg_times(way, max_vel)
    if any((t == 0.0) or not math.isfinite(t) for t in times):
        zero["status"] = DEGENERATE
        return zero
    dense = form == "dense"
    coef = (coef_dense if dense else coef_structured)(way, vel, acc, times)
    duration = total_time(times)
    length, n_len = get_length(coef, times, duration, dense)
    if seg_num > 0:
        sn = int(seg_num)
    else:
        sn = max(int(min_seg), int(min(length / ctrl_pt_dist, float(MAX_SEG))))
    dt = duration / float(sn)
    samples = []
    ts = 0.0
    while ts <= duration + 1e-4 and len(samples) < MAX_SEG + 2:
        samples.append(evaluate(coef, times, ts, 0, dense))
        ts += dt
    derivs = [evaluate(coef, times, 0.0, 1, dense), evaluate(coef, times, duration, 1, dense),
              evaluate(coef, times, 0.0, 2, dense), evaluate(coef, times, duration, 2, dense)]
    status = OK
    count = len(samples)
    if max_samples is not None and count > max_samples:
        status = OVER
        samples = samples[:max_samples]
    return {"status": status, "duration": duration, "length": length, "seg_num": sn, "dt": dt, "n_samples": count,
            "n_len": n_len, "samples": np.array(samples).reshape(-1, 3), "derivs": np.array(derivs),
            "seg_times": np.array(times), "coef": coef}


def joint_residuals(way, vel, acc, times, coef):
    """The invariants of the fit, each as a residual relative to the scale of what it compares:
    pos: every segment starts and ends on its way-points; vel, acc: continuous at every joint; start: the start
    velocity / acceleration are the inputs; end: the end ones are 0.  The scale of a derivative of order k at a joint
    is max(L / T^k) over the two segments that meet there (L their way-point distance, T their time), floored by the
    input it is compared with."""
    way = np.asarray(way, dtype=np.float64)
    S = len(times)

    def ev(k, t, d):
        out = []
        for a in range(3):
            s, pw = 0.0, 1.0
            for i in range(d, 6):
                c = 1
                for q in range(i, i - d, -1):
                    c *= q
                s += c * pw * coef[k][a][i]
                pw *= t
            out.append(s)
        return np.array(out)

    L = [float(np.linalg.norm(way[k + 1] - way[k])) for k in range(S)]
    sc = lambda k, d: L[k] / times[k] ** d
    res = {"pos": 0.0, "vel": 0.0, "acc": 0.0, "start": 0.0, "end": 0.0}
    for k in range(S):
        pscale = L[k]
        res["pos"] = max(res["pos"], float(np.abs(ev(k, 0.0, 0) - way[k]).max()) / pscale,
                         float(np.abs(ev(k, times[k], 0) - way[k + 1]).max()) / pscale)
        if k + 1 < S:
            for d, name in ((1, "vel"), (2, "acc")):
                s = max(sc(k, d), sc(k + 1, d))
                res[name] = max(res[name], float(np.abs(ev(k, times[k], d) - ev(k + 1, 0.0, d)).max()) / s)
    v = np.asarray(vel, dtype=np.float64)
    a = np.asarray(acc, dtype=np.float64)
    res["start"] = max(float(np.abs(ev(0, 0.0, 1) - v).max()) / max(sc(0, 1), float(np.abs(v).max())),
                       float(np.abs(ev(0, 0.0, 2) - a).max()) / max(sc(0, 2), float(np.abs(a).max())))
    res["end"] = max(float(np.abs(ev(S - 1, times[S - 1], 1)).max()) / sc(S - 1, 1),
                     float(np.abs(ev(S - 1, times[S - 1], 2)).max()) / sc(S - 1, 2))
    return res


# ---- the scenes the CPU and the GPU tests share --------------------------------------------------------------------
MAX_WAY = 256  # FUELMI_WPTRAJ_MAX_WAY
DEFAULTS = dict(max_vel=2.0, ctrl_pt_dist=0.45, min_seg=8)


def tour(seed, n, lo, hi):
    """n way-points, consecutive ones between lo and hi metres apart, directions uniform on the sphere"""
    rng = np.random.default_rng(seed)
    pts = [rng.uniform(-2.0, 2.0, size=3)]
    for _ in range(n - 1):
        d = rng.normal(size=3)
        pts.append(pts[-1] + d / np.linalg.norm(d) * rng.uniform(lo, hi))
    return np.array(pts)


def problem(seed, n, lo, hi, still=False, **cfg):
    rng = np.random.default_rng(1000 + seed)
    vel = np.zeros(3) if still else rng.normal(scale=0.7, size=3)
    acc = np.zeros(3) if still else rng.normal(scale=0.5, size=3)
    return dict(way=tour(seed, n, lo, hi), vel=vel, acc=acc, cfg=dict(DEFAULTS, **cfg))


def parity_cases():
    """tours whose shortest segment takes >= 0.2 s (0.2 m at max_vel 2): compared with the dense formulation.  Sizes
    3 (one interior way-point), 4, 5, the manager's usual handful, one per lane of a wave and one more, the cap."""
    out = [problem(s, n, 0.25, 2.0) for s, n in enumerate((3, 4, 5, 8, 13, 16, 33, 64, 65))]
    out.append(problem(20, 3, 0.3, 0.6, still=True))
    out.append(problem(21, 6, 0.5, 3.0, max_vel=1.0, ctrl_pt_dist=0.3))
    out.append(problem(22, 7, 0.5, 1.5, max_vel=3.0, ctrl_pt_dist=0.7, min_seg=12))
    out.append(problem(23, MAX_WAY, 0.21, 0.4))
    return out


def short_cases():
    """a segment as short as shortenPath's end_eps = 1e-3 m can leave (first, middle, last), and 1e-2 m: checked by
    the invariants of the fit, not against the dense inverses"""
    out = []
    for s, (n, at, eps) in enumerate(((5, 0, 1e-3), (6, 2, 1e-3), (5, 3, 1e-3), (9, 4, 1e-2), (4, 1, 1.5e-3))):
        p = problem(40 + s, n, 0.4, 2.0)
        w = p["way"]
        d = w[at + 1] - w[at]
        shift = d - d / np.linalg.norm(d) * eps
        w[at + 1:] -= shift
        out.append(p)
    return out


def zero_cases():
    """a zero-length segment first, in the middle and last"""
    out = []
    for s, at in enumerate((0, 2, 4)):
        p = problem(60 + s, 6, 0.4, 2.0)
        w = p["way"]
        w[at + 1:] -= w[at + 1] - w[at]
        assert np.array_equal(w[at], w[at + 1])
        out.append(p)
    return out


def mixed_batch(n):
    """n problems of 2 .. 40 way-points, some at rest, some with a zero-length segment"""
    rng = np.random.default_rng(77)
    probs = []
    for i in range(n):
        k = int(rng.integers(2, 41))
        p = problem(200 + i, k, 0.25, 1.5, still=(i % 7 == 0))
        if i % 23 == 5 and k > 3:
            p["way"][2] = p["way"][1]
        probs.append(p)
    return probs


def solve(p, form="dense", **kw):
    cfg = dict(p["cfg"], **kw)
    return plan(p["way"], p["vel"], p["acc"], form=form, **cfg)


def disagreement(a, b):
    """how far two results of one problem are apart: coefficients as c_i T^i (metres), samples (metres), derivatives
    (m/s and m/s^2 taken together) and length (metres)"""
    T = a["seg_times"]
    pw = np.array([[T[k] ** i for i in range(6)] for k in range(len(T))])[:, None, :]
    return {"coef": float(np.abs((a["coef"] - b["coef"]) * pw).max()),
            "samples": float(np.abs(a["samples"] - b["samples"]).max()),
            "derivs": float(np.abs(a["derivs"] - b["derivs"]).max()),
            "length": abs(a["length"] - b["length"])}


_TOL = {}


def parity_tolerance():
    """100 x the largest dense-vs-structured disagreement over parity_cases() (measured, per quantity)"""
    if not _TOL:
        worst = {"coef": 0.0, "samples": 0.0, "derivs": 0.0, "length": 0.0}
        for p in parity_cases():
            d = disagreement(solve(p, "dense"), solve(p, "structured"))
            for k in worst:
                worst[k] = max(worst[k], d[k])
        _TOL["measured"] = worst
        _TOL["tol"] = {k: 100.0 * v for k, v in worst.items()}
    return _TOL["measured"], _TOL["tol"]


def residual_bound():
    """100 x the structured formulation's own largest residual of each invariant over short_cases()"""
    worst = {}
    for p in short_cases():
        r = solve(p, "structured")
        for k, v in joint_residuals(p["way"], p["vel"], p["acc"], r["seg_times"], r["coef"]).items():
            worst[k] = max(worst.get(k, 0.0), float(v))
    return worst, {k: 100.0 * v for k, v in worst.items()}
