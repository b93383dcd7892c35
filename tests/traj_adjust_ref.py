"""The half of the reference's NonUniformBspline (bspline/src/non_uniform_bspline.cpp) that moves knots and measures a
spline, restated on the host in f64, scalar and in the reference's order -- stages a-g of include/fuelmi.h's block on
fuelmi_map_adjust_trajs:

  Spline     the class as it is: control_points_, p_, u_ and the limits; setUniformBspline's knots (:25-31), evaluateDeBoor /
             evaluateDeBoorT (:51-75), getDerivative (:77-106, a spline of its own with stored control points and the
             parent's knots cut at both ends), checkRatio (:135-160), lengthenTime (:162-176), getTimeSum, getLength
             (:271-281), getJerk (:283-298), getMeanAndMaxVel / Acc (:300-344, with the step as a parameter),
             reallocateTime (:346-441) and checkFeasibility (:443-487).  (The device stores no derivative spline and
             walks windows of 64 samples; this form shares nothing with those shortcuts.)
  adjust()   one problem through the stages in the contract's order: the loop of planner_manager.cpp:222-230, the
             sampling half of reparamBspline (:533-543), and what is defined where the reference is not (BADSPLINE, LONG).
  select()   selectBestTraj (:476-482) with the smallest index on ties, never a jerk that is not a number, -1 for none.

The Eigen expressions are taken as the project's stand-in (compat/Eigen) evaluates them, entry by entry: int * row is
double(int) * e, row / s is e / s, norm() is sqrt(((0 + x x) + y y) + z z).  That stand-in's norm() against real Eigen's
is the project's standing caveat.  Python floats are IEEE f64 without contraction and math.sqrt is
correctly rounded, so every number here is exact to the bit for the operations stated; the ternaries below are
std::max / std::min, so a value that is not a number takes the reference's way."""
import math

from traj_check_ref import knots

LENGTHEN, REALLOC, RESAMPLE, SELECT = 1, 2, 4, 8
OK, BADSPLINE, LONG = 0, 1, 2
MAX_CTRL, MAX_SAMPLES, MAX_PROB, MAX_STEPS = 1024, 4096, 1 << 16, 1 << 16
INFO = ("status", "feasible_in", "iters", "feasible", "feasible_out", "num_vel", "num_acc", "n_samples")
METRICS = ("duration_in", "ratio", "duration_out", "length", "jerk", "mean_vel", "max_vel", "mean_acc", "max_acc", "dt_out",
           "time_inc")
NI, NM = 8, 12
DEFAULTS = dict(limit_vel=2.0, limit_acc=2.0, limit_ratio=1.1, lengthen_cap=1.01, realloc_iters=3, length_res=0.01,
                stat_step=0.01)


def smax(a, b):  # std::max
    return b if a < b else a


def smin(a, b):  # std::min
    return b if b < a else a


def _norm(v):
    s = 0.0
    for e in v:
        s += e * e
    return math.sqrt(s)


class TooLong(Exception):
    pass


class Spline:
    def __init__(self, ctrl, p, u, limit_vel=2.0, limit_acc=2.0, limit_ratio=1.1):
        self.ctrl = [[float(c) for c in row] for row in ctrl]
        self.p = int(p)
        self.u = [float(v) for v in u]
        self.n = len(self.ctrl) - 1
        self.m = self.n + self.p + 1
        self.limit_vel, self.limit_acc, self.limit_ratio = float(limit_vel), float(limit_acc), float(limit_ratio)

    def time_span(self):  # getTimeSpan
        return self.u[self.p], self.u[self.m - self.p]

    def time_sum(self):  # getTimeSum
        return self.u[self.m - self.p] - self.u[self.p]

    def de_boor(self, uu):
        u, p = self.u, self.p
        ub = smin(smax(u[p], uu), u[self.m - p])
        k = p
        while u[k + 1] < ub:
            k += 1
        d = [list(self.ctrl[k - p + i]) for i in range(p + 1)]
        for r in range(1, p + 1):
            for i in range(p, r - 1, -1):
                alpha = (ub - u[i + k - p]) / (u[i + 1 + k - r] - u[i + k - p])
                d[i] = [(1 - alpha) * a + alpha * b for a, b in zip(d[i - 1], d[i])]
        return d[p]

    def at(self, t):  # evaluateDeBoorT
        return self.de_boor(t + self.u[self.p])

    def derivative(self):  # getDerivative
        u, p = self.u, self.p
        q = []
        for i in range(len(self.ctrl) - 1):
            den = u[i + p + 1] - u[i + 1]
            q.append([float(p) * (b - a) / den for a, b in zip(self.ctrl[i], self.ctrl[i + 1])])
        return Spline(q, p - 1, u[1:-1])

    def _vel(self, i):
        P, u, p = self.ctrl, self.u, self.p
        den = u[i + p + 1] - u[i + 1]
        return [float(p) * (b - a) / den for a, b in zip(P[i], P[i + 1])]

    def _acc(self, i):
        P, u, p = self.ctrl, self.u, self.p
        d1, d2, d3 = u[i + p + 2] - u[i + 2], u[i + p + 1] - u[i + 1], u[i + p + 1] - u[i + 2]
        s = float(p * (p - 1))
        return [s * ((c - b) / d1 - (b - a) / d2) / d3 for a, b, c in zip(P[i], P[i + 1], P[i + 2])]

    @staticmethod
    def _over(v, limit):
        return abs(v[0]) > limit + 1e-4 or abs(v[1]) > limit + 1e-4 or abs(v[2]) > limit + 1e-4

    def check_ratio(self):
        rows = len(self.ctrl)
        max_vel = -1.0
        for i in range(rows - 1):
            for e in self._vel(i):
                max_vel = smax(max_vel, abs(e))
        max_acc = -1.0
        for i in range(rows - 2):
            for e in self._acc(i):
                max_acc = smax(max_acc, abs(e))
        return smax(max_vel / self.limit_vel, math.sqrt(abs(max_acc) / self.limit_acc))

    def check_feasibility(self):
        rows = len(self.ctrl)
        fea = True
        for i in range(rows - 1):
            if self._over(self._vel(i), self.limit_vel):
                fea = False
        for i in range(rows - 2):
            if self._over(self._acc(i), self.limit_acc):
                fea = False
        return fea

    def lengthen_time(self, ratio):
        u, p = self.u, self.p
        num1 = 2 * p - 1
        num2 = (len(u) - 1) - 2 * p + 1
        if num1 >= num2:
            return
        delta_t = (ratio - 1.0) * (u[num2] - u[num1])
        t_inc = delta_t / float(num2 - num1)
        for i in range(num1 + 1, num2 + 1):
            u[i] += float(i - num1) * t_inc
        for i in range(num2 + 1, len(u)):
            u[i] += delta_t

    def reallocate_time(self, log=None):
        """log: a list that receives ("vel", i) / ("acc", i) for every row found infeasible (the tests' eyes)"""
        u, p = self.u, self.p
        rows = len(self.ctrl)
        fea = True
        for i in range(rows - 1):
            vel = self._vel(i)
            if self._over(vel, self.limit_vel):
                fea = False
                if log is not None:
                    log.append(("vel", i))
                max_vel = -1.0
                for e in vel:
                    max_vel = smax(max_vel, abs(e))
                ratio = max_vel / self.limit_vel + 1e-4
                if ratio > self.limit_ratio:
                    ratio = self.limit_ratio
                time_ori = u[i + p + 1] - u[i + 1]
                time_new = ratio * time_ori
                delta_t = time_new - time_ori
                t_inc = delta_t / float(p)
                for j in range(i + 2, i + p + 2):
                    u[j] += float(j - i - 1) * t_inc
                for j in range(i + p + 2, len(u)):
                    u[j] += delta_t
        for i in range(rows - 2):
            acc = self._acc(i)
            if self._over(acc, self.limit_acc):
                fea = False
                if log is not None:
                    log.append(("acc", i))
                max_acc = -1.0
                for e in acc:
                    max_acc = smax(max_acc, abs(e))
                ratio = math.sqrt(max_acc / self.limit_acc) + 1e-4
                if ratio > self.limit_ratio:
                    ratio = self.limit_ratio
                time_ori = u[i + p + 1] - u[i + 2]
                time_new = ratio * time_ori
                delta_t = time_new - time_ori
                t_inc = delta_t / float(p - 1)
                if i == 1 or i == 2:
                    for j in range(2, 6):
                        u[j] += float(j - 1) * t_inc
                    for j in range(6, len(u)):
                        u[j] += 4.0 * t_inc
                else:
                    for j in range(i + 3, i + p + 2):
                        u[j] += float(j - i - 2) * t_inc
                    for j in range(i + p + 2, len(u)):
                        u[j] += delta_t
        return fea

    def get_length(self, res, cap=MAX_STEPS):
        length = 0.0
        dur = self.time_sum()
        p_l = self.at(0.0)
        t, steps = res, 0
        while t <= dur + 1e-4:
            steps += 1
            if steps > cap:
                raise TooLong
            p_n = self.at(t)
            length += _norm([a - b for a, b in zip(p_n, p_l)])
            p_l = p_n
            t += res
        return length, steps

    def get_jerk(self):
        jt = self.derivative().derivative().derivative()
        times, c = jt.u, jt.ctrl
        jerk = 0.0
        for i in range(len(c)):
            for j in range(len(c[i])):
                jerk += (times[i + 1] - times[i]) * c[i][j] * c[i][j]
        return jerk

    def mean_max(self, order, step, cap=MAX_STEPS):
        """getMeanAndMaxVel (order 1) / getMeanAndMaxAcc (order 2): mean, max, num"""
        d = self.derivative() if order == 1 else self.derivative().derivative()
        tm, tmp = d.time_span()
        mx, mean, num = -1.0, 0.0, 0
        t = tm
        while t <= tmp:
            if num >= cap:
                raise TooLong
            vn = _norm(d.de_boor(t))
            mean += vn
            num += 1
            if vn > mx:
                mx = vn
            t += step
        return mean / float(num), mx, num


def spline_ok(n_ctrl, p, dt, max_ctrl=MAX_CTRL):
    return dt > 0.0 and math.isfinite(dt) and p + 1 <= n_ctrl <= max_ctrl


def adjust(ctrl, p, dt=None, knots_in=None, ops=0, ratio_in=None, max_samples=None, **cfg):
    """One problem: dict of INFO and METRICS entries, knots_out [n + p + 1], samples [n_samples][3] (RESAMPLE, else [])"""
    c = dict(DEFAULTS)
    c.update(cfg)
    ctrl = [list(map(float, row)) for row in ctrl]
    n = len(ctrl)
    out = {k: 0 for k in INFO}
    out.update({k: 0.0 for k in METRICS})
    out.update(knots_out=[0.0] * (n + p + 1), samples=[])
    if knots_in is None and not spline_ok(n, p, dt):  # (a device batch alone can hold one)
        out["status"] = BADSPLINE
        return out
    u = [float(v) for v in knots_in] if knots_in is not None else knots(n, p, float(dt))
    assert len(u) == n + p + 1
    s = Spline(ctrl, p, u, c["limit_vel"], c["limit_acc"], c["limit_ratio"])
    out["duration_in"] = s.time_sum()
    out["ratio"] = s.check_ratio()
    out["feasible_in"] = int(s.check_feasibility())
    if ops & LENGTHEN:
        s.lengthen_time(smin(c["lengthen_cap"], float(ratio_in) if ratio_in is not None else out["ratio"]))
    feasible, it = s.check_feasibility(), 0
    if ops & REALLOC:
        while not feasible:
            feasible = s.reallocate_time()
            it += 1
            if it >= c["realloc_iters"]:
                break
    out["iters"], out["feasible"] = it, int(feasible)
    out["feasible_out"] = int(s.check_feasibility())
    out["knots_out"] = list(s.u)
    out["duration_out"] = duration = s.time_sum()
    out["jerk"] = s.get_jerk()
    out["dt_out"] = dts = duration / float(n - p)
    out["time_inc"] = duration - out["duration_in"]
    try:
        length, _ = s.get_length(c["length_res"])
        mean_v, max_v, num_v = s.mean_max(1, c["stat_step"])
        mean_a, max_a, num_a = s.mean_max(2, c["stat_step"])
        samples = []
        if ops & RESAMPLE:
            t = 0.0
            while t <= duration + 1e-4:
                if len(samples) >= MAX_STEPS or (max_samples is not None and len(samples) >= max_samples):
                    raise TooLong
                samples.append(s.at(t))
                t += dts
    except TooLong:
        out["status"] = LONG
        return out
    out.update(length=length, mean_vel=mean_v, max_vel=max_v, num_vel=num_v, mean_acc=mean_a, max_acc=max_a, num_acc=num_a,
               n_samples=len(samples), samples=samples)
    return out


def select(group, results, n_group):
    """best [n_group] over results (adjust() dicts) with group [n_prob]"""
    best = [-1] * n_group
    for b, (g, r) in enumerate(zip(group, results)):
        if r["status"] != OK or r["jerk"] != r["jerk"]:
            continue
        if best[g] < 0 or r["jerk"] < results[best[g]]["jerk"]:
            best[g] = b
    return best
