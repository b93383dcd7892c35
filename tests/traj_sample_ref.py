"""What the reference does with a finished trajectory, restated on the host in f64 for uniform splines:

  Spline           setUniformBspline's knots (bspline/src/non_uniform_bspline.cpp:25-31, accumulated), the literal
                   evaluateDeBoor / evaluateDeBoorT (:51-75) and getDerivative (:77-106) as the class has them: a
                   derivative is a spline of its own, with stored control points Q[i] = double(p) * (P[i+1] - P[i]) /
                   (u[i+p+1] - u[i+1]), the parent's knots without the first and the last, and degree p - 1.  A degree-0
                   spline evaluates by the knot search alone.  (The device stores no derivative spline; it rebuilds the
                   points one span reads.  This form shares nothing with that shortcut.)
  sample()         COMMAND: traj_server's cmdCallback (plan_manage/src/traj_server.cpp:266-290) with traj_duration_ as
                   replanCallback leaves it (:166-172); STATE: the FSM's replan start state
                   (exploration_manager/src/fast_exploration_fsm.cpp:86-95).
  record_literal   the flight record as cmdCallback keeps it (:328-339): traj_cmd_ as a list, energy, last_time, and
                   calcPathLength (:49-56) over the whole list at the end.
  record_windowed  the same record as the device walks it: eight numbers carried from window to window (and from call to
                   call), the length added push by push.

traj_server.cpp is not part of oracle/_ref, so the mode logic and the record are pinned by reading; the evaluations are
pinned to the real NonUniformBspline (tests/test_traj_sample_cpu.py).  Defined where the reference is not
(include/fuelmi.h): PAST has jerk 0, INVALID has every output 0, no yaw spline gives yaw outputs 0, BADSPLINE.
Python floats are IEEE f64 without contraction and math.sqrt is correctly rounded, so every number here is exact to
the bit for the operations stated."""
import math

from traj_check_ref import knots

COMMAND, STATE = 0, 1
IN, PAST, INVALID, BADSPLINE = range(4)
MAX_CTRL, MAX_T, MAX_SAMPLES = 1024, 1 << 16, 1 << 21
PER_SAMPLE = ("status", "pos", "vel", "acc", "jerk", "yaw", "yawdot", "yawddot")


class Spline:
    """NonUniformBspline with the members evaluateDeBoor reads: control_points_ (rows), p_, u_, n_, m_"""

    def __init__(self, ctrl, p, u):
        self.ctrl = [[float(c) for c in row] for row in ctrl]
        self.p = int(p)
        self.u = [float(v) for v in u]
        self.n = len(self.ctrl) - 1
        self.m = self.n + self.p + 1

    @classmethod
    def uniform(cls, ctrl, p, dt):
        return cls(ctrl, p, knots(len(ctrl), p, float(dt)))  # m + 1 = rows + p knots

    def duration(self):  # getTimeSum
        return self.u[self.m - self.p] - self.u[self.p]

    def de_boor(self, uu):
        u, p = self.u, self.p
        ub = min(max(u[p], uu), u[self.m - p])  # (Python's max / min of two floats are std::max / std::min)
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

    def derivative(self):  # getDerivative: getDerivativeControlPoints, then the knots cut at both ends
        u, p = self.u, self.p
        q = []
        for i in range(len(self.ctrl) - 1):
            den = u[i + p + 1] - u[i + 1]
            q.append([float(p) * (b - a) / den for a, b in zip(self.ctrl[i], self.ctrl[i + 1])])
        return Spline(q, p - 1, u[1:-1])

    def family(self, orders):
        out = [self]
        for _ in range(orders):
            out.append(out[-1].derivative())
        return out


def spline_ok(n_ctrl, p, dt, max_ctrl=MAX_CTRL):
    return dt > 0.0 and math.isfinite(dt) and p + 1 <= n_ctrl <= max_ctrl


def sample(mode, ctrl, p, dt, t, yaw_ctrl=None, yaw_p=3, yaw_dt=None, t_stop=None):
    """Every sample of one problem: dict of status [n_t], pos / vel / acc / jerk [n_t][3], yaw / yawdot / yawddot [n_t],
    duration.  ctrl [n][3]; yaw_ctrl [ny] or None."""
    ctrl = [list(map(float, row)) for row in ctrl]
    n_t = len(t)
    zero3 = [0.0, 0.0, 0.0]
    out = dict(status=[], pos=[], vel=[], acc=[], jerk=[], yaw=[], yawdot=[], yawddot=[], duration=0.0)
    if not spline_ok(len(ctrl), p, dt):  # (a device batch alone can hold one)
        out.update(status=[BADSPLINE] * n_t, yaw=[0.0] * n_t, yawdot=[0.0] * n_t, yawddot=[0.0] * n_t)
        for k in ("pos", "vel", "acc", "jerk"):
            out[k] = [list(zero3) for _ in range(n_t)]
        return out
    traj = Spline.uniform(ctrl, p, dt).family(3)  # traj_[0], [1], [2] and [5] of bsplineCallback (:239-245)
    ytraj = None
    if yaw_ctrl is not None and len(yaw_ctrl) > 0:
        ytraj = Spline.uniform([[float(v)] for v in yaw_ctrl], yaw_p, yaw_dt).family(2)  # traj_[3], [4]; FSM's yawddot
    D = traj[0].duration()
    T = D if t_stop is None else min(float(t_stop), D)  # traj_duration_ = min(t_stop, traj_duration_)
    out["duration"] = D
    for tk in t:
        tk = float(tk)
        te, status = tk, IN
        if mode == COMMAND:
            if tk < T and tk >= 0.0:
                status = IN
            elif tk >= T:
                status, te = PAST, T
            else:
                status = INVALID
        if status == INVALID:
            vals = [list(zero3) for _ in range(4)]
            yv = [0.0, 0.0, 0.0]
        else:
            vals = [s.at(te) for s in traj]
            yv = [s.at(te)[0] for s in ytraj] if ytraj else [0.0, 0.0, 0.0]
            if status == PAST:
                vals[1:] = [list(zero3) for _ in range(3)]
                yv[1:] = [0.0, 0.0]
        out["status"].append(status)
        for key, v in zip(("pos", "vel", "acc", "jerk"), vals):
            out[key].append(v)
        for key, v in zip(("yaw", "yawdot", "yawddot"), yv):
            out[key].append(v)
    return out


def _norm(a, b):
    dx, dy, dz = a[0] - b[0], a[1] - b[1], a[2] - b[2]
    return math.sqrt(dx * dx + dy * dy + dz * dz)


def record_literal(t, s):
    """cmdCallback :328-339 over a whole tape from an empty record (t [n_t], s = sample()'s dict): the eight numbers"""
    traj_cmd, energy, last_time = [], 0.0, 0.0
    for k, tk in enumerate(t):
        if s["status"][k] != INVALID:  # (an INVALID sample touches nothing but last_time: defined, see include/fuelmi.h)
            pos, jer = s["pos"][k], s["jerk"][k]
            if len(traj_cmd) == 0:
                traj_cmd.append(pos)
            elif _norm(pos, traj_cmd[-1]) > 1e-6:
                traj_cmd.append(pos)
                dt = float(tk) - last_time
                energy += (jer[0] * jer[0] + jer[1] * jer[1] + jer[2] * jer[2]) * dt
        last_time = float(tk)
    length = 0.0  # calcPathLength
    for i in range(len(traj_cmd) - 1):
        length += _norm(traj_cmd[i + 1], traj_cmd[i])
    back = traj_cmd[-1] if traj_cmd else [0.0, 0.0, 0.0]
    return [1.0 if traj_cmd else 0.0, back[0], back[1], back[2], last_time, length, energy, float(len(traj_cmd))]


def record_windowed(flight, t, s, width=64):
    """the record as the device walks it: flight = have_last, last_pos[3], last_t, length, energy, n_cmd, carried through
    windows of `width` samples; returns the new eight numbers"""
    have, lp, last_t, length, energy, n_cmd = flight[0] != 0.0, list(flight[1:4]), flight[4], flight[5], flight[6], flight[7]
    for kb in range(0, len(t), width):
        for k in range(kb, min(kb + width, len(t))):
            if s["status"][k] != INVALID:
                pos, jer = s["pos"][k], s["jerk"][k]
                if not have:
                    have, lp, n_cmd = True, list(pos), 1.0
                else:
                    nrm = _norm(pos, lp)
                    if nrm > 1e-6:
                        lp = list(pos)
                        length = length + nrm
                        energy = energy + (jer[0] * jer[0] + jer[1] * jer[1] + jer[2] * jer[2]) * (float(t[k]) - last_t)
                        n_cmd = n_cmd + 1.0
            last_t = float(t[k])
    return [1.0 if have else 0.0, lp[0], lp[1], lp[2], last_t, length, energy, n_cmd]
