"""A Python restatement of fuelmi_map_local_segments (include/fuelmi.h): GlobalTrajData::getState, getTrajInfoInSphere
and getTrajInfoInDuration (plan_manage/include/plan_manage/plan_container.hpp:64-112) as paramLocalTraj / reparamLocalTraj
(plan_manage/src/planner_manager.cpp:605-634) call them, every operation in the reference's order.

The polynomial side is waypoint_traj_ref.evaluate with its literal_pow switch (True: `coeff * pow(t, n - k)` as the
reference writes it; False: the powers as repeated products, the device's form); the spline side is
traj_sample_ref.Spline (setUniformBspline's accumulated knots, getDerivative, evaluateDeBoorT with its clamp).  The fit
(parameterizeToBspline) is not restated here: the control points are compared with fuelmi_bspline_parameterize and the
oracle on the device.  Defined where the reference is not, as the header defines it: DEGENERATE, NO_LOCAL, -1.

Python floats are IEEE f64 without contraction and math.sqrt / math.floor are exact for the operations stated, so every
number of the product form is the device's to the bit."""
import math

import waypoint_traj_ref as wr
from traj_sample_ref import Spline

SPHERE, DURATION = 0, 1
OK, DEGENERATE, NO_LOCAL, MISFIT = range(4)
MAX_SEG = 1 << 20        # FUELMI_WPTRAJ_MAX_SEG
COUNT_CAP = MAX_SEG + 2  # counting stops behind the window of 64 points that passes it
WIN = 64
GLOBAL_HEAD, GLOBAL_TAIL, LOCAL = 0, 1, 2  # getState's branches


class NoLocal(Exception):
    """getState's local branch on a state without a local trajectory"""


class State:
    """GlobalTrajData with the members getState reads"""

    def __init__(self, seg_times, coef, global_duration, degree=3, local_ctrl=None, local_knot_span=0.0, local_ts=-1.0,
                 local_te=-1.0, time_change=0.0, last_time_inc=0.0):
        self.seg_times = [float(v) for v in seg_times]
        self.coef = [[[float(c) for c in ax] for ax in seg] for seg in coef]
        self.global_duration = float(global_duration)
        self.degree = int(degree)
        self.local_ctrl = None if local_ctrl is None else [[float(c) for c in row] for row in local_ctrl]
        self.local_knot_span = float(local_knot_span)
        self.local_ts, self.local_te = float(local_ts), float(local_te)
        self.time_change, self.last_time_inc = float(time_change), float(last_time_inc)
        # setLocalTraj: local_traj_[0 .. 2]
        self.family = None if self.local_ctrl is None else \
            Spline.uniform(self.local_ctrl, self.degree, self.local_knot_span).family(2)

    def as_dict(self):
        """what SDFMap.local_segments takes"""
        d = dict(seg_times=self.seg_times, coef=self.coef, global_duration=self.global_duration, local_ts=self.local_ts,
                 local_te=self.local_te, time_change=self.time_change, last_time_inc=self.last_time_inc)
        if self.local_ctrl is not None:
            d.update(local_ctrl=self.local_ctrl, local_knot_span=self.local_knot_span)
        return d

    def segment_of(self, t):
        """the index PolynomialTraj::evaluate's lookup ends on (clamped to the last segment)"""
        idx, ts = 0, t
        while idx < len(self.seg_times) - 1 and self.seg_times[idx] + 1e-4 < ts:
            ts -= self.seg_times[idx]
            idx += 1
        return idx

    def get_state(self, t, k, literal_pow=False, trace=None):
        if t >= -1e-3 and t <= self.local_ts:
            tt = t - self.time_change + self.last_time_inc
            if trace is not None:
                trace.append((GLOBAL_HEAD, self.segment_of(tt)))
            return wr.evaluate(self.coef, self.seg_times, tt, k, literal_pow)
        if t >= self.local_te and t <= self.global_duration + 1e-3:
            tt = t - self.time_change
            if trace is not None:
                trace.append((GLOBAL_TAIL, self.segment_of(tt)))
            return wr.evaluate(self.coef, self.seg_times, tt, k, literal_pow)
        if trace is not None:
            trace.append((LOCAL, -1))
        if self.family is None:
            raise NoLocal()
        return self.family[k].at(t - self.local_ts)


def _norm(a, b):
    x, y, z = a[0] - b[0], a[1] - b[1], a[2] - b[2]
    return math.sqrt(x * x + y * y + z * z)


def solve(state, mode, start_t, arg0, arg1, max_points=64, literal_pow=False, need_points=0):
    """One problem -> dict with the call's per-problem outputs (points: the rows written, at most max_points), and
    trace: (branch, segment) of every getState in the reference's order."""
    start_t, arg0, arg1 = float(start_t), float(arg0), float(arg1)
    trace = []
    r = {"status": OK, "n_steps": 0, "segment_len": 0.0, "seg_num": 0, "duration": 0.0, "dt": 0.0, "n_points": 0,
         "points": [], "derivs": [[0.0] * 3 for _ in range(4)], "n_ctrl": 0, "trace": trace}

    def gs(t, k):
        return state.get_state(t, k, literal_pow, trace)

    def no_local():
        r.update(status=NO_LOCAL, n_steps=0, segment_len=0.0, seg_num=0, duration=0.0, dt=0.0, n_points=0, points=[],
                 derivs=[[0.0] * 3 for _ in range(4)])
        return r
    try:
        if mode == SPHERE:
            radius, dist_pt = arg0, arg1
            gd = state.global_duration
            segment_len = segment_time = 0.0
            first = gs(start_t, 0)
            prev = cur = first
            n_steps = 0
            while _norm(cur, first) < radius and start_t + segment_time < gd - 1e-3:
                segment_time = min(segment_time + 0.2, gd - start_t)
                cur = gs(start_t + segment_time, 0)
                segment_len += _norm(cur, prev)
                prev = cur
                n_steps += 1
            seg_num = max(6, int(min(math.floor(segment_len / dist_pt), MAX_SEG)))
            duration = segment_time
            dt = duration / seg_num
            r.update(n_steps=n_steps, segment_len=segment_len, seg_num=seg_num)
        else:
            duration, dt = arg0, arg1
        r.update(duration=duration, dt=dt)
        if not (math.isfinite(dt) and dt > 0.0):
            r["status"] = DEGENERATE
            return r
        pts, n = [], 0
        tp = 0.0
        while tp <= duration + 1e-4:
            q = gs(start_t + tp, 0)
            if n < max_points:
                pts.append(q)
            n += 1
            tp += dt
            if n % WIN == 0 and n > COUNT_CAP:
                break
        derivs = [gs(start_t, 1), gs(start_t + duration, 1), gs(start_t, 2), gs(start_t + duration, 2)]
    except NoLocal:
        return no_local()
    if n < 2:
        r["status"] = DEGENERATE
        return r
    r.update(n_points=n, points=pts, derivs=derivs)
    if need_points and n != need_points:
        r["status"] = MISFIT
    elif n > max_points:
        r["status"] = -1
    else:
        r["n_ctrl"] = n + state.degree - 1
    return r
