"""FastPlannerManager::checkTrajCollision (plan_manage/src/planner_manager.cpp:96-118) restated on the host in f64, for a
uniform position spline: the knots of setUniformBspline (bspline/src/non_uniform_bspline.cpp:25-31, accumulated), the
literal evaluateDeBoor / evaluateDeBoorT (:51-75) and SDFMap::getInflateOccupancy(Vector3d)
(plan_env/include/plan_env/sdf_map.h:127-130 posToIndex, 163-169 isInMap, 217-226).

The step is stated twice:

  literal    the reference's loop, line by line: radius = 0, fut_t = step, while (radius < max_radius && t_now + fut_t <
             duration) { evaluate; occupied -> unsafe with distance = radius; radius = norm; fut_t += step }.
  first_hit  what the device computes: sample k = 1, 2, ... depends on k alone (its fut_t is `step` summed k times, its
             point, its occupancy, its radius r_k); the loop enters body k iff r_(k-1) < max_radius and t_now + fut_t_k <
             duration, so it ends in front of the FIRST k where that fails and the answer is the first occupied k before
             that end with distance = r_(k-1), r_0 = 0.  Evaluated a window of samples at a time with numpy (the window
             size changes nothing), every operation the literal form's in the literal form's order.

planner_manager.cpp is not part of oracle/_ref, so the loop itself is pinned by reading; the point evaluation is pinned
to the real NonUniformBspline (tests/test_traj_check_cpu.py).  Defined where the reference is not (include/fuelmi.h): a
point that is not finite or has |coordinate| >= 1e7 (the reference casts it to int), and more than CAP loop bodies.
"""
import math

import numpy as np

STEP, MAX_RADIUS = 0.02, 6.0  # planner_manager.cpp:102, 104
CAP = 1 << 20                 # FUELMI_TRAJCHK_MAX_SAMPLES
OK, NONFINITE, OVER = 0, 1, -1
END_HIT, END_RADIUS, END_DURATION, END_CAP, END_NONFINITE = range(5)
KEYS = ("status", "safe", "distance", "n_samples", "hit_index", "hit_t", "hit_pos", "end_reason", "duration")


class Grid:
    """what getInflateOccupancy reads: voxel counts, origin, resolution_inv and the inflated plane (int8, x-major)"""

    def __init__(self, nvox, origin, res_inv, infl):
        self.nvox = tuple(int(v) for v in nvox)
        self.origin = [float(v) for v in origin]
        self.res_inv = float(res_inv)
        self.infl = np.ascontiguousarray(infl, dtype=np.int8).reshape(self.nvox)

    def index(self, pt):
        """posToIndex: floor((pos - origin) * resolution_inv), as an exact Python int"""
        return [math.floor((pt[c] - self.origin[c]) * self.res_inv) for c in range(3)]

    def inflate_occupancy(self, pt):
        """getInflateOccupancy(Vector3d): -1 outside the map"""
        id_ = self.index(pt)
        if any(id_[c] < 0 or id_[c] > self.nvox[c] - 1 for c in range(3)):
            return -1
        return int(self.infl[id_[0], id_[1], id_[2]])


def knots(n_ctrl, p, dt):
    """setUniformBspline: u[i] = double(i - p) * dt for i <= p, then u[i] = u[i-1] + dt; m + 1 = n_ctrl + p + 1 knots"""
    u = []
    for i in range(n_ctrl + p + 1):
        u.append(float(i - p) * dt if i <= p else u[i - 1] + dt)
    return u


def deboor(u, p, ctrl, t):
    """evaluateDeBoorT(t) of the spline (ctrl [n][3], degree p, knots u).  std::max(a, b) is a < b ? b : a and std::min
    (a, b) is b < a ? b : a, which is what Python's max / min of two floats do, not-a-number included."""
    n = len(ctrl)
    v = t + u[p]
    ub = min(max(u[p], v), u[n])
    k = p
    while k < n - 1 and u[k + 1] < ub:  # (k < n - 1 never binds for ub <= u[n]; it keeps a not-a-number inside the arrays)
        k += 1
    d = [[float(c) for c in ctrl[k - p + i]] for i in range(p + 1)]
    with np.errstate(all="ignore"):
        for r in range(1, p + 1):
            for i in range(p, r - 1, -1):
                alpha = np.float64(ub - u[i + k - p]) / np.float64(u[i + 1 + k - r] - u[i + k - p])  # (0 / 0 is a number here)
                alpha = float(alpha)
                d[i] = [(1 - alpha) * d[i - 1][c] + alpha * d[i][c] for c in range(3)]
    return d[p]


def bad_point(pt):
    return not all(abs(c) < 1e7 for c in pt)


def _result(status, safe, distance, n_samples, hit_index, hit_t, hit_pos, end_reason, duration):
    return dict(status=status, safe=safe, distance=float(distance), n_samples=n_samples, hit_index=hit_index,
                hit_t=float(hit_t), hit_pos=[float(c) for c in (hit_pos if hit_pos is not None else (0.0, 0.0, 0.0))],
                end_reason=end_reason, duration=float(duration))


def _norm(a, b):
    dx, dy, dz = a[0] - b[0], a[1] - b[1], a[2] - b[2]
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float64(dx * dx + dy * dy + dz * dz)))


def check_literal(grid, ctrl, p, dt, t_now, step=STEP, max_radius=MAX_RADIUS, cap=CAP):
    """the reference's loop"""
    ctrl = np.asarray(ctrl, dtype=np.float64).reshape(-1, 3)
    n = len(ctrl)
    if not (dt > 0.0 and math.isfinite(dt)):  # (device batches only: the host route refuses it)
        return _result(NONFINITE, 0, 0.0, 0, 0, 0.0, None, END_NONFINITE, 0.0)
    u = knots(n, p, dt)
    duration = u[n] - u[p]                                   # local_data_.duration_ = getTimeSum()
    cur_pt = deboor(u, p, ctrl, t_now)                       # :99
    if bad_point(cur_pt):
        return _result(NONFINITE, 0, 0.0, 0, 0, t_now, None, END_NONFINITE, duration)
    radius = 0.0                                             # :100
    fut_t = step                                             # :102
    k = 0
    while radius < max_radius and t_now + fut_t < duration:  # :104
        if k == cap:
            return _result(OVER, 0, radius, cap, 0, 0.0, None, END_CAP, duration)
        k += 1
        fut_pt = deboor(u, p, ctrl, t_now + fut_t)           # :105
        if bad_point(fut_pt):
            return _result(NONFINITE, 0, 0.0, k, k, t_now + fut_t, None, END_NONFINITE, duration)
        if grid.inflate_occupancy(fut_pt) == 1:              # :107
            return _result(OK, 0, radius, k, k, t_now + fut_t, fut_pt, END_HIT, duration)  # :108 distance = radius
        radius = _norm(fut_pt, cur_pt)                       # :113
        fut_t += step                                        # :114
    reason = END_RADIUS if not radius < max_radius else END_DURATION
    return _result(OK, 1, -1.0, k, 0, 0.0, None, reason, duration)  # :117; the caller's distance stays as it was


def deboor_many(u, p, ctrl, t):
    """deboor() for an array of times: the same operations, element by element"""
    u = np.asarray(u, dtype=np.float64)
    ctrl = np.asarray(ctrl, dtype=np.float64).reshape(-1, 3)
    n = len(ctrl)
    with np.errstate(all="ignore"):
        v = t + u[p]
        ub = np.where(u[p] < v, v, u[p])
        ub = np.where(u[n] < ub, u[n], ub)
        k = np.full(len(t), p, dtype=np.int64)
        while True:
            adv = (k < n - 1) & (u[k + 1] < ub)
            if not adv.any():
                break
            k = k + adv
        d = [ctrl[k - p + i].copy() for i in range(p + 1)]
        for r in range(1, p + 1):
            for i in range(p, r - 1, -1):
                alpha = (ub - u[i + k - p]) / (u[i + 1 + k - r] - u[i + k - p])
                d[i] = (1 - alpha)[:, None] * d[i - 1] + alpha[:, None] * d[i]
    return d[p]


def inflated_many(grid, q):
    """getInflateOccupancy(q) == 1 for an array of points"""
    with np.errstate(all="ignore"):
        f = np.floor((q - np.array(grid.origin)) * grid.res_inv)
        inside = np.all((f >= 0) & (f <= np.array(grid.nvox) - 1), axis=1)
    out = np.zeros(len(q), dtype=bool)
    id_ = f[inside].astype(np.int64)
    out[inside] = grid.infl[id_[:, 0], id_[:, 1], id_[:, 2]] == 1
    return out


def sample_window(grid, u, p, ctrl, cur, t_now, step, fut_base, width):
    """samples kb .. kb + width - 1 of a walk whose first one has fut_t = fut_base: (t, points, r, bad, inflated, the next
    window's fut_base).  numpy's cumulative sum adds one element at a time, left to right: fut_t of sample j is fut_base
    plus `step` added j times, as the loop adds it."""
    acc = np.cumsum(np.concatenate([[fut_base], np.full(width, step)]))
    fut = acc[:width]
    t = t_now + fut
    q = deboor_many(u, p, ctrl, t)
    with np.errstate(all="ignore"):
        bad = ~np.all(np.abs(q) < 1e7, axis=1)
        dx, dy, dz = q[:, 0] - cur[0], q[:, 1] - cur[1], q[:, 2] - cur[2]
        r = np.sqrt(dx * dx + dy * dy + dz * dz)
    hit = ~bad & inflated_many(grid, np.where(bad[:, None], 0.0, q))
    return t, q, r, bad, hit, float(acc[width])


def check_first_hit(grid, ctrl, p, dt, t_now, step=STEP, max_radius=MAX_RADIUS, cap=CAP, width=64):
    """the first-hit form, `width` samples at a time"""
    ctrl = np.asarray(ctrl, dtype=np.float64).reshape(-1, 3)
    n = len(ctrl)
    if not (dt > 0.0 and math.isfinite(dt)):
        return _result(NONFINITE, 0, 0.0, 0, 0, 0.0, None, END_NONFINITE, 0.0)
    u = knots(n, p, dt)
    duration = u[n] - u[p]
    cur = deboor(u, p, ctrl, t_now)
    if bad_point(cur):
        return _result(NONFINITE, 0, 0.0, 0, 0, t_now, None, END_NONFINITE, duration)
    r_carry, fut_base, kb = 0.0, step, 1
    while True:
        t, q, r, bad, hit, nxt = sample_window(grid, u, p, ctrl, cur, t_now, step, fut_base, width)
        k = kb + np.arange(width)
        r_prev = np.concatenate([[r_carry], r[:-1]])
        with np.errstate(all="ignore"):
            end = ~(r_prev < max_radius) | ~(t < duration)
        over = k > cap
        event = end | over | bad | hit
        if event.any():
            j = int(np.argmax(event))
            kj, rp, tj = int(k[j]), float(r_prev[j]), float(t[j])
            if end[j]:
                return _result(OK, 1, -1.0, kj - 1, 0, 0.0, None, END_RADIUS if not rp < max_radius else END_DURATION, duration)
            if over[j]:
                return _result(OVER, 0, rp, cap, 0, 0.0, None, END_CAP, duration)
            if bad[j]:
                return _result(NONFINITE, 0, 0.0, kj, kj, tj, None, END_NONFINITE, duration)
            return _result(OK, 0, rp, kj, kj, tj, q[j], END_HIT, duration)
        r_carry, fut_base, kb = float(r[-1]), nxt, kb + width


def samples(grid, ctrl, p, dt, t_now, count, step=STEP):
    """the first `count` samples whether or not the loop reaches them, for the scenes' predicates: dict of t [count],
    pos [count, 3], r [count] (r[k-1] = r_k), inflated [count], index [count, 3] (posToIndex), and cur, duration, u"""
    ctrl = np.asarray(ctrl, dtype=np.float64).reshape(-1, 3)
    u = knots(len(ctrl), p, dt)
    cur = deboor(u, p, ctrl, t_now)
    t, q, r, bad, hit, _ = sample_window(grid, u, p, ctrl, cur, t_now, step, step, count)
    with np.errstate(all="ignore"):
        idx = np.floor((q - np.array(grid.origin)) * grid.res_inv)
    return dict(t=t, pos=q, r=r, inflated=hit, bad=bad, index=idx, cur=cur, duration=u[len(ctrl)] - u[p], u=u)
