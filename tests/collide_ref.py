"""FastPlannerManager::findCollisionRange (plan_manage/src/planner_manager.cpp:636-691) and the head of
optimizeTopoBspline (:553-577) restated on the host in f64, line by line.

The spline is tests/traj_check_ref.py's (setUniformBspline's accumulated knots, the literal evaluateDeBoor).  evaluateDeBoor
(u) takes the parameter itself where evaluateDeBoorT(t) adds u[p]; of a uniform spline u[p] = double(0) * dt = 0.0, so
traj_check_ref.deboor(t) is evaluateDeBoor(t) (asserted in collision_ranges).

The distance field is read like SDFMap::getDistance(Vector3d): the voxel of floor((p - origin) * resolution_inv), -1
outside the map.  `dist < clearance` is taken in one of three modes:
  f64    on the f64 array as it is (the reference)
  cut    on an f32 array through the cut between k and k + 1 (what the device does, fuel_amd/csrc/path_internal.h)
  f32    on an f32 array as plain numbers (what the device must NOT do; the scenes' predicates use it)

Python's float is the f64 of the reference; a division by zero goes through numpy so that it gives what IEEE gives.
Defined where the reference is not (include/fuelmi.h): NONFINITE, and -1 over max_events / max_pts / the caps."""
import math

import numpy as np

import traj_check_ref as tr

OK, NO_COLLISION, ENDS_IN_OBSTACLE, NONFINITE, OVER = 0, 1, 2, 3, -1
TICK = 0.05
CAP = 1 << 20        # FUELMI_TRAJCHK_MAX_SAMPLES
GUIDE_CAP = 65536    # FUELMI_GUIDE_MAX_PTS
G_OK, G_UNDEFINED = 0, 2  # FUELMI_TOPO_OK, FUELMI_TOPO_UNDEFINED
INT_KEYS = ("status", "n_ticks", "n_start_events", "n_end_events", "n_start_pts", "n_end_pts")
DBL_KEYS = ("t_s", "t_e", "first_start", "last_end")
G_INT_KEYS = ("status", "seg_num", "n_pts", "n_ctrl", "n_guide")


def kmax_strict(res, thresh):
    """the largest integer k >= 0 with res * sqrt(k) < thresh in f64, -1 when there is none"""
    k = max(int(math.floor((thresh / res) * (thresh / res))), 0)
    while res * math.sqrt(k + 1) < thresh:
        k += 1
    while k > 0 and not res * math.sqrt(k) < thresh:
        k -= 1
    return k if res * math.sqrt(k) < thresh else -1


def cut_strict(res, thresh):
    """field_cut(res, thresh, strict): `d32 <= cut` is `res * sqrt(k) < thresh`"""
    k = kmax_strict(res, thresh)
    return np.float32(-1.0) if k < 0 else np.float32(float(np.float32(res)) * math.sqrt(k + 0.5))


class Field:
    """origin, resolution_inv as the map holds it, and the distance array [nx, ny, nz]"""

    def __init__(self, origin, res, dist, mode="f64", res_inv=None):
        self.origin = [float(v) for v in origin]
        self.res = float(res)
        self.res_inv = 1.0 / self.res if res_inv is None else float(res_inv)
        self.mode = mode
        if mode == "f64":
            self.dist = np.ascontiguousarray(dist, dtype=np.float64)
        else:
            with np.errstate(over="ignore"):
                self.dist = np.ascontiguousarray(dist).astype(np.float32)
        self.nvox = self.dist.shape
        self._cuts = {}

    def index(self, pt):
        return [math.floor((pt[c] - self.origin[c]) * self.res_inv) for c in range(3)]

    def inside(self, pt):
        id_ = self.index(pt)
        return all(0 <= id_[c] <= self.nvox[c] - 1 for c in range(3))

    def unsafe(self, pt, clearance):
        """evaluateCoarseEDT(pt, -1.0) < clearance"""
        id_ = self.index(pt)
        if any(id_[c] < 0 or id_[c] > self.nvox[c] - 1 for c in range(3)):
            return -1.0 < clearance
        d = self.dist[id_[0], id_[1], id_[2]]
        if self.mode == "f64":
            return float(d) < clearance
        if self.mode == "f32":
            return float(d) < clearance
        if clearance not in self._cuts:
            self._cuts[clearance] = cut_strict(self.res, clearance)
        return bool(d <= self._cuts[clearance])


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _zero3():
    return [0.0, 0.0, 0.0]


def collision_ranges(field, ctrl, p, dt, clearance, max_events, max_pts, cap=CAP):
    """one problem of fuelmi_map_collision_ranges: a dict of its outputs; colli_start / colli_end / start_pts / end_pts are
    the full lists (the call holds their first max_events / max_pts rows)"""
    ctrl = np.asarray(ctrl, dtype=np.float64).reshape(-1, 3)
    n = len(ctrl)
    out = dict(status=NONFINITE, n_ticks=0, n_start_events=0, n_end_events=0, n_start_pts=0, n_end_pts=0, t_s=0.0, t_e=0.0,
               colli_start=[], colli_end=[], start_pts=[], end_pts=[], first_start=_zero3(), last_end=_zero3(), ticks=[])
    if not (dt > 0.0 and math.isfinite(dt)) or not np.isfinite(ctrl).all():
        return out
    u = tr.knots(n, p, dt)
    if not math.isfinite(u[n + p]):
        return out
    assert u[p] == 0.0
    ev = lambda t: tr.deboor(u, p, ctrl, t)  # noqa: E731  evaluateDeBoor(t)
    t_m, t_mp = u[p], u[n]                    # getTimeSpan
    last_safe = True
    t_s, t_e = -1.0, 0.0                      # (t_e: uninitialised in the reference, never read then)
    colli_start, colli_end, ticks = [], [], []
    tc = t_m
    over = False
    while tc <= t_mp + 1e-4:                  # :646
        if len(ticks) == cap:
            over = True
            break
        ptc = ev(tc)
        safe = not field.unsafe(ptc, clearance)
        ticks.append((tc, ptc, safe))
        if last_safe and not safe:
            colli_start.append(ev(tc - 0.05))
            if t_s < 0.0:
                t_s = tc - 0.05
        elif not last_safe and safe:
            colli_end.append(ptc)
            t_e = tc
        last_safe = safe
        tc += 0.05
    out.update(n_ticks=len(ticks), n_start_events=len(colli_start), n_end_events=len(colli_end), t_s=t_s, t_e=t_e,
               colli_start=colli_start, colli_end=colli_end, ticks=ticks)
    if colli_start:
        out["first_start"] = colli_start[0]
    if colli_end:
        out["last_end"] = colli_end[-1]
    if over:
        out["status"] = OVER
        return out
    if len(colli_start) == 0:                 # :661
        out["status"] = NO_COLLISION
        return out
    if len(colli_start) == 1 and len(colli_end) == 0:  # :663
        out["status"] = ENDS_IN_OBSTACLE
        return out
    start_pts, end_pts = [], []
    n_sp = n_ep = 0
    sn = int(math.ceil((t_s - t_m) / dt))     # :667
    step = _div(t_s - t_m, sn)
    tc = t_m
    while tc <= t_s + 1e-4 and n_sp <= cap:
        if n_sp < max_pts:
            start_pts.append(ev(tc))
        n_sp += 1
        tc += step
    sn = int(math.ceil((t_mp - t_e) / dt))    # :675
    step = _div(t_mp - t_e, sn)
    if step > 1e-4:
        tc = t_e
        while tc <= t_mp + 1e-4 and n_ep <= cap:
            if n_ep < max_pts:
                end_pts.append(ev(tc))
            n_ep += 1
            tc += step
    else:
        end_pts.append(ev(t_mp))
        n_ep = 1
    over = len(colli_start) > max_events or len(colli_end) > max_events or n_sp > max_pts or n_ep > max_pts
    out.update(status=OVER if over else OK, n_start_pts=n_sp, n_end_pts=n_ep, start_pts=start_pts, end_pts=end_pts)
    return out


def path_length(path):
    """pathLength (topo_prm.cpp:417-425)"""
    length = 0.0
    for i in range(len(path) - 1):
        length += _norm(path[i + 1], path[i])
    return length


def _norm(a, b):
    d = [a[0] - b[0], a[1] - b[1], a[2] - b[2]]
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float64(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])))


def discretize_path(path, pt_num):
    """discretizePath(path, pt_num) (:427-461), literal; None where a point has no segment"""
    if len(path) < 2 or pt_num < 2:
        return None
    len_list = [0.0]
    for i in range(len(path) - 1):
        len_list.append(_norm(path[i + 1], path[i]) + len_list[i])
    dl = _div(len_list[-1], float(pt_num - 1))
    out = []
    with np.errstate(all="ignore"):
        for i in range(pt_num):
            cur_l = float(np.float64(i) * np.float64(dl))
            idx = -1
            for j in range(len(len_list) - 1):
                if cur_l >= len_list[j] - 1e-4 and cur_l <= len_list[j + 1] + 1e-4:
                    idx = j
                    break
            if idx < 0:
                return None
            lam = np.float64(cur_l - len_list[idx]) / np.float64(len_list[idx + 1] - len_list[idx])
            out.append([float((1 - lam) * np.float64(path[idx][k]) + lam * np.float64(path[idx + 1][k])) for k in range(3)])
    return out


def guide_points(path, duration, ctrl_pt_dist, degree, max_guide, cap=GUIDE_CAP):
    """one path of fuelmi_map_guide_points: dict(status, seg_num, dt, n_pts, n_ctrl, n_guide, guide_pts (the full list),
    tmp_pts (discretizePath's points))"""
    path = [[float(c) for c in q] for q in np.asarray(path, dtype=np.float64).reshape(-1, 3)]
    out = dict(status=G_UNDEFINED, seg_num=0, dt=0.0, n_pts=0, n_ctrl=0, n_guide=0, guide_pts=[], tmp_pts=None)
    if len(path) < 2:
        return out
    q = _div(path_length(path), ctrl_pt_dist)
    if not math.isfinite(q):
        return out
    if not q < cap + 1.0:
        out["status"] = OVER
        return out
    seg_num = max(6, int(q))                  # :554-555
    dt = duration / float(seg_num)            # :556
    out.update(seg_num=seg_num, dt=dt)
    n_pts = 0
    tp = 0.0
    while tp <= duration + 1e-4:              # plan_container.hpp:77
        if n_pts == cap:
            out.update(status=OVER, n_pts=n_pts)
            return out
        n_pts += 1
        tp += dt
    n_ctrl = n_pts + 2                        # parameterizeToBspline: K + 2 rows
    out.update(n_pts=n_pts, n_ctrl=n_ctrl)
    tmp = discretize_path(path, 2 * n_ctrl - 7 if degree == 4 else n_ctrl - 2)
    if tmp is None:
        return out
    if degree == 4:                           # :572-575
        guide = [tmp[i] for i in range(len(tmp)) if i % 2 == 1 and i >= 5 and i <= len(tmp) - 6]
    else:                                     # :568-569
        guide = tmp[2:len(tmp) - 2]
    out.update(status=OVER if len(guide) > max_guide else G_OK, n_guide=len(guide), guide_pts=guide, tmp_pts=tmp)
    return out
