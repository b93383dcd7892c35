"""The restatement of the exact solve of the optimiser's quadratic phases (fuelmi_map_solve_quadratic): the rows of
BsplineOptimizer's objective for a mask within SMOOTHNESS | START | END | GUIDE | WAYPOINTS, stated literally from
bspline_opt/src/bspline_optimizer.cpp, and two ways to its minimiser:

  dense   every row c (a . q - b)^2 into a dense Hessian H = sum c a a^T and right-hand sides g = sum c a b,
          numpy.linalg.solve -- nothing of the kernel's organisation in it
  band    the kernel's own arithmetic in Python floats: four diagonals per row gathered in the kernel's order, the
          banded Cholesky, the two substitutions -- what the host build of the kernel's text must equal bit for bit

A problem is a dict (problem()): ctrl [N, dim], dt, mask, start / end [3, dim], end_n, guide [N - 2 order, dim], waypts
[k, dim], widx [k], weights (the ld_* and bspline_degree), bounds, box (lo, hi: the map's box, not yet shrunk).
Python floats are IEEE doubles and nothing here contracts a product into a sum, so the band form is what a device built
with -ffp-contract=off computes."""
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMOOTHNESS, START, END, GUIDE, WAYPOINTS = 1 << 0, 1 << 3, 1 << 4, 1 << 5, 1 << 6
GUIDE_PHASE = SMOOTHNESS | GUIDE | START | END
YAW_MASK = SMOOTHNESS | WAYPOINTS | START | END
OK, BOUNDED, DEGENERATE = 0, 1, 2
WEIGHTS = dict(ld_smooth=20.0, ld_start=100.0, ld_end=0.5, ld_guide=1.5, ld_waypt=0.3, bspline_degree=3)
BOX = ((-4.0, -3.0, 0.0), (4.0, 3.0, 2.2))
TOLERANCE_JSON = os.path.join(ROOT, "profiles", "quad_solve_tolerance.json")


def problem(ctrl, dt, mask=GUIDE_PHASE, start=None, end=None, end_n=3, guide=None, waypts=None, widx=None, weights=None,
            bounds=False, box=BOX, tag=""):
    ctrl = np.ascontiguousarray(ctrl, dtype=np.float64)
    if ctrl.ndim == 1:
        ctrl = ctrl.reshape(-1, 1)
    dim = ctrl.shape[1]
    w = dict(WEIGHTS, **(weights or {}))
    z = np.zeros((3, dim))
    return dict(tag=tag, ctrl=ctrl, dim=dim, dt=float(dt), mask=int(mask),
                start=z if start is None else np.asarray(start, dtype=np.float64).reshape(3, dim),
                end=z if end is None else np.asarray(end, dtype=np.float64).reshape(3, dim), end_n=int(end_n),
                guide=np.zeros((0, dim)) if guide is None else np.asarray(guide, dtype=np.float64).reshape(-1, dim),
                waypts=np.zeros((0, dim)) if waypts is None else np.asarray(waypts, dtype=np.float64).reshape(-1, dim),
                widx=[] if widx is None else [int(i) for i in widx], weights=w, bounds=bool(bounds), box=box)


def order_of(pr):
    """optimize() :124-127"""
    return 3 if pr["dim"] == 1 else int(pr["weights"]["bspline_degree"])


def n_guide(pr):
    return max(len(pr["ctrl"]) - 2 * order_of(pr), 0)


def pt_dist(q):
    """optimize() :136-140: the norms of the differences summed left to right, over the point count"""
    n, dim = len(q), len(q[0])
    s = 0.0
    for i in range(n - 1):
        t = 0.0
        for k in range(dim):
            d = float(q[i + 1][k]) - float(q[i][k])
            t += d * d
        s += math.sqrt(t)
    return s / float(n)


# ---- the rows, literally ---------------------------------------------------------------------------------------------
def rows(pr, ptd):
    """every term of the objective as (weight c, {index: coefficient}, target b [dim]): the cost is sum c |a . q - b|^2"""
    N, dim, dt, w, m = len(pr["ctrl"]), pr["dim"], pr["dt"], pr["weights"], pr["mask"]
    z = [0.0] * dim
    out = []
    if m & SMOOTHNESS:  # calcSmoothnessCost :263-266: ji = (q[i+3] - 3 q[i+2] + 3 q[i+1] - q[i]) / pt_dist_
        for i in range(N - 3):
            out.append((w["ld_smooth"], {i: -1.0 / ptd, i + 1: 3.0 / ptd, i + 2: -3.0 / ptd, i + 3: 1.0 / ptd}, z))
    if m & START:  # calcStartCost :369-389
        s = pr["start"]
        out.append((10.0 * w["ld_start"], {0: 1 / 6.0, 1: 4 / 6.0, 2: 1 / 6.0}, list(s[0])))      # w_pos = 10.0
        out.append((w["ld_start"], {0: -1 / (2 * dt), 2: 1 / (2 * dt)}, list(s[1])))
        out.append((w["ld_start"], {0: 1 / (dt * dt), 1: -2 / (dt * dt), 2: 1 / (dt * dt)}, list(s[2])))
    if m & END:  # calcEndCost :407-430, end_state_.size() of the three
        e = pr["end"]
        out.append((w["ld_end"], {N - 3: 1 / 6.0, N - 2: 4 / 6.0, N - 1: 1 / 6.0}, list(e[0])))
        if pr["end_n"] >= 2:
            out.append((w["ld_end"], {N - 3: -1 / (2 * dt), N - 1: 1 / (2 * dt)}, list(e[1])))
        if pr["end_n"] == 3:
            out.append((w["ld_end"], {N - 3: 1 / (dt * dt), N - 2: -2 / (dt * dt), N - 1: 1 / (dt * dt)}, list(e[2])))
    if m & GUIDE:  # calcGuideCost :468-474
        o = order_of(pr)
        for i in range(o, N - o):
            out.append((w["ld_guide"], {i: 1.0}, list(pr["guide"][i - o])))
    if m & WAYPOINTS:  # calcWaypointsCost :442-456
        for wp, i in zip(pr["waypts"], pr["widx"]):
            out.append((w["ld_waypt"], {i: 1 / 6.0, i + 1: 4 / 6.0, i + 2: 1 / 6.0}, list(wp)))
    return out


def combine_cost(pr, q, ptd):
    """combineCost :571-630 at q [N][dim] in the reference's order: per term per row the squared norm across the axes, rows
    left to right, f_combine += ld * f"""
    N, dim, dt, w, m = len(q), pr["dim"], pr["dt"], pr["weights"], pr["mask"]
    q = [[float(v) for v in r] for r in q]
    cost = 0.0
    if m & SMOOTHNESS:
        fs = 0.0
        for i in range(N - 3):
            s = 0.0
            for k in range(dim):
                ji = (q[i + 3][k] - 3 * q[i + 2][k] + 3 * q[i + 1][k] - q[i][k]) / ptd
                s += ji * ji
            fs += s
        cost += w["ld_smooth"] * fs
    if m & START:
        S = [[float(v) for v in r] for r in pr["start"]]
        f0 = 0.0
        s = 0.0
        for k in range(dim):
            dq = 1 / 6.0 * (q[0][k] + 4 * q[1][k] + q[2][k]) - S[0][k]
            s += dq * dq
        f0 += 10.0 * s
        s = 0.0
        for k in range(dim):
            dq = 1 / (2 * dt) * (q[2][k] - q[0][k]) - S[1][k]
            s += dq * dq
        f0 += s
        s = 0.0
        for k in range(dim):
            dq = 1 / (dt * dt) * (q[0][k] - 2 * q[1][k] + q[2][k]) - S[2][k]
            s += dq * dq
        f0 += s
        cost += w["ld_start"] * f0
    if m & END:
        E = [[float(v) for v in r] for r in pr["end"]]
        q3, q2, q1 = q[N - 3], q[N - 2], q[N - 1]
        fe = 0.0
        s = 0.0
        for k in range(dim):
            dq = 1 / 6.0 * (q1[k] + 4 * q2[k] + q3[k]) - E[0][k]
            s += dq * dq
        fe += s
        if pr["end_n"] >= 2:
            s = 0.0
            for k in range(dim):
                dq = 1 / (2 * dt) * (q1[k] - q3[k]) - E[1][k]
                s += dq * dq
            fe += s
        if pr["end_n"] == 3:
            s = 0.0
            for k in range(dim):
                dq = 1 / (dt * dt) * (q1[k] - 2 * q2[k] + q3[k]) - E[2][k]
                s += dq * dq
            fe += s
        cost += w["ld_end"] * fe
    if m & GUIDE:
        o = order_of(pr)
        fg = 0.0
        for i in range(o, N - o):
            s = 0.0
            for k in range(dim):
                d = q[i][k] - float(pr["guide"][i - o][k])
                s += d * d
            fg += s
        cost += w["ld_guide"] * fg
    if m & WAYPOINTS:
        fw = 0.0
        for wp, i in zip(pr["waypts"], pr["widx"]):
            s = 0.0
            for k in range(dim):
                dq = 1 / 6.0 * (q[i][k] + 4 * q[i + 1][k] + q[i + 2][k]) - float(wp[k])
                s += dq * dq
            fw += s
        cost += w["ld_waypt"] * fw
    return cost


# ---- the two solves ----------------------------------------------------------------------------------------------------
def dense_solve(pr, ptd):
    """-> q [N, dim], or None when numpy finds the Hessian singular"""
    N, dim = len(pr["ctrl"]), pr["dim"]
    H = np.zeros((N, N))
    g = np.zeros((N, dim))
    for c, a, b in rows(pr, ptd):
        idx = sorted(a)
        v = np.array([a[i] for i in idx])
        H[np.ix_(idx, idx)] += c * np.outer(v, v)
        g[idx] += c * np.outer(v, np.array(b, dtype=np.float64))
    try:
        return np.linalg.solve(H, g)
    except np.linalg.LinAlgError:
        return None


def _J(k):
    return -1.0 if k == 0 else 3.0 if k == 1 else -3.0 if k == 2 else 1.0


def _P(k):
    return 4.0 / 6.0 if k == 1 else 1.0 / 6.0


def _V(k, dt):
    return (-1.0 if k == 0 else 0.0 if k == 1 else 1.0) / (2 * dt)


def _A(k, dt):
    return (-2.0 if k == 1 else 1.0) / (dt * dt)


def band_system(pr, ptd):
    """the kernel's gather: band[r][d] = H(r, r - d), g[r][k]; the way-points summed per index first, in the order given"""
    N, dim, dt, w, m = len(pr["ctrl"]), pr["dim"], pr["dt"], pr["weights"], pr["mask"]
    o = order_of(pr)
    smooth, has_s, has_e = bool(m & SMOOTHNESS), bool(m & START), bool(m & END)
    nw = len(pr["widx"]) if m & WAYPOINTS else 0
    wc = [0.0] * N
    ws = [[0.0] * dim for _ in range(N)]
    for j in range(nw):
        i = pr["widx"][j]
        wc[i] += 1.0
        for k in range(dim):
            ws[i][k] += float(pr["waypts"][j][k])
    cs = w["ld_smooth"] if smooth else 0.0
    cp, cv, ce, cg, cw = 10.0 * w["ld_start"], w["ld_start"], w["ld_end"], w["ld_guide"], w["ld_waypt"]
    S = [[float(v) for v in r] for r in pr["start"]]
    E = [[float(v) for v in r] for r in pr["end"]]
    band = [[0.0] * 4 for _ in range(N)]
    g = [[0.0] * dim for _ in range(N)]
    for r in range(N):
        for d in range(4):
            c = r - d
            if c < 0:
                continue
            hd = 0.0
            if smooth:
                s = 0.0
                for i in range(max(0, r - 3), min(c, N - 4) + 1):
                    s += (_J(r - i) / ptd) * (_J(c - i) / ptd)
                hd += cs * s
            if has_s and r <= 2:
                hd += cp * (_P(r) * _P(c)) + cv * (_V(r, dt) * _V(c, dt)) + cv * (_A(r, dt) * _A(c, dt))
            if has_e and c >= N - 3:
                rr, cc = r - (N - 3), c - (N - 3)
                t = _P(rr) * _P(cc)
                if pr["end_n"] >= 2:
                    t += _V(rr, dt) * _V(cc, dt)
                if pr["end_n"] == 3:
                    t += _A(rr, dt) * _A(cc, dt)
                hd += ce * t
            if nw > 0:
                sw = 0.0
                for i in range(max(0, r - 2), min(c, N - 3) + 1):
                    sw += wc[i] * (_P(r - i) * _P(c - i))
                hd += cw * sw
            band[r][d] = hd
        guided = bool(m & GUIDE) and o <= r < N - o
        if guided:
            band[r][0] += cg
        for k in range(dim):
            v = 0.0
            if has_s and r <= 2:
                v += cp * (S[0][k] * _P(r)) + cv * (S[1][k] * _V(r, dt)) + cv * (S[2][k] * _A(r, dt))
            if has_e and r >= N - 3:
                rr = r - (N - 3)
                t = E[0][k] * _P(rr)
                if pr["end_n"] >= 2:
                    t += E[1][k] * _V(rr, dt)
                if pr["end_n"] == 3:
                    t += E[2][k] * _A(rr, dt)
                v += ce * t
            if guided:
                v += cg * float(pr["guide"][r - o][k])
            if nw > 0:
                sw = 0.0
                for i in range(max(0, r - 2), min(r, N - 3) + 1):
                    sw += ws[i][k] * _P(r - i)
                v += cw * sw
            g[r][k] = v
    return band, g


def band_solve(pr, ptd):
    """the kernel's banded Cholesky and substitutions -> q [N][dim], or None at a pivot that is <= 0 or not finite"""
    N, dim, hb = len(pr["ctrl"]), pr["dim"], 3
    band, g = band_system(pr, ptd)
    for j in range(N):
        s = band[j][0]
        for d in range(1, min(hb, j) + 1):
            s -= band[j][d] * band[j][d]
        if not (s > 0.0) or not math.isfinite(s):
            return None
        ljj = math.sqrt(s)
        band[j][0] = ljj
        for i in range(j + 1, min(j + hb, N - 1) + 1):
            t = band[i][i - j]
            for k in range(max(0, i - hb), j):
                t -= band[i][i - k] * band[j][j - k]
            band[i][i - j] = t / ljj
    for k in range(dim):
        for j in range(N):
            s = g[j][k]
            for d in range(1, min(hb, j) + 1):
                s -= band[j][d] * g[j - d][k]
            g[j][k] = s / band[j][0]
        for j in range(N - 1, -1, -1):
            s = g[j][k]
            for d in range(1, hb + 1):
                if j + d < N:
                    s -= band[j + d][d] * g[j + d][k]
            g[j][k] = s / band[j][0]
    return g


def shrunk_box(pr):
    return [pr["box"][0][k] + 0.1 for k in range(3)], [pr["box"][1][k] - 0.1 for k in range(3)]


def clamp_q0(pr):
    """optimize() :197-202"""
    lo, hi = shrunk_box(pr)
    return [[max(min(float(v), hi[k]), lo[k]) for k, v in enumerate(r)] for r in pr["ctrl"]]


def solve(pr, form="dense"):
    """-> dict(status, ctrl [N, dim], cost, pt_dist)"""
    ptd = pt_dist(pr["ctrl"])
    keep = dict(status=DEGENERATE, ctrl=np.array(pr["ctrl"], dtype=np.float64), cost=0.0, pt_dist=ptd)
    if (pr["mask"] & SMOOTHNESS) and (ptd == 0.0 or not math.isfinite(ptd)):
        return keep
    if form == "dense" and band_solve(pr, ptd) is None:  # (the status is the kernel's: its pivots decide)
        return keep
    q = dense_solve(pr, ptd) if form == "dense" else band_solve(pr, ptd)
    if q is None:
        return keep
    cost = combine_cost(pr, q, ptd)
    if not math.isfinite(cost):
        return keep
    if pr["bounds"] and pr["dim"] == 3:  # :206-214
        lo, hi = shrunk_box(pr)
        q0 = clamp_q0(pr)
        inside = all(max(q0[i][k] - 10.0, lo[k]) <= float(q[i][k]) <= min(q0[i][k] + 10.0, hi[k])
                     for i in range(len(q0)) for k in range(3))
        if not inside:
            return dict(status=BOUNDED, ctrl=np.array(q0), cost=combine_cost(pr, q0, ptd), pt_dist=ptd)
    return dict(status=OK, ctrl=np.array(q, dtype=np.float64), cost=cost, pt_dist=ptd)


_DIS = {}


def disagreement(pr):
    """the band form against the dense form on one problem: (max |control point difference|, |cost difference|); computed
    once per problem"""
    key = id(pr)
    if key not in _DIS:
        d, b = solve(pr, "dense"), solve(pr, "band")
        assert d["status"] == b["status"], pr["tag"]
        _DIS[key] = (pr, (float(np.abs(d["ctrl"] - b["ctrl"]).max()), abs(d["cost"] - b["cost"])))
    return _DIS[key][1]


def allowance(pr):
    """what a device result may differ from the dense form: 100 x the disagreement measured here for that problem (the yaw
    test's rule and margin: an ill-conditioned problem sets its own scale)"""
    dq, dc = disagreement(pr)
    return 100.0 * dq, 100.0 * dc


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import quad_solve_cases as qc
    table = {}
    for p in qc.numeric_cases():
        dq, dc = disagreement(p)
        table[p["tag"]] = dict(n_ctrl=len(p["ctrl"]), dim=p["dim"], ctrl=dq, cost=dc,
                               cost_at_minimiser=solve(p, "dense")["cost"])
        print("%-28s N %4d dim %d  band vs dense: ctrl %.3e cost %.3e" % (p["tag"], len(p["ctrl"]), p["dim"], dq, dc))
    if "--write" in sys.argv:
        with open(TOLERANCE_JSON, "w") as f:
            json.dump(dict(what="max |band form - dense form| of tests/quad_solve_ref.py per case of tests/quad_solve_cases.py; "
                                "the device allowance is 100 x these", cases=table), f, indent=1, sort_keys=True)
            f.write("\n")
