"""The scenes of the local segments of the global trajectory (fuel_amd/csrc/local_segment.hip):
tests/test_local_segment_cpu.py proves on the host that each sits on the edge it is drawn for,
tests/test_local_segment_gpu.py runs them on the device, tests/golden/make_localseg_golden.py records them from the
reference's own code.

Three kinds of state (localseg_ref.State):
  line    one segment x(t) = v t, y and z constant.  Its terms above the linear one are zero, so the reference's pow and
          dot, the product form and the device agree on every point TO THE BIT: the scenes that sit on an integer's edge
          (the exit step, floor(segment_len / dist_pt), the point count) are drawn on it and stay on their edge in every
          form
  uturn   one segment x(t) = 3 t - t^2 / 2: it leaves the sphere round its start and comes back
  tour    a min-jerk trajectory through five way-points (waypoint_traj_ref, the structured form the device computes);
          with_local() puts a local spline of the scene's degree over [1, 2] s

A scene is a dict: tag, state, mode, start_t, arg0, arg1, degree, max_points, recorded (False: the reference hangs, faults
or reads past a vector there), expect (outputs the scene is drawn for) and pred: a function of the restatement's result
that is true iff the scene sits on its edge.  Nothing here needs a GPU."""
import math

import numpy as np

import localseg_ref as lr
import waypoint_traj_ref as wr

SPHERE, DURATION = lr.SPHERE, lr.DURATION
V_LINE = 0.5
TOUR_WAY = [(0.0, 0.0, 1.0), (2.0, 0.6, 1.1), (4.0, -0.4, 1.3), (6.0, 0.2, 1.0), (8.0, 1.0, 1.2)]


def line(v=V_LINE, T=40.0, **kw):
    coef = np.zeros((1, 3, 6))
    coef[0, 0, 1] = v
    coef[0, 1, 0], coef[0, 2, 0] = 0.3, 1.0
    return lr.State([T], coef, T, **kw)


def uturn():
    coef = np.zeros((1, 3, 6))
    coef[0, 0, 1], coef[0, 0, 2] = 3.0, -0.5
    coef[0, 2, 0] = 1.0
    return lr.State([6.0], coef, 6.0)


_TOUR = {}


def tour(**kw):
    if not _TOUR:
        r = wr.plan(TOUR_WAY, (0.3, 0.0, 0.0), (0.0, 0.0, 0.0), 2.0, 0.45, form="structured")
        _TOUR.update(times=r["seg_times"], coef=r["coef"], duration=r["duration"])
    return lr.State(_TOUR["times"], _TOUR["coef"], _TOUR["duration"], **kw)


def with_local(base, degree=3, ts=1.0, te=2.0, span=0.25, time_change=0.0, last_time_inc=0.0, lift=0.05):
    """base with a local spline over [ts, te]: its control polygon follows the global trajectory, lifted in z so that
    the two are told apart"""
    n = int(round((te - ts) / span)) + degree
    ctrl = []
    for i in range(n):
        q = wr.evaluate(base.coef, base.seg_times, ts + (i - (degree - 1) / 2.0) * span, 0, False)
        ctrl.append([q[0], q[1], q[2] + lift])
    return lr.State(base.seg_times, base.coef, base.global_duration + time_change, degree=degree, local_ctrl=ctrl,
                    local_knot_span=span, local_ts=ts, local_te=te, time_change=time_change, last_time_inc=last_time_inc)


def scene(tag, state, mode, start_t, arg0, arg1, max_points=200, recorded=True, expect=None, pred=None):
    return dict(tag=tag, state=state, mode=mode, start_t=float(start_t), arg0=float(arg0), arg1=float(arg1),
                degree=state.degree, max_points=max_points, recorded=recorded, expect=expect or {}, pred=pred)


def restate(sc, literal_pow=False, **kw):
    return lr.solve(sc["state"], sc["mode"], sc["start_t"], sc["arg0"], sc["arg1"], max_points=sc["max_points"],
                    literal_pow=literal_pow, **kw)


def problem(sc, state_index=0):
    return (state_index, sc["mode"], sc["start_t"], sc["arg0"], sc["arg1"])


def up(v):
    return math.nextafter(v, math.inf)


def down(v):
    return math.nextafter(v, -math.inf)


def first_branch(which):
    return lambda r: r["trace"][0][0] == which


def first_segment(which):
    return lambda r: r["trace"][0][1] == which


def branch_runs(trace):
    """the branches of a trace without their repetitions"""
    out = []
    for b, _ in trace:
        if not out or out[-1] != b:
            out.append(b)
    return out


def get_state_scenes():
    """each pair takes different branches of getState at its first point (and at the two start derivatives)"""
    out = []
    loc = with_local(tour())
    gd = loc.global_duration
    for tag, t, which in (("t_minus_1e-3", -1e-3, lr.GLOBAL_HEAD), ("t_below_minus_1e-3", down(-1e-3), lr.LOCAL),
                          ("t_local_ts", loc.local_ts, lr.GLOBAL_HEAD), ("t_above_local_ts", up(loc.local_ts), lr.LOCAL),
                          ("t_local_te", loc.local_te, lr.GLOBAL_TAIL), ("t_below_local_te", down(loc.local_te), lr.LOCAL),
                          ("t_end_plus_1e-3", gd + 1e-3, lr.GLOBAL_TAIL), ("t_above_end_plus_1e-3", up(gd + 1e-3), lr.LOCAL)):
        # (a start past the end reads the polynomial more than 1e-4 past its last segment: the reference's lookup leaves
        # its vector there)
        out.append(scene(tag, loc, DURATION, t, 0.3, 0.1, recorded=tag != "t_end_plus_1e-3", expect={"n_points": 4},
                         pred=first_branch(which)))
    shifted = with_local(tour(), te=2.5, time_change=0.5, last_time_inc=0.2)
    out.append(scene("time_change_head", shifted, DURATION, 0.4, 0.5, 0.1, pred=first_branch(lr.GLOBAL_HEAD)))
    out.append(scene("time_change_tail", shifted, DURATION, 2.6, 0.5, 0.1, pred=first_branch(lr.GLOBAL_TAIL)))
    out.append(scene("time_change_sphere", shifted, SPHERE, 0.2, 2.5, 0.4))
    out.append(scene("no_local_state", tour(), DURATION, 0.5, 1.0, 0.125, expect={"n_points": 9},
                     pred=lambda r: all(b == lr.GLOBAL_TAIL for b, _ in r["trace"])))
    return out


def lookup_scenes():
    out = []
    t = tour()
    edge = t.seg_times[0] + 1e-4
    out.append(scene("lookup_on_edge", t, DURATION, edge, 0.3, 0.1, pred=first_segment(0)))
    out.append(scene("lookup_above_edge", t, DURATION, up(edge), 0.3, 0.1, pred=first_segment(1)))
    # (the polynomial is read 0.1 .. 0.4 s past its last segment: the reference's lookup leaves its vector there)
    late = tour(time_change=-0.5)
    out.append(scene("past_total", late, DURATION, late.global_duration - 0.4, 0.3, 0.1, recorded=False,
                     pred=lambda r: r["trace"][0] == (lr.GLOBAL_TAIL, len(late.seg_times) - 1) and
                     late.global_duration - 0.4 + 0.5 > sum(late.seg_times) + 1e-4))
    out.append(scene("one_segment", line(), DURATION, 1.0, 2.0, 0.25, expect={"n_points": 9}))
    out.append(scene("negative_t", tour(), DURATION, -5e-4, 0.3, 0.1, pred=first_branch(lr.GLOBAL_TAIL)))
    return out


def exit_radius(steps, v=V_LINE):
    """the line leaves the sphere in the body of step `steps`: half a step of margin on either side"""
    return v * (0.2 * steps - 0.1)


def _edge_dist(length, q):
    """a dist_pt with length / dist_pt == q exactly, and the next dist_pt above it (the quotient just under q); None
    where no double gives that quotient"""
    d = length / q
    for cand in (d, down(d), up(d), down(down(d)), up(up(d))):
        if length / cand == float(q):
            above = cand
            while length / above >= float(q):
                above = up(above)
            return cand, above
    return None


def quotient_edges():
    """(steps, segment_len, (d6, above), (d7, above)): the first walk along the line whose length has a dist_pt for both
    exact quotients"""
    for steps in range(20, 80):
        length = restate(scene("", line(), SPHERE, 0.0, exit_radius(steps), 1.0))["segment_len"]
        e6, e7 = _edge_dist(length, 6), _edge_dist(length, 7)
        if e6 and e7:
            return steps, length, e6, e7
    raise AssertionError("no walk with both quotients")


def sphere_scenes():
    out = []
    for steps in (1, 63, 64, 65, 128, 129):
        out.append(scene("exit_step_%d" % steps, line(), SPHERE, 0.0, exit_radius(steps), 0.45,
                         expect={"n_steps": steps}))
    t = tour()
    out.append(scene("exit_by_end", t, SPHERE, 0.37, 100.0, 0.45,
                     pred=lambda r: r["duration"] == t.global_duration - 0.37 and
                     math.fmod(r["duration"], 0.2) > 1e-3 and r["n_steps"] == int(r["duration"] / 0.2) + 1))
    out.append(scene("leaves_and_returns", uturn(), SPHERE, 0.0, 2.0, 0.3, expect={"n_steps": 4},
                     pred=lambda r: lr._norm(uturn().get_state(5.8, 0), uturn().get_state(0.0, 0)) < 2.0))
    loc = with_local(tour())
    out.append(scene("global_local_global", loc, SPHERE, 0.5, 3.5, 0.45,
                     pred=lambda r: branch_runs(r["trace"][:r["n_steps"] + 1]) ==
                     [lr.GLOBAL_HEAD, lr.LOCAL, lr.GLOBAL_TAIL]))
    # floor(segment_len / dist_pt) on its edges, on the line
    q_steps, _, (d6, _), (d7, d7_above) = quotient_edges()
    out.append(scene("quotient_6", line(), SPHERE, 0.0, exit_radius(q_steps), d6, expect={"seg_num": 6},
                     pred=lambda r: r["segment_len"] / d6 == 6.0))
    out.append(scene("quotient_under_7", line(), SPHERE, 0.0, exit_radius(q_steps), d7_above, expect={"seg_num": 6},
                     pred=lambda r: 6.999999999 < r["segment_len"] / d7_above < 7.0))
    out.append(scene("quotient_7", line(), SPHERE, 0.0, exit_radius(q_steps), d7, expect={"seg_num": 7},
                     pred=lambda r: r["segment_len"] / d7 == 7.0))
    out.append(scene("start_at_end", t, SPHERE, t.global_duration - 5e-4, 2.0, 0.45, recorded=False,
                     expect={"status": lr.DEGENERATE, "n_steps": 0, "seg_num": 6, "duration": 0.0, "dt": 0.0}))
    out.append(scene("sphere_deg4", with_local(tour(), degree=4), SPHERE, 0.5, 3.0, 0.45))
    out.append(scene("sphere_deg5", with_local(tour(), degree=5), SPHERE, 0.5, 3.0, 0.45))
    return out


def accumulated_edge(dt=0.1, lo=20, hi=400):
    """(duration, k): the accumulated tp of point k is above duration + 1e-4, k * dt is not -- the accumulation decides"""
    acc = 0.0
    for k in range(1, hi):
        acc += dt
        prod = k * dt
        if k >= lo and acc > prod:
            d = prod - 1e-4
            for _ in range(64):
                if prod <= d + 1e-4 < acc:
                    return d, k
                d = up(d) if d + 1e-4 < prod else down(d)
    raise AssertionError("no such point")


def duration_scenes():
    out = []
    for n in (2, 63, 64, 65, 129):
        dt = 0.05
        out.append(scene("points_%d" % n, line(), DURATION, 1.0, (n - 1) * dt + dt / 2, dt, expect={"n_points": n}))
    out.append(scene("over_max_points", line(), DURATION, 1.0, 64 * 0.05 + 0.025, 0.05, max_points=64,
                     expect={"status": -1, "n_points": 65, "n_ctrl": 0}))
    d, k = accumulated_edge()
    out.append(scene("accumulated_tp", line(), DURATION, 0.5, d, 0.1, expect={"n_points": k},
                     pred=lambda r: k * 0.1 <= d + 1e-4))
    loc4, loc5 = with_local(tour(), degree=4), with_local(tour(), degree=5)
    out.append(scene("duration_deg3", with_local(tour()), DURATION, 0.6, 1.8, 0.15))
    out.append(scene("duration_deg4", loc4, DURATION, 0.6, 1.8, 0.15))
    out.append(scene("duration_deg5", loc5, DURATION, 0.6, 1.8, 0.15))
    out.append(scene("one_point", line(), DURATION, 1.0, 0.05, 0.1, recorded=False,
                     expect={"status": lr.DEGENERATE, "n_points": 0}))
    out.append(scene("dt_zero", line(), DURATION, 1.0, 1.0, 0.0, recorded=False,
                     expect={"status": lr.DEGENERATE, "n_points": 0, "dt": 0.0, "duration": 1.0}))
    return out


def no_local_scenes():
    t = tour()
    return [scene("no_local_points", t, DURATION, t.global_duration - 0.2, 0.5, 0.1, recorded=False,
                  expect={"status": lr.NO_LOCAL, "n_points": 0, "duration": 0.0, "dt": 0.0}),
            scene("no_local_first", t, SPHERE, -1.5, 2.0, 0.45, recorded=False, expect={"status": lr.NO_LOCAL}),
            scene("no_local_deriv", t, DURATION, t.global_duration - 0.2, 0.2011, 0.1, recorded=False,
                  expect={"status": lr.NO_LOCAL})]


_SCENES = []


def scenes():
    if not _SCENES:
        _SCENES.extend(get_state_scenes() + lookup_scenes() + sphere_scenes() + duration_scenes() + no_local_scenes())
        assert len({s["tag"] for s in _SCENES}) == len(_SCENES)
    return _SCENES


def recorded_scenes():
    return [s for s in scenes() if s["recorded"]]


def groups(scs):
    """scenes that share a call: (degree, max_points) -> list"""
    g = {}
    for s in scs:
        g.setdefault((s["degree"], s["max_points"]), []).append(s)
    return g


def batch(scs):
    """(states, problems) of one call over scenes of one group: each scene its own state"""
    return [s["state"].as_dict() for s in scs], [problem(s, i) for i, s in enumerate(scs)]


def parity():
    """(the largest disagreement of the restatement's two forms over the recorded scenes, 100 x that): the reference
    calls pow and Eigen's dot, whose bits are not restated; the x 100 is waypoint_traj_ref.parity_tolerance's margin"""
    worst = 0.0
    for s in recorded_scenes():
        a, b = restate(s, False), restate(s, True)
        for key in ("segment_len", "duration", "dt"):
            worst = max(worst, abs(a[key] - b[key]))
        for key in ("points", "derivs"):
            if a[key]:
                worst = max(worst, float(np.abs(np.array(a[key]) - np.array(b[key])).max()))
    return worst, 100.0 * worst
