"""CPU checks of what fuel_amd.host's batched wrappers hand to the C entries: every wrapper runs against a recording
stand-in for libfuelmi.so that applies, per symbol, the arity and `argtype.from_param` of _lib.SYMBOLS -- a wrong argument
count or pointer kind fails here exactly as it would against the real library -- and returns a chosen code.  Per wrapper:
one ragged batch of two problems of different lengths, and the same batch with one problem over an explicit stride.  No
device and no library is needed."""
import ctypes as C
import functools
import types

import numpy as np
import pytest

from fuel_amd import _lib, host

I, D = np.int32, np.float64


class StandIn:
    """records (symbol, arguments) of every call; arguments are checked as ctypes would check them"""

    def __init__(self, rc=0):
        self.rc, self.calls = rc, []

    def __getattr__(self, name):
        if name not in _lib.SYMBOLS:
            raise AttributeError(name)
        res, argtypes = _lib.SYMBOLS[name]

        def fn(*args):
            assert len(args) == len(argtypes), "%s: %d arguments, the prototype has %d" % (name, len(args), len(argtypes))
            for k, (t, a) in enumerate(zip(argtypes, args)):
                try:
                    t.from_param(a)
                except (TypeError, C.ArgumentError) as e:
                    raise AssertionError("%s: argument %d: %s" % (name, k, e))
            if name == "fuelmi_last_error":
                return b"stand-in"
            if not name.endswith("_destroy"):  # (an object made by make() destroys its handle when it dies)
                self.calls.append((name, args))
            return None if res is None else self.rc
        return fn


def decoded(arg):
    """an argument as the test compares it: the array behind a pointer, the struct behind a byref, else the value"""
    if hasattr(arg, "_arr"):
        return np.asarray(arg._arr)
    if hasattr(arg, "_obj"):
        return arg._obj
    return arg.value if isinstance(arg, C.c_void_p) else arg


@pytest.fixture
def standin(monkeypatch):
    s = StandIn()
    monkeypatch.setattr(_lib, "_LIB", s)
    return s


def make(kind, L):
    """an SDFMap or a BsplineDeviceProblem (6 control points, 2 candidates, degree 3) over the stand-in, no device"""
    if kind == "map":
        t = host.SDFMap.__new__(host.SDFMap)
    else:
        t = host.BsplineDeviceProblem.__new__(host.BsplineDeviceProblem)
        b = _lib.BsplineBatch()
        b.cost_function, b.dim, b.point_num, b.n_traj, b.end_n, b.n_waypt = 0, 3, 6, 2, 3, 0
        t.problem, t.degree = types.SimpleNamespace(c=b, C=2, nvar=18), 3
    t.L, t.h = L, C.c_void_p(1)
    return t


def padded(rows, width, tail=(3,), dtype=D):
    """the padded array a wrapper must build: each row copied up to the width, zeros behind"""
    out = np.zeros((len(rows), width) + tuple(tail), dtype=dtype)
    for b, r in enumerate(rows):
        r = np.zeros((0,) + tuple(tail)) if r is None else np.asarray(r, dtype=dtype).reshape((-1,) + tuple(tail))
        k = min(len(r), width)
        out[b, :k] = r[:k]
    return out


def i32(*v):
    return np.array(v, dtype=I)


def f64(*v):
    return np.array(v, dtype=D)


A = np.arange(15, dtype=D).reshape(5, 3) * 0.1          # 5 control points
B = np.arange(21, dtype=D).reshape(7, 3) * 0.1 + 1.0    # 7 control points
KA, KB = np.arange(9, dtype=D) * 0.5, np.arange(11, dtype=D) * 0.25 + 1.0   # their knot vectors (degree 3)
P2, P4 = A[:2] + 5.0, B[:4] + 5.0
W3, W5 = A[:3] + 2.0, B[:5] + 2.0
V2 = np.arange(6, dtype=D).reshape(2, 3) * 0.01
SY = np.array([[0.1, 0.0, 0.0], [0.2, 0.1, 0.0]])
T = [[0.0, 0.1, 0.2], [0.05]]
Y = [[1.0, 2.0, 3.0, 4.0], None]
G = [[[0.1, 0.2, 0.3]], [[0.4, 0.5, 0.6], [0.7, 0.8, 0.9]]]          # gains of 1 and 2 layers, half_vert_num 1
STATES = [dict(seg_times=[1.0, 2.0], coef=np.ones((2, 3, 6)), global_duration=3.0),
          dict(seg_times=[1.5], coef=np.full((1, 3, 6), 2.0), global_duration=1.5, local_ctrl=A, local_knot_span=0.2,
               local_ts=0.5)]
PROBLEMS = [(0, 0, 0.1, 2.0, 0.3), (1, 1, 0.2, 1.0, 0.1)]
ST_COLS = {6: f64(3.0, 1.5), 9: f64(0.0, 0.2), 10: f64(-1.0, 0.5), 11: f64(-1.0, -1.0), 12: f64(0, 0), 13: f64(0, 0)}
PR_COLS = [i32(0, 1), i32(0, 1), f64(0.1, 0.2), f64(2.0, 1.0), f64(0.3, 0.1)]
SEL_RES = _lib.TRAJADJ_SELECT | _lib.TRAJADJ_RESAMPLE

TRAJCHK = dict(status=(I, (2,)), safe=(I, (2,)), distance=(D, (2,)), n_samples=(I, (2,)), hit_index=(I, (2,)),
               hit_t=(D, (2,)), hit_pos=(D, (2, 3)), end_reason=(I, (2,)), duration=(D, (2,)), limit=bool)


def yaw_result(ms, derivs):
    r = dict(status=(I, (2,)), duration=(D, (2,)), seg_num=(I, (2,)), dt_yaw=(D, (2,)), yaw_ctrl=(D, (2, ms + 3)),
             n_waypt=(I, (2,)), waypts=(D, (2, ms)), end_yaw=(D, (2,)), cost=(D, (2,)), limit=bool,
             yawdot_ctrl=(D, (2, ms + 2)) if derivs else None, yawddot_ctrl=(D, (2, ms + 1)) if derivs else None)
    return r


def smp_result(mt, flight=None):
    r = {k: (D, (2, mt, 3)) for k in ("pos", "vel", "acc", "jerk")}
    r.update({k: (D, (2, mt)) for k in ("yaw", "yawdot", "yawddot")})
    r.update(status=(I, (2, mt)), duration=(D, (2,)), flight=flight, n_t=(I, (2,)))
    return r


def adj_result(maxc, smp=None, best=None):
    r = dict(info=(I, (2, 8)), metrics=(D, (2, 12)), knots_out=(D, (2, maxc + 4)), samples=smp, best=best, n_ctrl=(I, (2,)))
    r.update({k: (I, (2,)) for k in _lib.TRAJADJ_INFO})
    r.update({k: (D, (2,)) for k in _lib.TRAJADJ_METRICS})
    return r


QUAD = lambda mc: dict(status=(I, (2,)), ctrl_out=(D, (2, mc, 3)), cost=(D, (2,)), pt_dist=(D, (2,)), ctrl=list)  # noqa: E731
QUAD_DEV = dict(status=(I, (2,)), ctrl_out=(D, (2, 6, 3)), cost=(D, (2,)), pt_dist=(D, (2,)))
COLR = lambda ev, mp: dict(  # noqa: E731
    {k: (I, (2,)) for k in ("status", "n_ticks", "n_start_events", "n_end_events", "n_start_pts", "n_end_pts")},
    t_s=(D, (2,)), t_e=(D, (2,)), colli_start=(D, (2, ev, 3)), colli_end=(D, (2, ev, 3)), start_pts=(D, (2, mp, 3)),
    end_pts=(D, (2, mp, 3)), first_start=(D, (2, 3)), last_end=(D, (2, 3)), limit=bool)
LOCSEG = dict({k: (I, (2,)) for k in ("status", "n_steps", "seg_num", "n_points", "n_ctrl")}, segment_len=(D, (2,)),
              duration=(D, (2,)), dt=(D, (2,)), points=(D, (2, 8, 3)), derivs=(D, (2, 4, 3)), ctrl=(D, (2, 10, 3)), limit=bool)
GAINS = lambda my: dict(status=(I, (2,)), gain=(D, (2, my)), n_cand=(I, (2, my)), n_visible=(I, (2, my)),  # noqa: E731
                        n_rays=(I, (2,)), limit=bool)
YAWPATH = lambda ml: dict(status=(I, (2,)), n_layer=(I, (2,)), path=(D, (2, ml)), path_vertex=(I, (2, ml)),  # noqa: E731
                          gains=(D, (2, ml, 3)), g_value=(D, (2, ml, 3)), n_rays=(I, (2, ml)), limit=bool)
KINO = dict({k: (I, (2,)) for k in ("status", "which", "iter_num", "use_node_num", "n_nodes", "shot", "seg_num", "n_samples")},
            t_shot=(D, (2,)), T_sum=(D, (2,)), ts=(D, (2,)), coef=(D, (2, 3, 4)), derivs=(D, (2, 4, 3)), samples=list,
            limit=bool)
KINO_NODES = dict(KINO, node_state=list, node_input=list, node_duration=list)
TOPO = dict(status=(I, (2,)), counts=(I, (2, 4)), events=(I, (2, 6)), n_nodes=(I, (2,)), raw_len=(I, (2, 2)),
            filt_len=(I, (2, 2)), sel_len=(I, (2, 3)), sel_length=(D, (2, 3)), nodes=list, raw=list, filt=list, sel=list,
            limit=bool)
GOAL = dict(status=(I, (2,)), length=(D, (2,)), n_way=(I, (2,)), next_goal=(D, (2, 3)), way=list, limit=bool)
WPT = dict(status=(I, (2,)), duration=(D, (2,)), length=(D, (2,)), seg_num=(I, (2,)), dt=(D, (2,)), n_samples=(I, (2,)),
           derivs=(D, (2, 4, 3)), samples=list, limit=bool)
PAIR = lambda t0, t1: lambda r: (isinstance(r, tuple) and len(r) == 2 and r[0].dtype == t0 and r[1].dtype == t1  # noqa: E731
                                 and r[0].shape == r[1].shape == (2,))

REFINE = [((0, 0, 0), (0, 0, 0), 0.0, [np.ones((2, 4)), np.ones((1, 4)) * 2]), ((1, 1, 1), (0, 0, 0), 0.5, [np.ones((3, 4)) * 3])]


def _localseg_args(first, ms, mc, more=()):
    """the eleven state arrays from position `first` on, for strides ms / mc, and further arguments"""
    a = {first: i32(2, 1), first + 1: padded([[1.0, 2.0], [1.5]], ms, ()),
         first + 2: padded([np.ones((2, 3, 6)), np.full((1, 3, 6), 2.0)], ms, (3, 6)), first + 4: i32(0, 5),
         first + 5: padded([None, A], mc)}
    a.update({first - 3 + k: v for k, v in ST_COLS.items()})
    a.update(more)
    return a


# id: (object, call, symbol, {position: expected argument}, [(position of a cfg, {field: value})], result, takes allow_limit)
# an expected argument is None (NULL), a number, or an array compared in dtype, shape and content
CASES = {
    "path_costs": ("map", lambda t, **k: t.path_costs(A[:2], B[:2], max_points=4, **k), "fuelmi_map_path_costs",
                   {2: 2, 3: A[:2], 4: B[:2]}, [(1, {"max_path_points": 4})],
                   lambda r: r[0].shape == (2,) and r[1].dtype == I and r[1].shape == (2,) and len(r[2]) == 2, False),
    "path_costs/no_paths": ("map", lambda t, **k: t.path_costs(A[:2], B[:2], max_points=0, **k), "fuelmi_map_path_costs",
                            {8: None}, [(1, {"max_path_points": 0})], lambda r: r[2] is None, False),
    "refine_tours": ("map", lambda t, **k: t.refine_tours(REFINE, 2.0, 1.0, 1.5, **k), "fuelmi_map_refine_tours",
                     {2: 2, 3: np.array([[0, 0, 0, 0, 0, 0, 0], [1, 1, 1, 0, 0, 0, 0.5]], dtype=D), 4: i32(0, 2, 3),
                      5: i32(0, 2, 3, 6), 6: np.repeat([1.0, 1.0, 2.0, 3.0, 3.0, 3.0], 4).reshape(6, 4), 9: None, 10: None},
                     [(1, {"vm": 2.0, "max_tour_points": 1024, "flags": 0})],
                     lambda r: [c.shape for c in r[0]] == [(2,), (1,)] and r[1].shape == (2,) and r[2] is None, False),
    "goal_paths": ("map", lambda t, **k: t.goal_paths(A[:2], B[:2], max_path_points=8, max_way_points=4, raw=False, **k),
                   "fuelmi_map_goal_paths", {2: 2, 3: A[:2], 4: B[:2], 10: None, 11: None},
                   [(1, {"max_way_points": 4, "path.max_path_points": 8})], GOAL, True),
    "goal_paths/raw": ("map", lambda t, **k: t.goal_paths(A[:2], B[:2], max_path_points=8, max_way_points=4, **k),
                       "fuelmi_map_goal_paths", {11: np.zeros((2, 8, 3))}, [], dict(GOAL, raw_len=(I, (2,)), raw=list), True),
    "waypoint_trajs": ("map", lambda t, **k: t.waypoint_trajs([W3, W5], V2, V2 * 2, coef=False, **k),
                       "fuelmi_map_waypoint_trajs", {2: 2, 3: i32(3, 5), 4: padded([W3, W5], 5), 5: V2, 6: V2 * 2, 15: None,
                                                     16: None},
                       [(1, {"max_way_points": 5, "max_samples": 128})], WPT, True),
    "waypoint_trajs/over": ("map", lambda t, **k: t.waypoint_trajs([W3, W5], V2, V2, max_way_points=4, max_samples=8, **k),
                            "fuelmi_map_waypoint_trajs", {3: i32(3, 5), 4: padded([W3, W5], 4), 15: np.zeros((2, 3)),
                                                          16: np.zeros((2, 3, 3, 6))},
                            [(1, {"max_way_points": 4, "max_samples": 8})], dict(WPT, seg_times=list, coef=list), True),
    "kino_paths": ("map", lambda t, **k: t.kino_paths(A[:2], V2, V2 * 2, B[:2], V2 * 3, nodes=False, max_path_nodes=8,
                                                       max_samples=16, **k), "fuelmi_map_kino_paths",
                   {2: 2, 3: A[:2], 4: V2, 5: V2 * 2, 6: B[:2], 7: V2 * 3, 13: None, 14: None, 15: None,
                    23: np.zeros((2, 16, 3))}, [(1, {"max_path_nodes": 8, "max_samples": 16})], KINO, True),
    "kino_paths/nodes": ("map", lambda t, **k: t.kino_paths(A[:2], V2, V2, B[:2], V2, max_path_nodes=8, **k),
                         "fuelmi_map_kino_paths", {13: np.zeros((2, 8, 6)), 14: np.zeros((2, 8, 3)), 15: np.zeros((2, 8))},
                         [], KINO_NODES, True),
    "topo_paths": ("map", lambda t, **k: t.topo_paths(A[:2], B[:2], np.ones((2, 4, 3)), start_pts=[P2, None],
                                                       max_raw_path2=2, reserve_num=3, max_path_points=5, max_nodes=6, **k),
                   "fuelmi_map_topo_paths", {2: 2, 3: A[:2], 4: B[:2], 5: 2, 6: i32(2, 0), 7: padded([P2, None], 2), 8: 0,
                                             9: i32(0, 0), 10: np.zeros((2, 0, 3)), 11: np.ones((2, 4, 3)),
                                             21: np.zeros((2, 2, 5, 3)), 25: np.zeros((2, 3, 5, 3))},
                   [(1, {"max_sample_num": 4, "max_nodes": 6})], TOPO, True),
    "collision_ranges": ("map", lambda t, **k: t.collision_ranges([A, B], 0.5, max_events=2, max_pts=3, **k),
                         "fuelmi_map_collision_ranges", {2: 2, 3: i32(5, 7), 4: padded([A, B], 7), 5: f64(0.5, 0.5)},
                         [(1, {"max_ctrl": 7, "max_events": 2, "max_pts": 3})], COLR(2, 3), True),
    "collision_ranges/over": ("map", lambda t, **k: t.collision_ranges([A, B], [0.5, 0.25], max_ctrl=6, max_events=2,
                                                                        max_pts=3, **k),
                              "fuelmi_map_collision_ranges", {3: i32(5, 7), 4: padded([A, B], 6), 5: f64(0.5, 0.25)},
                              [(1, {"max_ctrl": 6})], COLR(2, 3), True),
    "guide_points": ("map", lambda t, **k: t.guide_points([P2, P4], 1.5, max_guide=5, **k), "fuelmi_map_guide_points",
                     {1: 2, 2: 4, 3: padded([P2, P4], 4), 4: i32(2, 4), 5: f64(1.5, 1.5), 6: 0.5, 7: 3, 8: 5}, [],
                     dict({k: (I, (2,)) for k in ("status", "seg_num", "n_pts", "n_ctrl", "n_guide")}, dt=(D, (2,)),
                          guide_pts=(D, (2, 5, 3)), limit=bool), True),
    "guide_points/over": ("map", lambda t, **k: t.guide_points([P2, P4], 1.5, max_path_points=3, **k),
                          "fuelmi_map_guide_points", {2: 3, 3: padded([P2, P4], 3), 4: i32(2, 4)}, [], None, True),
    "local_segments": ("map", lambda t, **k: t.local_segments(STATES, PROBLEMS, max_points=8, **k),
                       "fuelmi_map_local_segments",
                       _localseg_args(3, 2, 5, {2: 2, 14: 2, 15: PR_COLS[0], 16: PR_COLS[1], 17: PR_COLS[2], 18: PR_COLS[3],
                                               19: PR_COLS[4]}),
                       [(1, {"degree": 3, "max_seg": 2, "max_ctrl": 5, "max_points": 8})], LOCSEG, True),
    "local_segments/over": ("map", lambda t, **k: t.local_segments(STATES, PROBLEMS, max_points=8, max_seg=1, max_ctrl=4, **k),
                            "fuelmi_map_local_segments", _localseg_args(3, 1, 4), [(1, {"max_seg": 1, "max_ctrl": 4})],
                            LOCSEG, True),
    "info_gains": ("map", lambda t, **k: t.info_gains(A[:2], [[0.1], [0.2, 0.3, 0.4]], **k), "fuelmi_map_info_gains",
                   {2: 2, 3: A[:2], 4: i32(1, 3), 5: padded([[0.1], [0.2, 0.3, 0.4]], 3, ()), 6: 0, 7: None, 8: None, 9: None},
                   [(1, {"max_yaw": 3, "max_ctrl": 1})], GAINS(3), True),
    "info_gains/over": ("map", lambda t, **k: t.info_gains(A[:2], [[0.1], [0.2, 0.3, 0.4]], ctrl=[A, B], path_of=[1, 0],
                                                            max_yaw=2, max_ctrl=6, **k), "fuelmi_map_info_gains",
                        {4: i32(1, 3), 5: padded([[0.1], [0.2, 0.3]], 2, ()), 6: 2, 7: i32(5, 7), 8: padded([A, B], 6),
                         9: i32(1, 0)}, [(1, {"max_yaw": 2, "max_ctrl": 6})], GAINS(2), True),
    "yaw_paths": ("map", lambda t, **k: t.yaw_paths([P2[:1], P2], [[0.1], [0.2, 0.3]], 0.5, half_vert_num=1, **k),
                  "fuelmi_map_yaw_paths", {2: 2, 3: i32(1, 2), 4: padded([P2[:1], P2], 2), 5: padded([[0.1], [0.2, 0.3]], 2, ()),
                                           6: f64(0.5, 0.5), 7: None, 8: None, 9: None},
                  [(1, {"max_layer": 2, "gain.max_yaw": 3})], YAWPATH(2), True),
    "yaw_paths/over": ("map", lambda t, **k: t.yaw_paths([P2[:1], P2], [[0.1], [0.2, 0.3]], 0.5, ctrl=[A, B], gains_in=G,
                                                          max_layer=1, max_ctrl=6, half_vert_num=1, **k),
                       "fuelmi_map_yaw_paths", {3: i32(1, 2), 4: padded([P2[:1], P2], 1), 5: padded([[0.1], [0.2]], 1, ()),
                                                7: i32(5, 7), 8: padded([A, B], 6), 9: padded(G, 1, (3,))},
                       [(1, {"max_layer": 1, "gain.max_ctrl": 6})], YAWPATH(1), True),
    "plan_yaws": ("map", lambda t, **k: t.plan_yaws([A, B], 0.5, SY, derivs=False, **k), "fuelmi_map_plan_yaws",
                  {3: 2, 4: i32(5, 7), 5: padded([A, B], 7), 6: f64(0.5, 0.5), 7: SY, 8: None, 18: None, 19: None},
                  [(1, {"ld_smooth": 20.0, "bspline_degree": 3}), (2, {"max_ctrl": 7, "max_seg": 12})], yaw_result(12, False),
                  True),
    "plan_yaws/knots_over": ("map", lambda t, **k: t.plan_yaws([A, B], None, SY, end_yaw=[0.3, 0.4], knots=[KA, KB],
                                                                max_ctrl=6, weights={"ld_smooth": 3.0}, max_seg=5, **k),
                             "fuelmi_map_plan_yaws_knots",
                             {4: i32(5, 7), 5: padded([A, B], 6), 6: padded([KA, KB], 10, ()), 8: f64(0.3, 0.4)},
                             [(1, {"ld_smooth": 3.0, "ld_dist": 10.0}), (2, {"max_ctrl": 6, "max_seg": 5})], yaw_result(5, True),
                             True),
    "solve_quadratic": ("map", lambda t, **k: t.solve_quadratic([A, B], 0.5, **k), "fuelmi_map_solve_quadratic",
                        {3: 2, 4: i32(5, 7), 5: padded([A, B], 7), 6: f64(0.5, 0.5), 7: None, 8: None, 9: None, 10: None,
                         11: None, 12: None},
                        [(1, {"ld_guide": 1.5}), (2, {"max_ctrl": 7, "max_waypt": 0, "dim": 3, "end_n": 3, "bounds": 0})],
                        QUAD(7), False),
    "solve_quadratic/over": ("map", lambda t, **k: t.solve_quadratic(
        [A, B], [0.5, 0.25], start_state=np.ones((2, 3, 3)), guide_pts=[np.zeros((0, 3)), A[:1]], waypoints=[A[:1], B[:2]],
        waypt_idx=[[2], [1, 3]], max_ctrl=6, bounds=True, **k), "fuelmi_map_solve_quadratic",
        {4: i32(5, 7), 5: padded([A, B], 6), 6: f64(0.5, 0.25), 7: np.ones((2, 3, 3)), 8: None, 9: np.zeros((2, 0, 3)),
         10: i32(1, 2), 11: padded([A[:1], B[:2]], 2), 12: padded([[2], [1, 3]], 2, (), I)},
        [(2, {"max_ctrl": 6, "max_waypt": 2, "bounds": 1})], QUAD(6), False),
    "check_trajs": ("map", lambda t, **k: t.check_trajs([A, B], 0.5, 0.1, **k), "fuelmi_map_check_trajs",
                    {2: 2, 3: i32(5, 7), 4: padded([A, B], 7), 5: f64(0.5, 0.5), 6: f64(0.1, 0.1)},
                    [(1, {"max_ctrl": 7, "degree": 3})], TRAJCHK, True),
    "check_trajs/knots_over": ("map", lambda t, **k: t.check_trajs([A, B], None, [0.1, 0.2], knots=[KA, KB], max_ctrl=6, **k),
                               "fuelmi_map_check_trajs_knots",
                               {3: i32(5, 7), 4: padded([A, B], 6), 5: padded([KA, KB], 10, ()), 6: f64(0.1, 0.2)},
                               [(1, {"max_ctrl": 6})], TRAJCHK, True),
    "sampleTrajs": ("map", lambda t, **k: t.sampleTrajs([A, B], 0.5, T, **k), "fuelmi_map_sample_trajs",
                    {2: 2, 3: i32(5, 7), 4: padded([A, B], 7), 5: f64(0.5, 0.5), 6: None, 7: None, 8: None, 9: None,
                     10: i32(3, 1), 11: padded(T, 3, ()), 21: None},
                    [(1, {"max_ctrl": 7, "max_yaw_ctrl": 0, "max_t": 3, "mode": 0})], smp_result(3), False),
    "sampleTrajs/knots_over": ("map", lambda t, **k: t.sample_trajs([A, B], None, T, yaw_ctrl=Y, yaw_dt=0.2, t_stop=1.0,
                                                                     flight=np.ones((2, 8)), max_ctrl=6, max_t=2, knots=[KA, KB],
                                                                     mode=1, **k), "fuelmi_map_sample_trajs_knots",
                               {3: i32(5, 7), 4: padded([A, B], 6), 5: padded([KA, KB], 10, ()), 6: i32(4, 0),
                                7: padded(Y, 4, ()), 8: f64(0.2, 0.2), 9: f64(1.0, 1.0), 10: i32(3, 1), 11: padded(T, 2, ()),
                                21: np.ones((2, 8))},
                               [(1, {"max_ctrl": 6, "max_yaw_ctrl": 4, "max_t": 2, "mode": 1})], smp_result(2, (D, (2, 8))),
                               False),
    "adjust_trajs": ("map", lambda t, **k: t.adjust_trajs([A, B], 0.5, **k), "fuelmi_map_adjust_trajs",
                     {2: 2, 3: i32(5, 7), 4: padded([A, B], 7), 5: f64(0.5, 0.5), 6: None, 7: None, 8: None, 12: None, 13: None},
                     [(1, {"ops": 0, "max_ctrl": 7, "max_samples": 0, "n_group": 0})], adj_result(7), False),
    "adjust_trajs/over": ("map", lambda t, **k: t.adjust_trajs([A, B], knots_in=[KA, KB], ratio_in=1.5, group=[0, 1],
                                                                ops=SEL_RES, max_ctrl=6, **k), "fuelmi_map_adjust_trajs",
                          {3: i32(5, 7), 4: padded([A, B], 6), 5: None, 6: padded([KA, KB], 10, ()), 7: f64(1.5, 1.5),
                           8: i32(0, 1), 12: np.zeros((2, 5, 3)), 13: i32(-1, -1)},
                          [(1, {"ops": SEL_RES, "max_ctrl": 6, "max_samples": 5, "n_group": 2})],
                          adj_result(6, (D, (2, 5, 3)), (I, (2,))), False),
    "dev.plan_yaws": ("dev", lambda t, **k: t.plan_yaws(SY, derivs=False, mode=1, **k), "fuelmi_bspline_dev_plan_yaws",
                      {2: SY, 3: None, 13: None, 14: None}, [(1, {"max_ctrl": 6, "max_seg": 256, "pos_degree": 3})],
                      yaw_result(256, False), True),
    "dev.plan_yaws/end": ("dev", lambda t, **k: t.plan_yaws(SY, end_yaw=0.3, **k), "fuelmi_bspline_dev_plan_yaws",
                          {3: f64(0.3, 0.3)}, [(1, {"max_seg": 12})], yaw_result(12, True), True),
    "dev.solve_quadratic": ("dev", lambda t, **k: t.solve_quadratic(**k), "fuelmi_bspline_dev_solve_quadratic", {2: None},
                            [(1, {"dim": 3, "max_ctrl": 6, "end_n": 3, "max_waypt": 0, "bounds": 0})], QUAD_DEV, False),
    "dev.check_trajs": ("dev", lambda t, **k: t.check_trajs([0.1, 0.2], **k), "fuelmi_bspline_dev_check_trajs",
                        {2: f64(0.1, 0.2)}, [(1, {"max_ctrl": 6, "degree": 3})], TRAJCHK, True),
    "dev.sample_trajs": ("dev", lambda t, **k: t.sample_trajs(T, max_t=2, **k), "fuelmi_bspline_dev_sample_trajs",
                         {2: None, 3: None, 4: None, 5: None, 6: i32(3, 1), 7: padded(T, 2, ()), 17: None},
                         [(1, {"max_ctrl": 6, "max_yaw_ctrl": 0, "max_t": 2})], smp_result(2), False),
    "dev.sample_trajs/yaw": ("dev", lambda t, **k: t.sample_trajs(T, yaw_ctrl=Y, yaw_dt=[0.2, 0.3], max_yaw_ctrl=3, **k),
                             "fuelmi_bspline_dev_sample_trajs", {2: i32(4, 0), 3: padded(Y, 3, ()), 4: f64(0.2, 0.3)},
                             [(1, {"max_yaw_ctrl": 3, "max_t": 3})], smp_result(3), False),
    "dev.adjust_trajs": ("dev", lambda t, **k: t.adjust_trajs(knots_in=[KA, KB], group=[1, 1], ops=SEL_RES, **k),
                         "fuelmi_bspline_dev_adjust_trajs",
                         {2: padded([KA, KB], 10, ()), 3: None, 4: i32(1, 1), 8: np.zeros((2, 5, 3)), 9: i32(-1, -1)},
                         [(1, {"max_ctrl": 6, "max_samples": 5, "n_group": 2})], adj_result(6, (D, (2, 5, 3)), (I, (2,))), False),
    "dev.load_waypoints": ("dev", lambda t, **k: t.load_waypoints([W3, W5], V2, V2 * 2, max_way_points=4, **k),
                           "fuelmi_bspline_dev_load_waypoints", {2: i32(3, 5), 3: padded([W3, W5], 4), 4: V2, 5: V2 * 2},
                           [(1, {"max_way_points": 4, "seg_num": 0, "max_samples": 1})], PAIR(I, D), True),
    "dev.load_local_segments": ("dev", lambda t, **k: t.load_local_segments(STATES, PROBLEMS, **k),
                                "fuelmi_bspline_dev_load_local_segments",
                                _localseg_args(4, 2, 5, {1: 2, 2: 5, 3: 2, 15: PR_COLS[0], 16: PR_COLS[1], 17: PR_COLS[2],
                                                        18: PR_COLS[3], 19: PR_COLS[4]}),
                                [], PAIR(I, D), False),
    "dev.load_kino": ("dev", lambda t, **k: t.load_kino(A[:2], V2, V2 * 2, B[:2], V2 * 3, max_samples=16, **k),
                      "fuelmi_bspline_dev_load_kino", {2: A[:2], 3: V2, 4: V2 * 2, 5: B[:2], 6: V2 * 3},
                      [(1, {"max_samples": 16, "max_path_nodes": 64})], PAIR(I, D), True),
}


def _same(got, want):
    if want is None:
        return got is None
    if isinstance(want, np.ndarray):
        return isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape and \
            got.flags.c_contiguous and np.array_equal(got, want)
    return not isinstance(got, np.ndarray) and got == want


@pytest.mark.parametrize("case", sorted(CASES))
def test_wrapper_hands_c_the_packed_batch(standin, case):
    kind, call, symbol, args, cfgs, result, _ = CASES[case]
    r = call(make(kind, standin))
    assert [c[0] for c in standin.calls] == [symbol]
    got = [decoded(a) for a in standin.calls[0][1]]
    for pos, want in args.items():
        assert _same(got[pos], want), "%s: argument %d is %r, expected %r" % (symbol, pos, got[pos], want)
    for pos, fields in cfgs:
        for name, want in fields.items():
            assert functools.reduce(getattr, name.split("."), got[pos]) == want, (symbol, pos, name)
    if callable(result):
        assert result(r)
    elif result is not None:
        assert sorted(r) == sorted(result)
        for key, want in result.items():
            if want is None:
                assert r[key] is None, key
            elif want in (list, bool):
                assert isinstance(r[key], (want, np.bool_)) and (want is bool or len(r[key]) == 2), key
            else:
                assert (r[key].dtype, r[key].shape) == (np.dtype(want[0]), want[1]), key


@pytest.mark.parametrize("case", sorted(c for c in CASES if CASES[c][6]))
def test_limit_code_is_a_flag_only_when_allowed(standin, case):
    kind, call = CASES[case][:2]
    standin.rc = _lib.ELIMIT
    r = call(make(kind, standin), allow_limit=True)
    if isinstance(r, dict):
        assert r["limit"] is True or r["limit"] == np.True_
    with pytest.raises(_lib.FuelmiError):
        call(make(kind, standin))
    standin.rc = 0
    r = call(make(kind, standin), allow_limit=True)
    if isinstance(r, dict):
        assert not r["limit"]


@pytest.mark.parametrize("case", sorted(CASES))
def test_any_other_code_raises(standin, case):
    kind, call = CASES[case][:2]
    standin.rc = _lib.EINVAL
    with pytest.raises(_lib.FuelmiError):
        call(make(kind, standin))


def test_views_and_copies(standin):
    """solve_quadratic's ctrl entries and adjust_trajs' named columns are views of the arrays C wrote; ragged lists are
    copies"""
    m = make("map", standin)
    o = m.solve_quadratic([A, B], 0.5)
    assert [c.shape for c in o["ctrl"]] == [(5, 3), (7, 3)] and all(np.shares_memory(c, o["ctrl_out"]) for c in o["ctrl"])
    o = m.adjust_trajs([A, B], 0.5)
    assert np.shares_memory(o["status"], o["info"]) and np.shares_memory(o["jerk"], o["metrics"])
    o = m.goal_paths(A[:2], B[:2], max_way_points=4)
    assert all(w.base is None for w in o["way"])


def test_a_missing_spline_source_is_refused(standin):
    m = make("map", standin)
    for call in (lambda **k: m.check_trajs([A, B], t_now=0.0, **k), lambda **k: m.plan_yaws([A, B], start_yaw=SY, **k),
                 lambda **k: m.sampleTrajs([A, B], t=T, **k)):
        with pytest.raises(ValueError):
            call(knot_span=None)
        with pytest.raises(ValueError):
            call(knot_span=0.5, knots=[KA, KB])
        with pytest.raises(ValueError):
            call(knot_span=None, knots=[KA])
    assert not standin.calls
