"""Python host mirror of the reference's C++ class interfaces over the libfuelmi C-ABI.

The production host layer is the C++ facade in fuel_amd/facade/ (same class names and
signatures as the reference).  These thin classes exist so tests and bench.py read like calls
into the reference: SDFMap (plan_env/include/plan_env/sdf_map.h:27-84), EDTEnvironment
(plan_env/include/plan_env/edt_environment.h:38-43), FrontierFinder
(active_perception/include/active_perception/frontier_finder.h:53-80) and BsplineOptimizer
(bspline_opt/include/bspline_opt/bspline_optimizer.h:36-59).  Everything computes on the GPU;
numpy arrays are only the host-side views the reference exposes (occupancy_buffer_ etc.).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (BsplineBatch, BsplineCfg, CloudCfg, ColRangeCfg, FrontierCfg, GainCfg, GoalCfg, KinoCfg, LocalSegCfg, MapCfg, MapInfo, PathCfg, QuadCfg, RefineCfg, RenderCfg, TopoCfg, TrajAdjCfg, TrajChkCfg, TrajSmpCfg, TspCfg,  # noqa: F401
                   WptrajCfg, YawCfg, YawPathCfg, check, lib)
# (_dp and _ip are also what the per-stage timing scripts build their argument lists with)
from ._pack import dp as _dp, ip as _ip, limited as _limited, outputs as _outputs, pack as _pack, per_problem as _per_problem
from ._pack import plan_query as _plan_query, ptr as _ptr, weights as _weights

# exploration.launch / algorithm.xml defaults (exploration_manager/launch/algorithm.xml:33-59,170-181)
DEFAULT_MAP = dict(resolution=0.1, ground_height=-1.0, obstacles_inflation=0.199,
                   local_bound_inflate=0.5, default_dist=0.0, optimistic=0, signed_dist=0,
                   p_hit=0.65, p_miss=0.35, p_min=0.12, p_max=0.90, p_occ=0.80,
                   max_ray_length=4.5, virtual_ceil_height=-10.0)
DEFAULT_BSPLINE = dict(ld_smooth=20.0, ld_dist=10.0, ld_feasi=2.0, ld_start=100.0, ld_end=0.5,
                       ld_guide=1.5, ld_waypt=0.3, ld_view=0.0, ld_time=1.0, dist0=0.7,
                       max_vel=2.0, max_acc=2.0, wnl=1.0, dlmin=0.0, bspline_degree=3)

SMOOTHNESS, DISTANCE, FEASIBILITY, START, END, GUIDE, WAYPOINTS, VIEWCONS, MINTIME = \
    (1 << k for k in range(9))
GUIDE_PHASE = SMOOTHNESS | GUIDE | START | END
NORMAL_PHASE = SMOOTHNESS | DISTANCE | FEASIBILITY | START | END
_I, _D = np.int32, np.float64


def _pack_waypoints(ways, vels, accs, max_vel, ctrl_pt_dist, min_seg, seg_num, max_way_points, max_samples):
    """lists of [k, 3] way-point arrays -> (n_way [n], way [n, max_way_points, 3], vel [n, 3], acc [n, 3], WptrajCfg)"""
    n_way, way, maxw = _pack(ways, max_way_points, 3, floor=3)
    vel = np.ascontiguousarray(vels, dtype=np.float64).reshape(len(n_way), 3)
    acc = np.ascontiguousarray(accs, dtype=np.float64).reshape(len(n_way), 3)
    c = WptrajCfg(float(max_vel), float(ctrl_pt_dist), int(min_seg), int(seg_num), maxw, int(max_samples))
    return n_way, way, vel, acc, c


def yaw_cfg(mode=0, pos_degree=3, max_ctrl=4, max_seg=None, seg_num=12, lookfwd=True, relax_time=1.0, forward_t=2.0,
            dt_target=0.3, end_back=0.1):
    """fuelmi_yaw_cfg with planYawExplore's / planYaw's constants; max_seg defaults to seg_num (EXPLORE) or the limit"""
    if max_seg is None:
        max_seg = seg_num if mode == _lib.YAW_EXPLORE else _lib.YAW_MAX_SEG
    return YawCfg(int(mode), int(pos_degree), int(max_ctrl), int(max_seg), int(seg_num), 1 if lookfwd else 0,
                  float(relax_time), float(forward_t), float(dt_target), float(end_back))


def quad_plan(cost_function=SMOOTHNESS | GUIDE | START | END, dim=3, max_ctrl=4, end_n=3, max_waypt=0, bounds=False):
    """(lanes per problem, LDS bytes, largest max_ctrl accepted) of the quadratic solve's kernel (fuelmi_quad_plan); host
    only"""
    return _plan_query(lib().fuelmi_quad_plan, 3, QuadCfg(int(cost_function), int(dim), int(max_ctrl), int(end_n),
                                                          int(max_waypt), 1 if bounds else 0))


def kino_cfg(max_tau=0.8, init_max_tau=1.0, max_vel=2.25, max_acc=2.0, w_time=10.0, horizon=5.0, resolution=0.025,
             lambda_heu=10.0, res=1 / 2.0, time_res=1 / 1.0, time_res_init=1 / 20.0, ts=0.45 / 2.0, allocate_num=100000,
             check_num=10, optimistic=False, min_seg=8, seg_num=0, max_path_nodes=64, max_samples=256):
    """fuelmi_kino_cfg with algorithm.xml's search/* values (max_vel includes vel_margin) and search()'s constants"""
    return KinoCfg(float(max_tau), float(init_max_tau), float(max_vel), float(max_acc), float(w_time), float(horizon),
                   float(resolution), float(lambda_heu), float(res), float(time_res), float(time_res_init), float(ts),
                   int(allocate_num), int(check_num), 1 if optimistic else 0, int(min_seg), int(seg_num),
                   int(max_path_nodes), int(max_samples))


def topo_cfg(sample_inflate=(1.0, 3.5, 1.0), clearance=0.2, ratio_to_short=5.5, max_sample_num=2000, max_raw_path=300,
             max_raw_path2=25, reserve_num=6, max_path_points=64, max_nodes=256):
    """fuelmi_topo_cfg with topo_algorithm.xml's topo_prm/* values (plan_manage/launch/topo_algorithm.xml:110-121)"""
    return TopoCfg((C.c_double * 3)(*[float(v) for v in sample_inflate]), float(clearance), float(ratio_to_short),
                   int(max_sample_num), int(max_raw_path), int(max_raw_path2), int(reserve_num), int(max_path_points),
                   int(max_nodes))


def colrange_cfg(degree=3, max_ctrl=4, max_events=8, max_pts=_lib.TOPO_MAX_POINTS_IN, clearance=0.2):
    """fuelmi_colrange_cfg: the spline's degree, topo_prm/clearance and the strides of the event and point arrays"""
    return ColRangeCfg(int(degree), int(max_ctrl), int(max_events), int(max_pts), float(clearance))


def gain_cfg(weight_type=_lib.GAIN_UNIFORM, in_box=True, factor=4, max_yaw=1, max_ctrl=1, far=4.5, top_ang=0.56125,
             left_ang=0.69222, right_ang=0.68901, lambda1=2.0, lambda2=1.0):
    """fuelmi_gain_cfg with HeadingPlanner's constants (heading_planner.cpp:119-128, :265) and algorithm.xml's lambdas"""
    return GainCfg(int(weight_type), 1 if in_box else 0, int(factor), int(max_yaw), int(max_ctrl), float(far),
                   float(top_ang), float(left_ang), float(right_ang), float(lambda1), float(lambda2))


def yawpath_cfg(half_vert_num=3, max_layer=7, yaw_diff=5 * 3.1415926 / 180.0, max_yaw_rate=60 * 3.1415926 / 180.0, w=10.0,
                **gain):
    """fuelmi_yawpath_cfg with topo_algorithm.xml's heading_planner/* values (plan_manage/launch/topo_algorithm.xml:151-157);
    gain: the fields of gain_cfg(), NON_UNIFORM unless said otherwise as in that file"""
    gain.setdefault("weight_type", _lib.GAIN_NON_UNIFORM)
    g = gain_cfg(**dict(gain, max_yaw=2 * int(half_vert_num) + 1))
    return YawPathCfg(g, int(half_vert_num), int(max_layer), float(yaw_diff), float(max_yaw_rate), float(w))


def yawpath_plan(cfg=None):
    """host only: the shape of the gain and search kernels for a YawPathCfg (fuelmi_yawpath_plan)"""
    return _plan_query(lib().fuelmi_yawpath_plan, 10, cfg if cfg is not None else yawpath_cfg(),
                       names=("lanes", "lds_bytes", "groups_per_workgroup", "max_cells", "max_yaw", "max_ctrl", "search_lanes",
                              "search_lds_bytes", "search_problems_per_workgroup", "max_layer"))


def _spline(ctrl, max_ctrl, floor=4, cols=3):
    """a list of [n_ctrl, cols] control-point arrays as (n, n_ctrl [n], ctrl [n, max_ctrl, cols], max_ctrl)"""
    n_ctrl, arr, maxc = _pack(ctrl, max_ctrl, cols, floor=floor)
    return len(n_ctrl), n_ctrl, arr, maxc


def _pack_localseg(states, problems, degree, max_seg, max_ctrl):
    """The host arrays fuelmi_map_local_segments and the batch loader share: (LocalSegCfg without max_points, n_traj,
    the state arrays, n_prob, the problem arrays).  A state is a dict: seg_times [S], coef [S, 3, 6], global_duration,
    and -- all optional, as setGlobalTraj leaves them -- local_ctrl [n, 3] with local_knot_span, local_ts (-1),
    local_te (-1), time_change (0), last_time_inc (0).  A problem is (state index, mode, start_t, arg0, arg1)."""
    n_seg, a_T, ms = _pack([st["seg_times"] for st in states], max_seg, 0, floor=1)
    n_cf, a_cf, _ = _pack([st["coef"] for st in states], ms, (3, 6))
    for i in np.flatnonzero(n_cf != n_seg):
        raise ValueError("local segments: state %d has %d segment times and %d coefficient blocks" % (i, n_seg[i], n_cf[i]))
    n_loc, a_lc, mc = _pack([st.get("local_ctrl") for st in states], max_ctrl, 3, floor=int(degree) + 1)

    def col(key, default):
        return np.array([float(st.get(key, default)) for st in states], dtype=np.float64)
    st_arr = [n_seg, a_T, a_cf, col("global_duration", 0.0), n_loc, a_lc, col("local_knot_span", 0.0), col("local_ts", -1.0),
              col("local_te", -1.0), col("time_change", 0.0), col("last_time_inc", 0.0)]
    pr = [tuple(q) for q in problems]
    pr_arr = [np.array([int(q[0]) for q in pr], dtype=np.int32), np.array([int(q[1]) for q in pr], dtype=np.int32)] + \
        [np.array([float(q[k]) for q in pr], dtype=np.float64) for k in (2, 3, 4)]
    return LocalSegCfg(int(degree), ms, mc, 0), len(states), st_arr, len(pr), pr_arr


def traj_check_cfg(degree=3, max_ctrl=4, step=0.02, max_radius=6.0):
    """fuelmi_trajchk_cfg with checkTrajCollision's literals (planner_manager.cpp:102, 104)"""
    return TrajChkCfg(int(degree), int(max_ctrl), float(step), float(max_radius))


def traj_sample_cfg(mode=_lib.TRAJSMP_COMMAND, degree=3, yaw_degree=3, max_ctrl=4, max_yaw_ctrl=0, max_t=0):
    """fuelmi_trajsmp_cfg: cmdCallback (TRAJSMP_COMMAND) or the FSM's replan state (TRAJSMP_STATE); planYawExplore's yaw
    degree"""
    return TrajSmpCfg(int(mode), int(degree), int(yaw_degree), int(max_ctrl), int(max_yaw_ctrl), int(max_t))


def _trajsmp_io(n, t, yaw_ctrl, yaw_dt, t_stop, flight, max_yaw_ctrl, max_t):
    """The host arrays both sampling calls share: (arguments from n_yaw_ctrl on, the result dict, the two strides).  t
    and yaw_ctrl are one 1-D array per problem (yaw_ctrl None, or None for a problem: no yaw spline)."""
    n_t, tt, maxt = _pack(t, max_t, 0)
    assert len(n_t) == n
    n_yaw = yaw = ydt = None
    maxy = int(max_yaw_ctrl) if max_yaw_ctrl is not None else 0
    if yaw_ctrl is not None:
        n_yaw, yaw, maxy = _pack(yaw_ctrl, max_yaw_ctrl, 0)
        assert len(n_yaw) == n
        ydt = _per_problem(yaw_dt, n)
    stop = _per_problem(t_stop, n, optional=True)
    fl = None if flight is None else np.array(flight, dtype=np.float64).reshape(n, 8)
    mt = max(maxt, 0)
    o, out = _outputs(n, [("status", _I, (mt,)), ("pos vel acc jerk", _D, (mt, 3)), ("yaw yawdot yawddot", _D, (mt,)),
                          ("duration", _D, ())])
    o.update(flight=fl, n_t=n_t)
    return (_ip(n_yaw), _dp(yaw), _dp(ydt), _dp(stop), _ip(n_t), _dp(tt), *out, _dp(fl)), o, maxy, maxt


def traj_adjust_cfg(ops=0, degree=3, max_ctrl=4, max_samples=0, realloc_iters=3, n_group=0, limit_vel=2.0, limit_acc=2.0,
                    limit_ratio=1.1, lengthen_cap=1.01, length_res=0.01, stat_step=0.01):
    """fuelmi_trajadj_cfg with the reference's values: setPhysicalLimits' limit_ratio, both callers' lengthenTime cap,
    the three passes of the reallocation loop, getMeanAndMaxVel's step"""
    return TrajAdjCfg(int(ops), int(degree), int(max_ctrl), int(max_samples), int(realloc_iters), int(n_group),
                      float(limit_vel), float(limit_acc), float(limit_ratio), float(lengthen_cap), float(length_res),
                      float(stat_step))


def _knot_source(n, ks, knot_span, knots):
    """What the calls that take a position spline's knot span or its whole knot vectors share: (span [n], "") or (knots
    [n, ks], "_knots"), the array and the suffix of the entry that takes it.  knots is one 1-D array per problem, as
    adjust_trajs takes knots_in and returns knots_out; exactly one of the two is given."""
    if (knots is None) == (knot_span is None):
        raise ValueError("give either knot_span or knots")
    if knots is None:
        return _per_problem(knot_span, n), ""
    if len(knots) != n:
        raise ValueError("knots: one array per problem")
    return _pack(knots, ks, 0)[1], "_knots"


def _trajadj_io(n, n_ctrl, degree, maxc, knots_in, ratio_in, group, ops, max_samples, n_group):
    """The host arrays both adjustment calls share: (arguments from knots_in on, the result dict, max_samples, n_group).
    knots_in is one 1-D array per problem."""
    ks = maxc + degree + 1
    kin = None if knots_in is None else _pack(knots_in, ks, 0, n=n)[1]
    rin = _per_problem(ratio_in, n, optional=True)
    grp = best = None
    if ops & _lib.TRAJADJ_SELECT:
        grp = _per_problem(0 if group is None else group, n, np.int32)
        if n_group is None:
            n_group = int(grp.max()) + 1 if n else 1
        best = np.full(max(int(n_group), 0), -1, dtype=np.int32)
    if ops & _lib.TRAJADJ_RESAMPLE and max_samples is None:
        max_samples = maxc - degree + 2
    o, out = _outputs(n, [("info", _I, (_lib.TRAJADJ_NI,)), ("metrics", _D, (_lib.TRAJADJ_NM,)), ("knots_out", _D, (ks,)),
                          ("samples", _D, (max(int(max_samples or 0), 0), 3), ops & _lib.TRAJADJ_RESAMPLE)])
    o.update(best=best, n_ctrl=n_ctrl)
    return (_dp(kin), _dp(rin), _ip(grp), *out, _ip(best)), o, int(max_samples or 0), int(n_group or 0)


def _trajadj_named(o):
    """the columns of info and metrics under their names (views)"""
    for k, name in enumerate(_lib.TRAJADJ_INFO):
        o[name] = o["info"][:, k]
    for k, name in enumerate(_lib.TRAJADJ_METRICS):
        o[name] = o["metrics"][:, k]
    return o


def cloud_plan(dims, lo, hi):
    """The geometry fuelmi_map_extract_cloud's kernels use for the inclusive box lo..hi of a dims grid
    (fuelmi_cloud_plan, host only).  Raises FuelmiError for a box that leaves the map."""
    return _plan_query(lib().fuelmi_cloud_plan, 8, _i3(dims), _i3(lo), _i3(hi),
                       names=("items_per_line", "lines", "items_per_workgroup", "workgroups", "scan_width", "scan_rounds",
                              "scratch_bytes", "voxels"))


# --- the stages an SDFMap runs on splines from the host and a BsplineDeviceProblem on its own: each body builds the inputs
# and results both share; `call` is the C entry with the spline source in front, taking the rest of the arguments ---
def _check_trajs(n, t_now, allow_limit, call):
    now = _per_problem(t_now, n)
    o, out = _outputs(n, [("status safe", _I, ()), ("distance", _D, ()), ("n_samples hit_index", _I, ()), ("hit_t", _D, ()),
                          ("hit_pos", _D, (3,)), ("end_reason", _I, ()), ("duration", _D, ())])
    o["limit"] = _limited(call(_dp(now), *out), allow_limit)
    return o


def _plan_yaws(n, yc, start_yaw, end_yaw, derivs, allow_limit, call):
    sy = np.ascontiguousarray(start_yaw, dtype=np.float64).reshape(n, 3)
    ey = _per_problem(end_yaw, n, optional=True)
    ms = max(int(yc.max_seg), 0)
    o, out = _outputs(n, [("status", _I, ()), ("duration", _D, ()), ("seg_num", _I, ()), ("dt_yaw", _D, ()),
                          ("yaw_ctrl", _D, (ms + 3,)), ("n_waypt", _I, ()), ("waypts", _D, (ms,)), ("end_yaw cost", _D, ()),
                          ("yawdot_ctrl", _D, (ms + 2,), derivs), ("yawddot_ctrl", _D, (ms + 1,), derivs)])
    o["limit"] = _limited(call(C.byref(yc), _dp(sy), _dp(ey), *out), allow_limit)
    return o


def _solve_quadratic(n, qc, call):
    o, out = _outputs(n, [("status", _I, ()), ("ctrl_out", _D, (max(qc.max_ctrl, 0), qc.dim)), ("cost pt_dist", _D, ())])
    check(call(C.byref(qc), *out))
    return o


def _kino(points, cfg, n, table, allow_limit, call):
    """start, velocity, acceleration, goal, goal velocity [n, 3] each (n None: as many as there are starts) and the fields
    of kino_cfg() -> (the KinoCfg, the results of table(cfg), the limit flag); call(cfg, n, the five arrays, the results)"""
    kc = kino_cfg(**cfg)
    arr = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 3) for a in points]
    if n is None:
        n = len(arr[0])
        assert all(len(a) == n for a in arr)
    elif any(len(a) != n for a in arr):
        raise ValueError("load_kino: one problem per candidate")
    o, out = _outputs(n, table(kc))
    return kc, o, _limited(call(C.byref(kc), n, *[_dp(a) for a in arr], *out), allow_limit)


def _d3(v):
    return (C.c_double * 3)(*[float(x) for x in v])


def _i3(v):
    return (C.c_int * 3)(*[int(x) for x in v])


class SDFMap:
    """fast_planner::SDFMap with the grid resident in HBM."""
    UNKNOWN, FREE, OCCUPIED = 0, 1, 2
    ESDF_AUTO, ESDF_PLAIN, ESDF_FAR, ESDF_PLAIN32 = -1, 0, 1, 2
    INFLATE_AUTO, INFLATE_FUSED, INFLATE_FACTORED = -1, 0, 1
    # family every newly created map is pinned to (None: the library's per-update choice); the parity tests run each
    # ESDF test once per family by setting this
    default_esdf_family = None

    def __init__(self, map_size, box_min=None, box_max=None, device=0, **params):
        self.L = lib()
        p = dict(DEFAULT_MAP)
        p.update(params)
        c = MapCfg()
        for k, v in p.items():
            setattr(c, k, v)
        org = (-map_size[0] / 2.0, -map_size[1] / 2.0, p["ground_height"])
        bmin = box_min if box_min is not None else org
        bmax = box_max if box_max is not None else tuple(org[i] + map_size[i] for i in range(3))
        for i in range(3):
            c.map_size[i] = float(map_size[i])
            c.box_min[i] = float(bmin[i])
            c.box_max[i] = float(bmax[i])
        c.device = device
        self.cfg = c
        h = C.c_void_p()
        check(self.L.fuelmi_map_create(C.byref(c), C.byref(h)))
        self.h = h
        info = MapInfo()
        check(self.L.fuelmi_map_get_info(self.h, C.byref(info)))
        self.info = info
        self.nvox = tuple(info.voxel_num)
        self.N = self.nvox[0] * self.nvox[1] * self.nvox[2]
        self.origin = np.array(info.origin)
        self.res = c.resolution
        if SDFMap.default_esdf_family is not None:
            self.setEsdfFamily(SDFMap.default_esdf_family)

    def setEsdfFamily(self, family):
        """pin the ESDF kernel family (ESDF_AUTO / _PLAIN / _FAR / _PLAIN32); all are exact"""
        check(self.L.fuelmi_map_set_esdf_family(self.h, int(family)))

    def lastEsdfFamily(self):
        """family the z/y pass of the last updateESDF3d ran"""
        return self.L.fuelmi_map_last_esdf_family(self.h)

    # fuelmi_map_esdf_plan's FUELMI_ESDF_K_*: kernel, number of template arguments, which of them is the bool FAR
    _ESDF_KERNELS = (("k_esdf_zy", 1, None), ("k_esdf_zy4", 2, 1), ("k_esdf_zy_pk2", 3, None), ("k_esdf_x", 2, None),
                     ("k_esdf_x4", 3, 2), ("k_esdf_x_pk2", 1, None))

    @staticmethod
    def esdfPlan(dims, lo, hi, family, optimistic=False, signed_dist=False):
        """The launches updateESDF3d issues for the box [lo, hi] of a dims grid with `family` (ESDF_PLAIN / _FAR /
        _PLAIN32; fuelmi_map_esdf_plan, host only): {"family": what lastEsdfFamily() then reports, "launches": [{"kernel",
        "grid", "block", "lds", "ZC", "nzc", "z0a"}, ...] in order z/y+, x+ (, z/y-, x- for signed maps)}.  Raises
        FuelmiError for a box the update refuses."""
        flags = (1 if optimistic else 0) | (2 if signed_dist else 0)
        out = _plan_query(lib().fuelmi_map_esdf_plan, 42, _i3(dims), _i3(lo), _i3(hi), int(family), flags)
        launches = []
        for i in range(out[0]):
            k, a0, a1, a2, grid, block, lds, zc, nzc, z0a = out[2 + 10 * i:12 + 10 * i]
            kname, nt, far = SDFMap._ESDF_KERNELS[k]
            targs = [("true" if a else "false") if j == far else str(a) for j, a in enumerate((a0, a1, a2)[:nt])]
            name = "%s<%s>" % (kname, ", ".join(targs))
            launches.append({"kernel": name, "grid": grid, "block": block, "lds": lds, "ZC": zc, "nzc": nzc, "z0a": z0a})
        return {"family": out[1], "launches": launches}

    @staticmethod
    def insertPlan():
        """The geometry the fusion kernels are compiled with (fuelmi_map_insert_plan, host only): lanes that share a ray
        walk, point slots per ray-walk and per classify workgroup, voxel extents of a ray workgroup's LDS miss cube."""
        out = _plan_query(lib().fuelmi_map_insert_plan, 8)
        return {"lanes_per_ray": out[0], "ray_slots": out[1], "classify_slots": out[2], "cube": (out[3], out[4], out[5])}

    def lastInflateKernel(self):
        """0: the fused inflation kernel ran in the last clearAndInflateLocalMap, 1: the factored pair"""
        return self.L.fuelmi_map_last_inflate_kernel(self.h)

    def setInflateKernel(self, kernel):
        """pin the inflation kernels (INFLATE_AUTO / _FUSED / _FACTORED); both forms compute the same bits.  FUSED exists
        for an inflation step of 2 only: FuelmiError (FUELMI_EINVAL) on a map with another step"""
        check(self.L.fuelmi_map_set_inflate_kernel(self.h, int(kernel)))

    @staticmethod
    def inflatePlan(dims, step, lo, hi, kernel=-1):
        """The word ranges and launches clearAndInflateLocalMap uses for the box [lo, hi] of a dims grid whose
        inflate_step is `step` under the pin `kernel` (fuelmi_map_inflate_plan, host only).  "grids": workgroups of 256
        of the fused kernel, the masking pass, the y/z pass and the x pass; 0 where a kernel does not run."""
        v = _plan_query(lib().fuelmi_map_inflate_plan, 16, _i3(dims), int(step), _i3(lo), _i3(hi), int(kernel))
        return {"kernel": v[0], "margin_words": v[1], "W": v[2], "out": (v[3], v[4]), "t": (v[5], v[6]), "s": (v[7], v[8]),
                "whole": bool(v[9]), "lds": v[10],
                "grids": {"fused": v[11], "box_and": v[12], "yz": v[13], "x": v[14]}}

    def close(self):
        if getattr(self, "h", None):
            self.L.fuelmi_map_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- reference API ---
    def inputPointCloud(self, points, camera_pos):
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        check(self.L.fuelmi_map_input_points(self.h, pts.ctypes.data, 12, len(pts), _d3(camera_pos)))

    @staticmethod
    def depthConfig(fx=387.229248046875, fy=387.229248046875, cx=321.04638671875, cy=243.44969177246094,
                    maxdist=5.0, mindist=0.2, margin=2, scaling=1000.0, skip=2):
        """map_ros/* parameters (exploration.launch:38-41, algorithm.xml:62-69)."""
        return _lib.DepthCfg(fx, fy, cx, cy, maxdist, mindist, margin, scaling, skip)

    def inputDepthImage(self, depth, camera_pos, camera_q_wxyz, cfg=None):
        """MapROS::depthPoseCallback's projection + fusion (map_ros.cpp:121-150,176-215) on the device.
        Returns proj_points_cnt."""
        img = np.ascontiguousarray(depth, dtype=np.uint16)
        cfg = cfg or self.depthConfig()
        n = C.c_int(0)
        q = (C.c_double * 4)(*[float(v) for v in camera_q_wxyz])
        check(self.L.fuelmi_map_input_depth(self.h, img.ctypes.data, img.shape[0], img.shape[1], C.byref(cfg),
                                            _d3(camera_pos), q, C.byref(n)))
        return n.value

    def inputDepthImageAt(self, ptr, rows, cols, camera_pos, camera_q_wxyz, cfg=None):
        """inputDepthImage for a frame addressed by a raw pointer: device memory (e.g. a torch CUDA tensor's
        data_ptr()), pinned / registered host memory, or pageable host memory.  The first two are read in place."""
        cfg = cfg or self.depthConfig()
        n = C.c_int(0)
        q = (C.c_double * 4)(*[float(v) for v in camera_q_wxyz])
        check(self.L.fuelmi_map_input_depth(self.h, C.c_void_p(int(ptr)), int(rows), int(cols), C.byref(cfg),
                                            _d3(camera_pos), q, C.byref(n)))
        return n.value

    def projectDepthImage(self, depth, camera_pos, camera_q_wxyz, cfg=None):
        """MapROS::proessDepthImage only: the projected world points (float32 [n,3])."""
        img = np.ascontiguousarray(depth, dtype=np.uint16)
        cfg = cfg or self.depthConfig()
        cap = img.shape[0] * img.shape[1]
        out = np.empty((cap, 3), dtype=np.float32)
        n = C.c_int(0)
        q = (C.c_double * 4)(*[float(v) for v in camera_q_wxyz])
        check(self.L.fuelmi_map_project_depth(self.h, img.ctypes.data, img.shape[0], img.shape[1], C.byref(cfg),
                                              _d3(camera_pos), q, out.ctypes.data, cap, C.byref(n)))
        return out[:n.value].copy()

    def clearAndInflateLocalMap(self):
        check(self.L.fuelmi_map_inflate_local(self.h))

    def updateESDF3d(self):
        check(self.L.fuelmi_map_update_esdf(self.h))

    def resetBuffer(self, lo=None, hi=None):
        if lo is None:
            check(self.L.fuelmi_map_reset_buffer_all(self.h))
        else:
            check(self.L.fuelmi_map_reset_buffer(self.h, _d3(lo), _d3(hi)))

    def setOccupied(self, pos, occ=1):
        pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
        check(self.L.fuelmi_map_set_occupied(self.h, _dp(pos), len(pos), occ))

    def getDistWithGrad(self, pos):
        pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
        d = np.empty(len(pos))
        g = np.empty((len(pos), 3))
        check(self.L.fuelmi_map_dist_grad(self.h, _dp(pos), len(pos), _dp(d), _dp(g)))
        return d, g

    def getDistance(self, pos):
        pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
        d = np.empty(len(pos))
        check(self.L.fuelmi_map_coarse_dist(self.h, _dp(pos), len(pos), _dp(d)))
        return d

    def getOccupancy(self, idx):
        idx = np.ascontiguousarray(idx, dtype=np.int32).reshape(-1, 3)
        o = np.empty(len(idx), dtype=np.int32)
        i = np.empty(len(idx), dtype=np.int32)
        check(self.L.fuelmi_map_query_state(self.h, _ip(idx), len(idx), _ip(o), _ip(i)))
        return o, i

    def getUpdatedBox(self, reset=False):
        a, b = (C.c_double * 3)(), (C.c_double * 3)()
        check(self.L.fuelmi_map_get_updated_box(self.h, a, b, int(reset)))
        return np.array(a), np.array(b)

    def setUpdatedBox(self, lo, hi):
        check(self.L.fuelmi_map_set_updated_box(self.h, _d3(lo), _d3(hi)))

    def getLocalBound(self):
        a, b = (C.c_int * 3)(), (C.c_int * 3)()
        check(self.L.fuelmi_map_get_local_bound(self.h, a, b))
        return tuple(a), tuple(b)

    def setLocalBound(self, lo, hi):
        check(self.L.fuelmi_map_set_local_bound(self.h, _i3(lo), _i3(hi)))

    def getBoxIndex(self):
        return tuple(self.info.box_min), tuple(self.info.box_max)

    # --- device <-> host ---
    def uploadOccupancy(self, occ):
        occ = np.ascontiguousarray(occ, dtype=np.float64).reshape(-1)
        assert occ.size == self.N
        check(self.L.fuelmi_map_upload_occupancy(self.h, _dp(occ)))

    def syncHost(self, occupancy=False, inflate=False, distance=False, box=None):
        """Refresh host mirrors (occupancy_buffer_, occupancy_buffer_inflate_, distance_buffer_)."""
        out = {}
        o = np.zeros(self.N) if occupancy else None
        i = np.zeros(self.N, dtype=np.int8) if inflate else None
        d = np.zeros(self.N) if distance else None
        bmin = _i3(box[0]) if box else None
        bmax = _i3(box[1]) if box else None
        check(self.L.fuelmi_map_sync_host(self.h, bmin, bmax, _dp(o),
                                          None if i is None else i.ctypes.data, _dp(d)))
        if occupancy:
            out["occupancy"] = o
        if inflate:
            out["inflate"] = i
        if distance:
            out["distance"] = d
        return out

    def synchronize(self):
        check(self.L.fuelmi_map_synchronize(self.h))

    # --- the scans of MapROS::publishMapLocal / publishMapAll / publishUnknown (include/fuelmi.h
    # fuelmi_map_extract_cloud) ---
    CLOUD_OCCUPIED, CLOUD_UNKNOWN, CLOUD_KNOWN, CLOUD_INFLATED = range(4)

    def _cloud_cfg(self, kind, lo, hi, z_low, z_high):
        return CloudCfg(int(kind), _i3(lo), _i3(hi), float(z_low), float(z_high))

    def count_voxels(self, kind, lo, hi, z_low=-np.inf, z_high=np.inf):
        """Voxels of the inclusive box lo..hi that extract_cloud would return (publishMapAll's known-voxel count: kind
        CLOUD_KNOWN, no bounds).  Nothing but the count crosses to the host."""
        n = C.c_int(-1)
        check(self.L.fuelmi_map_extract_cloud(self.h, C.byref(self._cloud_cfg(kind, lo, hi, z_low, z_high)), None, 0,
                                              C.byref(n)))
        return n.value

    def extract_cloud(self, kind, lo, hi, z_low=-np.inf, z_high=np.inf, cap=None):
        """The voxel centres (float32 [n, 3], x outermost, then y, then z) of the box's voxels of `kind` between the two
        truncation heights.  cap=None: counts first, then fetches exactly.  With a cap: (the first min(n_total, cap)
        points, n_total)."""
        cfg = self._cloud_cfg(kind, lo, hi, z_low, z_high)
        n = C.c_int(-1)
        if cap is None:
            k = self.count_voxels(kind, lo, hi, z_low, z_high)
            out = np.empty((k, 3), dtype=np.float32)
            if k:
                check(self.L.fuelmi_map_extract_cloud(self.h, C.byref(cfg), out.ctypes.data, k, C.byref(n)))
                assert n.value == k
            return out
        cap = int(cap)
        out = np.empty((max(cap, 0), 3), dtype=np.float32)
        rc = self.L.fuelmi_map_extract_cloud(self.h, C.byref(cfg), out.ctypes.data if cap > 0 else None, cap, C.byref(n))
        _limited(rc, True)
        return out[:min(n.value, cap)].copy(), n.value

    def cloud_times(self):
        """device milliseconds of the last extract_cloud / count_voxels: (count + scan, write, copy to the host)"""
        ms = np.zeros(3)
        check(self.L.fuelmi_map_cloud_times(self.h, _dp(ms)))
        return tuple(ms)

    # --- ViewNode::searchPath for a batch of pairs (include/fuelmi.h fuelmi_map_path_costs) ---
    PATH_LINE, PATH_LATTICE, PATH_NONE = 0, 1, 2

    def path_costs(self, p1, p2, res=0.4, edge_step=0.1, no_path_cost=1000.0, max_points=256):
        """(length [n], kind [n], paths: list of [k, 3] arrays, or None when max_points is 0).  A path longer than
        max_points raises FuelmiError (FUELMI_ELIMIT)."""
        p1 = np.ascontiguousarray(p1, dtype=np.float64).reshape(-1, 3)
        p2 = np.ascontiguousarray(p2, dtype=np.float64).reshape(-1, 3)
        assert len(p1) == len(p2)
        n = len(p1)
        c = PathCfg(float(res), float(edge_step), float(no_path_cost), int(max_points))
        length = np.empty(n)
        kind = np.empty(n, dtype=np.int32)
        plen = np.empty(n, dtype=np.int32)
        buf = np.empty((n, max_points, 3)) if max_points > 0 else None
        check(self.L.fuelmi_map_path_costs(self.h, C.byref(c), n, _dp(p1), _dp(p2), _dp(length), _ip(kind), _ip(plen),
                                           _dp(buf)))
        paths = None if buf is None else [buf[i, :plen[i]].copy() for i in range(n)]
        return length, kind, paths

    def path_stats(self):
        """of the last path_costs call: relaxation launches in all, the most of one chunk, lattice sources, chunks"""
        st = np.zeros(4, dtype=np.int32)
        check(self.L.fuelmi_map_path_stats(self.h, _ip(st)))
        return dict(zip(("launches", "max_chunk_launches", "sources", "chunks"), (int(v) for v in st)))

    # --- FastExplorationManager::refineLocalTour for a batch of problems (include/fuelmi.h fuelmi_map_refine_tours) ---
    def refine_tours(self, problems, vm, yd, w_dir, res=0.4, edge_step=0.1, no_path_cost=1000.0, tour_res=0.0,
                     max_tour_points=1024, last_argmin=False):
        """problems: list of (pos [3], vel [3], yaw, layers), layers a list of [k, 4] arrays (x, y, z, yaw).
        Returns (choices: list of int arrays, one index per layer, -1 when unreached; costs [B], +inf when unreached;
        tours: list of [k, 3] arrays when tour_res > 0, else None).  A polyline longer than max_tour_points raises
        FuelmiError (FUELMI_ELIMIT)."""
        B = len(problems)
        start = np.zeros((B, 7))
        layer_ptr, node_ptr, nodes = [0], [0], []
        for b, (pos, vel, yaw, layers) in enumerate(problems):
            start[b, :3], start[b, 3:6], start[b, 6] = pos, vel, yaw
            for layer in layers:
                layer = np.asarray(layer, dtype=np.float64).reshape(-1, 4)
                nodes.append(layer)
                node_ptr.append(node_ptr[-1] + len(layer))
            layer_ptr.append(layer_ptr[-1] + len(layers))
        nodes = np.ascontiguousarray(np.concatenate(nodes) if nodes else np.zeros((0, 4)))
        layer_ptr = np.array(layer_ptr, dtype=np.int32)
        node_ptr = np.array(node_ptr, dtype=np.int32)
        c = RefineCfg(PathCfg(float(res), float(edge_step), float(no_path_cost), 0), float(vm), float(yd), float(w_dir),
                      float(tour_res), int(max_tour_points), _lib.REFINE_LAST_ARGMIN if last_argmin else 0)
        choice = np.empty(layer_ptr[-1], dtype=np.int32)
        cost = np.empty(B)
        tlen = np.zeros(B, dtype=np.int32) if tour_res > 0 else None
        txyz = np.zeros((B, max_tour_points, 3)) if tour_res > 0 else None
        check(self.L.fuelmi_map_refine_tours(self.h, C.byref(c), B, _dp(start), _ip(layer_ptr), _ip(node_ptr),
                                             _dp(nodes), _ip(choice), _dp(cost), _ip(tlen), _dp(txyz)))
        choices = [choice[layer_ptr[b]:layer_ptr[b + 1]].copy() for b in range(B)]
        tours = None if txyz is None else [txyz[b, :tlen[b]].copy() for b in range(B)]
        return choices, cost, tours

    # --- the path to the next viewpoint for a batch of problems (include/fuelmi.h fuelmi_map_goal_paths) ---
    GOAL_CLOSE, GOAL_MID, GOAL_FAR, GOAL_NO_PATH = _lib.GOAL_CLOSE, _lib.GOAL_MID, _lib.GOAL_FAR, _lib.GOAL_NO_PATH

    def goal_paths(self, starts, goals, res=0.2, edge_step=0.1, shorten_dist=3.0, end_eps=1e-3, radius_close=1.5,
                   radius_far=5.0, max_path_points=4096, max_way_points=64, raw=True, allow_limit=False):
        """Astar::search + shortenPath + the length branch of planExploreMotion per (start, goal).  Returns a dict:
        status [n] (GOAL_*; -1: the raw path did not fit), length [n] (of the shortened path, before truncation), n_way
        [n], way (list of [k, 3] arrays, at most max_way_points each), next_goal [n, 3], and with raw: raw_len [n],
        raw (list of [k, 3] arrays, empty where the path did not fit), and limit (a count exceeded its maximum).
        FUELMI_ELIMIT raises FuelmiError unless allow_limit."""
        p1 = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 3)
        p2 = np.ascontiguousarray(goals, dtype=np.float64).reshape(-1, 3)
        assert len(p1) == len(p2)
        n = len(p1)
        c = GoalCfg(PathCfg(float(res), float(edge_step), 0.0, int(max_path_points)), float(shorten_dist),
                    float(end_eps), float(radius_close), float(radius_far), int(max_way_points))
        mw, mp = max(int(max_way_points), 0), max(int(max_path_points), 0)
        out, res = _outputs(n, [("status", _I, ()), ("length", _D, ()), ("n_way", _I, ()), ("way", _D, (mw, 3)),
                                ("next_goal", _D, (3,)), ("raw_len", _I, (), raw), ("raw", _D, (mp, 3), raw)])
        out["limit"] = _limited(self.L.fuelmi_map_goal_paths(self.h, C.byref(c), n, _dp(p1), _dp(p2), *res), allow_limit)
        way, rlen, rxyz = out["way"], out.pop("raw_len"), out.pop("raw")
        out["way"] = [way[b, :min(out["n_way"][b], mw)].copy() for b in range(n)]
        if raw:
            out["raw_len"] = rlen
            out["raw"] = [rxyz[b, :rlen[b] if rlen[b] <= mp else 0].copy() for b in range(n)]
        return out

    def goal_path_times(self):
        """device milliseconds of the last goal_paths call: (the lattice run, k_goal_shorten)"""
        ms = np.zeros(2)
        check(self.L.fuelmi_map_goal_path_times(self.h, _dp(ms)))
        return float(ms[0]), float(ms[1])

    # --- the min-jerk initial trajectory through way-points (include/fuelmi.h fuelmi_map_waypoint_trajs) ---
    WPTRAJ_OK, WPTRAJ_FEW, WPTRAJ_DEGENERATE = _lib.WPTRAJ_OK, _lib.WPTRAJ_FEW, _lib.WPTRAJ_DEGENERATE

    def waypoint_trajs(self, ways, vels, accs, max_vel=2.0, ctrl_pt_dist=0.45, min_seg=8, seg_num=0, max_way_points=None,
                       max_samples=128, coef=True, allow_limit=False):
        """The first half of planExploreTraj per problem: ways is a list of [k, 3] way-point arrays (what goal_paths
        returns as "way"), vels / accs [n, 3].  Returns a dict: status [n] (WPTRAJ_*; -1: more samples than max_samples),
        duration, length, seg_num, dt, n_samples [n], samples (list of [k, 3] arrays, at most max_samples each), derivs
        [n, 4, 3] (start vel, end vel, start acc, end acc), and with coef: seg_times (list of [S]) and coef (list of
        [S, 3, 6]); limit (a sample count exceeded max_samples).  FUELMI_ELIMIT raises FuelmiError unless allow_limit."""
        n_way, way, vel, acc, c = _pack_waypoints(ways, vels, accs, max_vel, ctrl_pt_dist, min_seg, seg_num,
                                                  max_way_points, max_samples)
        n, maxs, segs = len(n_way), max(c.max_samples, 0), max(c.max_way_points - 1, 0)
        out, res = _outputs(n, [("status", _I, ()), ("duration length", _D, ()), ("seg_num", _I, ()), ("dt", _D, ()),
                                ("n_samples", _I, ()), ("samples", _D, (maxs, 3)), ("derivs", _D, (4, 3)),
                                ("seg_times", _D, (segs,), coef), ("coef", _D, (segs, 3, 6), coef)])
        out["limit"] = _limited(self.L.fuelmi_map_waypoint_trajs(self.h, C.byref(c), n, _ip(n_way), _dp(way), _dp(vel),
                                                                 _dp(acc), *res), allow_limit)
        samples, tim, cf = out["samples"], out.pop("seg_times"), out.pop("coef")
        out["samples"] = [samples[b, :min(out["n_samples"][b], maxs)].copy() for b in range(n)]
        if coef:
            live = [max(int(n_way[b]) - 1, 0) if out["status"][b] in (0, -1) else 0 for b in range(n)]
            out["seg_times"] = [tim[b, :live[b]].copy() for b in range(n)]
            out["coef"] = [cf[b, :live[b]].copy() for b in range(n)]
        return out

    @staticmethod
    def waypoint_traj_plan(max_way_points):
        """(lanes per problem, LDS bytes, largest max_way_points accepted) of the way-point kernel; host only"""
        return _plan_query(lib().fuelmi_wptraj_plan, 3, WptrajCfg(2.0, 0.45, 8, 0, int(max_way_points), 1))

    # --- the kinodynamic search of the mid-range branch (include/fuelmi.h fuelmi_map_kino_paths) ---
    KINO_REACH_HORIZON, KINO_REACH_END, KINO_NO_PATH, KINO_NEAR_END, KINO_CLOSE_GOAL = (
        _lib.KINO_REACH_HORIZON, _lib.KINO_REACH_END, _lib.KINO_NO_PATH, _lib.KINO_NEAR_END, _lib.KINO_CLOSE_GOAL)

    def kino_paths(self, starts, vels, accs, goals, goal_vels, nodes=True, allow_limit=False, **cfg):
        """KinodynamicAstar::search (init, then the retry) + getSamples per problem; cfg: the fields of kino_cfg().
        Returns a dict: status (KINO_*; -1: over max_path_nodes / max_samples), which, iter_num, use_node_num, n_nodes,
        shot, t_shot, coef [n, 3, 4], T_sum, ts, seg_num, n_samples [n], samples (list of [k, 3]), derivs [n, 4, 3], and
        with nodes: node_state (list of [k, 6]), node_input (list of [k, 3]), node_duration (list of [k]); limit.
        FUELMI_ELIMIT raises FuelmiError unless allow_limit."""
        def table(c):
            maxn, maxs = max(c.max_path_nodes, 0), max(c.max_samples, 0)
            return [("status which iter_num use_node_num n_nodes", _I, ()), ("node_state", _D, (maxn, 6), nodes),
                    ("node_input", _D, (maxn, 3), nodes), ("node_duration", _D, (maxn,), nodes), ("shot", _I, ()),
                    ("t_shot", _D, ()), ("coef", _D, (3, 4)), ("T_sum ts", _D, ()), ("seg_num n_samples", _I, ()),
                    ("samples", _D, (maxs, 3)), ("derivs", _D, (4, 3))]
        c, out, out["limit"] = _kino((starts, vels, accs, goals, goal_vels), cfg, None, table, allow_limit,
                                     lambda *a: self.L.fuelmi_map_kino_paths(self.h, *a))
        for key, count in (("samples", "n_samples"), ("node_state", "n_nodes"), ("node_input", "n_nodes"),
                           ("node_duration", "n_nodes")):
            arr = out.pop(key)
            if arr is not None:
                out[key] = [arr[b, :min(int(k), arr.shape[1])].copy() for b, k in enumerate(out[count])]
        return out

    @staticmethod
    def kino_plan(**cfg):
        """host only: dict(lanes, lds_bytes, workspace_bytes, n_init, n_regular, max_prims, max_alloc, hash_slots)"""
        return _plan_query(lib().fuelmi_kino_plan, 8, kino_cfg(**cfg), ctype=C.c_longlong,
                           names=("lanes", "lds_bytes", "workspace_bytes", "n_init", "n_regular", "max_prims", "max_alloc",
                                  "hash_slots"))

    # --- the topological path search of guided replanning (include/fuelmi.h fuelmi_map_topo_paths) ---
    TOPO_OK, TOPO_NO_PATH, TOPO_UNDEFINED = _lib.TOPO_OK, _lib.TOPO_NO_PATH, _lib.TOPO_UNDEFINED

    def topo_paths(self, starts, ends, samples, start_pts=None, end_pts=None, allow_limit=False, **cfg):
        """TopologyPRM::findTopoPaths per problem over the given sample streams (samples [n, max_sample_num, 3], raw
        numbers in [-1, 1)); start_pts / end_pts: per problem a [k, 3] array (or None); cfg: the fields of topo_cfg(),
        max_sample_num taken from `samples`.  Returns a dict: status (TOPO_*; -1: over max_nodes / max_path_points / a
        cap), counts [n, 4], events [n, 6], n_nodes [n], per problem nodes (list of (id, type, xyz, neighbour ids),
        complete only up to max_nodes), raw / filt / sel (lists of [k, 3] arrays, cut at max_path_points) with their full
        lengths raw_len / filt_len / sel_len, sel_length (pathLength of each select path); limit.
        FUELMI_ELIMIT raises FuelmiError unless allow_limit."""
        st = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 3)
        en = np.ascontiguousarray(ends, dtype=np.float64).reshape(-1, 3)
        n = len(st)
        smp = np.ascontiguousarray(samples, dtype=np.float64).reshape(n, -1, 3) if n else np.zeros((0, 0, 3))
        c = topo_cfg(**dict(cfg, max_sample_num=smp.shape[1]))

        nsp, sp, ms = _pack(start_pts, None, 3, n=n)
        nep, ep, me = _pack(end_pts, None, 3, n=n)
        maxn, mpp, r2, rs = max(c.max_nodes, 0), max(c.max_path_points, 0), max(c.max_raw_path2, 0), max(c.reserve_num, 0)
        out, res = _outputs(n, [("status", _I, ()), ("counts", _I, (4,)), ("events", _I, (6,)), ("n_nodes", _I, ()),
                                ("nid nty", _I, (maxn,)), ("nxyz", _D, (maxn, 3)), ("off", _I, (maxn + 1,)),
                                ("ids", _I, (4 * maxn,)), ("raw", _D, (r2, mpp, 3)), ("raw_len", _I, (r2,)),
                                ("filt", _D, (r2, mpp, 3)), ("filt_len", _I, (r2,)), ("sel", _D, (rs, mpp, 3)),
                                ("sel_len", _I, (rs,)), ("sel_length", _D, (rs,))])
        out["limit"] = _limited(self.L.fuelmi_map_topo_paths(self.h, C.byref(c), n, _dp(st), _dp(en), ms, _ip(nsp), _dp(sp),
                                                             me, _ip(nep), _dp(ep), _dp(smp), *res), allow_limit)
        nid, nty, nxyz, off, ids = (out.pop(k) for k in ("nid", "nty", "nxyz", "off", "ids"))
        out["nodes"] = [[(int(nid[b, i]), int(nty[b, i]), nxyz[b, i].copy(), ids[b, off[b, i]:off[b, i + 1]].copy())
                         for i in range(min(int(out["n_nodes"][b]), maxn))] for b in range(n)]
        for key in ("raw", "filt", "sel"):
            arr, ln = out[key], out[key + "_len"]
            out[key] = [[arr[b, r, :min(int(ln[b, r]), mpp)].copy() for r in range(ln.shape[1]) if ln[b, r] > 0]
                        for b in range(n)]
        return out

    @staticmethod
    def topo_plan(**cfg):
        """host only: dict(lanes, lds_bytes, workspace_bytes, guard_chunk, max_samples, max_raw, max_path_points,
        max_dis_points, max_neighbors, undefined_raw_nodes, max_points_in, max_workspace)"""
        return _plan_query(lib().fuelmi_topo_plan, 12, topo_cfg(**cfg), ctype=C.c_longlong,
                           names=("lanes", "lds_bytes", "workspace_bytes", "guard_chunk", "max_samples", "max_raw",
                                  "max_path_points", "max_dis_points", "max_neighbors", "undefined_raw_nodes", "max_points_in",
                                  "max_workspace"))

    def topo_pool_bytes(self):
        """bytes of the map's grow-only workspace of topo_paths"""
        return int(self.L.fuelmi_map_topo_pool_bytes(self.h))

    # --- collision ranges and guide points of guided replanning (include/fuelmi.h fuelmi_map_collision_ranges) ---
    COLRANGE_OK, COLRANGE_NO_COLLISION = _lib.COLRANGE_OK, _lib.COLRANGE_NO_COLLISION
    COLRANGE_ENDS_IN_OBSTACLE, COLRANGE_NONFINITE = _lib.COLRANGE_ENDS_IN_OBSTACLE, _lib.COLRANGE_NONFINITE

    def collision_ranges(self, pos_ctrl, knot_span, allow_limit=False, max_ctrl=None, **cfg):
        """findCollisionRange per problem against the distance field on the device: pos_ctrl is a list of [n_ctrl, 3]
        control-point arrays of uniform position splines, knot_span [n]; cfg: the fields of colrange_cfg().  Returns a
        dict of arrays: status (COLRANGE_*; -1: over max_events / max_pts / the tick cap), n_ticks, n_start_events,
        n_end_events, t_s, t_e, colli_start / colli_end [n, max_events, 3], n_start_pts / n_end_pts, start_pts / end_pts
        [n, max_pts, 3] (the layout topo_paths' C entry takes), first_start / last_end [n, 3]; limit.  FUELMI_ELIMIT
        raises FuelmiError unless allow_limit."""
        n, n_ctrl, arr, maxc = _spline(pos_ctrl, max_ctrl)
        c = colrange_cfg(max_ctrl=maxc, **cfg)
        knot = _per_problem(knot_span, n)
        ev, mp = max(c.max_events, 0), max(c.max_pts, 0)
        o, out = _outputs(n, [("status n_ticks n_start_events n_end_events", _I, ()), ("t_s t_e", _D, ()),
                              ("colli_start colli_end", _D, (ev, 3)), ("n_start_pts", _I, ()), ("start_pts", _D, (mp, 3)),
                              ("n_end_pts", _I, ()), ("end_pts", _D, (mp, 3)), ("first_start last_end", _D, (3,))])
        o["limit"] = _limited(self.L.fuelmi_map_collision_ranges(self.h, C.byref(c), n, _ip(n_ctrl), _dp(arr), _dp(knot), *out),
                              allow_limit)
        return o

    @staticmethod
    def colrange_plan(cfg):
        """host only: dict(lanes, lds_bytes, waves, max_ticks, max_ctrl, max_pts) of the collision-range kernel for a
        ColRangeCfg"""
        return _plan_query(lib().fuelmi_colrange_plan, 6, cfg,
                           names=("lanes", "lds_bytes", "waves", "max_ticks", "max_ctrl", "max_pts"))

    def guide_points(self, paths, duration, ctrl_pt_dist=0.5, degree=3, max_guide=64, max_path_points=None,
                     allow_limit=False):
        """the head of optimizeTopoBspline per guide path: paths is a list of [k, 3] arrays (topo_paths' "sel"),
        duration [n] the local segment's duration.  Returns a dict of arrays: status (TOPO_OK, TOPO_UNDEFINED; -1: over
        max_guide or the point cap), seg_num, dt, n_pts, n_ctrl, n_guide, guide_pts [n, max_guide, 3] (rows as
        BsplineBatchProblem's guide_pts takes them for degrees 3 and 4); limit."""
        plen, arr, mpp = _pack(paths, max_path_points, 3, floor=1)
        n = len(plen)
        dur = _per_problem(duration, n)
        o, out = _outputs(n, [("status seg_num", _I, ()), ("dt", _D, ()), ("n_pts n_ctrl n_guide", _I, ()),
                              ("guide_pts", _D, (max(int(max_guide), 0), 3))])
        o["limit"] = _limited(self.L.fuelmi_map_guide_points(self.h, n, mpp, _dp(arr), _ip(plen), _dp(dur), float(ctrl_pt_dist),
                                                             int(degree), int(max_guide), *out), allow_limit)
        return o

    # --- local segments of the global trajectory (include/fuelmi.h fuelmi_map_local_segments) ---
    LOCALSEG_SPHERE, LOCALSEG_DURATION = _lib.LOCALSEG_SPHERE, _lib.LOCALSEG_DURATION
    LOCALSEG_OK, LOCALSEG_DEGENERATE = _lib.LOCALSEG_OK, _lib.LOCALSEG_DEGENERATE
    LOCALSEG_NO_LOCAL, LOCALSEG_MISFIT = _lib.LOCALSEG_NO_LOCAL, _lib.LOCALSEG_MISFIT

    def local_segments(self, states, problems, degree=3, max_points=64, max_seg=None, max_ctrl=None, allow_limit=False):
        """paramLocalTraj (LOCALSEG_SPHERE: arg0 = radius, arg1 = dist_pt) / reparamLocalTraj (LOCALSEG_DURATION: arg0 =
        duration, arg1 = dt) per problem on the states' global trajectories: states is a list of dicts (seg_times [S],
        coef [S, 3, 6], global_duration, and optionally local_ctrl [n, 3] with local_knot_span, local_ts, local_te,
        time_change, last_time_inc), problems a list of (state index, mode, start_t, arg0, arg1).  Returns a dict of
        arrays: status (LOCALSEG_*; -1: more than max_points points), n_steps, segment_len, seg_num, duration, dt,
        n_points, points [n, max_points, 3], derivs [n, 4, 3], n_ctrl, ctrl [n, max_points + degree - 1, 3]; limit.
        FUELMI_ELIMIT raises FuelmiError unless allow_limit."""
        c, nt, st_arr, n, pr_arr = _pack_localseg(states, problems, degree, max_seg, max_ctrl)
        c.max_points = int(max_points)
        mp = max(c.max_points, 0)
        o, out = _outputs(n, [("status n_steps", _I, ()), ("segment_len", _D, ()), ("seg_num", _I, ()), ("duration dt", _D, ()),
                              ("n_points", _I, ()), ("points", _D, (mp, 3)), ("derivs", _D, (4, 3)), ("n_ctrl", _I, ()),
                              ("ctrl", _D, (mp + max(c.degree, 1) - 1, 3))])
        o["limit"] = _limited(self.L.fuelmi_map_local_segments(self.h, C.byref(c), nt, *[_ptr(a) for a in st_arr], n,
                                                               *[_ptr(a) for a in pr_arr], *out), allow_limit)
        return o

    @staticmethod
    def localseg_plan(degree=3, max_seg=1, max_ctrl=4, max_points=64):
        """host only: dict(lanes, lds_bytes, waves, max_seg, max_ctrl, max_points, count_cap, fit_lds_bytes) of the
        local-segment kernel"""
        return _plan_query(lib().fuelmi_localseg_plan, 8, LocalSegCfg(int(degree), int(max_seg), int(max_ctrl), int(max_points)),
                           names=("lanes", "lds_bytes", "waves", "max_seg", "max_ctrl", "max_points", "count_cap",
                                  "fit_lds_bytes"))

    # --- information gain and yaw search of HeadingPlanner (include/fuelmi.h fuelmi_map_info_gains) ---
    GAIN_NON_UNIFORM, GAIN_UNIFORM = _lib.GAIN_NON_UNIFORM, _lib.GAIN_UNIFORM

    def info_gains(self, pos, yaws, ctrl=None, path_of=None, allow_limit=False, max_yaw=None, max_ctrl=None, **cfg):
        """calcInformationGain / calcInfoGain for view groups on the device's unknown and occupied planes: pos [n, 3],
        yaws a list of yaw lists (one per group); NON_UNIFORM: ctrl a list of [k, 3] control-point arrays and path_of [n]
        the array each group weighs with (default 0).  cfg: the fields of gain_cfg().  Returns a dict of arrays: status
        (-1: over the cell cap), gain / n_cand / n_visible [n, max_yaw], n_rays [n]; limit."""
        pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
        n = len(pos)
        n_yaw, ya, my = _pack(yaws, max_yaw, 0, floor=1)
        assert len(n_yaw) == n
        c = gain_cfg(**dict(cfg, max_yaw=my))
        n_ctrl = carr = pof = None
        n_path = 0
        if ctrl is not None:
            n_path, n_ctrl, carr, c.max_ctrl = _spline(ctrl, max_ctrl, floor=1)
            pof = _per_problem(0 if path_of is None else path_of, n, np.int32)
        o, out = _outputs(n, [("status", _I, ()), ("gain", _D, (my,)), ("n_cand n_visible", _I, (my,)), ("n_rays", _I, ())])
        o["limit"] = _limited(self.L.fuelmi_map_info_gains(self.h, C.byref(c), n, _dp(pos), _ip(n_yaw), _dp(ya), n_path,
                                                           _ip(n_ctrl), _dp(carr), _ip(pof), *out), allow_limit)
        return o

    def yaw_paths(self, pts, yaws, dt, ctrl=None, gains_in=None, allow_limit=False, max_layer=None, max_ctrl=None, **cfg):
        """searchPathOfYaw per problem: pts a list of [L, 3] way-points, yaws a list of [L] yaws, dt [n]; ctrl a list of
        [k, 3] control-point arrays, one per problem (NON_UNIFORM); gains_in a list of [L, 2h + 1] arrays: the search
        runs on those gains and no ray is walked.  cfg: the fields of yawpath_cfg().  Returns a dict of arrays: status
        (-1: a layer over the cell cap), n_layer, path / path_vertex [n, max_layer], gains / g_value
        [n, max_layer, 2h + 1], n_rays [n, max_layer]; limit."""
        n_layer, ya, ml = _pack(yaws, max_layer, 0, floor=1)
        n_pts, pa, _ = _pack(pts, ml, 3)
        n = len(n_pts)
        assert len(n_layer) == n and (n_pts == n_layer).all()
        c = yawpath_cfg(**dict(cfg, max_layer=ml))
        nv = 2 * c.half_vert_num + 1
        dta = _per_problem(dt, n)
        n_ctrl = carr = gin = None
        if ctrl is not None:
            n_path, n_ctrl, carr, c.gain.max_ctrl = _spline(ctrl, max_ctrl, floor=1)
            assert n_path == n
        if gains_in is not None:
            gin = _pack(gains_in, ml, nv, n=n)[1]
        o, out = _outputs(n, [("status", _I, ()), ("path", _D, (ml,)), ("path_vertex", _I, (ml,)),
                              ("gains g_value", _D, (ml, max(nv, 0))), ("n_rays", _I, (ml,))])
        o["n_layer"] = n_layer
        o["limit"] = _limited(self.L.fuelmi_map_yaw_paths(self.h, C.byref(c), n, _ip(n_layer), _dp(pa), _dp(ya), _dp(dta),
                                                          _ip(n_ctrl), _dp(carr), _dp(gin), *out), allow_limit)
        return o

    # --- the yaw trajectory of a position spline (include/fuelmi.h fuelmi_map_plan_yaws) ---
    YAW_EXPLORE, YAW_FOLLOW, YAW_OK, YAW_DEGENERATE = _lib.YAW_EXPLORE, _lib.YAW_FOLLOW, _lib.YAW_OK, _lib.YAW_DEGENERATE

    def plan_yaws(self, pos_ctrl, knot_span, start_yaw, end_yaw=None, weights=None, derivs=True, allow_limit=False,
                  max_ctrl=None, knots=None, **cfg):
        """planYawExplore (mode 0) / planYaw (mode 1) per problem: pos_ctrl is a list of [n_ctrl, 3] control-point arrays
        of uniform position splines, knot_span [n], start_yaw [n, 3] (yaw, rate, acceleration), end_yaw [n] (EXPLORE).
        weights: a BsplineCfg or a dict of ld_* (default: the launch file's); cfg: the fields of yaw_cfg().  Returns a
        dict of arrays: status, duration, seg_num, dt_yaw, yaw_ctrl [n, max_seg+3], n_waypt, waypts [n, max_seg],
        end_yaw, cost, yawdot_ctrl, yawddot_ctrl (with derivs), limit.  FUELMI_ELIMIT raises unless allow_limit.
        knots (with knot_span None): a list of 1-D arrays of n_ctrl + pos_degree + 1 knots, e.g. the rows of adjust_trajs'
        knots_out (fuelmi_map_plan_yaws_knots)."""
        n, n_ctrl, arr, maxc = _spline(pos_ctrl, max_ctrl)
        c = yaw_cfg(max_ctrl=maxc, **cfg)
        knot, suffix = _knot_source(n, max(maxc, 0) + c.pos_degree + 1, knot_span, knots)
        w = _weights(weights, DEFAULT_BSPLINE)
        fn = getattr(self.L, "fuelmi_map_plan_yaws" + suffix)
        return _plan_yaws(n, c, start_yaw, end_yaw, derivs, allow_limit,
                          lambda yc, *a: fn(self.h, C.byref(w), yc, n, _ip(n_ctrl), _dp(arr), _dp(knot), *a))

    @staticmethod
    def yaw_plan(cfg):
        """(lanes per problem, LDS bytes, largest max_ctrl accepted) of the yaw kernel for a YawCfg; host only"""
        return _plan_query(lib().fuelmi_yaw_plan, 3, cfg)

    # --- the exact solve of the optimiser's quadratic phases (include/fuelmi.h fuelmi_map_solve_quadratic) ---
    QUAD_OK, QUAD_BOUNDED, QUAD_DEGENERATE = _lib.QUAD_OK, _lib.QUAD_BOUNDED, _lib.QUAD_DEGENERATE

    def solve_quadratic(self, ctrl, knot_span, cost_function=GUIDE_PHASE, start_state=None, end_state=None, end_n=3,
                        guide_pts=None, waypoints=None, waypt_idx=None, weights=None, bounds=False, dim=3, max_ctrl=None,
                        max_waypt=None):
        """The minimiser of optimize()'s objective for a mask within SMOOTHNESS | START | END | GUIDE | WAYPOINTS, per
        problem: ctrl is a list of [n_ctrl, dim] control-point arrays (each its own length), knot_span [n], start_state /
        end_state [n, 3, dim], guide_pts a list of [n_ctrl - 2 order, dim] arrays, waypoints / waypt_idx lists of [k, dim] /
        [k] arrays.  weights: a BsplineCfg or a dict of its fields (default: the launch file's).  Returns a dict: status [n],
        ctrl (a list of [n_ctrl, dim] arrays), ctrl_out [n, max_ctrl, dim], cost [n], pt_dist [n]."""
        dim = int(dim)
        n, n_ctrl, carr, maxc = _spline(ctrl, max_ctrl, cols=dim)
        w = _weights(weights, DEFAULT_BSPLINE)
        order = 3 if dim == 1 else int(w.bspline_degree)
        knot = _per_problem(knot_span, n)
        st = None if start_state is None else np.ascontiguousarray(start_state, dtype=np.float64).reshape(n, 3, dim)
        en = None if end_state is None else np.ascontiguousarray(end_state, dtype=np.float64).reshape(n, 3, dim)
        garr = None if guide_pts is None else _pack(guide_pts, max(maxc - 2 * order, 0), dim, n=n)[1]
        maxw = int(max_waypt) if max_waypt is not None else max([len(np.atleast_1d(i)) for i in (waypt_idx or [])] + [0])
        warr = n_w = iarr = None
        if waypoints is not None:
            n_w, warr, _ = _pack(waypoints, maxw, dim, n=n)
            iarr = _pack(waypt_idx, maxw, 0, np.int32, n=n)[1]
        c = QuadCfg(int(cost_function), dim, maxc, int(end_n), maxw, 1 if bounds else 0)
        o = _solve_quadratic(n, c, lambda qc, *out: self.L.fuelmi_map_solve_quadratic(
            self.h, C.byref(w), qc, n, _ip(n_ctrl), _dp(carr), _dp(knot), _dp(st), _dp(en), _dp(garr), _ip(n_w), _dp(warr),
            _ip(iarr), *out))
        o["ctrl"] = [o["ctrl_out"][b, :n_ctrl[b]] for b in range(n)]
        return o

    # --- the safety check of flown trajectories (include/fuelmi.h fuelmi_map_check_trajs) ---
    def check_trajs(self, pos_ctrl, knot_span, t_now, allow_limit=False, max_ctrl=None, knots=None, **cfg):
        """checkTrajCollision per problem against the inflated plane on the device: pos_ctrl is a list of [n_ctrl, 3]
        control-point arrays of uniform position splines, knot_span [n], t_now [n]; cfg: the fields of traj_check_cfg().
        Returns a dict of arrays: status, safe, distance (-1 when safe), n_samples, hit_index, hit_t, hit_pos [n, 3],
        end_reason, duration, limit.  FUELMI_ELIMIT raises unless allow_limit.
        knots (with knot_span None): a list of 1-D arrays of n_ctrl + degree + 1 knots, e.g. the rows of adjust_trajs'
        knots_out (fuelmi_map_check_trajs_knots)."""
        n, n_ctrl, arr, maxc = _spline(pos_ctrl, max_ctrl)
        c = traj_check_cfg(max_ctrl=maxc, **cfg)
        knot, suffix = _knot_source(n, max(maxc, 0) + c.degree + 1, knot_span, knots)
        fn = getattr(self.L, "fuelmi_map_check_trajs" + suffix)
        return _check_trajs(n, t_now, allow_limit,
                            lambda *a: fn(self.h, C.byref(c), n, _ip(n_ctrl), _dp(arr), _dp(knot), *a))

    @staticmethod
    def traj_check_plan(cfg):
        """(lanes per problem, LDS bytes of a workgroup, largest max_ctrl accepted) of the check kernel for a TrajChkCfg;
        host only"""
        return _plan_query(lib().fuelmi_traj_check_plan, 3, cfg)

    # --- sampling of flown trajectories (include/fuelmi.h fuelmi_map_sample_trajs) ---
    def sampleTrajs(self, pos_ctrl, knot_span, t, yaw_ctrl=None, yaw_dt=None, t_stop=None, flight=None, max_ctrl=None,
                    max_yaw_ctrl=None, max_t=None, knots=None, **cfg):
        """cmdCallback (mode TRAJSMP_COMMAND, the default) or the FSM's replan state (TRAJSMP_STATE) per problem on the
        device: pos_ctrl is a list of [n_ctrl, 3] control-point arrays of uniform position splines, knot_span [n], t a list
        of 1-D arrays of sample times; yaw_ctrl a list of 1-D control-point arrays (None: no yaw spline) with yaw_dt [n];
        t_stop [n] or None; flight [n, 8] or None (a copy is updated and returned); cfg: mode, degree, yaw_degree.
        Returns a dict of arrays: status [n, max_t], pos / vel / acc / jerk [n, max_t, 3], yaw / yawdot / yawddot
        [n, max_t], duration [n], flight, n_t.
        knots (with knot_span None): a list of 1-D arrays of n_ctrl + degree + 1 position knots, e.g. the rows of
        adjust_trajs' knots_out (fuelmi_map_sample_trajs_knots); the yaw splines stay uniform."""
        n, n_ctrl, arr, maxc = _spline(pos_ctrl, max_ctrl)
        args, o, maxy, maxt = _trajsmp_io(n, t, yaw_ctrl, yaw_dt, t_stop, flight, max_yaw_ctrl, max_t)
        c = traj_sample_cfg(max_ctrl=maxc, max_yaw_ctrl=maxy, max_t=maxt, **cfg)
        knot, suffix = _knot_source(n, max(maxc, 0) + c.degree + 1, knot_span, knots)
        check(getattr(self.L, "fuelmi_map_sample_trajs" + suffix)(self.h, C.byref(c), n, _ip(n_ctrl), _dp(arr), _dp(knot),
                                                                  *args))
        return o

    sample_trajs = sampleTrajs

    @staticmethod
    def traj_sample_plan(cfg):
        """(lanes per problem, LDS bytes of a workgroup, largest max_ctrl accepted) of the sampling kernel for a
        TrajSmpCfg; host only"""
        return _plan_query(lib().fuelmi_traj_sample_plan, 3, cfg)

    # --- time adjustment and metrics of trajectories (include/fuelmi.h fuelmi_map_adjust_trajs) ---
    def adjust_trajs(self, pos_ctrl, knot_span=None, knots_in=None, ratio_in=None, group=None, ops=0, max_ctrl=None,
                     max_samples=None, n_group=None, **cfg):
        """checkRatio / checkFeasibility, then optionally lengthenTime (TRAJADJ_LENGTHEN), the reallocateTime loop
        (TRAJADJ_REALLOC), the metrics, reparamBspline's samples (TRAJADJ_RESAMPLE) and selectBestTraj per group
        (TRAJADJ_SELECT), per problem on the device: pos_ctrl is a list of [n_ctrl, 3] control-point arrays, with knot_span
        [n] or knots_in, a list of 1-D arrays of n_ctrl + degree + 1 knots; ratio_in [n] or None; group [n]; cfg: the
        other fields of traj_adjust_cfg.  Returns a dict of arrays: info [n, 8] and metrics [n, 12] and each of their
        columns under its name (status, iters, jerk, ...), knots_out [n, max_ctrl + degree + 1], samples
        [n, max_samples, 3] or None, best [n_group] or None, n_ctrl."""
        degree = int(cfg.get("degree", 3))
        n, n_ctrl, arr, maxc = _spline(pos_ctrl, max_ctrl, floor=degree + 1)
        args, o, maxs, ng = _trajadj_io(n, n_ctrl, degree, maxc, knots_in, ratio_in, group, int(ops), max_samples, n_group)
        c = traj_adjust_cfg(ops=ops, max_ctrl=maxc, max_samples=maxs, n_group=ng, **cfg)
        knot = _per_problem(knot_span, n, optional=True)
        check(self.L.fuelmi_map_adjust_trajs(self.h, C.byref(c), n, _ip(n_ctrl), _dp(arr), _dp(knot), *args))
        return _trajadj_named(o)

    @staticmethod
    def traj_adjust_plan(cfg):
        """(lanes per problem, LDS bytes of a workgroup, largest max_ctrl accepted) of the adjustment kernel for a
        TrajAdjCfg; host only"""
        return _plan_query(lib().fuelmi_traj_adjust_plan, 3, cfg)

    # --- measurement ---
    def timerBegin(self):
        check(self.L.fuelmi_timer_begin(self.h))

    def timerEnd(self):
        ms = C.c_float()
        check(self.L.fuelmi_timer_end(self.h, C.byref(ms)))
        return ms.value

    def profileEnable(self, mask):
        check(self.L.fuelmi_profile_enable(self.h, mask))

    def profileGet(self, stage):
        n = C.c_int()
        t = C.c_double()
        check(self.L.fuelmi_profile_get(self.h, stage, C.byref(n), C.byref(t)))
        return n.value, t.value

    def profileTimeline(self, stage, cap=4096):
        """(begin, end) of every bracket of a stage in ms after the profileEnable call that armed it"""
        a = np.empty(cap, dtype=np.float64)
        b = np.empty(cap, dtype=np.float64)
        n = C.c_int()
        check(self.L.fuelmi_profile_get_timeline(self.h, stage, _dp(a), _dp(b), cap, C.byref(n)))
        return a[:n.value].copy(), b[:n.value].copy()

    def profileSamples(self, stage, cap=4096):
        """Per-launch milliseconds of a stage since profileEnable."""
        ms = np.empty(cap)
        n = C.c_int()
        check(self.L.fuelmi_profile_get_samples(self.h, stage, _dp(ms), cap, C.byref(n)))
        return ms[:n.value].copy()


def tour_matrix(mat, scale=100):
    """findGlobalTour's conversion of getFullCostMatrix (fast_exploration_manager.cpp:368-374): int_cost = cost * scale
    truncated toward zero, as int32.  Raises ValueError where the reference's conversion is undefined (a non-finite
    value, |cost * scale| >= 2^31)."""
    m = np.asarray(mat, dtype=np.float64)
    if m.ndim != 2 or m.shape[0] != m.shape[1]:
        raise ValueError("tour_matrix: a square matrix is needed, got shape %s" % (m.shape,))
    x = m * scale
    if not np.isfinite(x).all():
        raise ValueError("tour_matrix: non-finite entry")
    if (np.abs(x) >= 2.0 ** 31).any():
        raise ValueError("tour_matrix: |cost * %g| >= 2^31" % scale)
    return np.trunc(x).astype(np.int32)


class TourSolver:
    """fuelmi_tsp: the global tour (FastExplorationManager::findGlobalTour's ATSP) for a batch of int32 matrices.
    solve(list of d x d matrices) -> (orders: list of int arrays starting at 0, costs: int64 array, methods: int array,
    0 exact / 1 heuristic).  The rules are include/fuelmi.h's; tests/tsp_ref.py restates them."""

    def __init__(self, device=0, restarts=_lib.TSP_DEFAULT_RESTARTS, kicks=_lib.TSP_DEFAULT_KICKS,
                 exact_max=_lib.TSP_DEFAULT_EXACT_MAX, seed=0):
        self.cfg = TspCfg(int(restarts), int(kicks), int(exact_max), int(seed))
        self._h = C.c_void_p()
        check(lib().fuelmi_tsp_create(int(device), C.byref(self.cfg), C.byref(self._h)))

    def solve(self, mats):
        mats = [np.ascontiguousarray(m, dtype=np.int32) for m in mats]
        for m in mats:
            if m.ndim != 2 or m.shape[0] != m.shape[1]:
                raise ValueError("TourSolver.solve: square matrices are needed, got shape %s" % (m.shape,))
        dims = np.array([m.shape[0] for m in mats], dtype=np.int32)
        dim_ptr = np.zeros(len(mats) + 1, dtype=np.int32)
        np.cumsum(dims, out=dim_ptr[1:])
        costs = np.concatenate([m.reshape(-1) for m in mats]) if mats else np.zeros(1, np.int32)
        order = np.zeros(max(1, int(dim_ptr[-1])), dtype=np.int32)
        cost = np.zeros(max(1, len(mats)), dtype=np.int64)
        method = np.zeros(max(1, len(mats)), dtype=np.int32)
        check(lib().fuelmi_tsp_solve(self._h, len(mats), _ip(dim_ptr), costs.ctypes.data_as(C.POINTER(C.c_int32)),
                                     _ip(order), cost.ctypes.data_as(C.POINTER(C.c_int64)), _ip(method)))
        orders = [order[dim_ptr[b]:dim_ptr[b + 1]].copy() for b in range(len(mats))]
        return orders, cost[:len(mats)], method[:len(mats)]

    def close(self):
        if self._h:
            lib().fuelmi_tsp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DepthRenderer:
    """fuelmi_render: the simulated depth camera pcl_render_node (uav_simulator/local_sensing) for a batch of poses, the
    frames left on the device.  model: _lib.RENDER_HOST_NODE (depth_render_node.cpp, the node built by default; `range`
    is its 5.0 m cull, inf switches it off) or _lib.RENDER_CUDA_NODE (depth_render.cu).  The rules are include/fuelmi.h's;
    tests/depth_render_ref.py restates them."""

    PLAN_KEYS = ("segment_lanes", "wave_min_size", "project_points", "project_workgroups", "splat_workgroups",
                 "convert_workgroups")

    def __init__(self, rows, cols, fx, fy, cx, cy, model=_lib.RENDER_HOST_NODE, range=5.0, max_poses=1, device=0):
        self.cfg = self.config(rows, cols, fx, fy, cx, cy, model, range, max_poses, device)
        self.rows, self.cols, self.max_poses = int(rows), int(cols), int(max_poses)
        self._h = C.c_void_p()
        check(lib().fuelmi_render_create(C.byref(self.cfg), C.byref(self._h)))

    @staticmethod
    def config(rows, cols, fx, fy, cx, cy, model=_lib.RENDER_HOST_NODE, range=5.0, max_poses=1, device=0):
        return RenderCfg(int(device), int(rows), int(cols), float(fx), float(fy), float(cx), float(cy), int(model),
                         float(range), int(max_poses))

    @staticmethod
    def pose_transform(pos, q_wxyz):
        """(T_cw, cam_pos) of a camera at `pos` with orientation (w, x, y, z): cam2world = [R(q) | pos], T_cw the first
        three rows of its general 4 x 4 inverse (the node's cam2world.inverse()), cam_pos its translation column."""
        w, x, y, z = (float(v) for v in q_wxyz)
        c2w = np.eye(4)
        c2w[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                       [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                       [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
        c2w[:3, 3] = np.asarray(pos, dtype=np.float64)
        return np.ascontiguousarray(np.linalg.inv(c2w)[:3, :]), c2w[:3, 3].copy()

    def set_cloud(self, xyz, n_points=None):
        """xyz: an array of n x 3 floats, or (with n_points) the address of as many floats in host or device memory."""
        if n_points is None:
            pts = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
            check(lib().fuelmi_render_set_cloud(self._h, C.c_void_p(pts.ctypes.data), len(pts)))
        else:
            check(lib().fuelmi_render_set_cloud(self._h, C.c_void_p(int(xyz)), int(n_points)))

    def render(self, T_cw, cam_pos, scaling=1000.0, metres=True, raw=True):
        """-> (metres [n, rows, cols] float32 or None, raw [n, rows, cols] uint16 or None, stats [n, 4] int32)"""
        T = np.ascontiguousarray(T_cw, dtype=np.float64).reshape(-1, 12)
        p = np.ascontiguousarray(cam_pos, dtype=np.float64).reshape(-1, 3)
        if len(T) != len(p):
            raise ValueError("DepthRenderer.render: %d transforms, %d camera positions" % (len(T), len(p)))
        n = len(T)
        m = np.empty((n, self.rows, self.cols), dtype=np.float32) if metres else None
        r = np.empty((n, self.rows, self.cols), dtype=np.uint16) if raw else None
        stats = np.zeros((max(n, 1), 4), dtype=np.int32)
        check(lib().fuelmi_render_depth(self._h, n, _dp(T), _dp(p), float(scaling), None if m is None else m.ctypes.data,
                                        None if r is None else r.ctypes.data, _ip(stats)))
        return m, r, stats[:n]

    def frame_raw_ptr(self, k):
        """device address of frame k's uint16 image (for SDFMap.inputDepthImageAt): valid until the next render, set_cloud
        or close"""
        p = lib().fuelmi_render_frame_raw(self._h, int(k))
        if not p:
            check(_lib.EINVAL)
        return p

    def frame_metres_ptr(self, k):
        p = lib().fuelmi_render_frame_metres(self._h, int(k))
        if not p:
            check(_lib.EINVAL)
        return p

    @classmethod
    def plan_for(cls, cfg, n_points):
        out = np.zeros(8, dtype=np.int32)
        check(lib().fuelmi_render_plan(C.byref(cfg), int(n_points), _ip(out)))
        d = dict(zip(cls.PLAN_KEYS, (int(v) for v in out[:6])))
        d["scratch_bytes"] = int(out[6]) + (int(out[7]) << 31)
        return d

    def plan(self, n_points=0):
        return self.plan_for(self.cfg, n_points)

    def times(self):
        """device milliseconds of the last render: cull + project, splat, convert"""
        ms = np.zeros(3)
        check(lib().fuelmi_render_times(self._h, _dp(ms)))
        return ms

    def close(self):
        if self._h:
            lib().fuelmi_render_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceBuffer:
    """A numpy array's bytes in device memory (fuelmi_device_alloc / _upload): .ptr is the device address."""

    def __init__(self, array, device=0):
        a = np.ascontiguousarray(array)
        self.L = lib()
        p = C.c_void_p()
        check(self.L.fuelmi_device_alloc(int(device), a.nbytes, C.byref(p)))
        self.ptr, self.nbytes = p.value, a.nbytes
        check(self.L.fuelmi_device_upload(C.c_void_p(self.ptr), a.ctypes.data, a.nbytes))

    def close(self):
        if getattr(self, "ptr", None):
            self.L.fuelmi_device_free(C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RegisteredHostBuffer:
    """A numpy array registered with the device (fuelmi_host_register: a camera driver's frame ring, read in place by
    the fusion kernels).  The registration is undone BEFORE the array's memory goes back to the allocator -- by close()
    or, at the latest, when this object dies: a registration that outlives its memory stays in the HIP runtime's
    address map, and a later pageable copy from whatever the allocator puts there fails with "invalid argument"."""

    def __init__(self, array):
        self.array = np.ascontiguousarray(array)
        self.L = lib()
        check(self.L.fuelmi_host_register(self.array.ctypes.data, self.array.nbytes))
        self.ptr, self.nbytes = self.array.ctypes.data, self.array.nbytes

    def close(self):
        if getattr(self, "ptr", None):
            self.L.fuelmi_host_unregister(C.c_void_p(self.ptr))
            self.ptr = None
        self.array = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EDTEnvironment:
    """fast_planner::EDTEnvironment: distance/gradient query facade over SDFMap."""

    def __init__(self):
        self.sdf_map_ = None

    def setMap(self, sdf_map):
        self.sdf_map_ = sdf_map

    def evaluateEDTWithGrad(self, pos, time=-1.0):
        return self.sdf_map_.getDistWithGrad(pos)

    def evaluateCoarseEDT(self, pos, time=-1.0):
        return self.sdf_map_.getDistance(pos)


class FrontierFinder:
    """Grid part of fast_planner::FrontierFinder (searchFrontiers / expandFrontier)."""

    def __init__(self, edt_or_map, cluster_min=100, min_z=0.4, cluster_size_xy=2.0, down_sample=3, split=False,
                 reference_order=False):
        """split=True: searchFrontiers ends with splitLargeFrontiers (frontier_finder.cpp:120,166-242) and
        every new cluster carries its down-sampled filtered_cells_.  reference_order=True: cells in the
        reference's BFS order, means / VoxelGrid centroids summed in that order (bit-exact against the reference;
        default: ascending voxel address, order-free means)."""
        self.L = lib()
        self.map = edt_or_map.sdf_map_ if isinstance(edt_or_map, EDTEnvironment) else edt_or_map
        cfg = FrontierCfg(cluster_min, min_z, cluster_size_xy, down_sample, int(split), int(reference_order))  # (True -> 1; pass 2 for "auto")
        h = C.c_void_p()
        check(self.L.fuelmi_frontier_create(self.map.h, C.byref(cfg), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.fuelmi_frontier_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def searchFrontiers(self):
        n = C.c_int()
        check(self.L.fuelmi_frontier_search(self.h, C.byref(n)))
        return n.value

    def searchFrontiersBegin(self):
        check(self.L.fuelmi_frontier_search_begin(self.h))

    def searchFrontiersEnd(self):
        n = C.c_int()
        check(self.L.fuelmi_frontier_search_end(self.h, C.byref(n)))
        return n.value

    def commit(self, dormant=False):
        check(self.L.fuelmi_frontier_commit(self.h, int(dormant)))

    def reset(self):
        check(self.L.fuelmi_frontier_reset(self.h))

    def sync(self):
        """wait for everything the finder has queued (incl. the regrouping tail of the last search)"""
        from ._lib import check as _c
        _c(self.L.fuelmi_frontier_synchronize(self.h))

    def stats(self):
        """(searches on the fast chain, on the legacy chain, fast-chain searches that fell back)"""
        return _plan_query(self.L.fuelmi_frontier_stats, 3, self.h)

    def resolvedInLaunch(self):
        """fast-chain searches resolved by the last workgroup of k_tile_cross itself (the others: by k_resolve)"""
        return self.L.fuelmi_frontier_resolved_in_launch(self.h)

    def pathStats(self):
        """(fast-chain searches that outgrew the in-launch resolve with no k_resolve queued behind it -- the late
        resolve --, fast-chain searches run again on a smaller tile)"""
        return _plan_query(self.L.fuelmi_frontier_path_stats, 2, self.h)

    def changedStats(self):
        """the changed-cluster test in front of the searches: {"paths": launches of (one workgroup, in-kernel barrier,
        two passes on an LDS table, two passes on a device table), "nc", "total", "mark": candidates, pooled cells and
        mark of the last test (mark 0 on the one-workgroup path), "rebuilds": device pool rebuilds so far, "pool_cap":
        the pool's capacity in cells}"""
        o = _plan_query(self.L.fuelmi_frontier_changed_stats, 9, self.h)
        return {"paths": tuple(o[:4]), "nc": o[4], "total": o[5], "mark": o[6], "rebuilds": o[7], "pool_cap": o[8]}

    def orderStats(self):
        """(order of the last search: 0 address / 1 reference BFS, searches in the reference's order, mode-2 searches
        that fell back to the address order, cells of the cluster that forced the last fallback)"""
        return _plan_query(self.L.fuelmi_frontier_order_stats, 4, self.h)

    def clusters(self, which=0):
        out = []
        cnt = self.L.fuelmi_frontier_count(self.h, which)
        if cnt < 0:
            check(cnt)
        for k in range(cnt):
            n = self.L.fuelmi_frontier_cluster_size(self.h, which, k)
            a = np.empty(n, dtype=np.int32)
            check(self.L.fuelmi_frontier_cluster_cells(self.h, which, k, _ip(a)))
            out.append(a)
        return out

    def clusterCentres(self, which=0):
        """cells_ of every cluster as voxel centres ([n, 3] doubles each), decoded by the library"""
        out = []
        cnt = self.L.fuelmi_frontier_count(self.h, which)
        if cnt < 0:
            check(cnt)
        for k in range(cnt):
            n = self.L.fuelmi_frontier_cluster_size(self.h, which, k)
            a = np.empty((n, 3))
            check(self.L.fuelmi_frontier_cluster_centres(self.h, which, k, _dp(a)))
            out.append(a)
        return out

    def keepPrevious(self, on=True):
        """fuelmi_frontier_keep_previous: a reset keeps the retired search's new clusters readable as list 3"""
        check(self.L.fuelmi_frontier_keep_previous(self.h, int(bool(on))))

    @staticmethod
    def viewpointConfig(rmin=1.5, rmax=2.5, rnum=3, dphi=15 * 3.1415926 / 180.0, clearance=0.21, min_visib_num=15,
                        min_candidate_dist=0.75, min_view_finish_fraction=0.2, top_angle=0.56125,
                        left_angle=0.69222, right_angle=0.68901, max_dist=4.5):
        """frontier/candidate_* and perception_utils/* of algorithm.xml:106-121."""
        return _lib.ViewpointCfg(rmin, rmax, rnum, dphi, clearance, min_visib_num, min_candidate_dist,
                                 min_view_finish_fraction, top_angle, left_angle, right_angle, max_dist)

    def setViewpointConfig(self, cfg):
        self.vcfg = cfg
        check(self.L.fuelmi_frontier_set_viewpoint_cfg(self.h, C.byref(cfg)))

    def computeFrontiersToVisit(self):
        """sampleViewpoints for the new clusters, then frontiers_ / dormant_frontiers_ (reference :392-423).
        Returns (new active, new dormant)."""
        a, d = C.c_int(), C.c_int()
        check(self.L.fuelmi_frontier_compute_to_visit(self.h, C.byref(a), C.byref(d)))
        return a.value, d.value

    def viewpoints(self, which, k):
        """(pos_yaw [n,4], visib_num [n]) of cluster k, best coverage first."""
        n = self.L.fuelmi_frontier_viewpoint_count(self.h, which, k)
        if n < 0:
            check(n)
        py = np.empty((n, 4))
        vis = np.empty(n, dtype=np.int32)
        if n:
            check(self.L.fuelmi_frontier_viewpoints(self.h, which, k, _dp(py), _ip(vis)))
        return py, vis

    def isFrontierCovered(self):
        c = C.c_int()
        check(self.L.fuelmi_frontier_is_covered(self.h, C.byref(c)))
        return bool(c.value)

    def getTopViewpointsInfo(self, cur_pos):
        """reference :425-450: per active frontier the best viewpoint farther than min_candidate_dist."""
        cur = np.asarray(cur_pos, dtype=float)
        pts, yaws, avgs = [], [], []
        for k in range(self.L.fuelmi_frontier_count(self.h, 1)):
            py, _ = self.viewpoints(1, k)
            pick = py[0]
            for v in py:
                if np.linalg.norm(v[:3] - cur) < self.vcfg.min_candidate_dist:
                    continue
                pick = v
                break
            pts.append(pick[:3].copy())
            yaws.append(float(pick[3]))
            avgs.append(self.clusterInfo(1, k)[0])
        return pts, yaws, avgs

    def filtered(self, which, k):
        """Frontier::filtered_cells_ of cluster k: float32 [n,3] (split=True searches only)."""
        n = self.L.fuelmi_frontier_cluster_filtered_size(self.h, which, k)
        if n < 0:
            check(n)
        out = np.empty((n, 3), dtype=np.float32)
        if n:
            check(self.L.fuelmi_frontier_cluster_filtered(self.h, which, k, out.ctypes.data))
        return out

    def getFrontiers(self):
        """clusters of frontiers_ as voxel-centre positions (reference: getFrontiers)."""
        nv = self.map.nvox
        res = []
        for a in self.clusters(1):
            idx = np.stack(np.unravel_index(a, nv), axis=1)
            res.append((idx + 0.5) * self.map.res + self.map.origin)
        return res

    def clusterInfo(self, which, k):
        o = np.empty(9)
        check(self.L.fuelmi_frontier_cluster_info(self.h, which, k, _dp(o)))
        return o[:3], o[3:6], o[6:9]

    def removedIds(self):
        n = self.L.fuelmi_frontier_removed_count(self.h)
        a = np.empty(max(n, 0), dtype=np.int32)
        if n > 0:
            check(self.L.fuelmi_frontier_removed_ids(self.h, _ip(a)))
        return a

    def flags(self):
        f = np.zeros(self.map.N, dtype=np.int8)
        check(self.L.fuelmi_frontier_get_flags(self.h, f.ctypes.data))
        return f


class BsplineBatchProblem:
    """Keeps the numpy arrays of one batch alive and exposes the C struct."""

    def __init__(self, x, point_num, cost_function, pt_dist, start_state=None, end_state=None, end_n=3,
                 dim=3, knot_span=None, time_lb=None, guide_pts=None, waypoints=None, waypt_idx=None,
                 view_pt=None, view_dir=None, view_idx=None):
        f64 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
        i32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
        self.x = f64(x)
        self.C = self.x.shape[0]
        self.nvar = self.x.shape[1]
        self.pt_dist = _per_problem(pt_dist, self.C)
        self.knot_span = _per_problem(knot_span if knot_span is not None else 0.0, self.C)
        self.time_lb = _per_problem(time_lb, self.C, optional=True)
        self.start_state = f64(start_state)
        self.end_state = f64(end_state)
        self.guide_pts = f64(guide_pts)
        self.waypoints = f64(waypoints)
        self.waypt_idx = i32(waypt_idx)
        self.view_pt = f64(view_pt)
        self.view_dir = f64(view_dir)
        self.view_idx = i32(view_idx)
        b = BsplineBatch()
        b.cost_function = cost_function
        b.dim = dim
        b.point_num = point_num
        b.n_traj = self.C
        b.x = _dp(self.x)
        b.pt_dist = _dp(self.pt_dist)
        b.knot_span = _dp(self.knot_span)
        b.time_lb = _dp(self.time_lb)
        b.start_state = _dp(self.start_state)
        b.end_state = _dp(self.end_state)
        b.end_n = end_n
        b.guide_pts = _dp(self.guide_pts)
        b.waypoints = _dp(self.waypoints)
        b.waypt_idx = _ip(self.waypt_idx)
        b.n_waypt = 0 if self.waypoints is None else self.waypoints.shape[1]
        b.view_pt = _dp(self.view_pt)
        b.view_dir = _dp(self.view_dir)
        b.view_idx = _ip(self.view_idx)
        self.c = b


class BsplineOptimizer:
    """Cost/gradient side of fast_planner::BsplineOptimizer, batched over candidates."""

    def __init__(self, **params):
        self.cfg = _weights(params, DEFAULT_BSPLINE)
        self.L = lib()
        self.env = None

    def setEnvironment(self, env):
        self.env = env

    def _map(self):
        return self.env.sdf_map_ if isinstance(self.env, EDTEnvironment) else self.env

    def combineCost(self, problem):
        """Evaluate C trajectories; returns (cost[C], grad[C, nvar])."""
        cost = np.empty(problem.C)
        grad = np.empty((problem.C, problem.nvar))
        check(self.L.fuelmi_bspline_cost_grad(self._map().h, C.byref(self.cfg), C.byref(problem.c),
                                              _dp(cost), _dp(grad)))
        return cost, grad

    def optimize(self, problem, max_eval=300, max_time=-1.0):
        """BsplineOptimizer::optimize() for the C trajectories of `problem` in ONE call (fuelmi_bspline_optimize: a
        query slot of the map -- no device allocation, re-entrant).  Returns (x [C, nvar], cost [C], evals [C])."""
        x = np.empty((problem.C, problem.nvar))
        cost = np.empty(problem.C)
        ev = np.empty(problem.C, dtype=np.int32)
        check(self.L.fuelmi_bspline_optimize(self._map().h, C.byref(self.cfg), C.byref(problem.c), int(max_eval),
                                             float(max_time), _dp(x), _dp(cost), _ip(ev)))
        return x, cost, ev

    def deviceProblem(self, problem):
        return BsplineDeviceProblem(self, problem)

    @staticmethod
    def optPlan(problem):
        """Which solve kernel optimize() and deviceProblem().optimize() run for `problem` (fuelmi_bspline_opt_plan, host
        only): (npl, waves per candidate, dynamic LDS bytes); npl 0 is the LDS-state kernel.  Raises FuelmiError for a
        batch neither call would take."""
        return _plan_query(lib().fuelmi_bspline_opt_plan, 3, problem.c)


class NonUniformBspline:
    """The two NonUniformBspline calls the planners wrap around optimize() (bspline/src/non_uniform_bspline.cpp),
    batched over candidates on the map's device."""

    @staticmethod
    def parameterizeToBspline(sdf_map, ts, points, derivs, degree=3):
        """ts [C], points [C][K][3], derivs [C][4][3] -> control points [C][K+degree-1][3] (:178-265)."""
        ts = np.ascontiguousarray(ts, dtype=np.float64)
        points = np.ascontiguousarray(points, dtype=np.float64)
        derivs = np.ascontiguousarray(derivs, dtype=np.float64)
        if points.ndim != 3 or points.shape[2] != 3 or ts.shape != (points.shape[0],) or \
                derivs.shape != (points.shape[0], 4, 3):
            raise ValueError("parameterizeToBspline: ts [C], points [C][K][3], derivs [C][4][3]")
        cn, k = points.shape[0], points.shape[1]
        ctrl = np.empty((cn, k + degree - 1, 3))
        check(lib().fuelmi_bspline_parameterize(sdf_map.h, cn, k, int(degree), _dp(ts), _dp(points), _dp(derivs),
                                                _dp(ctrl)))
        return ctrl

    @staticmethod
    def getBoundaryStates(sdf_map, ctrl, ts, degree=3, ks=2, ke=0):
        """ctrl [C][N][3], ts [C] -> (start [C][ks+1][3], end [C][ke+1][3]) (:107-122)."""
        ctrl = np.ascontiguousarray(ctrl, dtype=np.float64)
        ts = np.ascontiguousarray(ts, dtype=np.float64)
        if ctrl.ndim != 3 or ctrl.shape[2] != 3 or ts.shape != (ctrl.shape[0],):
            raise ValueError("getBoundaryStates: ctrl [C][N][3], ts [C]")
        cn = ctrl.shape[0]
        start = np.empty((cn, ks + 1, 3))
        end = np.empty((cn, ke + 1, 3))
        check(lib().fuelmi_bspline_boundary_states(sdf_map.h, cn, ctrl.shape[1], int(degree), _dp(ts), _dp(ctrl),
                                                   int(ks), int(ke), _dp(start), _dp(end)))
        return start, end


class BsplineDeviceProblem:
    def __init__(self, opt, problem):
        self.L = opt.L
        self.problem = problem
        self.degree = int(opt.cfg.bspline_degree)
        self.map = opt._map()
        h = C.c_void_p()
        check(self.L.fuelmi_bspline_dev_create(self.map.h, C.byref(opt.cfg), C.byref(problem.c), C.byref(h)))
        self.h = h

    def eval(self):
        check(self.L.fuelmi_bspline_dev_eval(self.h))

    def evalPinned(self, slot):
        check(self.L.fuelmi_bspline_dev_eval_pinned(self.h, int(slot)))

    def collect(self, slot):
        cost = np.empty(self.problem.C)
        grad = np.empty((self.problem.C, self.problem.nvar))
        check(self.L.fuelmi_bspline_dev_collect(self.h, int(slot), _dp(cost), _dp(grad)))
        return cost, grad

    def download(self):
        cost = np.empty(self.problem.C)
        grad = np.empty((self.problem.C, self.problem.nvar))
        check(self.L.fuelmi_bspline_dev_download(self.h, _dp(cost), _dp(grad)))
        return cost, grad

    def optimize(self, max_eval=300, max_time=-1.0):
        """BsplineOptimizer::optimize() for every candidate, on the device; max_time (seconds, <= 0: none) is the
        solver's wall-clock cap (set_maxtime).  Returns (best_x [C][nvar], best_cost [C], evaluations [C])."""
        c = self.problem.c
        nvar = c.dim * c.point_num + (1 if c.cost_function & MINTIME else 0)
        x = np.empty((c.n_traj, nvar))
        cost = np.empty(c.n_traj)
        ev = np.empty(c.n_traj, dtype=np.int32)
        check(self.L.fuelmi_bspline_dev_optimize_timed(self.h, int(max_eval), float(max_time), _dp(x), _dp(cost), _ip(ev)))
        return x, cost, ev

    def loadSamples(self, ts, points, derivs):
        """samples -> parameterizeToBspline -> getBoundaryStates(2, 0) -> setBoundaryStates + pt_dist_ on the
        device (planner_manager.cpp:161-184): ts [C], points [C][K][3], derivs [C][4][3]."""
        ts = np.ascontiguousarray(ts, dtype=np.float64)
        points = np.ascontiguousarray(points, dtype=np.float64)
        derivs = np.ascontiguousarray(derivs, dtype=np.float64)
        c = self.problem.c
        if ts.shape != (c.n_traj,) or points.ndim != 3 or points.shape[0] != c.n_traj or points.shape[2] != 3 \
                or derivs.shape != (c.n_traj, 4, 3):
            raise ValueError("loadSamples: ts [C], points [C][K][3], derivs [C][4][3]")
        check(self.L.fuelmi_bspline_dev_load_samples(self.h, points.shape[1], _dp(ts), _dp(points), _dp(derivs)))

    def load_waypoints(self, ways, vels, accs, max_vel=2.0, ctrl_pt_dist=0.45, min_seg=8, max_way_points=None,
                       allow_limit=False):
        """way-points -> min-jerk samples -> loadSamples' fit, without leaving the device (fuelmi_bspline_dev_load_waypoints):
        one problem per candidate, seg_num forced to point_num - bspline_degree.  Returns (status [C], duration [C]); a
        candidate whose status is not 0 keeps its state."""
        c = self.problem.c
        if len(ways) != c.n_traj:
            raise ValueError("load_waypoints: one list of way-points per candidate")
        n_way, way, vel, acc, wc = _pack_waypoints(ways, vels, accs, max_vel, ctrl_pt_dist, min_seg, 0, max_way_points, 1)
        o, out = _outputs(c.n_traj, [("status", _I, ()), ("duration", _D, ())])
        _limited(self.L.fuelmi_bspline_dev_load_waypoints(self.h, C.byref(wc), _ip(n_way), _dp(way), _dp(vel), _dp(acc), *out),
                 allow_limit)
        return o["status"], o["duration"]

    def load_local_segments(self, states, problems, max_seg=None, max_ctrl=None):
        """the global trajectory's local segment -> loadSamples' fit, without leaving the device
        (fuelmi_bspline_dev_load_local_segments): one problem per candidate, states / problems as SDFMap.local_segments
        takes them, the degree and the point count the batch's.  Returns (status [C], duration [C]); a candidate whose
        status is not LOCALSEG_OK (LOCALSEG_MISFIT: another point count than the batch's) keeps its state."""
        c = self.problem.c
        if len(problems) != c.n_traj:
            raise ValueError("load_local_segments: one problem per candidate")
        lc, nt, st_arr, n, pr_arr = _pack_localseg(states, problems, self.degree, max_seg, max_ctrl)
        o, out = _outputs(c.n_traj, [("status", _I, ()), ("duration", _D, ())])
        check(self.L.fuelmi_bspline_dev_load_local_segments(self.h, lc.max_seg, lc.max_ctrl, nt, *[_ptr(a) for a in st_arr],
                                                            *[_ptr(a) for a in pr_arr], *out))
        return o["status"], o["duration"]

    def load_kino(self, starts, vels, accs, goals, goal_vels, allow_limit=False, **cfg):
        """start / goal -> kinodynamic search -> getSamples -> loadSamples' fit, without leaving the device
        (fuelmi_bspline_dev_load_kino): one problem per candidate, seg_num forced to point_num - bspline_degree.  Returns
        (status [C], T_sum [C]); a candidate without a path keeps its state."""
        _, o, _ = _kino((starts, vels, accs, goals, goal_vels), cfg, self.problem.c.n_traj,
                        lambda kc: [("status", _I, ()), ("T_sum", _D, ())], allow_limit,
                        lambda kc, n, *a: self.L.fuelmi_bspline_dev_load_kino(self.h, kc, *a))
        return o["status"], o["T_sum"]

    def plan_yaws(self, start_yaw, end_yaw=None, derivs=True, allow_limit=False, **cfg):
        """The yaw trajectories of the candidates' optimised position splines, read from what the last optimize() left
        on the device (fuelmi_bspline_dev_plan_yaws); the batch's own weights.  Same result dict as SDFMap.plan_yaws."""
        c = self.problem.c
        cfg.setdefault("pos_degree", 3)
        return _plan_yaws(c.n_traj, yaw_cfg(max_ctrl=c.point_num, **cfg), start_yaw, end_yaw, derivs, allow_limit,
                          lambda *a: self.L.fuelmi_bspline_dev_plan_yaws(self.h, *a))

    def solve_quadratic(self, cost_function=GUIDE_PHASE, guide_pts=None, bounds=False):
        """The exact minimiser of a quadratic mask on what the batch holds (fuelmi_bspline_dev_solve_quadratic); the
        solution of every QUAD_OK candidate becomes the batch's variables, the next optimize() starts from it.  guide_pts
        [C, point_num - 2 order, 3]: this phase's guide points (None: the batch's own).  Returns a dict: status [C], ctrl_out
        [C, point_num, dim], cost [C], pt_dist [C]."""
        c = self.problem.c
        n = c.n_traj
        g = None if guide_pts is None else np.ascontiguousarray(guide_pts, dtype=np.float64)
        order = 3 if c.dim == 1 else self.degree
        if g is not None and g.size != n * max(c.point_num - 2 * order, 0) * 3:
            raise ValueError("solve_quadratic: guide_pts [C][point_num - 2 order][3]")
        qc = QuadCfg(int(cost_function), c.dim, c.point_num, max(c.end_n, 1), c.n_waypt, 1 if bounds else 0)
        return _solve_quadratic(n, qc, lambda q, *out: self.L.fuelmi_bspline_dev_solve_quadratic(self.h, q, _dp(g), *out))

    def check_trajs(self, t_now, allow_limit=False, **cfg):
        """The safety check of the candidates' optimised position splines against the batch's map, read from what the last
        optimize() left on the device (fuelmi_bspline_dev_check_trajs).  Same result dict as SDFMap.check_trajs."""
        c = self.problem.c
        cfg.setdefault("degree", 3)
        tc = traj_check_cfg(max_ctrl=c.point_num, **cfg)
        return _check_trajs(c.n_traj, t_now, allow_limit,
                            lambda *a: self.L.fuelmi_bspline_dev_check_trajs(self.h, C.byref(tc), *a))

    def sample_trajs(self, t, yaw_ctrl=None, yaw_dt=None, t_stop=None, flight=None, max_yaw_ctrl=None, max_t=None, **cfg):
        """The candidates' optimised position splines sampled as commands or replan states, read from what the last
        optimize() left on the device (fuelmi_bspline_dev_sample_trajs).  Arguments and result dict as
        SDFMap.sampleTrajs from t on."""
        c = self.problem.c
        n = c.n_traj
        cfg.setdefault("degree", 3)
        args, o, maxy, maxt = _trajsmp_io(n, t, yaw_ctrl, yaw_dt, t_stop, flight, max_yaw_ctrl, max_t)
        sc = traj_sample_cfg(max_ctrl=c.point_num, max_yaw_ctrl=maxy, max_t=maxt, **cfg)
        check(self.L.fuelmi_bspline_dev_sample_trajs(self.h, C.byref(sc), *args))
        return o

    def adjust_trajs(self, knots_in=None, ratio_in=None, group=None, ops=0, max_samples=None, n_group=None, **cfg):
        """The candidates' optimised position splines adjusted, measured and ranked, read from what the last optimize()
        left on the device (fuelmi_bspline_dev_adjust_trajs).  Arguments and result dict as SDFMap.adjust_trajs from
        knots_in on."""
        c = self.problem.c
        n = c.n_traj
        degree = int(cfg.setdefault("degree", 3))
        n_ctrl = np.full(n, c.point_num, dtype=np.int32)
        args, o, maxs, ng = _trajadj_io(n, n_ctrl, degree, c.point_num, knots_in, ratio_in, group, int(ops), max_samples,
                                        n_group)
        ac = traj_adjust_cfg(ops=ops, max_ctrl=c.point_num, max_samples=maxs, n_group=ng, **cfg)
        check(self.L.fuelmi_bspline_dev_adjust_trajs(self.h, C.byref(ac), *args))
        return _trajadj_named(o)

    KNOTS_UNIFORM, KNOTS_ADJUSTED = _lib.KNOTS_UNIFORM, _lib.KNOTS_ADJUSTED

    def set_knot_source(self, source):
        """Which knots check_trajs / sample_trajs / plan_yaws put under the candidates' position splines: KNOTS_UNIFORM
        (the default) or KNOTS_ADJUSTED, the knots the last adjust_trajs() left on the device
        (fuelmi_bspline_dev_set_knot_source).  KNOTS_ADJUSTED raises unless adjust_trajs() has run since the last
        optimize(); a reload or another optimize() puts the source back to KNOTS_UNIFORM."""
        check(self.L.fuelmi_bspline_dev_set_knot_source(self.h, int(source)))

    @property
    def knot_source(self):
        return int(self.L.fuelmi_bspline_dev_knot_source(self.h))

    def close(self):
        if getattr(self, "h", None):
            self.L.fuelmi_bspline_dev_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
