"""The scenes of HeadingPlanner's information gain and yaw search (fuel_amd/csrc/info_gain.hip): tests/test_heading_cpu.py
proves on the host that each sits on the edge it is drawn for and compares the restatement (tests/heading_ref.py) with the
recordings of the reference's own code, tests/test_heading_gpu.py runs them on the device,
tests/golden/make_heading_golden.py records them.

Maps: 64 x 64 x 24 voxels at 0.1 m (origin (-3.2, -3.2, -1)), far 1.2 .. 1.6 m, so a group is a few hundred subsampled
cells; one 128 x 128 x 32 map for the scene at the reference's defaults.  A map is (unknown cells, occupied cells,
exploration box); every cell that is neither is known free.
  open      all unknown, no obstacle
  wall      all unknown but a known occupied wall across the frustum of a camera at the origin looking along +x
  bubble    `wall` with a known-free ball of 0.6 m round that camera
  inner     all unknown, the exploration box well inside the map: boundBox clamps, isInBox cuts
  stripes   all unknown but an occupied ring in the ground layer (z index 0) round the camera's x, y and every third y
            index of the wall x index 0: the rays of a camera BELOW (beside) the map pass ray voxels that
            int(ray + offset) truncates to index 0 where floor would leave the map
  count_N   everything known free but exactly N of the candidate cells of COUNT_VIEW: the ballot windows
  mid       128 x 128 x 32, pillars, the half x < 0 known free

A gain scene is a dict: tag, kind "gain", map, pos, yaws, cfg (heading_ref.gain_cfg fields), ctrl, expect.
A path scene: tag, kind "path", map, pts, yaws, dt, ctrl, h, yaw_diff, max_yaw_rate, w, cfg, gains_in, expect,
assert_path (NON_UNIFORM scenes whose path the tests assert must have a decision margin, see test_heading_cpu.py).
Nothing here needs a GPU."""
import math

import numpy as np

import heading_ref as hr

RES, GROUND = 0.1, -1.0
L_FREE, L_OCC = math.log(0.12 / 0.88), math.log(0.9 / 0.1)
L_UNK = L_FREE - 0.01  # clamp_min_log - unknown_flag (sdf_map.cpp:55)
SMALL, MID = (6.4, 6.4, 2.4), (12.8, 12.8, 3.2)
CAM = (0.02, 0.03, 0.21)  # off the voxel centres
COUNTS = (0, 1, 63, 64, 65, 129)
COUNT_VIEW = dict(pos=CAM, yaw=0.3, cfg=dict(far=1.6, factor=2))
PI = math.pi
_MAPS, _REST = {}, {}


class MapSpec:
    def __init__(self, name, map_size, unk, occ, box_min=None, box_max=None):
        self.name, self.map_size = name, map_size
        self.origin = (-map_size[0] / 2.0, -map_size[1] / 2.0, GROUND)
        self.nvox = tuple(int(math.ceil(map_size[i] / RES)) for i in range(3))
        assert unk.shape == self.nvox and not (unk & occ).any()
        self.unk, self.occ = unk, occ
        self.box_min = tuple(box_min) if box_min is not None else self.origin
        self.box_max = tuple(box_max) if box_max is not None else tuple(self.origin[i] + map_size[i] for i in range(3))
        self.kw = dict(resolution=RES, ground_height=GROUND)

    def log_odds(self):
        return np.where(self.unk, L_UNK, np.where(self.occ, L_OCC, L_FREE))

    def ref(self, res_inv=None):
        return hr.Map(self.origin, RES, self.unk, self.occ, self.box_min, self.box_max, res_inv)


def _nv(size):
    return tuple(int(math.ceil(s / RES)) for s in size)


def _centres(nv, origin):
    return np.meshgrid(*[(np.arange(n) + 0.5) * RES + o for n, o in zip(nv, origin)], indexing="ij")


def _build(name):
    nv = _nv(SMALL)
    org = (-3.2, -3.2, GROUND)
    unk, occ = np.ones(nv, dtype=bool), np.zeros(nv, dtype=bool)
    if name == "open":
        return MapSpec(name, SMALL, unk, occ)
    if name in ("wall", "bubble"):
        occ[40:42, 26:40, 8:20] = True  # x = 0.8 .. 1.0 m, half the frustum's width
        unk &= ~occ
        if name == "bubble":
            X, Y, Z = _centres(nv, org)
            ball = (X - CAM[0]) ** 2 + (Y - CAM[1]) ** 2 + (Z - CAM[2]) ** 2 < 0.6 ** 2
            unk &= ~ball
        return MapSpec(name, SMALL, unk, occ)
    if name == "inner":
        return MapSpec(name, SMALL, unk, occ, (-2.0, -1.5, -0.5), (2.0, 1.5, 0.9))
    if name == "stripes":
        X, Y, _ = _centres(nv, org)
        d = np.sqrt((X[:, :, 0] - CAM[0]) ** 2 + (Y[:, :, 0] - CAM[1]) ** 2)
        occ[:, :, 0] = (d > 0.12) & (d < 0.3)
        occ[0, ::3, :] = True
        unk &= ~occ
        return MapSpec(name, SMALL, unk, occ)
    if name.startswith("count_"):
        n = int(name[6:])
        m = spec("open").ref()
        cells = hr.view(m, hr.gain_cfg(**COUNT_VIEW["cfg"]), COUNT_VIEW["pos"], COUNT_VIEW["yaw"])
        assert len(cells) >= max(COUNTS)
        keep = np.zeros(nv, dtype=bool)
        pick = np.random.default_rng(11).permutation(len(cells))[:n]
        for k in pick:
            keep[cells[k][0]] = True
        return MapSpec(name, SMALL, keep, occ)
    if name == "mid":
        nv = _nv(MID)
        unk, occ = np.ones(nv, dtype=bool), np.zeros(nv, dtype=bool)
        rng = np.random.default_rng(7)
        for _ in range(40):
            x, y = rng.integers(4, nv[0] - 8), rng.integers(4, nv[1] - 8)
            occ[x:x + rng.integers(2, 5), y:y + rng.integers(2, 5), 0:rng.integers(10, nv[2])] = True
        unk[:nv[0] // 2] = False
        unk &= ~occ
        return MapSpec(name, MID, unk, occ)
    raise KeyError(name)


def spec(name):
    if name not in _MAPS:
        _MAPS[name] = _build(name)
    return _MAPS[name]


def gscene(tag, map_, pos, yaws, ctrl=None, expect=None, **cfg):
    cfg.setdefault("far", 1.4)
    return dict(tag=tag, kind="gain", map=map_, pos=tuple(float(v) for v in pos), yaws=[float(y) for y in yaws],
                cfg=hr.gain_cfg(**cfg), ctrl=None if ctrl is None else np.array(ctrl, dtype=np.float64).reshape(-1, 3),
                expect=dict(expect or {}))


def pscene(tag, map_, pts, yaws, dt=0.5, ctrl=None, h=1, yaw_diff=0.3, max_yaw_rate=1.0, w=10.0, gains_in=None,
           expect=None, assert_path=True, **cfg):
    cfg.setdefault("far", 1.3)
    return dict(tag=tag, kind="path", map=map_, pts=np.array(pts, dtype=np.float64).reshape(-1, 3),
                yaws=[float(y) for y in yaws], dt=float(dt),
                ctrl=None if ctrl is None else np.array(ctrl, dtype=np.float64).reshape(-1, 3), h=int(h),
                yaw_diff=float(yaw_diff), max_yaw_rate=float(max_yaw_rate), w=float(w),
                gains_in=None if gains_in is None else np.array(gains_in, dtype=np.float64), cfg=hr.gain_cfg(**cfg),
                expect=dict(expect or {}), assert_path=assert_path)


CTRL3 = [(-0.5, 0.0, 0.2), (0.3, 0.1, 0.2), (1.1, 0.4, 0.3)]
NU = hr.NON_UNIFORM


def gain_scenes():
    s = [
        # box, subsampling, frustum and in_box on an empty map: every candidate is visible
        gscene("open_1", "open", CAM, [0.0]),
        gscene("open_1_nobox", "open", CAM, [0.0], in_box=False),
        gscene("open_2", "open", CAM, [0.4, -2.0]),
        gscene("open_11", "open", CAM, [0.1 + 0.2 * (j - 5) for j in range(11)]),
        gscene("open_cap", "open", CAM, [0.2 * j for j in range(hr.MAX_YAW)], far=1.2),
        gscene("open_pi", "open", CAM, [PI, -PI, math.nextafter(PI, 4.0)]),
        gscene("open_factor1", "open", CAM, [0.7], far=1.2, factor=1),
        gscene("open_factor3", "open", CAM, [0.7, 2.2], factor=3),
        # shadows
        gscene("wall_1", "wall", CAM, [0.0]),
        gscene("wall_11", "wall", CAM, [0.15 * (j - 5) for j in range(11)], far=1.6),
        gscene("bubble_3", "bubble", CAM, [-0.4, 0.0, 0.4], far=1.6),
        # the exploration box: a camera at its edge (boundBox clamps), outside it looking away (ub < lb), in_box on / off
        gscene("inner_edge", "inner", (1.0, 0.02, 0.2), [0.0, 0.5]),
        gscene("inner_edge_nobox", "inner", (1.0, 0.02, 0.2), [0.0, 0.5], in_box=False),
        gscene("inner_empty", "inner", (2.5, 0.02, 0.2), [0.0], expect=dict(n_cand=[0], n_rays=0, cells=0)),
        gscene("inner_corner", "inner", (-1.9, -1.4, 0.8), [0.8, 2.4, -2.4]),
        # the map's edge: a camera below the map (ray voxels truncate toward zero), one beside it
        gscene("stripes_below", "stripes", (0.02, 0.03, -1.17), [0.0, 1.0], in_box=False),
        gscene("stripes_beside", "stripes", (-3.33, 0.03, -0.8), [0.0], in_box=False),
        gscene("open_outside_corner", "open", (3.0, 3.0, 1.3), [PI / 4, -3 * PI / 4]),
        # the weights
        gscene("nu_one_ctrl", "wall", CAM, [0.0, 0.3], ctrl=[(0.5, 0.0, 0.2)], weight_type=NU),
        gscene("nu_nearest_first", "open", CAM, [0.0], ctrl=[(0.9, 0.0, 0.2), (-1.0, 0.0, 0.2), (-2.0, 0.5, 0.2)],
               weight_type=NU),
        gscene("nu_nearest_last", "open", CAM, [0.0], ctrl=[(-2.0, 0.5, 0.2), (-1.0, 0.0, 0.2), (0.9, 0.0, 0.2)],
               weight_type=NU),
        gscene("nu_equal_first_wins", "open", CAM, [0.0, 0.5], ctrl=[(0.9, 0.0, 0.2), (-1.0, 0.0, 0.2), (0.9, 0.0, 0.2)],
               weight_type=NU),
        gscene("nu_wall_11", "wall", CAM, [0.15 * (j - 5) for j in range(11)], ctrl=CTRL3, weight_type=NU, far=1.6),
        gscene("nu_lambdas", "bubble", CAM, [0.2], ctrl=CTRL3, weight_type=NU, lambda1=0.3, lambda2=4.0, far=1.6),
    ]
    for n in COUNTS:
        s.append(gscene("count_%d" % n, "count_%d" % n, COUNT_VIEW["pos"], [COUNT_VIEW["yaw"]],
                        expect=dict(n_cand=[n], n_visible=[n], n_rays=n), **COUNT_VIEW["cfg"]))
        s.append(gscene("count_%d_3" % n, "count_%d" % n, COUNT_VIEW["pos"],
                        [COUNT_VIEW["yaw"] - 0.2, COUNT_VIEW["yaw"], COUNT_VIEW["yaw"] + 0.2], **COUNT_VIEW["cfg"]))
    return s


def _line(n, start=(-0.6, 0.02, 0.21), step=(0.25, 0.04, 0.0)):
    return [tuple(start[k] + i * step[k] for k in range(3)) for i in range(n)]


def path_scenes():
    eq = np.full((4, 5), 2.5)
    worse_first = np.zeros((4, 3))
    worse_first[1] = (1.0, 5.0, 3.0)   # layer 1: vertex 1 is best
    worse_first[2] = (2.0, 2.0, 2.0)   # layer 2: every vertex's first predecessor (vertex 0 of layer 1) is worse
    at_rate = np.zeros((4, 3))
    at_rate[1] = (1.0, 2.0, 3.0)
    at_rate[2] = (3.0, 2.0, 1.0)
    s = [
        pscene("layers_1", "open", _line(1), [0.3], weight_type=hr.UNIFORM, expect=dict(path=[0.3], n_rays=[0])),
        pscene("layers_2", "open", _line(2), [0.3, 0.5], weight_type=hr.UNIFORM, expect=dict(path=[0.3, 0.5], n_rays=[0, 0])),
        pscene("layers_3", "wall", _line(3), [0.0, 0.2, 0.1], weight_type=hr.UNIFORM),
        pscene("layers_7_h0", "wall", _line(7), [0.1 * i for i in range(7)], h=0, weight_type=hr.UNIFORM),
        pscene("layers_7_h5", "bubble", _line(7), [0.0] * 7, h=5, yaw_diff=0.2, weight_type=hr.UNIFORM, w=3.0, far=1.6),
        pscene("layers_max", "wall", _line(hr.MAX_LAYER, step=(0.02, 0.0, 0.0)), [0.01 * i for i in range(hr.MAX_LAYER)],
               h=1, weight_type=hr.UNIFORM, far=1.2),
        pscene("nu_layers_5", "wall", _line(5), [0.0, 0.1, 0.0, -0.1, 0.0], ctrl=_line(8, step=(0.2, 0.03, 0.0)), h=2,
               weight_type=NU, far=1.6, w=0.37),
        pscene("nu_layers_3_pi", "bubble", _line(3), [PI, -PI, PI], ctrl=CTRL3, h=1, weight_type=NU, far=1.6, w=0.37),
        # the recurrence on given gains: exact numbers
        pscene("in_all_equal", "open", _line(4), [0.0] * 4, h=2, gains_in=eq, max_yaw_rate=100.0,
               expect=dict(path_vertex=[0, 4, 4, 0])),
        pscene("in_first_worse", "open", _line(4), [0.0] * 4, h=1, gains_in=worse_first, max_yaw_rate=100.0,
               expect=dict(path_vertex=[0, 1, 2, 0])),
        pscene("in_at_rate", "open", _line(4), [0.0] * 4, h=1, yaw_diff=0.5, dt=1.0, max_yaw_rate=0.5, w=8.0,
               gains_in=at_rate),
        pscene("in_over_rate", "open", _line(4), [0.0] * 4, h=1, yaw_diff=0.5, dt=1.0, max_yaw_rate=0.25, w=8.0,
               gains_in=at_rate),
    ]
    return s


def mid_scene():
    """the reference's defaults: far 4.5, 11 yaws, 7 layers, NON_UNIFORM with topo_algorithm.xml's parameters"""
    pts = [(-0.9 + 0.45 * i, -2.1 + 0.3 * i, 0.31 + 0.05 * i) for i in range(7)]
    return pscene("mid_defaults", "mid", pts, [0.55 + 0.04 * i for i in range(7)], dt=0.4,
                  ctrl=[(-1.5 + 0.4 * i, -2.5 + 0.27 * i, 0.3) for i in range(12)], h=5, yaw_diff=5 * 3.1415926 / 180.0,
                  max_yaw_rate=60 * 3.1415926 / 180.0, w=10.0, weight_type=NU, far=4.5)


def all_scenes():
    return gain_scenes() + path_scenes() + [mid_scene()]


def restate(sc, order="device"):
    """the restatement's result of a scene, computed once"""
    key = (sc["tag"], order)
    if key not in _REST:
        m = spec(sc["map"]).ref()
        if sc["kind"] == "gain":
            _REST[key] = hr.info_gains(m, sc["cfg"], sc["pos"], sc["yaws"], sc["ctrl"], order)
        else:
            _REST[key] = hr.search_path_of_yaw(m, sc["cfg"], sc["pts"], sc["yaws"], sc["dt"], sc["ctrl"], sc["h"],
                                               sc["yaw_diff"], sc["max_yaw_rate"], sc["w"], sc["gains_in"], order)
    return _REST[key]


def parity_pairs():
    """(gain in the reference's order, gain in the device's order) of every NON_UNIFORM view of every scene"""
    out = []
    for sc in all_scenes():
        if sc["cfg"]["weight_type"] != NU or (sc["kind"] == "path" and sc["gains_in"] is not None):
            continue
        a, b = restate(sc, "reference"), restate(sc, "device")
        ga = a["gain"] if sc["kind"] == "gain" else [g for row in a["gains"] for g in row]
        gb = b["gain"] if sc["kind"] == "gain" else [g for row in b["gains"] for g in row]
        out += list(zip(ga, gb))
    return out
