"""The maps and scenes of the cloud extraction (fuel_amd/csrc/map_cloud.hip): tests/test_map_cloud_cpu.py proves on the
host that each scene sits on the edge it is drawn for, tests/test_map_cloud_gpu.py runs them on the device, every scene
with every kind.

A map state is a hand-written f64 log-odds array (uploaded with uploadOccupancy) and its inflation in numpy.  A scene is a
dict: tag, map, state, lo, hi (inclusive voxel box), z_low, z_high and pred: a function of (scene, clouds) -- clouds[kind]
the restatement's cloud of the scene -- that is true iff the scene sits on its edge.  The sizes that depend on the
kernels' geometry (items per workgroup, the scan's width) are read from fuelmi_cloud_plan, which needs no device."""
import math

import numpy as np

import map_cloud_ref as mr

P_MIN, P_OCC, P_MAX = 0.12, 0.80, 0.90  # DEFAULT_MAP
CLAMP_MIN, MIN_OCC, CLAMP_MAX = mr.logit(P_MIN), mr.logit(P_OCC), mr.logit(P_MAX)
THR = CLAMP_MIN - 1e-3                                # the unknown threshold
V_UNKNOWN, V_FREE, V_OCC = CLAMP_MIN - 0.01, CLAMP_MIN, CLAMP_MAX  # the initial value (sdf_map.cpp:61), the clamps
INFLATION = 0.199
UP, DOWN = np.inf, -np.inf

# name -> voxels, resolution, ground height.  map_size = (n - 0.25) * resolution: ceil() gives n whatever the division
# rounds to, and no origin sits on the voxel grid
MAPS = {
    "a": ((24, 20, 25), 0.1, -1.0),     # nz odd and coprime to 64: the 480 lines start at every bit offset
    "b": ((6, 5, 130), 0.1, -1.0),      # three chunks per line, the last one 2 bits wide
    "c1": ((3, 3, 64), 0.1, -1.0),      # lines exactly word-aligned
    "c2": ((3, 2, 128), 0.1, -1.0),
    "d": ((24, 20, 25), 0.15, -0.37),   # positions that are no short decimals
    "f": ((260, 3, 5), 0.1, -1.0),      # long in x: boxes of 257 and 513 lines
}


def plan(dims, lo, hi):
    import fuel_amd.host as fh
    return fh.cloud_plan(dims, lo, hi)


def full_box(nvox):
    return (0, 0, 0), tuple(n - 1 for n in nvox)


class MapSpec:
    def __init__(self, name, nvox=None, res=None, ground=None):
        if nvox is None:
            nvox, res, ground = MAPS[name]
        self.name, self.nvox, self.res = name, tuple(nvox), res
        self.map_size = tuple((n - 0.25) * res for n in nvox)
        self.kw = dict(resolution=res, ground_height=ground)
        self.origin = np.array([-self.map_size[0] / 2.0, -self.map_size[1] / 2.0, ground])  # SDFMap::initMap
        self.P = mr.Params(res, self.origin, MIN_OCC, CLAMP_MIN)
        self.step = int(math.ceil(INFLATION / res))
        self._states = {}

    def initmap_nvox(self):
        return tuple(int(math.ceil(self.map_size[i] / self.res)) for i in range(3))

    def state(self, name):
        """(occ3, infl3) of a named state"""
        if name not in self._states:
            occ = STATES[name](self)
            self._states[name] = (occ, mr.inflate(self.P, occ, self.step))
        return self._states[name]

    def pos_z(self, z):
        return float(mr.axis_pos(self.P, z, 2))


_SPECS = {}


def spec(name):
    if name not in _SPECS:
        _SPECS[name] = MapSpec(name)
    return _SPECS[name]


# ---- states ---------------------------------------------------------------------------------------------------------------
LEAK_BOX = ((5, 4, 6), (11, 9, 17))  # of maps a / d: strictly inside, z range inside one or two words of every line
ONE_BOX = ((3, 2, 1), (20, 17, 23))


def st_fresh(m):
    return np.full(m.nvox, V_UNKNOWN)


def st_free(m):
    return np.full(m.nvox, V_FREE)


def st_random(m):
    """about half unknown, 45 % free, 5 % occupied (the occupied share of fuel_amd/synth's explored state)"""
    rng = np.random.default_rng(sum(m.nvox) * 7 + int(m.res * 100))
    r = rng.random(m.nvox)
    return np.where(r < 0.5, V_UNKNOWN, np.where(r < 0.95, V_FREE, V_OCC))


def _shell(m, inside, outside):
    occ = np.full(m.nvox, outside)
    lo, hi = LEAK_BOX
    occ[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = inside
    return occ


def _single(m, v, fg, bg):
    occ = np.full(m.nvox, bg)
    occ[tuple(v)] = fg
    return occ


def _stripes(m, fg, bg):
    """even lines: chunk 0 full and chunk 1 empty; odd lines the other way round"""
    occ = np.full(m.nvox, bg)
    line = (np.arange(m.nvox[0])[:, None] * m.nvox[1] + np.arange(m.nvox[1])[None, :]) % 2
    z = np.arange(m.nvox[2])[None, None, :]
    occ[((line[:, :, None] == 0) & (z < 64)) | ((line[:, :, None] == 1) & (z >= 64) & (z < 128))] = fg
    return occ


THR_VALUES = [MIN_OCC, np.nextafter(MIN_OCC, UP), np.nextafter(MIN_OCC, DOWN), np.nextafter(THR, UP), np.nextafter(THR, DOWN),
              V_FREE, V_UNKNOWN, V_OCC]


def st_thr(m):
    """every value next to a threshold, none ON the unknown threshold"""
    n = m.nvox[0] * m.nvox[1] * m.nvox[2]
    return np.array(THR_VALUES)[np.arange(n) % len(THR_VALUES)].reshape(m.nvox)


def st_thr_exact(m):
    """... and the unknown threshold itself in every third voxel: the documented deviation of KNOWN"""
    occ = st_thr(m).reshape(-1).copy()
    occ[::3] = THR
    return occ.reshape(m.nvox)


STATES = {
    "fresh": st_fresh,  # as created: UNKNOWN returns every voxel, KNOWN none
    "free": st_free,    # nothing set in the occupied, unknown and inflated planes
    "random": st_random,
    "leak_occ": lambda m: _shell(m, V_FREE, V_OCC),          # occupied (and known) everywhere but inside LEAK_BOX
    "leak_unk": lambda m: _shell(m, V_FREE, V_UNKNOWN),      # unknown everywhere but inside
    "leak_known": lambda m: _shell(m, V_UNKNOWN, V_FREE),    # known everywhere but inside
    "one_occ_first": lambda m: _single(m, ONE_BOX[0], V_OCC, V_FREE),
    "one_occ_last": lambda m: _single(m, ONE_BOX[1], V_OCC, V_FREE),
    "one_unk_first": lambda m: _single(m, ONE_BOX[0], V_UNKNOWN, V_FREE),
    "one_unk_last": lambda m: _single(m, ONE_BOX[1], V_UNKNOWN, V_FREE),
    "one_known_first": lambda m: _single(m, ONE_BOX[0], V_FREE, V_UNKNOWN),
    "one_known_last": lambda m: _single(m, ONE_BOX[1], V_FREE, V_UNKNOWN),
    "stripes_occ": lambda m: _stripes(m, V_OCC, V_FREE),
    "stripes_unk": lambda m: _stripes(m, V_UNKNOWN, V_FREE),
    "thr": st_thr,
    "thr_exact": st_thr_exact,
}
DEVIATION_STATE = "thr_exact"


def state_is_off_threshold(occ3):
    """no log-odds value on the unknown threshold and no NaN: KNOWN as the plane's complement equals the reference's test"""
    return not np.isnan(occ3).any() and not (occ3 == THR).any()


# ---- scenes ---------------------------------------------------------------------------------------------------------------
def scene(tag, map_, state, lo, hi, z_low=DOWN, z_high=UP, pred=None):
    return dict(tag=tag, map=map_, state=state, lo=tuple(int(v) for v in lo), hi=tuple(int(v) for v in hi),
                z_low=float(z_low), z_high=float(z_high), pred=pred)


def restate(sc, kind, occ3=None, infl3=None, known_as="reference"):
    m = spec(sc["map"])
    o, i = m.state(sc["state"])
    return mr.extract(m.P, o if occ3 is None else occ3, i if infl3 is None else infl3, kind, sc["lo"], sc["hi"],
                      sc["z_low"], sc["z_high"], known_as)


def box_voxels(sc):
    return int(np.prod([max(sc["hi"][k] - sc["lo"][k] + 1, 0) for k in range(3)]))


def items_of(sc):
    p = plan(spec(sc["map"]).nvox, sc["lo"], sc["hi"])
    return p["items_per_line"] * p["lines"]


def box_with_items(k):
    """(map, lo, hi): a box of exactly k work items with a full z extent, away from the low faces where it fits"""
    for name in ("a", "f"):
        nx, ny, nz = spec(name).nvox
        cpl = (nz + 63) // 64
        if k % cpl:
            continue
        lines = k // cpl
        for ylen in range(min(ny, lines), 0, -1):
            if lines % ylen == 0 and lines // ylen <= nx:
                xlen = lines // ylen
                x0, y0 = min(1, nx - xlen), min(1, ny - ylen)
                return name, (x0, y0, 0), (x0 + xlen - 1, y0 + ylen - 1, nz - 1)
    raise ValueError("no box of %d items" % k)


def p_mixed(sc, clouds):  # a general box: something selected and something not, for the three occupancy kinds
    v = box_voxels(sc)
    return all(0 < len(clouds[k]) < v for k in (mr.OCCUPIED, mr.UNKNOWN, mr.KNOWN))


def p_items(k):
    return lambda sc, clouds: items_of(sc) == k and len(clouds[mr.UNKNOWN]) + len(clouds[mr.KNOWN]) == box_voxels(sc)


def p_leak(kind):
    """nothing of the kind inside the box; every voxel just outside each of its six faces is set: z - 1 and z + 1 lie in the
    same words as the box's bits, the y-lines either side are the adjacent bits, the x-slabs either side a slab away"""
    def pred(sc, clouds):
        m = spec(sc["map"])
        sel = mr.select(m.P, *m.state(sc["state"]), kind)
        lo, hi = sc["lo"], sc["hi"]
        faces = []
        for a in range(3):
            for at in (lo[a] - 1, hi[a] + 1):
                sl = [slice(lo[k], hi[k] + 1) for k in range(3)]
                sl[a] = at
                faces.append(bool(sel[tuple(sl)].all()))
        return len(clouds[kind]) == 0 and all(faces)
    return pred


def p_single(kind, which):
    def pred(sc, clouds):
        m = spec(sc["map"])
        v = sc["lo"] if which == "first" else sc["hi"]
        return len(clouds[kind]) == 1 and np.array_equal(clouds[kind][0], mr.index_to_pos(m.P, v).astype(np.float32))
    return pred


def p_stripes(kind):
    def pred(sc, clouds):
        m = spec(sc["map"])
        sel = mr.select(m.P, *m.state(sc["state"]), kind)
        return bool(sel[0, 0, :64].all() and not sel[0, 0, 64:].any() and not sel[0, 1, :64].any() and sel[0, 1, 64:128].all())
    return pred


def p_thr(sc, clouds):
    m = spec(sc["map"])
    occ, infl = m.state(sc["state"])
    o = mr.select(m.P, occ, infl, mr.OCCUPIED)
    u = mr.select(m.P, occ, infl, mr.UNKNOWN)
    return bool(not o[occ == MIN_OCC].any() and o[occ == np.nextafter(MIN_OCC, UP)].all() and (occ == MIN_OCC).any()
                and not u[occ == np.nextafter(THR, UP)].any() and u[occ == np.nextafter(THR, DOWN)].all()
                and (occ == np.nextafter(THR, DOWN)).any() and state_is_off_threshold(occ))


def p_deviation(sc, clouds):
    """on the threshold the reference's KNOWN test is false and the plane's complement true: exactly those voxels differ"""
    m = spec(sc["map"])
    occ, _ = m.state(sc["state"])
    n_on = int((occ == THR).sum())
    plane = restate(sc, mr.KNOWN, known_as="plane")
    return n_on > 0 and len(plane) == len(clouds[mr.KNOWN]) + n_on


def p_layers(kind, dropped_layers):
    """the truncation drops exactly the voxels of `dropped_layers` z-layers of the (full-height) box, and some are dropped"""
    def pred(sc, clouds):
        m = spec(sc["map"])
        allpts = restate(dict(sc, z_low=DOWN, z_high=UP), kind)
        zs = np.float32(mr.axis_pos(m.P, np.array(dropped_layers, dtype=np.int64), 2))
        want = allpts[~np.isin(allpts[:, 2], zs)]
        ok = np.array_equal(want, clouds[kind])
        return ok and (not dropped_layers or len(want) < len(allpts))
    return pred


def _scenes():
    S = []
    # --- box placement ---
    for name in MAPS:
        m = spec(name)
        S.append(scene("whole_" + name, name, "random", *full_box(m.nvox), pred=p_mixed))
    S.append(scene("one_voxel", "a", "random", (7, 9, 11), (7, 9, 11), pred=lambda sc, c: box_voxels(sc) == 1))
    S.append(scene("one_line", "a", "random", (7, 9, 0), (7, 9, 24), pred=lambda sc, c: items_of(sc) == 1))
    S.append(scene("one_line_b", "b", "random", (2, 3, 0), (2, 3, 129), pred=lambda sc, c: items_of(sc) == 3))
    S.append(scene("part_line_b", "b", "random", (1, 1, 3), (4, 3, 68), pred=lambda sc, c: items_of(sc) == 24))  # 64 + 2 bits
    wg = plan(spec("a").nvox, *full_box(spec("a").nvox))["items_per_workgroup"]
    for k in sorted({1, 63, 64, 65, wg - 1, wg, wg + 1, 2 * wg + 1}):
        name, lo, hi = box_with_items(k)
        S.append(scene("items_%d" % k, name, "random", lo, hi, pred=p_items(k)))
    nx, ny, nz = spec("a").nvox
    faces = {"x0": ((0, 3, 4), (2, 7, 9)), "x1": ((nx - 3, 3, 4), (nx - 1, 7, 9)), "y0": ((3, 0, 4), (7, 2, 9)),
             "y1": ((3, ny - 3, 4), (7, ny - 1, 9)), "z0": ((3, 4, 0), (7, 9, 2)), "z1": ((3, 4, nz - 3), (7, 9, nz - 1))}
    for f, (lo, hi) in faces.items():
        for name in ("a", "d"):
            S.append(scene("face_%s_%s" % (f, name), name, "random", lo, hi, pred=p_mixed))
    # --- leakage ---
    for kind, st in ((mr.OCCUPIED, "leak_occ"), (mr.UNKNOWN, "leak_unk"), (mr.KNOWN, "leak_known")):
        S.append(scene(st, "a", st, *LEAK_BOX, pred=p_leak(kind)))
    # --- density ---
    for name in ("a", "b", "c1", "c2"):
        m = spec(name)
        S.append(scene("fresh_" + name, name, "fresh", *full_box(m.nvox),
                       pred=lambda sc, c: len(c[mr.UNKNOWN]) == box_voxels(sc) and len(c[mr.KNOWN]) == 0))
        S.append(scene("free_" + name, name, "free", *full_box(m.nvox),
                       pred=lambda sc, c: len(c[mr.OCCUPIED]) == len(c[mr.UNKNOWN]) == len(c[mr.INFLATED]) == 0
                       and len(c[mr.KNOWN]) == box_voxels(sc)))
    S.append(scene("fresh_part_a", "a", "fresh", (2, 3, 5), (21, 18, 22),
                   pred=lambda sc, c: len(c[mr.UNKNOWN]) == box_voxels(sc)))
    for kind, key in ((mr.OCCUPIED, "occ"), (mr.UNKNOWN, "unk"), (mr.KNOWN, "known")):
        for which in ("first", "last"):
            st = "one_%s_%s" % (key, which)
            S.append(scene(st, "a", st, *ONE_BOX, pred=p_single(kind, which)))
    S.append(scene("stripes_occ", "b", "stripes_occ", *full_box(spec("b").nvox), pred=p_stripes(mr.OCCUPIED)))
    S.append(scene("stripes_unk", "b", "stripes_unk", *full_box(spec("b").nvox), pred=p_stripes(mr.UNKNOWN)))
    S.append(scene("stripes_occ_c2", "c2", "stripes_occ", *full_box(spec("c2").nvox), pred=p_stripes(mr.OCCUPIED)))
    # --- thresholds ---
    S.append(scene("thr", "a", "thr", *full_box(spec("a").nvox), pred=p_thr))
    S.append(scene("thr_exact", "a", DEVIATION_STATE, *full_box(spec("a").nvox), pred=p_deviation))
    # --- truncation: full-height boxes of maps a and d ---
    for name in ("a", "d"):
        m = spec(name)
        lo, hi = (1, 2, 0), (m.nvox[0] - 2, m.nvox[1] - 3, m.nvox[2] - 1)
        zt, zb, top = 17, 4, m.nvox[2]
        ph, pl = m.pos_z(zt), m.pos_z(zb)
        for kind in (mr.UNKNOWN,):
            S.append(scene("zhigh_on_" + name, name, "random", lo, hi, z_high=ph, pred=p_layers(kind, list(range(zt + 1, top)))))
            S.append(scene("zhigh_below_" + name, name, "random", lo, hi, z_high=np.nextafter(ph, DOWN),
                           pred=p_layers(kind, list(range(zt, top)))))
            S.append(scene("zlow_on_" + name, name, "random", lo, hi, z_low=pl, pred=p_layers(kind, list(range(0, zb)))))
            S.append(scene("zlow_above_" + name, name, "random", lo, hi, z_low=np.nextafter(pl, UP),
                           pred=p_layers(kind, list(range(0, zb + 1)))))
            S.append(scene("zboth_" + name, name, "random", lo, hi, z_low=pl, z_high=ph,
                           pred=p_layers(kind, list(range(0, zb)) + list(range(zt + 1, top)))))
            S.append(scene("zinf_" + name, name, "random", lo, hi, z_low=DOWN, z_high=UP, pred=p_layers(kind, [])))
            S.append(scene("znan_" + name, name, "random", lo, hi, z_low=np.nan, z_high=np.nan, pred=p_layers(kind, [])))
            S.append(scene("znan_high_" + name, name, "random", lo, hi, z_low=pl, z_high=np.nan,
                           pred=p_layers(kind, list(range(0, zb)))))
            S.append(scene("zcrossed_" + name, name, "random", lo, hi, z_low=ph, z_high=pl,
                           pred=lambda sc, c: all(len(c[k]) == 0 for k in mr.KINDS)))
            S.append(scene("zinf_crossed_" + name, name, "random", lo, hi, z_low=UP, z_high=DOWN,
                           pred=lambda sc, c: all(len(c[k]) == 0 for k in mr.KINDS)))
    S.append(scene("ztrunc_b", "b", "random", (0, 0, 1), (5, 4, 129), z_low=spec("b").pos_z(63), z_high=spec("b").pos_z(64),
                   pred=lambda sc, c: len(c[mr.UNKNOWN]) + len(c[mr.KNOWN]) == 2 * 30))  # one layer either side of a chunk edge
    return S


_SCENES = None


def scenes():
    global _SCENES
    if _SCENES is None:
        _SCENES = _scenes()
        tags = [s["tag"] for s in _SCENES]
        assert len(set(tags)) == len(tags)
    return _SCENES


# cap scenes: (scene tag, kind, cap as a function of n_total)
CAP_SCENE = "whole_a"
CAPS = (("n", lambda n: n), ("n-1", lambda n: n - 1), ("1", lambda n: 1), ("n+1", lambda n: n + 1))

# empty boxes (lo > hi on each axis in turn, also with the other coordinates outside the map: the loops do not run) and
# refusals (lo <= hi, but the box leaves the map) of map a
EMPTY_BOXES = [((5, 2, 3), (4, 9, 9)), ((2, 7, 3), (9, 6, 9)), ((2, 3, 9), (9, 9, 8)), ((5, -3, 0), (4, 99, 99))]
BAD_BOXES = [((-1, 0, 0), (3, 3, 3)), ((0, -1, 0), (3, 3, 3)), ((0, 0, -1), (3, 3, 3)), ((0, 0, 0), (24, 3, 3)),
             ((0, 0, 0), (3, 20, 3)), ((0, 0, 0), (3, 3, 25)), ((30, 30, 30), (40, 40, 40))]
BAD_KINDS = (-1, 4, 1 << 20)


# ---- map E: one map whose full box needs more workgroups than one round of the scan holds ----------------------------------
def map_e():
    """sized from the plan: lines of 8 voxels (one item each), a little more than scan_width * items_per_workgroup of them"""
    p = plan((8, 8, 8), (0, 0, 0), (7, 7, 7))
    need = p["scan_width"] * p["items_per_workgroup"] + 16 * p["items_per_workgroup"]  # 16 workgroups into round two
    ny = 512
    nx = -(-need // ny)
    m = MapSpec("e", (nx, ny, 8), 0.1, -1.0)
    return m


def e_state(m):
    rng = np.random.default_rng(11)
    r = rng.random(m.nvox)
    return np.where(r < 0.5, V_UNKNOWN, np.where(r < 0.97, V_FREE, V_OCC))
