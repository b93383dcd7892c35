"""The scenes of the trajectory safety check (fuel_amd/csrc/traj_check.hip): tests/test_traj_check_cpu.py proves on the
host that each reaches the edge it is drawn for, tests/test_traj_check_gpu.py runs them on the device.

Two small maps with hand-written occupancy (unknown everywhere except the painted voxels), inflated in numpy exactly as
clearAndInflateLocalMap does it (plan_env/src/sdf_map.cpp:434-461: a cube of +-ceil(obstacles_inflation / resolution)
voxels per occupied voxel, written through the LINEAR address, so a cube that leaves a y or z face wraps into the
neighbouring line); the CPU test compares that plane with the oracle's, the GPU test with the device's.

A scene is a dict: tag, map ("a" / "b"), ctrl [n, 3], degree, dt, t_now, step, max_radius, expect (the outputs the scene
is drawn for) and pred: a function of (samples, grid, scene) -- samples = traj_check_ref.samples(), every sample's time,
point, radius, voxel index and inflated bit whether or not the loop reaches it -- that is true iff the scene sits on its
edge.  Nothing here needs a GPU."""
import math

import numpy as np

import traj_check_ref as tr

L_MIN, L_MAX = math.log(0.12 / 0.88), math.log(0.90 / 0.10)  # DEFAULT_MAP's p_min / p_max as log-odds
UNKNOWN, FREE, OCCUPIED = L_MIN - 0.01, L_MIN, L_MAX
INFLATION = 0.199

MAPS = {
    # 40 x 40 x 20 voxels at 0.1 m, origin on the voxel grid
    "a": dict(map_size=(4.0, 4.0, 2.0), kw=dict(resolution=0.1, ground_height=-1.0),
              occupied=[(30, 20, 10), (15, 12, 10)], free=[((2, 30, 8), (12, 36, 13))]),
    # 0.15 m, origin off the voxel grid; one occupied voxel on every face for the six "outside" scenes
    "b": dict(map_size=(4.5, 3.3, 2.1), kw=dict(resolution=0.15, ground_height=-0.37), occupied="faces", free=[]),
}
FACE_L1, FACE_L2 = 4, 11  # lateral voxel index where a face scene leaves the map / of the occupied border voxel


class MapSpec:
    def __init__(self, name):
        m = MAPS[name]
        self.name, self.map_size, self.kw = name, m["map_size"], dict(m["kw"])
        self.res = self.kw["resolution"]
        self.res_inv = 1.0 / self.res
        self.origin = np.array([-self.map_size[0] / 2.0, -self.map_size[1] / 2.0, self.kw["ground_height"]])
        self.nvox = tuple(int(math.ceil(self.map_size[i] / self.res)) for i in range(3))  # SDFMap::initMap
        occ = m["occupied"]
        if occ == "faces":
            occ = [face_voxel(self.nvox, a, s) for a in range(3) for s in (0, 1)]
        self.occupied = [tuple(v) for v in occ]
        o3 = np.full(self.nvox, UNKNOWN)
        for lo, hi in m["free"]:
            o3[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = FREE
        for v in self.occupied:
            o3[v] = OCCUPIED
        self.occ3 = o3
        self.infl3 = inflate(o3, int(math.ceil(INFLATION / self.res)))

    def grid(self, infl=None):
        return tr.Grid(self.nvox, self.origin, self.res_inv, self.infl3 if infl is None else infl)

    def centre(self, idx):
        return self.origin + (np.asarray(idx, dtype=float) + 0.5) * self.res


def face_voxel(nvox, a, s):
    """the occupied border voxel of face (axis a, side s): on the face, at FACE_L2 along the next axis, mid-way along
    the third"""
    v = [0, 0, 0]
    v[a] = 0 if s == 0 else nvox[a] - 1
    v[(a + 1) % 3] = FACE_L2
    v[(a + 2) % 3] = nvox[(a + 2) % 3] // 2
    return tuple(v)


def inflate(occ3, step):
    """clearAndInflateLocalMap over the whole map: every voxel with occupancy > min_occupancy_log marks the cube of
    +-step voxels around it, each through toAddress() and kept iff 0 <= address < N"""
    nx, ny, nz = occ3.shape
    src = np.argwhere(occ3 > math.log(0.80 / 0.20))
    r = np.arange(-step, step + 1)
    off = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)
    pts = (src[:, None, :] + off[None, :, :]).reshape(-1, 3)
    adr = (pts[:, 0] * ny + pts[:, 1]) * nz + pts[:, 2]
    adr = adr[(adr >= 0) & (adr < nx * ny * nz)]
    out = np.zeros(nx * ny * nz, dtype=np.int8)
    out[adr] = 1
    return out.reshape(occ3.shape)


_SPECS = {}


def spec(name):
    if name not in _SPECS:
        _SPECS[name] = MapSpec(name)
    return _SPECS[name]


def scene(tag, map_, ctrl, dt, t_now=0.0, degree=3, step=tr.STEP, max_radius=tr.MAX_RADIUS, expect=None, pred=None):
    return dict(tag=tag, map=map_, ctrl=np.ascontiguousarray(ctrl, dtype=np.float64).reshape(-1, 3), dt=float(dt),
                t_now=float(t_now), degree=int(degree), step=float(step), max_radius=float(max_radius),
                expect=dict(expect or {}), pred=pred)


def restate(sc, form="first_hit", grid=None, **kw):
    g = grid if grid is not None else spec(sc["map"]).grid()
    f = tr.check_first_hit if form == "first_hit" else tr.check_literal
    return f(g, sc["ctrl"], sc["degree"], sc["dt"], sc["t_now"], sc["step"], sc["max_radius"], **kw)


def scene_samples(sc, count=None, grid=None):
    g = grid if grid is not None else spec(sc["map"]).grid()
    if count is None:  # every sample the time condition could admit, and a few more
        u = tr.knots(len(sc["ctrl"]), sc["degree"], sc["dt"])
        span = u[len(sc["ctrl"])] - u[sc["degree"]] - sc["t_now"]
        count = int(min(max(span / sc["step"], 0.0), 4000.0)) + 8
    return tr.samples(g, sc["ctrl"], sc["degree"], sc["dt"], sc["t_now"], count, sc["step"])


# ---- building blocks ----------------------------------------------------------------------------------------------------
SPEED, DT = 0.5, 0.2       # 0.01 m per sample of 0.02 s
HIT_Y, HIT_Z = 0.05, 0.05  # through the middle of voxel (.., 20, 10) of map a: the first obstacle's line
BAND_X = 0.8               # low x face of the band the voxel (30, 20, 10) inflates: indices 28 .. 32
FREE_Y = -1.55             # a line nothing inflates (y index 4)


def line(start, direction, n_ctrl, speed=SPEED, dt=DT):
    """equally spaced collinear control points: a cubic uniform spline through them is the straight flight
    start + speed t direction (its point at t = 0 is the second control point)"""
    d = np.asarray(direction, dtype=float)
    return np.asarray(start, dtype=float)[None, :] + (np.arange(n_ctrl)[:, None] - 1) * (speed * dt) * d[None, :]


def polyline(points, spacing):
    """control points every `spacing` along a polyline, corners included"""
    out = [np.asarray(points[0], dtype=float)]
    for a, b in zip(points[:-1], points[1:]):
        a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
        n = max(int(round(np.linalg.norm(b - a) / spacing)), 1)
        out += [a + (b - a) * (i / n) for i in range(1, n + 1)]
    return np.array(out)


def wiggle(start, n_ctrl, seed, spacing=0.1, amp=0.05):
    """a gently curved flight along +x: spacing per control point, a seeded lateral perturbation"""
    rng = np.random.default_rng(seed)
    c = line(start, (1.0, 0.0, 0.0), n_ctrl, speed=spacing, dt=1.0)
    c[:, 1:] += amp * rng.uniform(-1.0, 1.0, size=(n_ctrl, 2))
    return c


def duration_of(n_ctrl, degree, dt):
    u = tr.knots(n_ctrl, degree, dt)
    return u[n_ctrl] - u[degree]


def _occ_at(sc, idx):
    return spec(sc["map"]).occ3[tuple(int(v) for v in idx)]


# ---- window edges -------------------------------------------------------------------------------------------------------
HIT_SAMPLES = (1, 63, 64, 65, 128, 129)


def hit_scene(k, max_radius=tr.MAX_RADIUS, tag=None):
    """sample k is the first inside the band: x0 + 0.01 k >= BAND_X > x0 + 0.01 (k - 1)"""
    x0 = BAND_X - 0.01 * k + 0.005

    def pred(s, g, sc):
        hit_voxel_occ = _occ_at(sc, s["index"][k - 1])
        return (not s["inflated"][:k - 1].any() and bool(s["inflated"][k - 1]) and bool((s["t"][:k] < s["duration"]).all())
                and bool((s["r"][:k - 1] < sc["max_radius"]).all())
                and hit_voxel_occ < math.log(4.0))  # inflated, not occupied: the rim of the cube
    return scene(tag or "hit_%d" % k, "a", line((x0, HIT_Y, HIT_Z), (1, 0, 0), 24), DT, max_radius=max_radius,
                 expect=dict(safe=0, hit_index=k, n_samples=k, end_reason=tr.END_HIT), pred=pred)


def end_radius_scene(k):
    """the loop ends in front of body k: r_(k-1) = 0.01 (k - 1) is the first radius that is not below max_radius"""
    R = 0.01 * (k - 1) - 0.005

    def pred(s, g, sc):
        unknown = all(_occ_at(sc, i) < L_MIN - 1e-3 for i in s["index"][:k - 1])
        return bool((s["r"][:k - 2] < R).all()) and s["r"][k - 2] >= R and not s["inflated"][:k].any() and unknown
    return scene("end_radius_%d" % k, "a", line((-1.2, FREE_Y, 0.05), (1, 0, 0), 24), DT, max_radius=R,
                 expect=dict(safe=1, n_samples=k - 1, end_reason=tr.END_RADIUS), pred=pred)


def end_time_scene(k, tag=None, free=False):
    """the loop ends in front of body k: t_now + fut_t_k is the first time that is not below the duration"""
    dur = duration_of(24, 3, DT)
    start = (-3.5, 1.25, 0.05) if free else (-1.2, FREE_Y, 0.05)  # free: the flight's last 0.6 s cross the known-free box

    def pred(s, g, sc):
        ok = bool((s["t"][:k - 1] < dur).all()) and not s["t"][k - 1] < dur and not s["inflated"][:k].any()
        if free and k > 1:
            ok = ok and all(abs(_occ_at(sc, i) - FREE) == 0.0 for i in s["index"][:min(k - 1, 20)])
        return ok
    return scene(tag or "end_time_%d" % k, "a", line(start, (1, 0, 0), 24), DT, t_now=dur - (k - 0.5) * tr.STEP,
                 expect=dict(safe=1, n_samples=k - 1, end_reason=tr.END_DURATION), pred=pred)


def no_sample_exact_scene():
    """t_now = duration - step as the machine computes it: whether that admits a first sample is the comparison's"""
    dur = duration_of(24, 3, DT)
    t_now = dur - tr.STEP
    n = 1 if t_now + tr.STEP < dur else 0
    return scene("none_exact", "a", line((-1.2, FREE_Y, 0.05), (1, 0, 0), 24), DT, t_now=t_now,
                 expect=dict(safe=1, n_samples=n, end_reason=tr.END_DURATION), pred=lambda s, g, sc: n == 0)


# ---- the radius rule ----------------------------------------------------------------------------------------------------
R_EDGE = 0.635  # between r_63 = 0.63 and r_64 = 0.64


def radius_out_and_back_scene():
    """0.5 m in front of the band: flies 0.8 m away from it, past max_radius = 0.5, and back into it"""
    y, z = HIT_Y, HIT_Z
    ctrl = polyline([(0.6, y, z), (-0.3, y, z), (1.2, y, z)], 0.1)
    R = 0.5

    sc = scene("radius_out_and_back", "a", ctrl, DT, max_radius=R, expect=dict(safe=1, end_reason=tr.END_RADIUS))
    k1 = int(np.nonzero(~(scene_samples(sc)["r"] < R))[0][0]) + 1  # the first sample whose radius is not below R
    sc["expect"]["n_samples"] = k1

    def pred(s, g, sc):
        back = [k for k in range(k1 + 2, len(s["r"]) + 1) if s["inflated"][k - 1] and s["r"][k - 2] < R
                and s["t"][k - 1] < s["duration"]]
        return not s["inflated"][:k1].any() and bool((s["r"][:k1 - 1] < R).all()) and len(back) > 0
    sc["pred"] = pred
    return sc


def radius_equal_scene(k=40):
    """max_radius = r_k itself: radius < max_radius is false, the loop ends behind body k"""
    base = scene("radius_equal", "a", wiggle((-1.2, -1.5, 0.05), 24, seed=8), DT)
    R = float(scene_samples(base, k)["r"][k - 1])

    def pred(s, g, sc):
        return s["r"][k - 1] == R and bool((s["r"][:k - 1] < R).all()) and not s["inflated"][:k].any()
    return scene("radius_equal", "a", base["ctrl"], DT, max_radius=R,
                 expect=dict(safe=1, n_samples=k, end_reason=tr.END_RADIUS), pred=pred)


# ---- accumulated time ---------------------------------------------------------------------------------------------------
def accumulated_time_scene():
    """a t_now for which `step` summed k times and k * step disagree about sample k being the last one"""
    dur = duration_of(24, 3, DT)
    acc, found = 0.0, None
    for k in range(1, 200):
        acc = acc + tr.STEP  # fut_t of sample k
        prod = k * tr.STEP
        if acc == prod:
            continue
        for base in (dur - acc, dur - prod):
            for t_now in (base, np.nextafter(base, -np.inf), np.nextafter(base, np.inf)):
                t_now = float(t_now)
                if (t_now + acc < dur) != (t_now + prod < dur):
                    found = (k, t_now, t_now + acc < dur)
                    break
            if found:
                break
        if found:
            break
    assert found, "no sample whose accumulated time and k * step fall on different sides of the duration"
    k, t_now, admitted = found
    n = k if admitted else k - 1  # (sample k + 1 is a whole step later: it never passes)

    def pred(s, g, sc):
        return (s["t"][k - 1] < dur) == admitted and ((t_now + k * tr.STEP) < dur) != admitted and n >= 1
    return scene("accumulated_time", "a", line((-1.2, FREE_Y, 0.05), (1, 0, 0), 24), DT, t_now=t_now,
                 expect=dict(safe=1, n_samples=n, end_reason=tr.END_DURATION), pred=pred)


def on_knot_scene():
    """step = 0.125 and a knot span of 0.5 are exact in binary: sample 4 sits on the knot u[p + 1] exactly, and the knot
    search's `<` keeps it in the span below"""
    ctrl = wiggle((-1.2, -1.5, 0.05), 10, seed=5, spacing=0.2)

    def pred(s, g, sc):
        u = s["u"]
        return s["t"][3] + u[3] == u[4] and s["t"][7] + u[3] == u[5]
    return scene("on_knot", "a", ctrl, 0.5, step=0.125, expect=dict(safe=1, end_reason=tr.END_DURATION), pred=pred)


def clamp_low_scene():
    """t_now = -0.5: cur and the first 24 samples are clamped to the spline's start; then the flight runs into the band"""
    x0 = BAND_X - 0.3

    def pred(s, g, sc):
        return bool((s["t"][:24] < 0.0).all()) and bool((s["r"][:24] == 0.0).all()) and s["r"][40] > 0.0
    return scene("clamp_low", "a", line((x0, HIT_Y, HIT_Z), (1, 0, 0), 12), DT, t_now=-0.5,
                 expect=dict(safe=0, end_reason=tr.END_HIT), pred=pred)


def clamp_high_scene():
    dur = duration_of(12, 3, DT)
    return scene("clamp_high", "a", line((-1.2, FREE_Y, 0.05), (1, 0, 0), 12), DT, t_now=dur + 1.0,
                 expect=dict(safe=1, n_samples=0, end_reason=tr.END_DURATION), pred=lambda s, g, sc: True)


# ---- map edges ----------------------------------------------------------------------------------------------------------
FACES = [(a, s) for a in range(3) for s in (0, 1)]


def face_scene(a, s):
    """map b: leaves the map through face (a, s) at lateral index FACE_L1 -- 0.05 m, less than a voxel -- and then flies,
    outside, along the face until it is in front of the occupied border voxel at FACE_L2: posToIndex gives -1 (or n)
    there and the sample passes; a truncating cast (low faces) or an index clamped into the map would read the
    inflated border"""
    m = spec("b")
    b, c = (a + 1) % 3, (a + 2) % 3
    face = m.origin[a] if s == 0 else m.origin[a] + m.nvox[a] * m.res
    sign = -1.0 if s == 0 else 1.0
    vb = face_voxel(m.nvox, a, s)

    def pt(along, lateral_idx):
        p = np.zeros(3)
        p[a] = along
        p[b] = m.origin[b] + (lateral_idx + 0.5) * m.res
        p[c] = m.origin[c] + (vb[c] + 0.5) * m.res
        return p
    out = face + sign * 0.05
    ctrl = polyline([pt(face - sign * 3.5 * m.res, FACE_L1), pt(out, FACE_L1), pt(out, FACE_L2 + 1)], 0.05)
    assert 4 <= len(ctrl) <= 40

    def pred(s_, g, sc):
        live = s_["t"] < s_["duration"]
        idx = s_["index"]
        want = -1 if s == 0 else m.nvox[a]
        front = live & (idx[:, a] == want) & (np.abs(idx[:, b] - vb[b]) <= 2) & (idx[:, c] == vb[c])
        clamped_reads_inflated = m.infl3[vb] == 1
        return bool(front.any()) and not s_["inflated"][live].any() and bool(clamped_reads_inflated)
    return scene("face_%s%s" % ("xyz"[a], "-+"[s]), "b", ctrl, 0.1,
                 expect=dict(safe=1, end_reason=tr.END_DURATION), pred=pred)


def voxel_boundary_scene():
    """map a, second obstacle (15, 12, 10): its cube's low y face is y index 10, the plane y = -1.0 exactly.  A flight in
    that plane hits iff floor() puts a coordinate that IS the boundary into the upper voxel"""
    m = spec("a")

    def pred(s, g, sc):
        k = sc["expect"]["hit_index"]
        on = (s["pos"][:, 1] - m.origin[1]) * m.res_inv
        return bool(on[k - 1] == 10.0) and s["index"][k - 1, 1] == 10 and not s["inflated"][:k - 1].any()
    sc = scene("voxel_boundary", "a", line((-1.2, -1.0, 0.05), (1, 0, 0), 16), DT, expect=dict(safe=0, end_reason=tr.END_HIT),
               pred=pred)
    sc["expect"]["hit_index"] = restate(sc)["hit_index"]
    return sc


# ---- degrees, sizes -----------------------------------------------------------------------------------------------------
def degree_scenes():
    out = []
    for d in (3, 4, 5):
        out.append(scene("deg%d_hit" % d, "a", wiggle((-0.9, HIT_Y, HIT_Z), 40, seed=10 + d, spacing=0.06), 0.12, degree=d,
                         expect=dict(safe=0, end_reason=tr.END_HIT),
                         pred=lambda s, g, sc: len(sc["ctrl"]) == 40))
        out.append(scene("deg%d_safe" % d, "a", wiggle((-1.5, FREE_Y, 0.3), 17 + d, seed=20 + d), DT, degree=d,
                         expect=dict(safe=1, end_reason=tr.END_DURATION), pred=lambda s, g, sc: True))
        out.append(scene("deg%d_min" % d, "a", wiggle((BAND_X - 0.02, HIT_Y, HIT_Z), d + 1, seed=30 + d), 0.4, degree=d,
                         expect=dict(safe=0, end_reason=tr.END_HIT),  # the smallest spline of its degree: one span
                         pred=lambda s, g, sc: len(sc["ctrl"]) == sc["degree"] + 1))
    return out


# ---- defined results ----------------------------------------------------------------------------------------------------
STILL = (-1.2, -1.2, 0.0)
CAP_STEP = 1e-3  # the smallest step the call accepts


def still(n_ctrl):
    return np.repeat(np.array([STILL]), n_ctrl, axis=0)


def nonfinite_scene():
    """a knot span of 1e308: the first knots are -inf, the first alpha is inf / inf"""
    return scene("nonfinite", "a", wiggle((-1.2, -1.5, 0.05), 12, seed=3), 1e308,
                 expect=dict(status=tr.NONFINITE, safe=0, distance=0.0, n_samples=0, end_reason=tr.END_NONFINITE),
                 pred=lambda s, g, sc: not all(math.isfinite(c) for c in s["cur"]))


def cap_scene():
    """hovering for 1110 s at steps of 1 ms: 2^20 bodies and the loop would go on"""
    return scene("cap", "a", still(40), 30.0, step=CAP_STEP,
                 expect=dict(status=tr.OVER, safe=0, n_samples=tr.CAP, end_reason=tr.END_CAP, distance=0.0),
                 pred=lambda s, g, sc: duration_of(40, 3, 30.0) > (tr.CAP + 2) * CAP_STEP)


def cap_exact_scene():
    """exactly 2^20 bodies, then the duration ends the loop: not over the cap"""
    dur = duration_of(40, 3, 30.0)
    return scene("cap_exact", "a", still(40), 30.0, step=CAP_STEP, t_now=dur - (tr.CAP + 0.5) * CAP_STEP,
                 expect=dict(status=tr.OK, safe=1, n_samples=tr.CAP, end_reason=tr.END_DURATION),
                 pred=lambda s, g, sc: True)


def quick_scenes():
    """every scene but the two that walk 2^20 samples"""
    out = [hit_scene(k) for k in HIT_SAMPLES]
    out += [end_radius_scene(k) for k in (64, 65)] + [end_time_scene(k) for k in (64, 65)]
    out += [end_time_scene(1, "none"), end_time_scene(2, "one"), no_sample_exact_scene(), end_time_scene(30, "known_free", True)]
    out += [hit_scene(64, R_EDGE, "radius_first_over_checked"), radius_out_and_back_scene(), radius_equal_scene()]
    k65 = hit_scene(65, R_EDGE, "radius_one_past_unchecked")
    k65["expect"] = dict(safe=1, n_samples=64, end_reason=tr.END_RADIUS)
    k65["pred"] = lambda s, g, sc: (s["r"][62] < R_EDGE <= s["r"][63] and bool(s["inflated"][64])
                                    and not s["inflated"][:64].any())
    out.append(k65)
    out += [accumulated_time_scene(), on_knot_scene(), clamp_low_scene(), clamp_high_scene()]
    out += [face_scene(a, s) for a, s in FACES] + [voxel_boundary_scene()]
    out += degree_scenes() + [nonfinite_scene()]
    return out


def long_scenes():
    return [cap_scene(), cap_exact_scene()]
