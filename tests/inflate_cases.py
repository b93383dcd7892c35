"""The scene table of the obstacle-inflation edge tests: one list, SCENES, that the oracle-only test of the table
(test_inflate_edges_cpu.py), the host build of the inflation kernels under sanitizers
(tests/golden/check_inflate_host_build.py) and the device test (test_inflate_edges_gpu.py) all walk.

A scene is a map (voxel dimensions, inflation step), its occupancy (occupied addresses at l_max, known-free elsewhere,
some unknown voxels, optionally voxels exactly on the two thresholds), inflated bits set before the first call
(setOccupied) and a sequence of calls of clearAndInflateLocalMap, each a local bound and, optionally, a kernel pin of its
own.  `drawn` says which edge the scene is there for; test_inflate_edges_cpu.py checks that it hits it.

The table has four axes -- geometry (GEOMETRY), step (STEPS), box (BOX_CLASSES) and content (CONTENT_CLASSES) -- and is
no full product: every value of every axis appears, and every kernel (fused, factored with k_inflate_yz<2>, factored
with the loop form k_inflate_yz<0>) appears with every geometry.

The resolution is a power of two, so ceil(map_size / resolution) is exact; obstacles_inflation = (step - 0.5) *
resolution gives ceil(obstacles_inflation / resolution) == step."""
import functools

import numpy as np

RES = 0.125
AUTO, FUSED, FACTORED = -1, 0, 1
STEPS = (0, 1, 2, 3, 31)
STEP_REFUSED = 32

# dimensions -> what the geometry hits
GEOMETRY = {
    (5, 3, 7): "nyz = 21: a word spans z-lines, y-rows and x-planes; two words; N % 64 = 41",
    (9, 4, 16): "nyz = 64: x shifts are whole words; N a whole number of words",
    (6, 5, 31): "start & 63 == 0 in k_inflate_yz<2> for dy = +2",
    (6, 5, 33): "start & 63 == 0 in k_inflate_yz<2> for dy = -2",
    (4, 3, 62): "start & 63 == 0 in k_inflate_yz<2> for dy = +1",
    (4, 3, 66): "start & 63 == 0 in k_inflate_yz<2> for dy = -1",
    (6, 3, 64): "nz = 64 with nyz % 64 == 0: every funnel shift of the fused kernel is 0",
    (3, 2, 255): "the largest nz",
    (16, 16, 64): "W = 256: one full tile of the fused kernel",
    (1, 257, 64): "W = 257: a tile of one word; nx = 1",
    (32, 64, 64): "W = 2048: 8 workgroups in k_inflate_x",
    (33, 64, 64): "W = 2112: 9 workgroups in k_inflate_x, a grid of 16",
}
BOX_CLASSES = ("whole", "voxel_mod0", "voxel_mod63", "flush_low", "flush_high", "outside_neighbours", "survive",
               "sequence")
CONTENT_CLASSES = ("wrap", "empty", "full", "at_occ_threshold", "at_unknown_threshold")


def adr(dims, x, y, z):
    return (x * dims[1] + y) * dims[2] + z


def idx(dims, a):
    return (a // (dims[1] * dims[2]), (a // dims[2]) % dims[1], a % dims[2])


def full_box(dims):
    return (0, 0, 0), tuple(d - 1 for d in dims)


def corners(dims):
    return [adr(dims, x, y, z) for x in (0, dims[0] - 1) for y in (0, dims[1] - 1) for z in (0, dims[2] - 1)]


def face_centres(dims):
    c = [d // 2 for d in dims]
    out = []
    for k in range(3):
        for v in (0, dims[k] - 1):
            p = list(c)
            p[k] = v
            out.append(adr(dims, *p))
    return out


class Scene:
    def __init__(self, name, dims, step, occupied, calls, box, content=(), pre=(), at_occ_threshold=(),
                 at_unknown_threshold=(), drawn=None, full_by_reach=False):
        self.name, self.dims, self.step = name, tuple(dims), int(step)
        self.nvox = self.dims
        self.N = dims[0] * dims[1] * dims[2]
        self.nyz = dims[1] * dims[2]
        self.W = (self.N + 63) // 64
        self.occupied = tuple(sorted(set(int(a) for a in occupied)))
        # (lo, hi, pin): pin None = the pin of the run; a pin of its own = this call always runs that kernel
        self.calls = tuple((tuple(c[0]), tuple(c[1]), c[2] if len(c) > 2 else None) for c in calls)
        self.box = tuple(box)          # BOX_CLASSES the scene stands for
        self.content = tuple(content)  # CONTENT_CLASSES the scene stands for
        self.pre = tuple(int(a) for a in pre)
        self.at_occ_threshold = tuple(int(a) for a in at_occ_threshold)
        self.at_unknown_threshold = tuple(int(a) for a in at_unknown_threshold)
        self.drawn = dict(drawn or {})
        self.full_by_reach = full_by_reach  # the stamp is larger than the map: every voxel ends up inflated
        assert self.dims in GEOMETRY and self.step in STEPS, name
        assert all(b in BOX_CLASSES for b in self.box) and all(c in CONTENT_CLASSES for c in self.content), name
        assert all(0 <= a < self.N for a in self.occupied + self.pre + self.at_occ_threshold + self.at_unknown_threshold)
        for lo, hi, pin in self.calls:
            assert all(0 <= lo[k] <= hi[k] < dims[k] for k in range(3)), name
            assert pin in (None, FACTORED) or (pin == FUSED and step == 2), name
        special = set(self.occupied) | set(self.at_occ_threshold) | set(self.at_unknown_threshold)
        # some unknown voxels in every scene: every 7th address that holds nothing else
        self.unknown = tuple(a for a in range(3, self.N, 7) if a not in special) if "full" not in self.content else ()

    def __repr__(self):
        return self.name

    @property
    def map_size(self):
        return tuple(d * RES for d in self.dims)

    @property
    def inflation(self):
        return (self.step - 0.5) * RES if self.step else 0.0

    @property
    def map_kw(self):
        return dict(resolution=RES, obstacles_inflation=self.inflation, ground_height=0.0)

    @property
    def pins(self):
        """the pins a run of the scene may use; AUTO first"""
        return (AUTO, FUSED, FACTORED) if self.step == 2 else (AUTO, FACTORED)

    def kernel_of(self, pin, call):
        """the kernel lastInflateKernel() must report for `call` in a run under `pin`: no map of the table is large
        enough for AUTO to leave the fused kernel at step 2"""
        p = call[2] if call[2] is not None else pin
        return (FUSED if self.step == 2 else FACTORED) if p == AUTO else p

    def log_odds(self, l_min, l_max, l_occ):
        """the full occupancy array from the map's own constants (clamp_min_log, clamp_max_log, min_occupancy_log)"""
        occ = np.full(self.N, l_min)                                   # known free
        occ[list(self.unknown)] = l_min - 0.01                         # unknown: what a new map holds
        occ[list(self.at_unknown_threshold)] = l_min - 1e-3            # not unknown: the comparison is strict
        occ[list(self.at_occ_threshold)] = l_occ                       # not occupied: the comparison is strict
        occ[list(self.occupied)] = l_max
        return occ

    def centre(self, a):
        """the position of voxel a's centre (setOccupied takes positions)"""
        org = (-self.map_size[0] / 2.0, -self.map_size[1] / 2.0, 0.0)
        return tuple(org[k] + (i + 0.5) * RES for k, i in enumerate(idx(self.dims, a)))

    def reach(self):
        return self.step * (self.nyz + self.dims[2] + 1)

    def reach_range(self, call):
        """the addresses a stamp of a source inside the call's box can touch"""
        lo, hi = call[0], call[1]
        return max(0, adr(self.dims, *lo) - self.reach()), min(self.N - 1, adr(self.dims, *hi) + self.reach())

    def stamp(self, a):
        """the addresses the reference's stamp of voxel a sets: only the final address is range-checked"""
        s = self.step
        d = np.arange(-s, s + 1)
        x, y, z = idx(self.dims, a)
        t = ((x + d)[:, None, None] * self.dims[1] + (y + d)[None, :, None]) * self.dims[2] + (z + d)[None, None, :]
        t = t.reshape(-1)
        return t[(t >= 0) & (t < self.N)]

    def in_box(self, a, call):
        return all(call[0][k] <= i <= call[1][k] for k, i in enumerate(idx(self.dims, a)))


@functools.lru_cache(maxsize=None)
def _expected(name, with_pre):
    from oracle import fuel_oracle as fo
    sc = BY_NAME[name]
    om = fo.OracleMap(sc.map_size, **sc.map_kw)
    assert om.nvox == sc.nvox, (om.nvox, sc.nvox)
    assert int(np.ceil(om.cfg.obstacles_inflation / om.cfg.resolution)) == sc.step
    occ = sc.log_odds(om.l_min, om.l_max, om.l_occ)
    om.occ[:] = occ
    if with_pre:
        for a in sc.pre:
            om.set_occupied(sc.centre(a))
        assert om.infl.sum() == len(set(sc.pre))
    planes = []
    for lo, hi, _ in sc.calls:
        om.set_local_bound(lo, hi)
        om.inflate_local()
        p = om.infl.copy()
        p.setflags(write=False)
        planes.append(p)
    occ.setflags(write=False)
    return occ, tuple(planes), (om.l_min, om.l_max, om.l_occ)


def expected(sc, with_pre=True):
    """(log-odds, the oracle's inflated plane after every call, (l_min, l_max, l_occ)); computed once, read-only"""
    return _expected(sc.name, with_pre)


def clipped_dilation(sc, call):
    """what a dilation clipped at the map faces (no wrap) gives for one call on an empty inflated plane"""
    lo, hi = call[0], call[1]
    src = np.zeros(sc.dims, dtype=bool)
    for a in sc.occupied:
        if sc.in_box(a, call):
            src[idx(sc.dims, a)] = True
    out = src.copy()
    for axis in range(3):
        acc = out.copy()
        for d in range(1, min(sc.step, sc.dims[axis] - 1) + 1):
            sl_a, sl_b = [slice(None)] * 3, [slice(None)] * 3
            sl_a[axis], sl_b[axis] = slice(d, None), slice(None, -d)
            acc[tuple(sl_a)] |= out[tuple(sl_b)]
            acc[tuple(sl_b)] |= out[tuple(sl_a)]
        out = acc
    return out.reshape(-1).astype(np.int8)


def _scenes():
    S = []

    def add(*a, **k):
        S.append(Scene(*a, **k))

    # ---- step 2: fused and factored (k_inflate_yz<2>) with every geometry ---------------------------------------
    d = (5, 3, 7)
    add("g5x3x7_s2_wrap", d, 2, [adr(d, 0, 0, 0), adr(d, 4, 2, 6), adr(d, 2, 1, 0)], [full_box(d)], ["whole"], ["wrap"], drawn={"wrap": True})
    add("g5x3x7_s2_full", d, 2, range(105), [full_box(d)], ["whole"], ["full"])
    add("g5x3x7_s2_subbox", d, 2, [adr(d, 2, 1, 3), adr(d, 0, 0, 0), adr(d, 4, 2, 6)], [((1, 0, 1), (3, 2, 5))], [])
    d = (9, 4, 16)
    add("g9x4x16_s2_faces", d, 2, face_centres(d) + corners(d)[:2], [full_box(d)], ["whole"], ["wrap"],
        drawn={"wrap": True, "shift0": ("x", 1), "W": 9})
    add("g9x4x16_s2_outside", d, 2,
        [adr(d, 4, 2, 8)] + [adr(d, 2, 2, 8), adr(d, 7, 2, 8), adr(d, 4, 0, 8), adr(d, 4, 3, 8), adr(d, 4, 2, 4), adr(d, 4, 2, 12)],
        [((3, 1, 5), (6, 2, 11))], ["outside_neighbours"], drawn={"not_a_source": True})
    d = (6, 5, 31)
    add("g6x5x31_s2", d, 2, [adr(d, 0, 0, 0), adr(d, 3, 2, 15), adr(d, 5, 4, 30), adr(d, 2, 4, 1)], [full_box(d)],
        ["whole"], ["wrap"], drawn={"wrap": True, "shift0": ("yz2", 2)})
    add("g6x5x31_s2_flush_low", d, 2, [adr(d, 0, 0, 0), adr(d, 1, 1, 8), adr(d, 4, 3, 20)], [((0, 0, 0), (2, 2, 12))],
        ["flush_low"], drawn={"shift0": ("yz2", 2)})
    d = (6, 5, 33)
    add("g6x5x33_s2", d, 2, [adr(d, 0, 4, 32), adr(d, 3, 0, 0), adr(d, 2, 2, 16), adr(d, 5, 4, 32)], [full_box(d)],
        ["whole"], ["wrap"], drawn={"wrap": True, "shift0": ("yz2", -2)})
    add("g6x5x33_s2_flush_high", d, 2, [adr(d, 5, 4, 32), adr(d, 4, 3, 25), adr(d, 1, 1, 3)], [((3, 2, 20), (5, 4, 32))],
        ["flush_high"], drawn={"shift0": ("yz2", -2)})
    d = (4, 3, 62)
    add("g4x3x62_s2", d, 2, [adr(d, 0, 0, 61), adr(d, 1, 1, 30), adr(d, 3, 2, 0), adr(d, 2, 0, 1)], [full_box(d)],
        ["whole"], ["wrap"], drawn={"wrap": True, "shift0": ("yz2", 1)})
    add("g4x3x62_s2_voxels", d, 2, [64, 127, 300], [(idx(d, 64), idx(d, 64)), (idx(d, 127), idx(d, 127))],
        ["voxel_mod0", "voxel_mod63", "sequence"], drawn={"voxel_mod": (0, 63)})
    d = (4, 3, 66)
    add("g4x3x66_s2", d, 2, [adr(d, 0, 0, 0), adr(d, 1, 2, 65), adr(d, 2, 1, 33), adr(d, 3, 2, 65)], [full_box(d)],
        ["whole"], ["wrap"], drawn={"wrap": True, "shift0": ("yz2", -1)})
    add("g4x3x66_s2_survive", d, 2, [adr(d, 1, 1, 30), adr(d, 2, 1, 40)], [((1, 1, 20), (2, 1, 45))], ["survive"],
        pre=[adr(d, 1, 1, 10), adr(d, 0, 0, 5), adr(d, 3, 2, 60), adr(d, 1, 1, 35), adr(d, 2, 1, 21), adr(d, 1, 2, 30)],
        drawn={"survive": True, "shift0": ("yz2", -1)})
    d = (6, 3, 64)
    add("g6x3x64_s2", d, 2, [adr(d, 0, 0, 0), adr(d, 2, 1, 63), adr(d, 3, 2, 0), adr(d, 5, 2, 63), adr(d, 4, 0, 31)],
        [full_box(d)], ["whole"], ["wrap"], drawn={"wrap": True, "shift0": ("fused", None)})
    add("g6x3x64_s2_subbox", d, 2, [adr(d, 2, 1, 63), adr(d, 3, 1, 0), adr(d, 0, 0, 0), adr(d, 3, 2, 32)],
        [((2, 1, 0), (3, 2, 63))], [], drawn={"shift0": ("fused", None)})
    d = (3, 2, 255)
    add("g3x2x255_s2", d, 2, [adr(d, 0, 0, 0), adr(d, 1, 1, 127), adr(d, 2, 0, 1)], [full_box(d)],
        ["whole"], ["wrap"], drawn={"wrap": True})
    add("g3x2x255_s2_sequence", d, 2, [adr(d, 0, 0, 3), adr(d, 1, 0, 100), adr(d, 1, 1, 200), adr(d, 2, 1, 250), adr(d, 2, 0, 64)],
        [full_box(d), ((1, 0, 90), (1, 1, 210)), ((2, 0, 60), (2, 1, 254))], ["whole", "sequence"])
    d = (16, 16, 64)
    add("g16x16x64_s2", d, 2, corners(d) + face_centres(d) + [adr(d, 5, 9, 20)], [full_box(d)], ["whole"], ["wrap"],
        drawn={"wrap": True, "W": 256, "out_words": 256})
    add("g16x16x64_s2_voxel0", d, 2, [adr(d, 7, 8, 0), adr(d, 7, 8, 1), adr(d, 7, 7, 63)], [((7, 8, 0), (7, 8, 0))],
        ["voxel_mod0"], drawn={"voxel_mod": (0,)})
    add("g16x16x64_s2_voxel63", d, 2, [adr(d, 7, 8, 63), adr(d, 7, 8, 62), adr(d, 7, 9, 0)], [((7, 8, 63), (7, 8, 63))],
        ["voxel_mod63"], drawn={"voxel_mod": (63,)})
    add("g16x16x64_s2_stale", d, 2,
        [adr(d, 2, 3, 10), adr(d, 8, 8, 32), adr(d, 12, 4, 50), adr(d, 13, 13, 5), adr(d, 4, 12, 60)],
        [((1, 1, 1), (14, 14, 62), FACTORED), ((7, 7, 30), (9, 9, 34), FUSED), ((11, 3, 45), (13, 5, 55), FACTORED),
         ((3, 11, 55), (5, 13, 63), FACTORED)], ["sequence"])
    d = (1, 257, 64)
    add("g1x257x64_s2", d, 2, corners(d) + [adr(d, 0, 128, 32), adr(d, 0, 60, 0), adr(d, 0, 200, 63)], [full_box(d)],
        ["whole"], ["wrap"], drawn={"wrap": True, "W": 257, "out_words": 257, "nx1": True})
    add("g1x257x64_s2_subbox", d, 2, [adr(d, 0, 100, 10), adr(d, 0, 150, 60), adr(d, 0, 99, 10), adr(d, 0, 256, 63)],
        [((0, 100, 0), (0, 256, 63))], ["flush_high"], drawn={"nx1": True})
    d = (32, 64, 64)
    add("g32x64x64_s2", d, 2, corners(d) + face_centres(d) + [adr(d, 10, 20, 30), adr(d, 25, 50, 7)], [full_box(d)],
        ["whole"], ["wrap"], drawn={"wrap": True, "W": 2048, "x_blocks": 8, "x_grid": 8})
    d = (33, 64, 64)
    add("g33x64x64_s2", d, 2, corners(d) + face_centres(d) + [adr(d, 32, 1, 1), adr(d, 16, 40, 33)], [full_box(d)],
        ["whole"], ["wrap"], drawn={"wrap": True, "W": 2112, "x_blocks": 9, "x_grid": 16})
    add("g33x64x64_s2_sequence", d, 2, [adr(d, 3, 3, 3), adr(d, 16, 32, 32), adr(d, 30, 60, 60), adr(d, 20, 10, 50)],
        [((1, 1, 1), (31, 62, 62)), ((15, 30, 30), (17, 34, 34)), ((29, 58, 58), (32, 63, 63))],
        ["sequence", "flush_high"])

    # ---- the loop form k_inflate_yz<0> with every geometry, steps 0, 1, 3, 31 -----------------------------------
    d = (5, 3, 7)
    add("g5x3x7_s1_wrap", d, 1, [adr(d, 0, 0, 0), adr(d, 4, 2, 6), adr(d, 2, 1, 0)], [full_box(d)], ["whole"], ["wrap"], drawn={"wrap": True})
    add("g5x3x7_s31_one_seed", d, 31, [adr(d, 2, 1, 3)], [full_box(d)], ["whole"], full_by_reach=True)
    add("g5x3x7_s0", d, 0, corners(d) + [adr(d, 2, 1, 3), adr(d, 0, 2, 6)], [((1, 0, 1), (3, 2, 5)), full_box(d)],
        ["whole", "sequence", "survive"], pre=[adr(d, 1, 1, 0), adr(d, 2, 2, 2)], drawn={"survive": True})
    d = (9, 4, 16)
    add("g9x4x16_s3_corners", d, 3, corners(d), [full_box(d)], ["whole"], ["wrap"], drawn={"wrap": True, "shift0": ("x", 3)})
    add("g9x4x16_s1_thresholds", d, 1, [adr(d, 4, 2, 8)], [full_box(d), ((0, 0, 0), (8, 3, 7))], ["whole", "flush_low"],
        ["at_occ_threshold", "at_unknown_threshold"], at_occ_threshold=[adr(d, 1, 1, 3), adr(d, 7, 2, 12)],
        at_unknown_threshold=[adr(d, 2, 2, 5), adr(d, 6, 1, 10)], drawn={"thresholds": True})
    d = (6, 5, 31)
    add("g6x5x31_s1_subbox", d, 1, [adr(d, 2, 2, 10), adr(d, 3, 3, 20), adr(d, 1, 2, 10), adr(d, 2, 2, 21)],
        [((2, 1, 5), (4, 3, 20))], ["outside_neighbours"], drawn={"not_a_source": True})
    d = (6, 5, 33)
    add("g6x5x33_s0", d, 0, [adr(d, 0, 0, 0), adr(d, 5, 4, 32), adr(d, 2, 2, 2), adr(d, 0, 1, 31), adr(d, 0, 3, 28)],
        [full_box(d), (idx(d, 64), idx(d, 64)), (idx(d, 127), idx(d, 127))], ["whole", "voxel_mod0", "voxel_mod63", "sequence"],
        drawn={"voxel_mod": (0, 63), "shift0": ("yz0", 0)})
    d = (4, 3, 62)
    add("g4x3x62_s31_two_seeds", d, 31, [adr(d, 1, 1, 30), adr(d, 3, 2, 61)], [full_box(d)], ["whole"], full_by_reach=True)
    add("g4x3x62_s3_empty", d, 3, [], [((1, 0, 10), (2, 2, 50)), full_box(d)], ["whole", "survive", "sequence"], ["empty"],
        pre=[adr(d, 0, 0, 0), adr(d, 1, 1, 30), adr(d, 3, 2, 61)], drawn={"survive": True})
    d = (4, 3, 66)
    add("g4x3x66_s3", d, 3, [adr(d, 0, 0, 0), adr(d, 2, 1, 33)], [full_box(d)], ["whole"], ["wrap"],
        drawn={"wrap": True})
    d = (6, 3, 64)
    add("g6x3x64_s1", d, 1, corners(d) + [adr(d, 3, 1, 32)], [full_box(d), ((0, 0, 0), (2, 1, 31))], ["whole", "flush_low"],
        ["wrap"], drawn={"wrap": True, "shift0": ("x", 1)})
    d = (3, 2, 255)
    add("g3x2x255_s31_one_seed", d, 31, [adr(d, 1, 0, 10)], [full_box(d)], ["whole"], ["wrap"], drawn={"wrap": True})
    add("g3x2x255_s1_full", d, 1, range(3 * 2 * 255), [full_box(d), ((1, 0, 100), (1, 1, 150))], ["whole", "sequence"], ["full"])
    d = (16, 16, 64)
    add("g16x16x64_s3_survive", d, 3, [adr(d, 8, 8, 32), adr(d, 7, 7, 30)], [((6, 6, 24), (9, 9, 40))], ["survive"],
        pre=[adr(d, 8, 8, 20), adr(d, 8, 8, 25), adr(d, 3, 8, 32), adr(d, 8, 8, 32), adr(d, 9, 9, 28), adr(d, 8, 2, 32), adr(d, 15, 15, 63)],
        drawn={"survive": True, "W": 256})
    add("g16x16x64_s1_voxels", d, 1, [adr(d, 3, 4, 0), adr(d, 3, 4, 63), adr(d, 3, 5, 0)],
        [((3, 4, 0), (3, 4, 0)), ((3, 4, 63), (3, 4, 63))], ["voxel_mod0", "voxel_mod63", "sequence"],
        drawn={"voxel_mod": (0, 63)})
    d = (1, 257, 64)
    add("g1x257x64_s1", d, 1, corners(d) + [adr(d, 0, 128, 0), adr(d, 0, 128, 63)], [full_box(d)], ["whole"], ["wrap"],
        drawn={"wrap": True, "W": 257, "nx1": True})
    add("g1x257x64_s0_empty", d, 0, [], [full_box(d)], ["whole"], ["empty"], pre=[0, 16447, 8000], drawn={"nx1": True})
    d = (32, 64, 64)
    add("g32x64x64_s3", d, 3, corners(d) + [adr(d, 16, 32, 32), adr(d, 5, 60, 2)], [full_box(d)], ["whole"], ["wrap"],
        drawn={"wrap": True, "W": 2048, "x_blocks": 8, "x_grid": 8})
    add("g32x64x64_s1_outside", d, 1,
        [adr(d, 16, 32, 32)] + [adr(d, 9, 32, 32), adr(d, 21, 32, 32), adr(d, 16, 19, 32), adr(d, 16, 41, 32),
                                adr(d, 16, 32, 15), adr(d, 16, 32, 49)],
        [((10, 20, 16), (20, 40, 48))], ["outside_neighbours"], drawn={"not_a_source": True})
    d = (33, 64, 64)
    add("g33x64x64_s31_two_seeds", d, 31, [adr(d, 0, 0, 0), adr(d, 32, 63, 63)], [full_box(d)], ["whole"], ["wrap"],
        drawn={"wrap": True, "W": 2112, "x_blocks": 9, "x_grid": 16})
    add("g33x64x64_s0", d, 0, corners(d) + face_centres(d), [full_box(d), ((0, 0, 0), (16, 31, 31))],
        ["whole", "flush_low", "sequence"], drawn={"W": 2112, "x_blocks": 9, "x_grid": 16})
    add("g33x64x64_s3_survive", d, 3, [adr(d, 16, 32, 32)], [((14, 30, 26), (18, 34, 38))], ["survive"],
        pre=[adr(d, 16, 32, 20), adr(d, 16, 32, 27), adr(d, 10, 32, 32), adr(d, 16, 32, 32), adr(d, 16, 36, 33), adr(d, 0, 0, 0)],
        drawn={"survive": True})
    return S


SCENES = _scenes()
BY_NAME = {sc.name: sc for sc in SCENES}
assert len(BY_NAME) == len(SCENES)
