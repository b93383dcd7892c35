"""Scenes for the frontier split (fuel_amd/csrc/frontier_split.hip) on axis-aligned clusters and at its table edges.

Every scene is a helpers.vp_patch_scene: the floor occupied, rectangular unknown patches in its top layer, so that the
free voxels above an a x b patch are one cluster of exactly a * b cells in one z layer.  A scene names its patches
("plates") with what the split must do to them, and carries a predicate on the oracle's split trace
(oracle.fuel_oracle.OracleFrontier.split_trace) that is true only if the scene sits on the edge it was drawn for;
tests/test_frontier_split_cpu.py checks every predicate without a GPU, tests/test_frontier_split_gpu.py runs the scenes
on the device.

Leaf boundaries of the VoxelGrid fall on global multiples of down_sample * 0.1 m; with the map origin at (-8, -7) that
is in front of x index 2 (mod 3) and y index 1 (mod 3) at down_sample 3, and in front of x index 2 and y index 4 (mod 6)
at down_sample 6.  A plate is "balanced" when the leaves cut its SHORT side mirror-symmetrically: the centroids'
cross sum is then (sum dx) * (sum dy) = 0 up to rounding, whatever the leaves do along the long side, and the first
principal direction is the long axis exactly -- with both components of normalise(b, lambda - a) being rounding residue.
A plate whose leaves are ragged on both sides has a real cross term of some 1e-3 of a - d: the well-conditioned control.
"""
import copy
import functools

import numpy as np

import helpers
from oracle import fuel_oracle as fo

T = fo.TRACE_FIELDS
# The direction rule's threshold and the two measured figures it lies between: the largest ratio that is
# rounding residue on these scenes, over every summation order tried (test_frontier_split_cpu.py measures it again and
# holds it below NOISE_MAX), and the smallest ratio over every split node of the explored worlds, the pillar golden and
# the smoke run (1.034e-3, world seed 7).  SNAP_TAU is their geometric mean; oracle/fuel_oracle.cpp,
# compat/Eigen/Eigenvalues and fuel_amd/csrc/frontier_split.hip carry the same number.
NOISE_MAX = 1.04e-7
WORLD_MIN = 1.03e-3
SNAP_TAU = 1.03e-5
MAP_SIZE = (16.0, 14.0, 3.0)   # 160 x 140 x 30 voxels of 0.1 m, the largest map the scenes may use
DOWN_SAMPLES = (1, 2, 3, 6)
ON_CUT = 1e-9                  # |dot| below this: the cell sits on the cut
OFF_CUT = 1e-2                 # |dot| above this: it does not (half a voxel on a plate; a direction moves by 1e-12)


class Plate:
    """one patch and what the split has to do with it.  kind: "x" / "y" (long axis; every cut perpendicular to it),
    "square" (isotropic: one fixed direction), "oblique" (control: a real, well-conditioned direction), None (table
    and count scenes: nothing said about the direction)"""

    def __init__(self, x0, y0, a, b, kind=None, paint=True):
        """paint=False: the plate only names a region (the bounding box of a cluster painted by other patches)"""
        self.x0, self.y0, self.a, self.b, self.kind, self.paint = x0, y0, a, b, kind, paint

    @property
    def rect(self):
        return self.x0, self.y0, self.a, self.b

    def holds(self, x, y):
        return (x >= self.x0) & (x < self.x0 + self.a) & (y >= self.y0) & (y < self.y0 + self.b)


class SplitScene:
    def __init__(self, name, plates, pred, parity=None, extra=(), **finder):
        """parity: "even" (no cell on any cut), "odd" (some node has a whole column on its cut) or None (not a
        direction scene).  extra: patches that are not plates (a staircase is one cluster of many patches)."""
        self.name, self.plates, self.pred, self.parity = name, list(plates), pred, parity
        self.finder = dict(cluster_min=0)
        self.finder.update(finder)
        self.patches = [p.rect for p in self.plates if p.paint] + list(extra)
        self.cells = int(vp_scene(self).paint_cells)

    @property
    def direction(self):
        return self.parity is not None


def vp_scene(scene):
    s = helpers.vp_patch_scene(scene.patches, map_size=MAP_SIZE, finder=scene.finder)
    mask = np.zeros((160, 140), dtype=bool)
    for x0, y0, a, b in scene.patches:
        assert 4 <= x0 and x0 + a <= 156 and 4 <= y0 and y0 + b <= 136, (scene.name, x0, y0, a, b)
        mask[x0:x0 + a, y0:y0 + b] = True
    s.paint_cells = mask.sum()
    return s


class Run:
    """one oracle run of a scene: the map, the finder after search(), its pieces and the split trace"""

    def __init__(self, scene, reference_order):
        self.scene, self.reference_order = scene, reference_order
        self.vp = vp_scene(scene)
        om = helpers.vp_map(self.vp)
        om.occ[:] = helpers.vp_occupancy(om, self.vp.paint)
        om.set_local_bound(*helpers.full_box(om.nvox))
        om.inflate_local()
        self.om = om
        self.roots = self._search(split=False).clusters(0)
        self.of = self._search(split=True, trace=True)
        self.rec, self.terms = self.of.split_trace()
        self.pieces = self.of.clusters(0)

    def _search(self, split, trace=False):
        kw = dict(self.scene.finder)
        if not split:
            kw.pop("cluster_size_xy", None)
        of = fo.OracleFrontier(self.om, split=split, canonical_order=not self.reference_order, **kw)
        if trace:
            of.trace_splits()
        self.om.set_updated_box(*helpers.vp_whole_map(self.om))
        of.search()
        return of

    def xy(self, adr):
        """voxel x, y of linear addresses"""
        nv = self.om.nvox
        adr = np.asarray(adr)
        return adr // (nv[1] * nv[2]), (adr // nv[2]) % nv[1]

    def col(self, name):
        return self.rec[:, T[name]]

    @property
    def split_nodes(self):
        return self.rec[self.rec[:, T["split"]] == 1]

    def plate_of(self, row):
        """the plate a trace record belongs to, by its mean"""
        vx = (row[T["mean_x"]] - self.om.origin[0]) / self.om.res
        vy = (row[T["mean_y"]] - self.om.origin[1]) / self.om.res
        hit = [p for p in self.scene.plates if p.x0 <= vx <= p.x0 + p.a and p.y0 <= vy <= p.y0 + p.b]
        assert len(hit) == 1, (self.scene.name, vx, vy)
        return hit[0]

    def node_terms(self, row):
        t0, nf = int(row[T["term0"]]), int(row[T["nf"]])
        return self.terms[t0:t0 + nf]


@functools.lru_cache(maxsize=None)
def oracle_run(name, reference_order=False):
    return Run(SCENES[name], reference_order)


@functools.lru_cache(maxsize=None)
def oracle_run_as(name, finder_of, reference_order=False):
    """the oracle's run of one scene's patches under another scene's finder parameters (the reuse sequence)"""
    scene = copy.copy(SCENES[name])
    scene.name, scene.finder, scene.pred = "%s as %s" % (name, finder_of), dict(SCENES[finder_of].finder), None
    return Run(scene, reference_order)


def cov_ratios(row):
    """(|b| / |a - d|, max(|a - d|, |b|) / tr) of a split node's covariance: how far it is from the two zones in which
    normalise(b, lambda - a) is residue"""
    nf = row[T["nf"]]
    a, b, d = row[T["sxx"]] / nf, 0.5 * (row[T["sxy"]] + row[T["syx"]]) / nf, row[T["syy"]] / nf
    gap = abs(a - d)
    return (abs(b) / gap if gap > 0 else np.inf), max(gap, abs(b)) / (a + d)


# ---- predicates ------------------------------------------------------------------------------------------------------
# a balanced plate's |b| / |a - d| is rounding: of the f64 sums (1e-16) and of the float centroids (2^-24 * 8 m = 5e-7 m
# on deviations of 0.5 m and more); a control's is the cross term that ragged leaves really have
RESIDUE = 1e-6
REAL = 1e-4


def pred_direction(run):
    """every plate splits; on plates and lines b is residue next to a - d on every node, on squares b and a - d are
    residue next to the trace at the root, on controls the cross term is real (plates: at the root); and the parity is
    what the scene says"""
    sp = run.split_nodes
    seen = set()
    for row in sp:
        p = run.plate_of(row)
        seen.add(p)
        axis, iso = cov_ratios(row)
        nf = row[T["nf"]]
        a, d = row[T["sxx"]] / nf, row[T["syy"]] / nf
        if p.kind == "x" and not (axis <= RESIDUE and a > d):
            return False
        if p.kind == "y" and not (axis <= RESIDUE and a < d):
            return False
        if p.kind == "square" and row[T["depth"]] == 0 and not iso <= RESIDUE:
            return False
        if p.kind == "oblique" and (row[T["depth"]] == 0 or not p.paint) and not (axis >= REAL and iso >= REAL):
            return False  # (below an oblique cut the pieces of a plate are no rectangles: nothing is said about them)
    if seen != set(run.scene.plates):
        return False
    on_cut = sp[:, T["min_abs_dot"]] <= ON_CUT
    off_cut = sp[:, T["min_abs_dot"]] >= OFF_CUT
    if not np.all(on_cut | off_cut):
        return False
    return bool(on_cut.any()) if run.scene.parity == "odd" else bool(off_cut.all())


def pred_sums_fallback(run):
    """nothing splits, and every aligned run of 1024 cells in cluster order holds more than 128 clusters (k_sp_sums'
    LDS table has 128 entries; the cells reach it grouped by cluster)"""
    cells = run.col("cells")
    return len(run.rec) >= 300 and not run.col("split").any() and cells.max() * 128 < 1024 and cells.sum() >= 1024


def pred_stats_fallback(run):
    """every root splits once and none of their halves does.  At the first level -- where need_split is decided and the
    covariance read -- no node owns more than 3 leaf slots and there are at least 1024 slots: any 1024 of them, in
    whatever order the device lists them, hold 342 nodes or more, and k_sp_stats' block-local table has 256 entries.
    Some of those nodes (the diagonal pairs) have a direction that is not snapped: a wrong covariance term moves it.
    The second level (2 slots per node at most) overflows as well, with nothing depending on it."""
    depth, nf, split = run.col("depth"), run.col("nf"), run.col("split")
    l0, l1 = depth == 0, depth == 1
    if not (l0.sum() >= 300 and split[l0].all() and not split[l1].any() and depth.max() == 1):
        return False
    for lvl in (l0, l1):
        if not (nf[lvl].sum() >= 1024 and 1024 / nf[lvl].max() > 256):
            return False
    free = [min(cov_ratios(row)) >= REAL for row in run.rec[l0]]
    return bool((run.col("cells")[l0] == 16).sum() >= 300 and sum(free) >= 40)


def pred_count(n_final, crosses=False):
    def pred(run):
        depth = run.col("depth")
        ok = len(run.pieces) == n_final and len(run.pieces) == (run.col("split") == 0).sum()
        if crosses:  # nodes known after level 0 and after level 1: k_sp_rank / k_sp_decide see one tile, then two
            ok = ok and (depth == 0).sum() <= 256 < len(run.rec)
        return bool(ok)
    return pred


def pred_depth(run):
    return bool(run.col("depth").max() >= 6 and max(len(p) for p in run.pieces) <= 3)


def pred_depth_marginal(run):
    """depth 6 is reached, by pieces of 4 cells whose half-length IS cluster_size_xy: some are cut, some are not"""
    sizes = np.array([len(p) for p in run.pieces])
    return bool(run.col("depth").max() >= 6 and (sizes == 4).any() and (sizes == 2).any()
                and np.isin(sizes, (2, 4)).all())


# ---- scenes ----------------------------------------------------------------------------------------------------------
def _direction_scenes():
    sc = []
    for ds in DOWN_SAMPLES:
        kw = dict(down_sample=ds, cluster_size_xy=1.0)
        # long sides of 64 and 128 halve evenly down to the last level: no cell ever sits on a cut.  Short sides of 4
        # start at y = 2 (mod 6) / x = 0 (mod 6): leaves of 2 + 2 at down_sample 3 and 6.  The copies are shifted along
        # the long side, which moves the leaf boundaries (and the ragged first and last leaves) by one and two voxels.
        even = [Plate(6, 8, 64, 4, "x"), Plate(73, 8, 64, 4, "x"), Plate(8, 14, 64, 4, "x"), Plate(5, 20, 128, 1, "x"),
                Plate(7, 23, 128, 1, "x"), Plate(6, 28, 4, 64, "y"), Plate(12, 29, 4, 64, "y"), Plate(18, 30, 4, 64, "y"),
                Plate(150, 5, 1, 128, "y"), Plate(153, 6, 1, 128, "y")]
        sc.append(SplitScene("even_ds%d" % ds, even, pred_direction, parity="even", **kw))
        # 63 and 127 put a whole column on the first cut, 50 and 51 on the second or first; a short side of 7 starts
        # at 2 (mod 3): leaves of 2 + 3 + 2 (no start balances 7 cells on leaves of 2 or 6: down_sample 1 and 3 only)
        odd = [Plate(6, 8, 63, 4, "x"), Plate(73, 8, 63, 4, "x"), Plate(5, 26, 127, 1, "x"), Plate(6, 32, 4, 63, "y"),
               Plate(12, 33, 4, 63, "y"), Plate(150, 5, 1, 127, "y")]
        if ds in (1, 3):
            odd += [Plate(6, 14, 51, 7, "x"), Plate(61, 14, 50, 7, "x"), Plate(24, 32, 7, 51, "y")]
        sc.append(SplitScene("odd_ds%d" % ds, odd, pred_direction, parity="odd", **kw))
        # squares whose leaves are the same along x and y (1 + 30 + 1 cells at down_sample 3 and 6): a = d and b = 0 up
        # to rounding.  cluster_size_xy 1.5 splits 32 x 32 and its 16 x 32 halves and stops at 16 x 16.
        sq = [Plate(7, 9, 32, 32, "square"), Plate(49, 45, 32, 32, "square")]
        sc.append(SplitScene("square_ds%d" % ds, sq, pred_direction, parity="even", down_sample=ds, cluster_size_xy=1.5))
    # controls: a staircase of 5 x 3 steps (a band at 34 degrees), and plates whose leaves are ragged on both sides
    # (short side 1 + 3, long side 1 + 3 * 21): real cross terms
    stairs = [(20 + 3 * i, 40 + 2 * i, 5, 3) for i in range(14)]
    ctl = [Plate(20, 40, 3 * 13 + 5, 2 * 13 + 3, "oblique", paint=False), Plate(7, 9, 64, 4, "oblique"),
           Plate(100, 60, 4, 64, "oblique")]
    sc.append(SplitScene("controls", ctl, pred_direction, parity="even", extra=stairs, down_sample=3,
                         cluster_size_xy=1.0))
    return sc


def _grid(n, a, b, x0, y0, px, py, cols):
    return [Plate(x0 + px * (i % cols), y0 + py * (i // cols), a, b) for i in range(n)]


def _table_scenes():
    sc = []
    # 2 x 2 patches, 3 voxels apart: 320 clusters of 4 cells, 256 of them in every 1024 cells
    sc.append(SplitScene("sums_fallback", _grid(320, 2, 2, 6, 6, 3, 3, 40), pred_sums_fallback, down_sample=3,
                         cluster_size_xy=1.0))
    # 2 x 8 patches on leaves of 6 voxels: x = 0 (mod 3) keeps both columns in one leaf, y = 3 (mod 6) cuts the 8 cells
    # 1 + 6 + 1, whose end centroids lie 0.35 m from the mean -- 3 slots per node; the 2 x 4 halves hold leaves of 1 + 3
    # and stay whole.  Their direction is the y axis, snapped; the diagonal pairs below them (2 x 6 in one leaf, 2 x 6
    # in the leaf above it, joined at a corner: 2 slots, centroids 0.316 m from the mean) have b / (a - d) = 3 / 8
    pairs = [(8 + 6 * i, y0, 2, 6) for y0 in (106, 124) for i in range(25)]
    pairs += [(x0 + 2, y0 + 6, a, b) for x0, y0, a, b in pairs]
    sc.append(SplitScene("stats_fallback", _grid(352, 2, 8, 6, 9, 3, 12, 44), pred_stats_fallback, extra=pairs,
                         down_sample=6, cluster_size_xy=0.3))
    # final piece counts around the regrouping's 256 switch and k_sp_rank's tile: 2 x 8 patches give two pieces each,
    # a 2 x 2 patch one
    for n_final in (255, 256, 257, 513):
        plates = _grid(n_final // 2, 2, 8, 6, 6, 3, 9, 44)
        if n_final % 2:
            plates.append(Plate(6, 6 + 9 * 8, 2, 2))
        sc.append(SplitScene("pieces_%d" % n_final, plates, pred_count(n_final, crosses=n_final == 255), down_sample=3,
                             cluster_size_xy=0.3))
    # a line of 128 halves six times down to pieces of 4, whose end cells lie 0.15 m from the mean.  With
    # cluster_size_xy = 0.15 exactly, whether such a piece is cut a seventh time hangs on the float rounding of its end
    # cells' centres (5e-7 m, either sign): no start of the line on this map has all 32 cut, so that scene proves the
    # depth and the bit-equality of the marginal decisions; 0.149 cuts every one, down to pieces of 2
    sc.append(SplitScene("deep_line", [Plate(5, 20, 128, 1)], pred_depth_marginal, down_sample=1, cluster_size_xy=0.15))
    sc.append(SplitScene("deep_line_tight", [Plate(5, 20, 128, 1)], pred_depth, down_sample=1, cluster_size_xy=0.149))
    return sc


SCENES = {s.name: s for s in _direction_scenes() + _table_scenes()}
DIRECTION = [n for n, s in SCENES.items() if s.direction]
ODD = [n for n in DIRECTION if SCENES[n].parity == "odd"]
LARGEST = max(SCENES, key=lambda n: SCENES[n].cells)
SMALLEST = min(SCENES, key=lambda n: SCENES[n].cells)

# the edges the issue names -> the scenes drawn for them
COVERAGE = {
    "x-long plates": ["even_ds3", "odd_ds3"], "y-long plates": ["even_ds3", "odd_ds3"],
    "squares": ["square_ds%d" % d for d in DOWN_SAMPLES], "one-voxel lines": ["even_ds1", "even_ds3", "odd_ds3"],
    "diagonal band": ["controls"], "shifted plates": ["even_ds3", "even_ds6"],
    "down_sample 1, 2, 3, 6": ["even_ds1", "even_ds2", "even_ds3", "even_ds6"],
    "even long side": ["even_ds%d" % d for d in DOWN_SAMPLES], "odd long side": ["odd_ds%d" % d for d in DOWN_SAMPLES],
    "k_sp_sums global fallback": ["sums_fallback"], "k_sp_stats global fallback": ["stats_fallback"],
    "255 / 256 / 257 / 513 pieces": ["pieces_255", "pieces_256", "pieces_257", "pieces_513"],
    "node count crosses 256 between levels": ["pieces_255"], "deep recursion": ["deep_line", "deep_line_tight"],
    "reuse large, small, large": [LARGEST, SMALLEST],
}
