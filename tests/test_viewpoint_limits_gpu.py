"""Viewpoint sampling (k_vp_sample and the voxel walk ray_clear<false>) at its wave, candidate and map edges (GPU).

Every test builds a hand-written state with helpers.vp_* (known free, unknown and occupied boxes; no fusion), gives the
same log-odds to the device map, inflates on both sides and compares computeFrontiersToVisit through the C-ABI with
oracle.fuel_oracle.OracleFrontier: the same active / dormant partition, per cluster the same viewpoints in the same
order, equal coverage counts, bit-equal positions, yaws within 1e-9 rad on the circle (NaN where the oracle has NaN),
equal cell sets.  Before it looks at the device, each test asserts from the oracle and the inputs alone that the edge
it is named after was reached (helpers.vp_guard_*; test_viewpoint_limits_cpu.py runs the same guards without a GPU),
and that no candidate coincides with a filtered cell: normalized() of a zero vector divides by zero in the Eigen
stand-in the oracle was pinned with, where real Eigen would not, so such a coincidence (distance <= 1e-6) is kept
out of the scenes.  test_oracle_vs_reference_cpu.py pins the oracle to the real reference on these scenes."""
import numpy as np
import pytest

import helpers
from oracle import fuel_oracle as fo

pytestmark = pytest.mark.gpu

YAW_TOL = 1e-9
ORDERS = pytest.mark.parametrize("reference_order", [False, True], ids=["device_order", "reference_order"])


@pytest.fixture(scope="module")
def fa():
    import fuel_amd
    fuel_amd.lib()
    return fuel_amd


def _device(fa, scene, om, reference_order=False):
    """the device twin of an oracle map that was painted and inflated: (gm, gf), nothing searched yet"""
    gm = fa.SDFMap(scene.map_size, *scene.box_args(), **scene.map_kw)
    assert tuple(gm.nvox) == tuple(om.nvox)
    gm.uploadOccupancy(om.occ)
    gm.setLocalBound(*helpers.full_box(om.nvox))
    gm.clearAndInflateLocalMap()
    gf = fa.FrontierFinder(gm, split=True, reference_order=reference_order, **scene.finder)
    gf.setViewpointConfig(gf.viewpointConfig(**scene.vcfg))
    return gm, gf


def _same_lists(of, gf, reference_order, tag):
    """the committed lists of both sides, by the acceptance criteria of this suite; returns the viewpoint total"""
    total = 0
    for which in (1, 2):
        co, cg = of.clusters(which), gf.clusters(which)
        assert len(co) == len(cg), "%s: list %d holds %d clusters, the oracle's %d" % (tag, which, len(cg), len(co))
        for k, (a, b) in enumerate(zip(co, cg)):
            if reference_order:
                assert np.array_equal(a, b), "%s: cells of cluster %d/%d" % (tag, which, k)
            else:
                assert np.array_equal(np.sort(a), b), "%s: cells of cluster %d/%d" % (tag, which, k)
            (pa, va), (pb, vb) = of.viewpoints(which, k), gf.viewpoints(which, k)
            assert len(va) == len(vb), "%s: cluster %d/%d has %d viewpoints, the oracle's %d" % (
                tag, which, k, len(vb), len(va))
            assert np.array_equal(va, vb), "%s: visib_num of cluster %d/%d" % (tag, which, k)
            assert np.array_equal(pa[:, :3], pb[:, :3]), "%s: positions of cluster %d/%d" % (tag, which, k)
            nan = np.isnan(pa[:, 3])
            assert np.array_equal(nan, np.isnan(pb[:, 3])), "%s: NaN yaws of cluster %d/%d" % (tag, which, k)
            d = np.abs(pa[~nan, 3] - pb[~nan, 3])
            assert d.size == 0 or np.minimum(d, 2 * np.pi - d).max() <= YAW_TOL, "%s: yaws of cluster %d/%d" % (
                tag, which, k)
            assert np.all(np.abs(pb[~nan, 3]) <= np.pi), "%s: a yaw of cluster %d/%d outside [-pi, pi]" % (tag, which, k)
            assert which == 1 or len(va) == 0
            total += len(va)
    return total


def _compare(fa, scene, om, of, reference_order=False, tag=""):
    """search + computeFrontiersToVisit on the device against an oracle that already ran them"""
    assert helpers.vp_min_cell_distance(of, scene.vcfg) > 1e-6, "a candidate coincides with a filtered cell"
    gm, gf = _device(fa, scene, om, reference_order)
    try:
        gm.setUpdatedBox(*helpers.vp_whole_map(om))
        n_new = len(of.clusters(1)) + len(of.clusters(2))
        assert gf.searchFrontiers() == n_new, tag
        for k in range(n_new):
            assert np.array_equal(of.filtered(0, k).astype(np.float32), gf.filtered(0, k)), "%s: filtered %d" % (tag, k)
        na, nd = gf.computeFrontiersToVisit()
        assert (na, nd) == (len(of.clusters(1)), len(of.clusters(2))), (tag, na, nd)
        return _same_lists(of, gf, reference_order, tag)
    finally:
        gf.close()
        gm.close()


# ---- 1: cells per cluster -------------------------------------------------------------------------------------------
@ORDERS
@pytest.mark.parametrize("down_sample", [1, 3])
def test_cells_per_cluster(fa, down_sample, reference_order):
    """nf of 1, 2, 63, 64, 65, 128, 129 and 193 in one scene (down_sample = 1): the first, last and one-past-last lane
    of every stride of the bearing loop (i = 1 + lane) and of the visible-cell loop (i0 += 64 with a ballot); at
    down_sample = 3 the same patches leave ragged leaf counts."""
    scene = helpers.vp_scene_cells(down_sample)
    om, of = helpers.vp_oracle(scene, reference_order)
    if down_sample == 1:
        helpers.vp_guard_cells(of)
    assert _compare(fa, scene, om, of, reference_order) > 500


# ---- 2: clearance block ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(helpers.VP_CLEARANCES))
def test_clearance_block_last_voxel(fa, name):
    """isNearUnknown over (2v + 1)^2 * 3 voxels for v = 0, 1, 2, 4 and the clearance 0.3 m whose quotient floors to 2:
    a lone unknown voxel at the block's last corner (+v, +v, +1) must reject the candidate -- it sits in the block's
    last stride of 64 -- and one at +3, +3, +1 must not where v = 2."""
    scene, flips, stays = helpers.vp_scene_clearance(name)
    om, of = helpers.vp_guard_clearance(name, scene, flips, stays)
    assert _compare(fa, scene, om, of, tag=name) > 100


# ---- 3: strict comparisons ------------------------------------------------------------------------------------------
@ORDERS
@pytest.mark.parametrize("ulps", [-1, 0, 1])
@pytest.mark.parametrize("face", ["x_min", "y_max"])
def test_candidate_on_the_box_face(fa, face, ulps, reference_order):
    """isInBox(pos) is strict: a candidate whose coordinate equals the box face is outside, one ulp inside it is in"""
    scene, p, inside = helpers.vp_scene_box_face(face, ulps, reference_order)
    om, of = helpers.vp_oracle(scene, reference_order)
    assert (p in helpers.vp_positions(of)) == inside == (ulps == (-1 if face == "x_min" else 1))
    assert _compare(fa, scene, om, of, reference_order) > 20


def test_min_visib_num_is_a_strict_bound(fa):
    """visib_num > min_visib_num: at v, a count at least three candidates have exactly, they are dropped; at v - 1 kept"""
    v, n = helpers.vp_min_visib_edge()
    helpers.vp_guard_min_visib(v, n)
    got = []
    for m in (v, v - 1):
        scene = helpers.vp_scene_occluded(min_visib_num=m)
        om, of = helpers.vp_oracle(scene)
        got.append(_compare(fa, scene, om, of, tag="min_visib_num=%d" % m))
    assert got[1] - got[0] == n >= helpers.VP_MIN_VISIB_TIES, (got, n)


def test_max_dist_between_and_on_a_cell(fa):
    """insideFOV drops a cell farther than max_dist, keeps one at exactly max_dist: the bound between the nearest and
    the farthest cell of a cluster, equal to one cell's distance (the double sampleViewpoints computes), one ulp less"""
    base, p, edges = helpers.vp_max_dist_edges()
    helpers.vp_guard_max_dist(base, p, edges)
    for name, d in edges.items():
        scene = base.variant(max_dist=d)
        om, of = helpers.vp_oracle(scene)
        _compare(fa, scene, om, of, tag=name)


def test_collinear_cells(fa):
    """every cell on the line through the candidate along x: ref x dir is exactly 0 (the sign test `< 0` must not fire)
    and every dot product +-1, acos at the ends of its domain"""
    scene = helpers.vp_scene_collinear()
    om, of = helpers.vp_oracle(scene)
    helpers.vp_guard_collinear(scene, of)
    assert _compare(fa, scene, om, of) > 50


# ---- 4: frustum -----------------------------------------------------------------------------------------------------
@ORDERS
@pytest.mark.parametrize("family", ["patch", "room"])
def test_narrow_asymmetric_frustum(fa, family, reference_order):
    """top 0.25, left 0.45, right 0.20: the planes cut through the clusters (a quarter of the candidates or more see
    fewer cells than the cluster has) and exchanging left and right changes the counts, so a swapped normal shows"""
    scene = helpers.vp_scene_frustum(family)
    om, of = helpers.vp_oracle(scene, reference_order)
    helpers.vp_guard_frustum(family, of, reference_order)
    assert _compare(fa, scene, om, of, reference_order) > 40


# ---- 5: yaw wrap ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,dphi,want", [("patch", None, (1, "below")),
                                              ("patch", helpers.VP_DPHI_ABOVE, (1, -1, "below")),
                                              ("step", None, ("above",))], ids=["below_axis", "above_axis", "step"])
def test_yaw_wrap_next_to_pi(fa, family, dphi, want):
    """Candidates due +x of clusters that are symmetric in y: mean bearings next to atan2's branch cut.  The default
    candidate_dphi puts the phi ~ 0 column a hair below the axis (yaws just under +pi only: the construction gives one
    side); a dphi from a pi rounded up puts it above (both sides).  On flat patches the sums leave [-pi, pi] only below
    -pi (the first wrap loop), on the stepped block above +pi (the second).  Yaws are compared on the circle, where a
    missing wrap would not show: every device yaw must also lie in [-pi, pi] (_same_lists)."""
    scene = helpers.vp_scene_yaw_wrap(family)
    if dphi is not None:
        scene.vcfg["dphi"] = dphi
    om, of = helpers.vp_oracle(scene)
    got = helpers.vp_guard_yaw_wrap(of)
    assert all(got[w] >= helpers.VP_YAW_MIN for w in want), got
    assert _compare(fa, scene, om, of) > 50


# ---- 6: grid arithmetic ---------------------------------------------------------------------------------------------
@ORDERS
@pytest.mark.parametrize("grid", list(helpers.VP_GRIDS))
def test_occluded_scene_across_grids(fa, grid, reference_order):
    """the room scene with pillars at 0.05 / 0.1 / 0.15 m, with an origin that is no multiple of the resolution in x, y
    and z (posToIndex floors, the ray walk truncates toward zero) and odd nz (bit-plane rows straddle words)"""
    scene = helpers.vp_scene_occluded(grid)
    om, of = helpers.vp_oracle(scene, reference_order)
    if grid != "r0.10_aligned":
        assert om.nvox[2] % 2 == 1 and all(abs(o / om.res - round(o / om.res)) > 0.05 for o in om.origin)
    helpers.vp_guard_occluded(grid, of, reference_order)
    assert _compare(fa, scene, om, of, reference_order, grid) >= 60


# ---- 7: map and box faces -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beyond", [False, True], ids=["box_is_map", "box_beyond_map"])
def test_clusters_against_the_map_faces(fa, beyond):
    """candidates, clearance blocks and rays that reach indices outside the map (idx_in_map false: the voxel passes)"""
    scene = helpers.vp_scene_faces(beyond)
    om, of = helpers.vp_oracle(scene)
    helpers.vp_guard_faces(om, of, scene.vcfg, beyond)
    assert _compare(fa, scene, om, of) > 200


def test_candidate_less_than_a_voxel_below_the_map(fa):
    """posToIndex floors: a candidate less than a voxel outside the low x face has index -1 (outside the map, never
    inflated), not the 0 a truncating cast would give -- where an occupied voxel waits"""
    scene, hit = helpers.vp_scene_floor_probe()
    om, of = helpers.vp_oracle(scene)
    helpers.vp_guard_floor_probe(om, of, hit)
    assert _compare(fa, scene, om, of) > 100


# ---- 8: candidate tables --------------------------------------------------------------------------------------------
def test_candidate_tables(fa):
    """candidate_rnum 1 / 5, candidate_dphi 0.5 (does not divide 2 pi) / 7.0 (one angle per circle), rmin 0.05"""
    ns = {}
    for name, kw in helpers.VP_TABLES.items():
        scene = helpers.vp_scene_occluded(**kw)
        om, of = helpers.vp_oracle(scene)
        ns[name] = helpers.vp_guard_tables(of, scene.vcfg)
        assert _compare(fa, scene, om, of, tag=name) > 0
    assert ns == helpers.VP_TABLE_NS and len(set(ns.values())) >= 5, ns


# ---- 9: rounds and staging ------------------------------------------------------------------------------------------
def test_rounds_share_and_regrow_the_staging_buffer(fa):
    """One finder: a small round, isFrontierCovered, a round that needs several times the staging bytes, isFrontierCovered,
    a small round again; a computeFrontiersToVisit with no new clusters in between returns (0, 0) and changes nothing."""
    scenes = [helpers.vp_scene_rounds(r) for r in range(3)]
    om = helpers.vp_map(scenes[0])
    om.set_local_bound(*helpers.full_box(om.nvox))
    of = fo.OracleFrontier(om, split=True, canonical_order=True, **scenes[0].finder)
    of.set_viewpoint_cfg(fo.viewpoint_cfg(**scenes[0].vcfg))
    gm = gf = None
    need, dormant, covered = [], 0, []
    ns = len(helpers.vp_candidate_offsets(scenes[0].vcfg))
    try:
        for r, scene in enumerate(scenes):
            om.occ[:] = helpers.vp_occupancy(om, scene.paint)
            om.inflate_local()
            if gm is None:
                gm, gf = _device(fa, scene, om)
            else:
                gm.uploadOccupancy(om.occ)
                gm.clearAndInflateLocalMap()
            om.set_updated_box(*helpers.vp_whole_map(om))
            gm.setUpdatedBox(*helpers.vp_whole_map(om))
            if r:
                covered.append(of.is_covered())
                assert gf.isFrontierCovered() == covered[-1], "round %d: isFrontierCovered" % r
                om.set_updated_box(*helpers.vp_whole_map(om))
                gm.setUpdatedBox(*helpers.vp_whole_map(om))
            n = of.search()
            assert gf.searchFrontiers() == n > 0, "round %d" % r
            assert np.array_equal(of.removed_ids(), gf.removedIds()), "round %d" % r
            need.append(helpers.vp_stage_bytes(n, ns, sum(len(of.filtered(0, k)) for k in range(n))))
            before = (len(of.clusters(1)), len(of.clusters(2)))
            of.compute_to_visit()
            na, nd = gf.computeFrontiersToVisit()
            assert (na, nd) == (len(of.clusters(1)) - before[0], len(of.clusters(2)) - before[1]), "round %d" % r
            dormant += nd
            assert _same_lists(of, gf, False, "round %d" % r) > 0
            assert gf.computeFrontiersToVisit() == (0, 0)
            _same_lists(of, gf, False, "round %d, after the empty call" % r)
            om.set_updated_box(*helpers.vp_whole_map(om))
            gm.setUpdatedBox(*helpers.vp_whole_map(om))
            assert not gf.isFrontierCovered() and not of.is_covered(), "round %d: nothing changed yet" % r
    finally:
        if gf is not None:
            gf.close()
        if gm is not None:
            gm.close()
    helpers.vp_guard_stage_growth(need)
    assert dormant > 0 and covered == [True, True], (dormant, covered)
