"""Round-6 parity tests (GPU): what VERDICT r5 found missing -- the ORACLE at the largest size."""
import numpy as np
import pytest

import helpers
from oracle import fuel_oracle as fo

pytestmark = pytest.mark.gpu

ESDF_TOL = 1e-4   # north_star: ESDF values within 1e-4
BIG = 1e6


@pytest.fixture(scope="module")
def fa():
    import fuel_amd
    fuel_amd.lib()
    return fuel_amd


def test_full_size_g800_full_box_against_the_oracle(fa):
    """BASELINE.json configs[3]'s map (800 x 800 x 200 @ 0.1 m, bench.py --workload G800), FULL box, against the oracle
    itself (VERDICT r5 missing #5 / next #6; round 5 had properties and family-vs-family equality only): inflation
    bit-exact (sdf_map.cpp:434-471) with the FACTORED inflation kernels asserted to have run (the box's address range is
    above the fused kernel's limit -- this is the only size where they do), ESDF within 1e-4 over the whole box
    (sdf_map.cpp:152-199) with the packed 16-bit family asserted to have run (its <0,4,4> z/y instantiation), and one
    fresh full-box frontier search: sorted cell sets of every cluster, cluster order, flags
    (frontier_finder.cpp:54-121).  The oracle needs ~6 GB of host memory and ~10 s of one core for this."""
    import bench
    map_size, box, occ, _, _ = bench.build_inputs("G800", seed=42, n_traj=1)
    om = fo.OracleMap(map_size, *box)
    assert om.nvox == (800, 800, 200)
    om.occ[:] = occ
    gm = fa.SDFMap(map_size, *box)
    gm.uploadOccupancy(occ)
    lo, hi = helpers.full_box(om.nvox)
    om.set_local_bound(lo, hi)
    gm.setLocalBound(lo, hi)
    om.inflate_local()
    gm.clearAndInflateLocalMap()
    assert gm.lastInflateKernel() == 1, "the factored inflation pair was expected to run on the 128 M-voxel box"
    gm.updateESDF3d()
    assert gm.lastEsdfFamily() == 0, "the packed family was expected to run"
    h = gm.syncHost(inflate=True, distance=True)
    assert np.array_equal(h["inflate"], om.infl), "inflated occupancy not bit-exact"
    del h["inflate"]
    om.update_esdf()
    worst = 0.0
    d_g = h["distance"].reshape(om.nvox)
    d_o = om.dist.reshape(om.nvox)
    for x0 in range(0, om.nvox[0], 100):   # (slab by slab: the clipped copies of two 1-GB fields at once are not needed)
        a = np.clip(d_o[x0:x0 + 100], -BIG, BIG)
        b = np.clip(d_g[x0:x0 + 100], -BIG, BIG)
        worst = max(worst, float(np.abs(a - b).max()))
    assert worst <= ESDF_TOL, "ESDF differs from the oracle by %g" % worst
    del h, d_g
    of = fo.OracleFrontier(om, 100)
    gf = fa.FrontierFinder(gm, cluster_min=100)
    om.set_updated_box(*box)
    gm.setUpdatedBox(*box)
    n_o, n_g = of.search(), gf.searchFrontiers()
    assert n_o == n_g and n_o > 0
    for a, b in zip(of.clusters(0), gf.clusters(0)):
        assert np.array_equal(np.sort(a), b)
    assert np.array_equal(of.flags, gf.flags())
    gf.close()
    gm.close()


def test_legacy_chain_on_the_headline_map(fa):
    """The round-1 frontier chain (global lock-free union-find + multisplit: what a search falls back to when a table
    of the tile chain overflows, and what every finder with cluster_min < 1 runs) on the 400 x 400 x 100 headline map,
    full exploration box, against the oracle (its only G400-size coverage was through the fast
    chain).  cluster_min = 0 keeps every component, and two fresh searches in a row run on the finder's two buffer sets.  Cell sets per cluster, cluster order, flags
    (frontier_finder.cpp:54-164)."""
    import bench
    map_size, box, occ, _, _ = bench.build_inputs("G400", seed=42, n_traj=1)
    om = fo.OracleMap(map_size, *box)
    om.occ[:] = occ
    gm = fa.SDFMap(map_size, *box)
    gm.uploadOccupancy(occ)
    of = fo.OracleFrontier(om, 0)
    gf = fa.FrontierFinder(gm, cluster_min=0)
    for rnd in range(2):
        if rnd:
            of = fo.OracleFrontier(om, 0)
            gf.reset()
        om.set_updated_box(*box)
        gm.setUpdatedBox(*box)
        n_o, n_g = of.search(), gf.searchFrontiers()
        assert n_o == n_g and n_o > 0, (n_o, n_g)
        for a, b in zip(of.clusters(0), gf.clusters(0)):
            assert np.array_equal(np.sort(a), b)
        assert np.array_equal(of.flags, gf.flags())
    assert gf.stats()[0] == 0 and gf.stats()[1] >= 2, gf.stats()  # (fast, legacy, fallbacks)
    gf.close()
    gm.close()


def test_headline_search_is_resolved_by_the_cross_kernels_last_workgroup(fa):
    """Round 6: the last workgroup of k_tile_cross joins the tile roots itself (agent-scope pair stores, a
    last-workgroup-done counter, no fence) when the search has at most 1 024 of them -- the headline map's full-box search
    has 779.  The CHOICE is asserted (a silent fall-through to the k_resolve launch would pass every parity test), then
    the result against the oracle as everywhere: cell sets, cluster order, flags, and the same again on the finder's
    other buffer set (frontier_finder.cpp:54-164)."""
    import bench
    map_size, box, occ, _, _ = bench.build_inputs("G400", seed=42, n_traj=1)
    om = fo.OracleMap(map_size, *box)
    om.occ[:] = occ
    gm = fa.SDFMap(map_size, *box)
    gm.uploadOccupancy(occ)
    gf = fa.FrontierFinder(gm, cluster_min=100)
    for rnd in range(2):
        of = fo.OracleFrontier(om, 100)
        if rnd:
            gf.reset()
        om.set_updated_box(*box)
        gm.setUpdatedBox(*box)
        n_o, n_g = of.search(), gf.searchFrontiers()
        assert n_o == n_g and n_o > 0
        for a, b in zip(of.clusters(0), gf.clusters(0)):
            assert np.array_equal(np.sort(a), b)
        assert np.array_equal(of.flags, gf.flags())
    assert gf.stats() == (2, 0, 0), gf.stats()
    assert gf.resolvedInLaunch() == 2, "the searches were resolved by k_resolve, not inside k_tile_cross"
    gf.close()
    gm.close()


def test_search_that_outgrows_the_in_launch_resolve(fa):
    """A finder whose last search was resolved inside k_tile_cross with room to spare does not queue k_resolve for the next
    one.  Here the next one has thousands of tile-local components (a lattice of isolated unknown voxels appears in free
    space: each a little shell of frontier cells, none of them a kept cluster) -- more than the launch holds: the chain
    reports that, _search_end queues k_resolve + k_tile_out itself and collects the result.  Three searches against the
    oracle -- fresh full box, a small updated box, the full box after the change: cell sets, cluster order, flags
    (frontier_finder.cpp:54-164)."""
    import bench
    map_size, box, occ, _, _ = bench.build_inputs("G400", seed=42, n_traj=1)
    om = fo.OracleMap(map_size, *box)
    om.occ[:] = occ
    nv = om.nvox
    gm = fa.SDFMap(map_size, *box)
    gm.uploadOccupancy(om.occ)
    of = fo.OracleFrontier(om, 100)
    gf = fa.FrontierFinder(gm, cluster_min=100)
    lo = np.array(box[0]) + np.array([6.0, 6.0, 0.0])
    small = (tuple(lo), tuple(lo + np.array([3.0, 3.0, 2.0])))
    for rnd, ub in enumerate((box, small, box)):
        if rnd == 2:
            o3 = om.occ.reshape(nv)
            free = (o3 >= om.l_min - 1e-3) & (o3 <= om.l_occ)
            lat = np.zeros(nv, dtype=bool)
            lat[10::20, 10::20, 5::10] = True
            o3[free & lat] = om.l_min - 0.01  # unknown
            gm.uploadOccupancy(om.occ)
        om.set_updated_box(*ub)
        gm.setUpdatedBox(*ub)
        n_o, n_g = of.search(), gf.searchFrontiers()
        assert n_o == n_g, (rnd, n_o, n_g)
        for a, b in zip(of.clusters(0), gf.clusters(0)):
            assert np.array_equal(np.sort(a), b)
        assert np.array_equal(of.flags, gf.flags())
        of.commit()
        gf.commit()
        if rnd == 1:
            assert gf.resolvedInLaunch() == 2, "the first two searches were expected to be resolved inside k_tile_cross"
    assert gf.stats() == (3, 0, 0), gf.stats()
    assert gf.resolvedInLaunch() == 2, "the last search was expected to outgrow the launch (k_resolve queued by _search_end)"
    assert gf.pathStats() == (1, 0), "one late resolve (k_resolve + k_tile_out queued by _search_end) was expected: %s" % (gf.pathStats(),)
    gf.close()
    gm.close()


def test_full_height_frontier_wall_retiles_instead_of_falling_back(fa):
    """A frontier WALL: everything with x < 20 m known free, everything beyond unknown -- the plane x = 199 is one
    frontier surface of 400 x 100 cells, 3 200 of them in every 8 x 32 tile it crosses, more than a tile holds (2 048).
    The chain reports the capacity, runs again on the menu's next tile (8 x 16: 1 600 cells) and answers -- the legacy
    chain (ten times slower) is not needed.  Cells, cluster order, flags against the oracle (frontier_finder.cpp:54-164);
    stats say (1 fast, 0 legacy, 0 fallbacks)."""
    import bench
    map_size, box, occ, _, _ = bench.build_inputs("G400", seed=42, n_traj=1)
    om = fo.OracleMap(map_size, *box)
    nv = om.nvox
    o3 = np.full(nv, om.l_min - 0.01)   # unknown
    o3[:200, :, :] = om.l_min            # known free
    om.occ[:] = o3.reshape(-1)
    gm = fa.SDFMap(map_size, *box)
    gm.uploadOccupancy(om.occ)
    gf = fa.FrontierFinder(gm, cluster_min=100)
    for rnd in range(2):  # (the second fresh search starts on the smaller tile the first one ended on)
        of = fo.OracleFrontier(om, 100)
        if rnd:
            gf.reset()
        om.set_updated_box(*box)
        gm.setUpdatedBox(*box)
        n_o, n_g = of.search(), gf.searchFrontiers()
        assert n_o == n_g and n_o >= 1, (n_o, n_g)
        for a, b in zip(of.clusters(0), gf.clusters(0)):
            assert np.array_equal(np.sort(a), b)
        assert np.array_equal(of.flags, gf.flags())
    assert gf.stats() == (2, 0, 0), gf.stats()
    gf.close()
    gm.close()


def test_small_empty_and_full_searches_behind_each_other(fa):
    """Searches of every size behind each other on one finder: the full box, a small updated box (resolved inside
    k_tile_cross, after which k_resolve is no longer queued), an updated box outside the exploration box (an empty search:
    no kernel at all), the small box again -- each against the oracle (cells, flags), none left waiting for a result
    nobody publishes."""
    map_size = (12.0, 10.0, 4.0)
    om, _, _, box = helpers.explored_oracle_map(map_size, 25, 20, width=120, height=90)
    gm = fa.SDFMap(tuple(om.cfg.map_size), box[0], box[1])
    gm.uploadOccupancy(om.occ)
    of = fo.OracleFrontier(om, 10)
    gf = fa.FrontierFinder(gm, cluster_min=10)
    lo = np.array(box[0])
    boxes = [box, (tuple(lo + 1.0), tuple(lo + 2.5)), (tuple(lo - 30.0), tuple(lo - 20.0)), (tuple(lo + 1.0), tuple(lo + 2.5))]
    for ub in boxes:
        om.set_updated_box(*ub)
        gm.setUpdatedBox(*ub)
        n_o, n_g = of.search(), gf.searchFrontiers()
        assert n_o == n_g, (ub, n_o, n_g)
        for a, b in zip(of.clusters(0), gf.clusters(0)):
            assert np.array_equal(np.sort(a), b)
        assert np.array_equal(of.flags, gf.flags())
        of.commit()
        gf.commit()
    gf.close()
    gm.close()
