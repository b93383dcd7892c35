"""The fast frontier chain at its kept-cluster capacities (GPU), on helpers.capacity_layout: a G400-geometry map that
is known free except for N isolated unknown blocks, one kept cluster each, many of them across tile boundaries.

A full-box search there runs on 8 x 32 tiles, ntx = 48 tile columns (test_frontier_capacity_cpu pins that).  The
last workgroup of k_tile_cross resolves a search in the LDS of its launch: max(cross_lds, resolve_lds_bytes(1024)) =
40 KiB at nz = 100, rcap = 1024 tile roots and a (kept cluster x tile column) matrix of 2 rcap = 2048 entries, so
floor(2048 / 48) = 42 clusters.  A search with 43 or more is left to the kernel k_resolve (2 FR_RCAP = 16384 =
FR_PMCAP entries); more than FR_KCAP = 256 kept clusters send it to the legacy chain.  Every search is compared with
the oracle (frontier_finder.cpp:54-164), and the path it took is asserted: a silent detour is still oracle-equal."""
import numpy as np
import pytest

import helpers
from oracle import fuel_oracle as fo

pytestmark = pytest.mark.gpu

INFO_TOL = 1e-9


@pytest.fixture(scope="module")
def fa():
    import fuel_amd
    fuel_amd.lib()
    return fuel_amd


@pytest.fixture
def maps(fa):
    om = helpers.capacity_map()
    gm = fa.SDFMap(helpers.CAP_MAP, *_box(om))
    yield om, gm
    gm.close()


def _box(om):
    return tuple(om.cfg.box_min), tuple(om.cfg.box_max)


def _state(om, gm, blocks, upload=True):
    om.occ[:] = helpers.capacity_occupancy(om, blocks)
    if upload:
        gm.uploadOccupancy(om.occ)


def _updated(om, gm, lo, hi):
    om.set_updated_box(lo, hi)
    gm.setUpdatedBox(lo, hi)


def _equal(of, gf, n, tag):
    """new clusters of the last search: count, cell sets, order, clusterInfo of every cluster; the flag plane"""
    co, cg = of.clusters(0), gf.clusters(0)
    assert len(co) == len(cg) == n, (tag, len(co), len(cg), n)
    for k, (a, b) in enumerate(zip(co, cg)):
        assert np.array_equal(np.sort(a), b), "%s: cells of cluster %d" % (tag, k)
        for u, v in zip(of.cluster_info(0, k), gf.clusterInfo(0, k)):
            assert np.abs(np.asarray(u) - np.asarray(v)).max() <= INFO_TOL, "%s: clusterInfo of cluster %d" % (tag, k)
    assert np.array_equal(of.flags, gf.flags()), "%s: flags" % tag


def _block_box(om, blocks, pad=0.2):
    """metric box around index boxes [lo, hi), padded"""
    lo = np.min([b[0] for b in blocks], axis=0)
    hi = np.max([b[1] for b in blocks], axis=0)
    return (tuple(om.origin + lo * om.res - pad), tuple(om.origin + hi * om.res + pad))


@pytest.mark.parametrize("n", helpers.CAP_SWEEP)
def test_kept_cluster_count_sweep(fa, maps, n):
    """A fresh finder (k_resolve queued behind the chain), cluster_min = 100, one full-box search with n kept clusters.
    n <= 42: resolved inside k_tile_cross; 43..256: by k_resolve, no fallback (before the fix, n >= 43 took the legacy
    chain as capacity code 17); 257 > FR_KCAP: the legacy chain, as a fallback of the fast one -- with a second radix
    pass there."""
    om, gm = maps
    assert helpers.capacity_tiles(om)[4] == 48  # (42 / 43 straddle floor(2048 / 48))
    blocks, _ = helpers.capacity_layout(om, n)
    _state(om, gm, blocks)
    gf = fa.FrontierFinder(gm, cluster_min=100)
    of = fo.OracleFrontier(om, 100)
    _updated(om, gm, *_box(om))
    n_o, n_g = of.search(), gf.searchFrontiers()
    assert n_o == n_g == n, (n_o, n_g)
    _equal(of, gf, n, "n=%d" % n)
    if n <= 256:
        assert gf.stats() == (1, 0, 0), gf.stats()
        assert gf.resolvedInLaunch() == (1 if n <= 42 else 0), gf.resolvedInLaunch()
        assert gf.pathStats() == (0, 0), gf.pathStats()
    else:
        assert gf.stats() == (0, 0, 1), gf.stats()  # (frontier_collect_fast: n_fast back, n_fallback up)
    gf.close()


@pytest.mark.parametrize("slabs", [False, True], ids=["cubes", "slabs"])
def test_cluster_min_edge_on_the_fast_chain(fa, maps, slabs):
    """Clusters of exactly S cells (helpers.CUBE_SHELL, claimed by one of their own cells; helpers.SLAB_SHELL, claimed
    by an NQ seed outside the box, which counts): all kept at cluster_min = S - 1, none at S -- the reference's
    size > cluster_min against the chain's siz > cluster_min / sum + 1 > cluster_min."""
    om, gm = maps
    n = 8 if slabs else 16
    S = helpers.SLAB_SHELL if slabs else helpers.CUBE_SHELL
    blocks, _ = helpers.capacity_layout(om, n, faces=False, slabs=slabs)
    _state(om, gm, blocks)
    for cm, want in ((S - 1, n), (S, 0)):
        gf = fa.FrontierFinder(gm, cluster_min=cm)
        of = fo.OracleFrontier(om, cm)
        _updated(om, gm, *_box(om))
        n_o, n_g = of.search(), gf.searchFrontiers()
        assert n_o == n_g == want, (cm, n_o, n_g)
        _equal(of, gf, want, "cluster_min=%d" % cm)
        assert gf.stats()[0] == 1 and gf.stats()[2] == 0, gf.stats()
        gf.close()


def test_both_resolve_hand_offs_with_many_clusters(fa, maps):
    """One finder, three searches on 64 clusters: (1) a small updated box, resolved in the launch with few tile roots --
    k_resolve is not queued for the next search; (2) the full box: the launch cannot hold the cluster matrix, nobody is
    queued behind it, so _search_end queues k_resolve + k_tile_out (the late resolve); (3) after reset(), the full box
    again: k_resolve is queued this time and does the work.  No search falls back to the legacy chain."""
    om, gm = maps
    blocks, _ = helpers.capacity_layout(om, 64)
    _state(om, gm, blocks)
    box = _box(om)
    gf = fa.FrontierFinder(gm, cluster_min=100)
    of = fo.OracleFrontier(om, 100)
    lo = np.array(box[0]) + np.array([6.0, 6.0, 0.0])
    small = (tuple(lo), tuple(lo + np.array([3.0, 3.0, 2.0])))
    _updated(om, gm, *small)
    n_o, n1 = of.search(), gf.searchFrontiers()
    assert n_o == n1 and n1 <= 64 - 43, (n_o, n1)
    _equal(of, gf, n1, "small box")
    assert gf.resolvedInLaunch() == 1 and gf.pathStats() == (0, 0)
    of.commit()
    gf.commit()
    _updated(om, gm, *box)
    n_o, n_g = of.search(), gf.searchFrontiers()
    assert n_o == n_g == 64 - n1, (n_o, n_g)
    _equal(of, gf, n_g, "full box after the small one")
    assert gf.pathStats() == (1, 0), "the late resolve was expected: %s" % (gf.pathStats(),)
    assert gf.resolvedInLaunch() == 1 and gf.stats() == (2, 0, 0), (gf.resolvedInLaunch(), gf.stats())
    gf.reset()
    of = fo.OracleFrontier(om, 100)
    _updated(om, gm, *box)
    n_o, n_g = of.search(), gf.searchFrontiers()
    assert n_o == n_g == 64, (n_o, n_g)
    _equal(of, gf, 64, "full box after reset")
    assert gf.pathStats() == (1, 0) and gf.resolvedInLaunch() == 1, (gf.pathStats(), gf.resolvedInLaunch())
    assert gf.stats() == (3, 0, 0), gf.stats()
    gf.close()


def test_frame_fused_beside_a_many_cluster_search(fa, maps):
    """Streaming: a new occupancy is uploaded between _search_begin and _search_end of a 64-cluster search (three
    cubes gone, three new).  The search answers for the state it began on -- before the fix it failed with ELIMIT, the
    error for a fast-chain overflow after a fusion -- and the next search, over the changed blocks, removes and adds
    what the oracle does (new clusters, removed ids, flags)."""
    om, gm = maps
    b64, _ = helpers.capacity_layout(om, 64)
    b67, _ = helpers.capacity_layout(om, 67)
    gone = [b64[10], b64[31], b64[50]]
    b2 = [b for b in b67 if b not in gone]
    _state(om, gm, b64)
    box = _box(om)
    gf = fa.FrontierFinder(gm, cluster_min=100)
    of = fo.OracleFrontier(om, 100)
    _updated(om, gm, *box)
    gf.searchFrontiersBegin()
    _state(om, gm, b2)                   # the next frame, fused beside the running search ...
    om.occ[:] = helpers.capacity_occupancy(om, b64)
    n_o = of.search()                    # ... which the oracle answers on the state before it
    n_g = gf.searchFrontiersEnd()
    assert n_o == n_g == 64, (n_o, n_g)
    _equal(of, gf, 64, "search beside the fusion")
    assert gf.stats() == (1, 0, 0), gf.stats()
    of.commit()
    gf.commit()
    _state(om, gm, b2, upload=False)
    _updated(om, gm, *_block_box(om, gone + b67[64:]))
    n_o, n_g = of.search(), gf.searchFrontiers()
    assert n_o == n_g == 3, (n_o, n_g)
    _equal(of, gf, 3, "search of the changed blocks")
    assert np.array_equal(of.removed_ids(), gf.removedIds()) and len(gf.removedIds()) == 3
    assert gf.stats()[2] == 0, gf.stats()
    gf.close()


def test_recovery_after_a_legitimate_elimit(fa, maps):
    """A search whose fast chain overflows (more than FR_KCAP = 256 new clusters) after a frame was fused beside it
    fails with ELIMIT: the occupancy it was about is gone.  The contract of that path: the next search looks at the
    whole box again, and after it the finder's committed clusters and flag plane equal the oracle's, which ran the
    missed search and the next one normally.  Compared as a set of sorted cell arrays: the two histories differ, so
    cluster order and removed ids are not part of the contract."""
    om, gm = maps
    box = _box(om)
    b40, _ = helpers.capacity_layout(om, 40)
    b300, _ = helpers.capacity_layout(om, 300)
    b302, _ = helpers.capacity_layout(om, 302)
    bB = [b for b in b302 if b not in b300[40:48]]  # state B: eight of A's new blocks gone, two more
    _state(om, gm, b40)
    gf = fa.FrontierFinder(gm, cluster_min=100)
    of = fo.OracleFrontier(om, 100)
    _updated(om, gm, *box)
    n_o, n_g = of.search(), gf.searchFrontiers()
    assert n_o == n_g == 40, (n_o, n_g)
    _equal(of, gf, 40, "first search")
    of.commit()
    gf.commit()
    _state(om, gm, b300)                 # state A: 260 new clusters
    _updated(om, gm, *box)
    gf.searchFrontiersBegin()
    gm.uploadOccupancy(helpers.capacity_occupancy(om, bB))  # state B fused beside it
    with pytest.raises(fa.FuelmiError):
        gf.searchFrontiersEnd()
    assert of.search() == 260            # the oracle's search of state A, committed
    of.commit()
    _state(om, gm, bB, upload=False)
    _updated(om, gm, *box)
    of.search()
    of.commit()
    gf.searchFrontiers()                 # (the whole box, whatever the updated box says)
    gf.commit()
    as_set = lambda cl: sorted(tuple(np.sort(c)) for c in cl)  # noqa: E731
    assert len(gf.clusters(1)) == len(of.clusters(1)) == len(bB), (len(gf.clusters(1)), len(of.clusters(1)))
    assert as_set(gf.clusters(1)) == as_set(of.clusters(1)), "committed clusters differ from the oracle's"
    assert np.array_equal(of.flags, gf.flags()), "the flag plane and the cluster lists parted ways"
    gf.close()
