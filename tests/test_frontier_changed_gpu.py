"""The changed-cluster test in front of a search (frontier_changed.hip; searchFrontiers' removal of outdated clusters,
frontier_finder.cpp:62-93) at the edges of its four paths, on helpers.changed_* layouts: every committed cluster is a
candidate of a full-box search, so nc and total are what the layout plans (test_frontier_changed_cpu pins them on the
oracle).  Every case asserts the path it took (FrontierFinder.changedStats) and compares with the oracle: the new
clusters, removedIds, both committed lists and the flag plane."""
import numpy as np
import pytest

import helpers
from oracle import fuel_oracle as fo

pytestmark = pytest.mark.gpu

INFO_TOL = 1e-9
CM = helpers.CHG_CLUSTER_MIN


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


def _upload(om, gm, occ):
    om.occ[:] = occ
    gm.uploadOccupancy(om.occ)


def _search(om, gm, of, gf, box=None):
    box = box or _box(om)
    om.set_updated_box(*box)
    gm.setUpdatedBox(*box)
    n_o, n_g = of.search(), gf.searchFrontiers()
    assert n_o == n_g, (n_o, n_g)
    return n_g


def _equal(of, gf, tag, lists=True):
    """new clusters (cells, order, clusterInfo), removed ids, the committed lists with their cells, the flag plane"""
    for which in (0, 1, 2) if lists else (0,):
        co, cg = of.clusters(which), gf.clusters(which)
        assert len(co) == len(cg), (tag, which, len(co), len(cg))
        for k, (a, b) in enumerate(zip(co, cg)):
            assert np.array_equal(np.sort(a), b), "%s: cells of cluster %d of list %d" % (tag, k, which)
            if which == 0:
                for u, v in zip(of.cluster_info(0, k), gf.clusterInfo(0, k)):
                    assert np.abs(np.asarray(u) - np.asarray(v)).max() <= INFO_TOL, "%s: clusterInfo %d" % (tag, k)
    assert np.array_equal(of.removed_ids(), gf.removedIds()), (tag, of.removed_ids(), gf.removedIds())
    assert np.array_equal(of.flags, gf.flags()), "%s: flags" % tag


def _expect(gf, before, path, nc, total):
    st = gf.changedStats()
    want = list(before["paths"])
    want[helpers.RM_PATHS.index(path)] += 1
    assert st["paths"] == tuple(want), (st, path)
    assert (st["nc"], st["total"]) == (nc, total), st
    assert (st["mark"] == 0) == (path == "one"), st
    return st


def _committed(fa, om, gm, shapes):
    """fresh finder and oracle, the layout's clusters found by a full-box search and committed"""
    _upload(om, gm, helpers.capacity_occupancy(om, helpers.changed_blocks(om, shapes)))
    gf = fa.FrontierFinder(gm, cluster_min=CM)
    of = fo.OracleFrontier(om, CM)
    assert _search(om, gm, of, gf) == len(shapes)
    _equal(of, gf, "layout", lists=False)
    of.commit()
    gf.commit()
    return of, gf


def _where(cand, total, head=True):
    """pooled positions of the changed cells: the first cell of the first candidate; two more clusters of the first
    wave (behind its first changed lane; head: the table starts with helpers.WAVE_HEAD single voxels); the last cell,
    at total - 1 (the NQ seed of a seed-claimed last candidate); one cell either side of a workgroup boundary, each in
    a cluster that spans its boundary"""
    starts = np.cumsum([0] + [len(c) for _, _, c in cand])
    owner = lambda i: int(np.searchsorted(starts, i, side="right") - 1)  # noqa: E731
    pos = [0, starts[3] + 2, starts[7] + 5, total - 1] if head else [0, total - 1]
    used = {owner(i) for i in pos}
    for side in (-1, 0):
        b = next(b for b in range(256, total - 1, 256)
                 if owner(b - 1) == owner(b) and owner(b) not in used)
        pos.append(b + side)
        used.add(owner(b))
    assert not head or (all(owner(i) < 11 for i in pos[:3]) and pos[2] < 64)
    return pos, sorted({owner(i) for i in pos})


def _cells_at(cand, pos):
    flat = np.concatenate([c for _, _, c in cand])
    return flat[np.asarray(pos)]


@pytest.mark.parametrize("name", list(helpers.CHG_EDGES))
def test_path_edges(fa, maps, name):
    """Each edge layout: a search with nothing changed (nothing removed, flags untouched), then one with a cell changed
    at every position of _where -- the first cell, the wave, the last seed, both sides of a workgroup boundary"""
    om, gm = maps
    n, total, path = helpers.CHG_EDGES[name]
    of, gf = _committed(fa, om, gm, helpers.changed_edge_shapes(name))
    cand = helpers.changed_candidates(of, om, *_box(om))
    assert (len(cand), sum(len(c) for _, _, c in cand)) == (n, total)
    st0 = gf.changedStats()
    assert _search(om, gm, of, gf) == 0
    st1 = _expect(gf, st0, path, n, total)
    assert len(gf.removedIds()) == 0
    _equal(of, gf, name + " unchanged", lists=False)
    pos, owners = _where(cand, total)
    _upload(om, gm, helpers.occupy(om, _cells_at(cand, pos)))
    _search(om, gm, of, gf)
    st2 = _expect(gf, st1, path, n, total)
    assert st2["mark"] > st1["mark"] or path == "one"
    assert list(gf.removedIds()) == [k - r for r, k in enumerate(owners)]
    _equal(of, gf, name)
    gf.close()


@pytest.mark.parametrize("name", ["bar_2049", "table_nc1025"])
def test_host_copied_candidates(fa, maps, name):
    """The committed lists read (materialised on the host) before the changed-cluster test"""
    om, gm = maps
    n, total, path = helpers.CHG_EDGES[name]
    of, gf = _committed(fa, om, gm, helpers.changed_edge_shapes(name))
    assert len(gf.clusters(1)) == n
    cand = helpers.changed_candidates(of, om, *_box(om))
    pos, owners = _where(cand, total)
    _upload(om, gm, helpers.occupy(om, _cells_at(cand, pos)))
    st0 = gf.changedStats()
    _search(om, gm, of, gf)
    _expect(gf, st0, path, n, total)
    assert list(gf.removedIds()) == [k - r for r, k in enumerate(owners)]
    _equal(of, gf, name + " host-copied")
    gf.close()


@pytest.mark.parametrize("name", ["bar_2049", "staged_131073", "table_nc1025"])
def test_active_and_dormant_candidates(fa, maps, name):
    """The first x slot committed active, the rest dormant: removedIds count positions in the active list as it
    shrinks, dormant clusters are dropped silently"""
    om, gm = maps
    n, total, path = helpers.CHG_EDGES[name]
    shapes = helpers.changed_edge_shapes(name)
    _upload(om, gm, helpers.capacity_occupancy(om, helpers.changed_blocks(om, shapes)))
    gf = fa.FrontierFinder(gm, cluster_min=CM)
    of = fo.OracleFrontier(om, CM)
    lo, hi = _box(om)
    first = (lo, (lo[0] + 0.05, hi[1], hi[2]))  # scanned up to x index blo + 10: the first x slot
    n1 = _search(om, gm, of, gf, first)
    assert 0 < n1 < n
    of.commit()
    gf.commit()
    assert _search(om, gm, of, gf) == n - n1
    of.commit(dormant=True)
    gf.commit(dormant=True)
    cand = helpers.changed_candidates(of, om, lo, hi)
    assert len(cand) == n and [w for w, _, _ in cand] == [1] * n1 + [2] * (n - n1)
    pos, owners = _where(cand, total)
    more = (n1 - 2, n1)  # the last cells of an active cluster and of the first dormant one
    pos += [int(np.cumsum([len(c) for _, _, c in cand])[k]) - 1 for k in more]
    owners = sorted(set(owners) | set(more))
    _upload(om, gm, helpers.occupy(om, _cells_at(cand, pos)))
    st0 = gf.changedStats()
    _search(om, gm, of, gf)
    _expect(gf, st0, path, n, total)
    assert list(gf.removedIds()) == [k - r for r, k in enumerate(o for o in owners if o < n1)]
    _equal(of, gf, name + " active + dormant")
    gf.close()


def test_mark_grows_across_a_table_growth(fa, maps):
    """A barrier-path test, then a candidate table that grows (more than 1.5 nc + 64 candidates), then another
    barrier-path test: the second must not reuse a mark -- k_rm_pool_bar's release words still hold the first one's"""
    om, gm = maps
    shapes = helpers.changed_shapes(600, 72 + 150 * 586 + 200)
    _upload(om, gm, helpers.capacity_occupancy(om, helpers.changed_blocks(om, shapes)))
    gf = fa.FrontierFinder(gm, cluster_min=CM)
    of = fo.OracleFrontier(om, CM)
    lo, hi = _box(om)
    n1 = _search(om, gm, of, gf, (lo, (hi[0], lo[1], hi[2])))  # y lines up to blo + 10: the first y slot
    of.commit()
    gf.commit()
    cand = helpers.changed_candidates(of, om, lo, hi)
    assert len(cand) == n1 and helpers.rm_path(n1, sum(len(c) for _, _, c in cand)) == "bar"
    marks = []
    st0 = gf.changedStats()
    assert _search(om, gm, of, gf) == 600 - n1
    st = _expect(gf, st0, "bar", n1, sum(len(c) for _, _, c in cand))
    marks.append(st["mark"])
    _equal(of, gf, "first barrier test", lists=False)
    of.commit()
    gf.commit()
    cand = helpers.changed_candidates(of, om, lo, hi)
    total = sum(len(c) for _, _, c in cand)
    assert len(cand) == 600 > 1.5 * n1 + 64 and helpers.rm_path(600, total) == "bar"
    pos, owners = _where(cand, total, head=False)  # (the first search's clusters lead the table)
    _upload(om, gm, helpers.occupy(om, _cells_at(cand, pos)))
    _search(om, gm, of, gf)
    st = _expect(gf, st, "bar", 600, total)
    assert st["mark"] > max(marks), "a mark was reused after the candidate table grew: %s" % (marks + [st["mark"]])
    assert list(gf.removedIds()) == [k - r for r, k in enumerate(owners)]
    _equal(of, gf, "barrier test after the growth")
    gf.close()


def _cycle(om, gm, of, gf, occ, tag):
    _upload(om, gm, occ)
    _search(om, gm, of, gf)
    _equal(of, gf, tag, lists=False)
    of.commit()
    gf.commit()


def test_pool_compaction(fa, maps):
    """One 350 760-cell shell committed, changed and grown again until the pool (1 << 20 cells) is full of holes: the
    third commit compacts it (no growth), and a changed-cluster test reads the rebuilt pool"""
    om, gm = maps
    blocks = [((11, 11, 16), (381, 381, 68))]
    occ = helpers.capacity_occupancy(om, blocks)
    gf = fa.FrontierFinder(gm, cluster_min=CM)
    of = fo.OracleFrontier(om, CM)
    _cycle(om, gm, of, gf, occ, "huge shell")
    assert gf.changedStats()["pool_cap"] == 1 << 20
    for r in range(3):
        cells = np.sort(of.clusters(1)[0])
        occ = occ.copy()
        occ[cells[[0, len(cells) // 2, -1][r]]] = om.l_max
        st0 = gf.changedStats()
        _cycle(om, gm, of, gf, occ, "cycle %d" % r)
        st = _expect(gf, st0, "staged", 1, len(cells))
        assert st["rebuilds"] == (0 if r < 1 else 1) and st["pool_cap"] == 1 << 20, (r, st)
    _equal(of, gf, "after the compaction")
    gf.close()


def _with_blocks(om, occ, blocks):
    o = occ.copy()
    for lo, hi in blocks:
        o.reshape(om.nvox)[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = om.l_min - 0.01
    return o


def test_pool_growth(fa, maps):
    """Two shells and a slab over the top face, 527 k live cells: the commit that overflows the pool rebuilds it at
    twice the size (live > cap / 2), and a changed-cluster test -- the slab's seed changed -- reads the grown pool"""
    om, gm = maps
    _, bhi = om.box_index()
    a, b = ((11, 11, 15), (381, 190, 70)), ((11, 200, 15), (381, 381, 70))
    slab = ((11, 11, bhi[2]), (381, 389, bhi[2] + 5))
    gf = fa.FrontierFinder(gm, cluster_min=CM)
    of = fo.OracleFrontier(om, CM)
    _cycle(om, gm, of, gf, helpers.capacity_occupancy(om, [a]), "A")

    def changed(occ, which, k=0, at=0):
        occ = occ.copy()
        occ[np.sort(of.clusters(which)[k])[at]] = om.l_max
        return occ

    occ = changed(helpers.capacity_occupancy(om, [a, b]), 1)
    _cycle(om, gm, of, gf, occ, "A changed, B")
    occ = changed(_with_blocks(om, occ, [slab]), 1, 0, 5)
    _cycle(om, gm, of, gf, occ, "A changed, slab")
    assert gf.changedStats()["rebuilds"] == 0
    k_b = int(np.argmax([len(c) for c in of.clusters(1)]))
    live = sum(len(c) for c in of.clusters(1))
    assert live > (1 << 20) // 2
    _cycle(om, gm, of, gf, changed(occ, 1, k_b, 7), "B changed: the pool grows")
    st = gf.changedStats()
    assert st["rebuilds"] == 1 and st["pool_cap"] == 1 << 21, st
    seed_k = next(k for k, c in enumerate(of.clusters(1)) if np.unravel_index(c[0], om.nvox)[2] == bhi[2])
    cand = helpers.changed_candidates(of, om, *_box(om), device_order=False)
    assert len(cand) == 3
    _upload(om, gm, helpers.occupy(om, [of.clusters(1)[seed_k][0]]))
    _search(om, gm, of, gf)
    _expect(gf, st, "staged", 3, sum(len(c) for _, _, c in cand))
    assert list(gf.removedIds()) == [seed_k]
    _equal(of, gf, "slab seed changed in the grown pool")
    gf.close()


@pytest.mark.parametrize("name,k", [("table_nc1025", -1), ("staged_131073", 400)])
def test_is_frontier_covered_threshold(fa, maps, name, k):
    """isFrontierCovered (k_vp_changed over the same pool and offsets): a cluster with exactly
    int(min_view_finish_fraction * n) changed cells covers, one fewer does not"""
    om, gm = maps
    of, gf = _committed(fa, om, gm, helpers.changed_edge_shapes(name))
    of.set_viewpoint_cfg(fo.viewpoint_cfg())
    gf.setViewpointConfig(gf.viewpointConfig())
    cand = helpers.changed_candidates(of, om, *_box(om))
    cells = cand[k][2]
    thresh = int(0.2 * len(cells))
    assert thresh >= 2
    pick = np.concatenate([cells[:thresh // 2], cells[len(cells) - (thresh - thresh // 2):]])  # first and last pooled
    base = om.occ.copy()
    for m, want in ((thresh, True), (thresh - 1, False)):
        om.occ[:] = base
        _upload(om, gm, helpers.occupy(om, pick[:m]))
        om.set_updated_box(*_box(om))
        gm.setUpdatedBox(*_box(om))
        assert of.is_covered() == want
        assert gf.isFrontierCovered() == want, (name, m)
    gf.close()
