"""The fixture of test_frontier_capacity_gpu (helpers.capacity_layout) against the oracle, without a GPU: that it keeps
exactly the planned number of clusters, that its blocks straddle the tile boundaries they were drawn across, and that
its shells have the sizes the cluster_min edge tests rely on (frontier_finder.cpp:54-164)."""
import numpy as np
import pytest

import helpers
from oracle import fuel_oracle as fo


@pytest.fixture(scope="module")
def om():
    return helpers.capacity_map()


def _search(om, blocks, cluster_min):
    om.occ[:] = helpers.capacity_occupancy(om, blocks)
    om.set_updated_box(tuple(om.cfg.box_min), tuple(om.cfg.box_max))
    of = fo.OracleFrontier(om, cluster_min)
    return of.search(), of


def test_full_box_search_runs_on_8_x_32_tiles(om):
    """The geometry the GPU sweep's in-launch edge (42 / 43 clusters) is computed for: tile origin at the exploration
    box's low corner, the menu's 8 x 32 tile (16 x 32 leaves 288 < 512 tiles), 48 tile columns."""
    blo, _ = om.box_index()
    assert helpers.capacity_tiles(om) == (blo[0], blo[1], 8, 32, 48)


@pytest.mark.parametrize("n", helpers.CAP_SWEEP)
def test_fixture_keeps_exactly_n_clusters(om, n):
    blocks, plan = helpers.capacity_layout(om, n)
    assert len(blocks) == n
    got = {"x": 0, "y": 0, "corner": 0, "none": 0}
    for lo, hi in blocks:
        got[helpers.block_straddle(om, lo, hi)] += 1
    assert got == plan, "the blocks drifted off the tile boundaries they were placed across"
    assert 4 * (n - plan["none"]) >= n and plan["corner"] >= 1
    k, of = _search(om, blocks, 100)
    assert k == n
    sizes = sorted({len(c) for c in of.clusters(0)})
    assert sizes == [helpers.SLAB_SHELL, 125, helpers.CUBE_SHELL], sizes  # (box-face cubes lose the face outside)


@pytest.mark.parametrize("slabs", [False, True], ids=["cubes", "slabs"])
def test_fixture_shell_size_is_the_keep_edge(om, slabs):
    """Every cluster of the one-size layouts has S cells as the oracle counts them (a slab's: its underside plus the
    NQ seed that claims it): kept at cluster_min = S - 1, dropped at S (size > cluster_min)."""
    n = 8 if slabs else 16
    S = helpers.SLAB_SHELL if slabs else helpers.CUBE_SHELL
    blocks, _ = helpers.capacity_layout(om, n, faces=False, slabs=slabs)
    k, of = _search(om, blocks, S - 1)
    assert k == n and all(len(c) == S for c in of.clusters(0))
    assert _search(om, blocks, S)[0] == 0


def test_fixture_layouts_grow_by_appending(om):
    """capacity_layout(n + k) starts with capacity_layout(n): the streaming and recovery tests add blocks that way."""
    a, _ = helpers.capacity_layout(om, 64)
    b, _ = helpers.capacity_layout(om, 302)
    assert b[:64] == a
    assert len({lo for lo, _ in b}) == len(b)
