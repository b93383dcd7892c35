"""The fixture of test_frontier_changed_gpu (helpers.changed_*) against the oracle, without a GPU: every planned
layout keeps one cluster per block, in the order of its list, with the shell sizes it was planned with, and its
committed clusters form a candidate table whose candidate count nc and pooled cell count total hit the edges of
remove_changed_begin's four paths (frontier_changed.hip) exactly."""
import numpy as np
import pytest

import helpers
from oracle import fuel_oracle as fo

@pytest.fixture(scope="module")
def om():
    return helpers.capacity_map()


def _committed(om, shapes):
    om.occ[:] = helpers.capacity_occupancy(om, helpers.changed_blocks(om, shapes))
    box = (tuple(om.cfg.box_min), tuple(om.cfg.box_max))
    om.set_updated_box(*box)
    of = fo.OracleFrontier(om, helpers.CHG_CLUSTER_MIN)
    n = of.search()
    of.commit()
    return n, of, box


def test_rm_path_edges():
    """the path follows from nc and total exactly as remove_changed_begin decides it"""
    assert [helpers.rm_path(1, t) for t in (2048, 2049, 131072, 131073)] == ["one", "bar", "bar", "staged"]
    assert [helpers.rm_path(n, 100) for n in (1024, 1025)] == ["one", "table"]
    assert [helpers.rm_path(n, 6000) for n in (1024, 1025)] == ["bar", "table"]
    assert [helpers.rm_path(n, 140000) for n in (1024, 1025)] == ["staged", "table"]


@pytest.mark.parametrize("name", list(helpers.CHG_EDGES))
def test_layout_hits_the_planned_edge(om, name):
    n, total, path = helpers.CHG_EDGES[name]
    shapes = helpers.changed_edge_shapes(name)
    assert len(shapes) == n and sum(map(helpers.shell_size, shapes)) == total
    k, of, box = _committed(om, shapes)
    assert k == n
    assert [len(c) for c in of.clusters(1)] == [helpers.shell_size(s) for s in shapes], "clusters out of list order"
    cand = helpers.changed_candidates(of, om, *box)
    assert len(cand) == n and sum(len(c) for _, _, c in cand) == total
    assert helpers.rm_path(len(cand), total) == path
    # the last candidate is seed-claimed: its NQ seed sits at pooled position total - 1, outside the box
    blo, bhi = om.box_index()
    seed = np.unravel_index(cand[-1][2][-1], om.nvox)
    assert seed[2] == bhi[2] and cand[-1][2][-1] == of.clusters(1)[-1][0]
    # the wave head: single voxels, several clusters in the first 64 pooled cells
    assert all(len(c) == 6 for _, _, c in cand[:helpers.WAVE_HEAD])


def test_overlap_slack_decides_the_candidates(om):
    """haveOverlap with 1e-3 slack: a box that ends within 1e-3 of a cluster's box still makes it a candidate"""
    shapes = helpers.changed_shapes(24, 2048)
    _, of, _ = _committed(om, shapes)
    _, bmin, bmax = of.cluster_info(1, 0)
    lo = np.asarray(bmax) + np.array([0.0009, 0.0, 0.0])
    assert len(helpers.changed_candidates(of, om, tuple(lo), tuple(lo + 0.05))) >= 1
    lo = np.asarray(bmax) + np.array([0.0011, 0.0, 0.0])
    assert all(k != 0 for _, k, _ in helpers.changed_candidates(of, om, tuple(lo), tuple(lo + 0.05)))


def test_an_occupied_shell_cell_changes_its_cluster_only(om):
    """one shell cell made occupied: the oracle drops exactly that cluster and grows the rest of its shell again"""
    shapes = helpers.changed_shapes(24, 2049)
    _, of, box = _committed(om, shapes)
    cand = helpers.changed_candidates(of, om, *box)
    om.occ[:] = helpers.occupy(om, [cand[14][2][7]])
    om.set_updated_box(*box)
    assert of.search() == 1 and list(of.removed_ids()) == [14]
    assert len(of.clusters(0)[0]) == len(cand[14][2]) - 1
