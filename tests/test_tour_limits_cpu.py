"""The fixtures of the tour-stack limit tests (tests/test_tsp_limits_gpu.py, test_refine_limits_gpu.py,
test_path_cost_limits_gpu.py) reach the branches they are there for; restatements only, no device."""
import numpy as np
import pytest

import path_cost_ref as pr
import tsp_ref as tr
from test_path_cost_limits_gpu import HOPS
from test_refine_limits_gpu import TIES, _deep, _wide
from test_tsp_limits_gpu import LARGE, extreme, heuristic_matrix

TSP_ILS_THREADS, TSP_TABLE_CHUNK = 512, 64 << 20  # tsp.hip
PC_SEG, PC_NCK = 64, 128                           # path_cost.hip


# ---- ATSP -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", LARGE + (600,))
def test_planted_instances_need_every_move_type(d):
    c = heuristic_matrix(d) if d in LARGE else tr.planted_matrix(600, 600)[0]
    counts = {}
    order, cost = tr.local_search(c, tr.nearest_neighbour(c), counts)
    assert counts.get("2opt", 0) >= 1 and counts.get("or_fwd", 0) >= 1 and counts.get("or_rev", 0) >= 1, counts
    assert sum(counts.values()) >= 10, counts
    assert cost < tr.tour_cost(c, tr.nearest_neighbour(c))
    if d == 600:  # the extreme-entry copy makes the same moves
        counts2 = {}
        order2, _ = tr.local_search(extreme(c, 600), tr.nearest_neighbour(extreme(c, 600)), counts2)
        assert counts2 == counts and order2 == order


def test_tsp_sizes_reach_their_branches():
    chunk = lambda d: (d + TSP_ILS_THREADS - 1) // TSP_ILS_THREADS  # noqa: E731  ils_prefix's positions per lane
    assert [chunk(d) for d in LARGE] == [1, 1, 2, 2, 2, 2]
    assert 7 * 1024 * 1024 < 1 << 23  # ils_descend's move index stays exact in float before the row split
    # Held-Karp tables: eight d = 17 tables fill a chunk exactly, a ninth opens the next
    hk = lambda d: (1 << (d - 1)) * (d - 1) * 8  # noqa: E731
    assert 8 * hk(17) == TSP_TABLE_CHUNK
    # d = 5: four positions 1..4 for the double bridge's three distinct points
    for r in range(2):
        for k in range(2):
            pts = tr.kick_points(0, r, k, 5)
            assert len(set(pts)) == 3 and 1 <= min(pts) and max(pts) <= 4


# ---- refinement -----------------------------------------------------------------------------------------------------------
def test_refine_fixtures_reach_their_branches():
    assert [len(l) for l in _wide(1)[3]] == [256] * 4
    deep = [len(l) for l in _deep(2)[3]]
    assert len(deep) == 64 and min(deep) >= 3 and max(deep) <= 8
    mus = [mu for mu, _ in TIES]
    assert {mu // 64 for mu in mus} == {0, 1, 2, 3}   # every predecessor stride of a lane
    assert {mu % 64 for mu in mus} >= {0, 63}         # the first and the last lane
    assert {mv % 4 for _, mv in TIES} == {0, 1, 2, 3}  # every wave holds a winner
    assert max(mus) == 255                            # the largest byte parent


# ---- path costs ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def serpentine():
    om, pm = pr.serpentine_map()
    goals, lat = pr.goals_at_hops(pm, om, pr.SERP_P1, HOPS, pr.SERP_RES)
    return om, pm, goals, lat


def test_serpentine_goals_have_their_hop_counts(serpentine):
    om, pm, goals, lat = serpentine
    assert lat.E[2] == 1  # one lattice layer
    for H in HOPS:
        kind, length, path = pr.search_path(pm, om, pr.SERP_P1, goals[H], res=pr.SERP_RES, lattice=lat)
        assert kind == 1 and len(path) == H + 2, (H, kind, len(path))
    segs = {H: (H + PC_SEG - 1) // PC_SEG for H in HOPS}
    assert segs[63] == 1 and segs[64] == 1 and segs[65] == 2 and segs[128] == 2 and segs[129] == 3
    assert segs[8192] == PC_NCK and segs[8193] == PC_NCK + 1  # the last checkpointed path and the per-point walk
    # the front winds: the farthest node is far more lattice edges away than the lattice is wide
    assert np.isfinite(lat.d).sum() > 0.2 * lat.d.size and np.nanmax(np.where(np.isfinite(lat.d), lat.d, np.nan)) > 500


def test_chunk_case_spans_two_chunks():
    om, pm = pr.chunk_map()
    p1, p2, chunk = pr.chunk_case(pm, om)
    assert len({tuple(p) for p in p1}) == len(p1)
    assert max(chunk) >= 1 and chunk == sorted(chunk)
    nodes = [pr.lattice_nodes(pm, a, pr.CHUNK_RES) for a in p1]
    assert 0.6e6 < min(nodes) and max(nodes) < 1.2e6
    assert sum(nodes) > pr.CHUNK_NODE_BUDGET
