"""fuelmi_map_path_costs at its limits against the restatement (tests/path_cost_ref.py): paths of 63 .. 8193 lattice
edges on a serpentine (k_path_goal's checkpoint segments of PC_SEG = 64 and their joins, and the per-point walk past
PC_NCK * PC_SEG = 8192 edges), a winding relaxation of many hundreds of launches, and sources spread over more than one
chunk of CHUNK_NODE_BUDGET lattice nodes."""
import time

import numpy as np
import pytest

import path_cost_ref as pr

pytestmark = pytest.mark.gpu
HOPS = (63, 64, 65, 128, 129, 8192, 8193)


def _device_twin(om, size, box):
    """the device map of an oracle map's occupancy; its inflated / unknown voxels must be the oracle's"""
    import fuel_amd
    gm = fuel_amd.SDFMap(size, box[0], box[1], device=0)
    gm.uploadOccupancy(np.array(om.occ, dtype=np.float64))
    nv = gm.nvox
    gm.setLocalBound((0, 0, 0), (nv[0] - 1, nv[1] - 1, nv[2] - 1))
    gm.clearAndInflateLocalMap()
    pm = pr.PathMap.from_device(gm)
    assert np.array_equal(pm.bad, pr.PathMap.from_oracle(om).bad)
    return gm


@pytest.fixture(scope="module")
def serpentine():
    om, pm = pr.serpentine_map()
    goals, lat = pr.goals_at_hops(pm, om, pr.SERP_P1, HOPS, pr.SERP_RES)
    gm = _device_twin(om, pr.SERP_SIZE, pr.SERP_BOX)
    yield gm, om, pm, goals, lat
    gm.close()


def test_long_paths_bit_for_bit(serpentine):
    gm, om, pm, goals, lat = serpentine
    p1 = np.repeat([pr.SERP_P1], len(HOPS), axis=0)
    p2 = np.array([goals[H] for H in HOPS])
    t0 = time.perf_counter()
    length, kind, paths = gm.path_costs(p1, p2, res=pr.SERP_RES, max_points=max(HOPS) + 2)
    dt = time.perf_counter() - t0
    st = gm.path_stats()
    print("serpentine: %d relaxation launches, %.2f s with paths" % (st["launches"], dt))
    assert st["sources"] == 1 and st["chunks"] == 1
    assert st["launches"] > 500  # a winding front: many more launches than POLL_EVERY
    for k, H in enumerate(HOPS):
        rk, rl, rp = pr.search_path(pm, om, p1[k], p2[k], res=pr.SERP_RES, lattice=lat)
        assert rk == 1 and len(rp) == H + 2
        assert kind[k] == 1 and len(paths[k]) == H + 2, (H, kind[k], len(paths[k]))
        assert length[k] == rl, (H, length[k], rl)
        assert np.array_equal(paths[k], rp), H
    # lengths only: the same bits
    l0, k0, p0 = gm.path_costs(p1, p2, res=pr.SERP_RES, max_points=0)
    assert p0 is None and np.array_equal(k0, kind) and l0.tobytes() == length.tobytes()


def test_several_chunks():
    om, pm = pr.chunk_map()
    p1, p2, chunk = pr.chunk_case(pm, om)
    assert max(chunk) >= 1
    gm = _device_twin(om, pr.CHUNK_SIZE, pr.CHUNK_BOX)
    length, kind, paths = gm.path_costs(p1, p2, res=pr.CHUNK_RES, max_points=1024)
    st = gm.path_stats()
    assert st["sources"] == len(p1) and st["chunks"] == max(chunk) + 1, st
    assert (kind == 1).all(), np.bincount(kind)
    last1 = max(i for i in range(len(p1)) if chunk[i] == 0)
    for i in (last1, last1 + 1, len(p1) - 1):
        lat = pr.Lattice(pm, p1[i], pr.CHUNK_RES)
        lat.d = lat.csgraph_dist()
        rk, rl, rp = pr.search_path(pm, om, p1[i], p2[i], res=pr.CHUNK_RES, lattice=lat)
        assert kind[i] == rk and length[i] == rl and np.array_equal(paths[i], rp), i
    for i in range(len(p1)):
        l1, k1, q1 = gm.path_costs(p1[i:i + 1], p2[i:i + 1], res=pr.CHUNK_RES, max_points=1024)
        assert k1[0] == kind[i] and l1[0].tobytes() == length[i].tobytes() and np.array_equal(q1[0], paths[i]), i
    gm.close()
