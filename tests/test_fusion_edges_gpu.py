"""Depth fusion on the device at the edges of its kernels (k_insert_classify / k_insert_raycast / k_insert_update): the
scenarios of tests/fusion_edges.py, fused frame by frame into an fa.SDFMap and an OracleMap of the same keywords and
compared bit for bit -- occupancy log-odds, local bound, updated box -- at every compare frame.  The oracle is pinned to
the real reference on the same scenarios in test_fusion_edges_cpu.py, which also proves that each scenario reaches its
edge (char counter wrap, lane hand-over at j / 4, every branch of the cube placement, counts around the wave and the
workgroup, an origin off the voxel grid, frames that drop every point).  Everything fed in is ordinary valid input."""
import ctypes

import numpy as np
import pytest

import fusion_edges as fe
from oracle import fuel_oracle as fo
from test_gpu_parity import assert_map_equal, sorted_clusters

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fa():
    import fuel_amd
    assert fuel_amd.lib().fuelmi_device_count() > 0, "no GPU visible: the HIP path cannot run"
    return fuel_amd


def twin(fa, sc):
    box = fe.exploration_box(sc)
    return fo.OracleMap(sc["map_size"], *box, **sc["map_kw"]), fa.SDFMap(sc["map_size"], *box, **sc["map_kw"])


def feed(gm, pts, cam, raw):
    """inputPointCloud, or the raw entry point with pcl::PointXYZ's 16-byte records"""
    if not raw:
        gm.inputPointCloud(pts, cam)
        return
    from fuel_amd._lib import check
    rec = np.zeros((len(pts), 4), dtype=np.float32)
    rec[:, :3] = pts
    rec[:, 3] = 1.0
    check(gm.L.fuelmi_map_input_points(gm.h, rec.ctypes.data, 16, len(rec), (ctypes.c_double * 3)(*cam)))


def assert_fusion_equal(om, gm, what):
    occ = gm.syncHost(occupancy=True)["occupancy"]
    diff = np.flatnonzero(occ != om.occ)
    assert np.array_equal(occ, om.occ), "%s: %d voxels differ, first at index %s (device %r, oracle %r)" % (
        what, len(diff), np.unravel_index(diff[0], om.nvox), occ[diff[0]], om.occ[diff[0]])
    assert gm.getLocalBound() == om.get_local_bound(), what
    assert np.array_equal(np.concatenate(gm.getUpdatedBox()), np.concatenate(om.get_updated_box())), what
    return om.N


def near_depth_frame(gm, cam):
    """an inputDepthImage whose pixels are all nearer than depth_filter_mindist: nothing is projected, the call
    returns 0 and must leave the map and the frame counter alone"""
    img = np.full((24, 32), 100, dtype=np.uint16)  # 0.1 m < 0.2 m
    assert gm.inputDepthImage(img, cam, (1.0, 0.0, 0.0, 0.0)) == 0


def state_planes_equal(fa, om, gm, name):
    """what syncHost does not show: the occupied / unknown bit planes k_insert_update rewrites, through their readers"""
    om.inflate_local()
    om.update_esdf()
    gm.clearAndInflateLocalMap()
    gm.updateESDF3d()
    assert_map_equal(om, gm, om.get_local_bound())
    of = fo.OracleFrontier(om, 10)
    gf = fa.FrontierFinder(gm, cluster_min=10)
    n_o, n_g = of.search(), gf.searchFrontiers()
    assert n_o == n_g, name
    ours = gf.clusters(0)
    assert len(ours) == n_o, name
    for a, b in zip(sorted_clusters(of.clusters(0)), ours):
        assert np.array_equal(a, b), name
    assert np.array_equal(of.flags, gf.flags()), name
    return n_o


def run_scenario(fa, name, sc, depth_noop_after=()):
    om, gm = twin(fa, sc)
    try:
        compared = 0
        for k, (pts, cam) in enumerate(sc["frames"]):
            om.input_points(pts, cam)
            feed(gm, pts, cam, raw=k % 2 == 1)
            if k in depth_noop_after:
                near_depth_frame(gm, cam)
            if k in sc["compare"]:
                compared += assert_fusion_equal(om, gm, "%s, after frame %d of %d (%d points)" % (
                    name, k + 1, len(sc["frames"]), len(pts)))
        clusters = None
        base = name.split("+")[0]
        if base in fe.STATE_PLANES:
            clusters = state_planes_equal(fa, om, gm, name)
            # (the 4 x 4 x 2 m map of the directed counter scenario holds no cluster of 10 cells)
            assert clusters > 0 or base == "A_counter_directed", "%s: the frontier search found nothing to compare" % name
        print("%s: %d frames, %d voxels compared%s" % (name, len(sc["frames"]), compared,
                                                        "" if clusters is None else ", %d frontier clusters" % clusters))
    finally:
        gm.close()


@pytest.mark.parametrize("name", list(fe.SCENARIOS))
def test_fusion_scenario(fa, name):
    run_scenario(fa, name, fe.SCENARIOS[name]())


@pytest.mark.parametrize("name", ["A_counter_directed", "A_counter_random"])
def test_counter_with_empty_depth_frames_between_the_wrap_frames(fa, name):
    """between frames 254 / 255 and 255 / 256 a depth image with nothing to project: the counter was advanced for it
    and must be rolled back, or frame 255 is no longer the one that equals the initial flag"""
    run_scenario(fa, name + "+depth", fe.SCENARIOS[name](), depth_noop_after=(253, 254))


@pytest.mark.parametrize("raw_first", [False, True])
def test_nan_records_add_nothing(fa, raw_first):
    """NaN records in slot 0, in the last slot, at the wave and workgroup edges and between equal neighbours: the frame
    gives exactly the map the frame without those records gives.  Both clouds go through both entry points (the raw
    16-byte records are what a device projection leaves in dropped slots)."""
    sc = fe.scenario(fe.D_MAP, [])
    om, gm = twin(fa, sc)
    try:
        for k, (dirty, clean, cam) in enumerate(fe.nan_frames()):
            om.input_points(clean, cam)
            feed(gm, dirty, cam, raw=(k % 2 == 0) == raw_first)
            assert_fusion_equal(om, gm, "NaN frame %d" % k)
    finally:
        gm.close()
