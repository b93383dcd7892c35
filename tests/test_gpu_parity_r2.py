"""Round-2 parity cases through the C-ABI against the oracle: the virtual ceiling of clearAndInflateLocalMap,
fusion from a camera outside the map (wrapped miss addresses), the optimistic ESDF at BASELINE's full
400x400x100 size and on a sparse map (long outward scans)."""
import numpy as np
import pytest

import helpers
from oracle import fuel_oracle as fo

pytestmark = pytest.mark.gpu

ESDF_TOL = 1e-4
BIG = 1e6


@pytest.fixture(scope="module")
def fa():
    import fuel_amd
    assert fuel_amd.lib().fuelmi_device_count() > 0, "no GPU visible: the HIP path cannot run"
    return fuel_amd


def assert_map_equal(om, gm, box_idx=None, esdf=True):
    h = gm.syncHost(occupancy=True, inflate=True, distance=esdf)
    assert np.array_equal(h["occupancy"], om.occ), "occupancy log-odds not bit-exact"
    assert np.array_equal(h["inflate"], om.infl), "inflated occupancy not bit-exact"
    if esdf:
        d_o = np.clip(om.dist, -BIG, BIG).reshape(om.nvox)
        d_g = np.clip(h["distance"], -BIG, BIG).reshape(om.nvox)
        if box_idx is not None:
            sl = tuple(slice(box_idx[0][i], box_idx[1][i] + 1) for i in range(3))
            d_o, d_g = d_o[sl], d_g[sl]
        assert np.abs(d_o - d_g).max() <= ESDF_TOL
    return h


@pytest.mark.parametrize("ceil_h", [1.5, 1.55, 2.95])
def test_virtual_ceiling(fa, ceil_h):
    """sdf_map.cpp:464-471 (3.2 m in kino_algorithm.xml:75 / topo_algorithm.xml:70): the ceiling row is written
    over the x,y extent of the local bound after the stamps; the next call inflates it; fusion keeps touching it;
    the frontier scan sees it as occupied.  Pinned against the real sdf_map.cpp on the CPU
    (test_oracle_vs_reference_cpu.py::test_virtual_ceiling_matches_reference)."""
    map_size = (10.0, 8.0, 4.0)
    box = ((-4.0, -3.0, 0.0), (4.0, 3.0, 2.2))
    om = fo.OracleMap(map_size, *box, virtual_ceil_height=ceil_h)
    gm = fa.SDFMap(map_size, *box, virtual_ceil_height=ceil_h)
    truth = om.fixture_world(3, 14)
    of = fo.OracleFrontier(om, 10)
    gf = fa.FrontierFinder(gm, cluster_min=10)
    for k in range(12):
        pose = om.fixture_camera(truth, 5, k, 12, 0.9)
        pts = om.fixture_render(truth, pose, 160, 120, 2, 2)
        om.input_points(pts, pose[:3])
        gm.inputPointCloud(pts, pose[:3])
        om.inflate_local()
        gm.clearAndInflateLocalMap()
        if k % 3 == 2:
            om.update_esdf()
            gm.updateESDF3d()
            assert_map_equal(om, gm, om.get_local_bound())
            assert of.search() == gf.searchFrontiers()
            for a, b in zip(of.clusters(0), gf.clusters(0)):
                assert np.array_equal(np.sort(a), b)
            assert np.array_equal(of.flags, gf.flags())
            of.commit()
            gf.commit()
    ceil_id = int(np.floor((ceil_h - om.origin[2]) * (1.0 / om.res)))
    assert (om.occ.reshape(om.nvox)[:, :, ceil_id] == om.l_max).sum() > 500
    # local bounds whose z range ends at the ceiling row, below it, above it: the row is written all the same
    occ = om.occ.copy()
    for zhi in (ceil_id, ceil_id - 3, om.nvox[2] - 1):
        occ.reshape(om.nvox)[20:40, 10:30, ceil_id] = om.l_min
        om.occ[:] = occ
        gm.uploadOccupancy(occ)
        lo, hi = (15, 5, 2), (45, 35, zhi)
        om.set_local_bound(lo, hi)
        gm.setLocalBound(lo, hi)
        om.inflate_local()
        gm.clearAndInflateLocalMap()
        om.update_esdf()
        gm.updateESDF3d()
        assert_map_equal(om, gm, (lo, hi))
        occ = om.occ.copy()
        # the occupancy STATE planes follow the ceiling too (the frontier scan and the queries read them)
        idx = np.stack(np.meshgrid(np.arange(18, 42), np.arange(8, 32), [ceil_id - 1, ceil_id, ceil_id + 1],
                                   indexing="ij"), -1).reshape(-1, 3)
        st_o = np.array([om.L.fo_map_get_occupancy_idx(om.h, (fo.C.c_int * 3)(*map(int, i))) for i in idx])
        assert np.array_equal(st_o, gm.getOccupancy(idx)[0])
    gm.close()


def test_ceiling_above_or_below_the_map_is_ignored(fa):
    """a ceiling row outside [0, nz) would index another z-line in the reference (undefined behaviour when it
    leaves the array); the device leaves the map untouched"""
    for h, ground in ((7.0, -1.0), (-0.3, 0.0)):  # ceil_id = 80 >= nz, ceil_id = -3
        gm = fa.SDFMap((4.0, 3.0, 2.0), virtual_ceil_height=h, ground_height=ground)
        before = gm.syncHost(occupancy=True)["occupancy"].copy()
        gm.setLocalBound((0, 0, 0), (39, 29, 19))
        gm.clearAndInflateLocalMap()
        assert np.array_equal(gm.syncHost(occupancy=True)["occupancy"], before)
        gm.close()


def outside_camera_frames(origin, map_size, n_rounds=3, seed=4):
    """camera beyond the +z / +y faces of the map, end points inside it and within max_ray_length: every ray
    cell has a linear address in [0, N) (cells past a +y / +z face alias voxels of the next row / slab), which is
    the part of this situation the reference defines -- setCacheOccupancy (sdf_map.cpp:243-257) has NO bounds
    test, a cell past a -x/+x face or behind the last row is undefined behaviour there."""
    rng = np.random.default_rng(seed)
    cams = [(0.3, 0.2, 2.3), (0.0, 2.8, 0.5), (0.5, 0.5, 1.0), (-1.2, 2.7, 2.2)]
    lo = origin + 0.15
    hi = origin + np.array(map_size) - 0.15
    lo[0] += 1.0
    hi[0] -= 1.0
    for cam in cams * n_rounds:
        cam = np.array(cam) + rng.normal(scale=0.03, size=3)
        d = rng.normal(size=(900, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        pts = cam + d * rng.uniform(0.5, 4.3, size=(900, 1))
        yield pts[np.all((pts > lo) & (pts < hi), axis=1)].astype(np.float32), cam


def test_fusion_with_the_camera_outside_the_map(fa):
    """inputPointCloud has no isInMap(camera) test (cloudPoseCallback feeds it directly): rays start at in-map end
    points and walk towards a camera above / beside the map, marking misses at ALIASED addresses outside the
    index box of camera and end points.  They must be applied in the same frame (they used to fall
    outside the update window and surface frames later).  Pinned against the real sdf_map.cpp on the CPU
    (test_oracle_vs_reference_cpu.py::test_fusion_from_outside_the_map_matches_reference)."""
    map_size = (6.0, 5.0, 3.0)
    om = fo.OracleMap(map_size)
    gm = fa.SDFMap(map_size)
    for k, (pts, cam) in enumerate(outside_camera_frames(om.origin, map_size)):
        om.input_points(pts, cam)
        gm.inputPointCloud(pts, cam)
        assert om.get_local_bound() == gm.getLocalBound(), k
        h = gm.syncHost(occupancy=True)
        assert np.array_equal(h["occupancy"], om.occ), "frame %d (camera %s)" % (k, cam)
    gm.close()


@pytest.fixture(params=["plain", "far", "plain32"])
def esdf_kernels(request, fa, monkeypatch):
    """every ESDF kernel family (esdf.hip: the packed 16-bit plain z/y pass, the far-field kernels, the 32-bit plain
    pass; esdf_use_far picks per update from the statistic of the place, fuelmi_map_set_esdf_family pins one): they
    must give the same bits"""
    fam = {"plain": fa.SDFMap.ESDF_PLAIN, "far": fa.SDFMap.ESDF_FAR, "plain32": fa.SDFMap.ESDF_PLAIN32}[request.param]
    monkeypatch.setattr(fa.SDFMap, "default_esdf_family", fam)
    return request.param


@pytest.mark.parametrize("signed", [0, 1])
def test_full_size_g400_optimistic_esdf(fa, signed, esdf_kernels):
    """updateESDF3d with optimistic = true (topo_algorithm.xml:71-72: only inflated voxels are sources) on the
    400x400x100 grid, full box: distances are 10-100x those of the headline configuration, the outward scans
    run long.  Against the oracle (<= 1e-4 m) plus exact-integer squared distances and zero on sources."""
    from fuel_amd import synth
    map_size = (40.0, 40.0, 10.0)
    w = synth.World.for_map_size(map_size)
    truth = w.world(42, 400)
    occ, _ = w.known_state(truth, 42, 120)
    org = (-20.0, -20.0, -1.0)
    box = ((org[0] + 1, org[1] + 1, 0.0), (19.0, 19.0, 7.0))
    om = fo.OracleMap(map_size, *box, optimistic=1, signed_dist=signed)
    om.occ[:] = occ
    gm = fa.SDFMap(map_size, *box, optimistic=1, signed_dist=signed)
    gm.uploadOccupancy(occ)
    lo, hi = helpers.full_box(om.nvox)
    om.set_local_bound(lo, hi)
    gm.setLocalBound(lo, hi)
    om.inflate_local()
    om.update_esdf()
    gm.clearAndInflateLocalMap()
    gm.updateESDF3d()
    h = gm.syncHost(inflate=True, distance=True)
    assert np.array_equal(h["inflate"], om.infl)
    d_o = np.clip(om.dist, -BIG, BIG)
    d_g = np.clip(h["distance"], -BIG, BIG)
    assert np.abs(d_o - d_g).max() <= ESDF_TOL
    if not signed:
        assert np.all(d_g[om.infl == 1] == 0.0)
        sq = (d_g / om.res) ** 2
        assert np.abs(sq - np.rint(sq)).max() < 2e-2  # squared voxel distances are integers (f32 store)
    gm.close()


def test_sparse_map_long_scans(fa, esdf_kernels):
    """optimistic ESDF on a mostly free map with a handful of obstacle voxels and NO floor: z-lines and whole
    x-slabs without a source (INF through the passes), distances of hundreds of voxels; plus the all-free box
    (no source at all: the reference's res*sqrt(DBL_MAX) everywhere)."""
    map_size = (30.0, 26.0, 6.0)
    om = fo.OracleMap(map_size, optimistic=1)
    gm = fa.SDFMap(map_size, optimistic=1)
    nv = om.nvox
    rng = np.random.default_rng(12)
    occ = np.full(om.N, om.l_min)  # known free
    for _ in range(40):
        i = rng.integers([3, 3, 3], np.array(nv) - 3)
        occ.reshape(nv)[i[0], i[1], i[2]] = om.l_max
    occ.reshape(nv)[200:203, 50:180, 30:34] = om.l_max  # one wall
    om.occ[:] = occ
    gm.uploadOccupancy(occ)
    for lo, hi in [helpers.full_box(nv), ((10, 10, 5), (150, 120, 50)), ((220, 0, 0), (299, 259, 59))]:
        om.set_local_bound(lo, hi)
        gm.setLocalBound(lo, hi)
        om.inflate_local()
        om.update_esdf()
        gm.clearAndInflateLocalMap()
        gm.updateESDF3d()
        assert_map_equal(om, gm, (lo, hi))
    gm.close()


@pytest.mark.parametrize("optimistic, signed, map_size", [(0, 0, (9.0, 7.0, 4.0)), (1, 0, (9.0, 7.0, 4.0)),
                                                          (0, 0, (3.2, 84.0, 2.4)), (0, 1, (3.2, 84.0, 2.4))],
                         ids=["0", "1", "long_y", "long_y_signed"])
def test_esdf_kernel_families_agree_on_ragged_boxes(fa, optimistic, signed, map_size, esdf_kernels):
    """half-explored world (short scans) and boxes that are not 4-aligned in z, not 8-aligned in x / y: the block
    minima of the FAR kernels have partial last blocks and garbage columns outside the box.  The thin map's y lines of
    833 - 840 voxels take the packed z/y pass's 2-segment chunks (k_esdf_zy_pk2<MODE, 2, NW>), in both signs."""
    if map_size[1] < 80:
        om, _, _, box = helpers.explored_oracle_map(map_size, 14, 25, optimistic=optimistic, signed_dist=signed)
    else:  # (the camera fixtures need a room: the thin map gets seeded obstacles and an unknown end instead)
        om, box = fo.OracleMap(map_size, optimistic=optimistic, signed_dist=signed), (None, None)
        rng = np.random.default_rng(5)
        occ = om.occ.reshape(om.nvox)
        occ[:] = om.l_min
        idx = rng.integers(0, om.nvox, size=(80, 3))
        occ[idx[:, 0], idx[:, 1], idx[:, 2]] = om.l_occ + 0.5
        occ[:, 600:, :] = om.unknown_value
    gm = fa.SDFMap(tuple(om.cfg.map_size), box[0], box[1], optimistic=optimistic, signed_dist=signed)
    gm.uploadOccupancy(om.occ)
    nv = om.nvox
    for lo, hi in [helpers.full_box(nv), ((3, 5, 1), (nv[0] - 6, nv[1] - 2, nv[2] - 3)), ((17, 9, 2), (58, 43, 30)),
                   ((0, 0, 5), (9, 8, 6))]:
        if any(h >= n for h, n in zip(hi, nv)):
            continue  # (the room's boxes that leave the thin map)
        om.set_local_bound(lo, hi)
        gm.setLocalBound(lo, hi)
        om.inflate_local()
        om.update_esdf()
        gm.clearAndInflateLocalMap()
        gm.updateESDF3d()
        if hi[1] - lo[1] + 1 > 832:
            packed = [k for k in helpers.esdf_plan_kernels(fa, gm, lo, hi) if k.startswith("k_esdf_zy_pk2")]
            want = {"plain": ["k_esdf_zy_pk2<0, 2, 2>"], "far": [], "plain32": []}[esdf_kernels]
            assert packed == want + (["k_esdf_zy_pk2<2, 2, 2>"] if signed and esdf_kernels != "plain32" else [])
        assert_map_equal(om, gm, (lo, hi))
    gm.close()


def test_esdf_switches_kernels_from_the_previous_update(fa, monkeypatch):
    """the adaptive path: an explored hall (optimistic, floor + one pillar) makes the first update report mostly
    far outputs, the second one then runs the FAR kernels; a half-explored map keeps the plain ones.  Either way
    the distances equal the oracle's, and the stage timings show the hall getting cheaper on the second update."""
    map_size = (20.0, 20.0, 6.0)
    om = fo.OracleMap(map_size, optimistic=1)
    gm = fa.SDFMap(map_size, optimistic=1)
    nv = om.nvox
    occ = np.full(om.N, om.l_min).reshape(nv)
    occ[:, :, 0] = om.l_max
    occ[90:96, 100:104, 1:40] = om.l_max
    om.occ[:] = occ.reshape(-1)
    gm.uploadOccupancy(om.occ)
    lo, hi = helpers.full_box(nv)
    om.set_local_bound(lo, hi)
    gm.setLocalBound(lo, hi)
    om.inflate_local()
    om.update_esdf()
    gm.clearAndInflateLocalMap()
    from fuel_amd._lib import K_ESDF_ZY, K_ESDF_X
    gm.profileEnable((1 << K_ESDF_ZY) | (1 << K_ESDF_X))
    fams = []
    for _ in range(3):
        gm.updateESDF3d()
        assert_map_equal(om, gm, (lo, hi))
        fams.append(gm.lastEsdfFamily())
    esdf_ms = gm.profileSamples(K_ESDF_ZY)[:3] + gm.profileSamples(K_ESDF_X)[:3]
    print("explored hall, ESDF ms per update:", ["%.3f" % v for v in esdf_ms], "families", fams)
    # the statement under test is the CHOICE (durations are printed, and asserted only under -m perf)
    assert fams == [fa.SDFMap.ESDF_PLAIN, fa.SDFMap.ESDF_FAR, fa.SDFMap.ESDF_FAR], fams
    gm.close()


def test_sync_host_is_box_limited_and_registered_mirrors_match(fa):
    """fuelmi_map_sync_host refreshes exactly the box (bytes outside keep what the caller had), through the
    staged path (pageable buffers) and through registered mirrors (the kernel stores straight into the caller's
    pinned buffers); both give the same bytes."""
    import ctypes as C
    from fuel_amd._lib import check
    om, _, _, box = helpers.explored_oracle_map((8.0, 6.0, 4.0), 12, 20)
    gm = fa.SDFMap(tuple(om.cfg.map_size), box[0], box[1])
    gm.uploadOccupancy(om.occ)
    lo, hi = helpers.full_box(om.nvox)
    om.set_local_bound(lo, hi)
    gm.setLocalBound(lo, hi)
    om.inflate_local()
    om.update_esdf()
    gm.clearAndInflateLocalMap()
    gm.updateESDF3d()
    full = gm.syncHost(occupancy=True, inflate=True, distance=True)
    N = om.N
    dp = C.POINTER(C.c_double)
    for blo, bhi in [((10, 5, 3), (60, 40, 30)), ((0, 0, 0), (79, 0, 39)), ((33, 17, 9), (33, 17, 9)),
                     ((5, 0, 0), (20, 59, 39))]:
        sl = tuple(slice(blo[i], bhi[i] + 1) for i in range(3))
        results = []
        for registered in (False, True):
            o = np.full(N, -7.0)
            i8 = np.full(N, 9, dtype=np.int8)
            d = np.full(N, -5.0)
            if registered:
                check(gm.L.fuelmi_map_register_mirrors(gm.h, o.ctypes.data_as(dp), i8.ctypes.data, d.ctypes.data_as(dp)))
            check(gm.L.fuelmi_map_sync_host(gm.h, (C.c_int * 3)(*blo), (C.c_int * 3)(*bhi), o.ctypes.data_as(dp),
                                            i8.ctypes.data, d.ctypes.data_as(dp)))
            if registered:
                check(gm.L.fuelmi_map_unregister_mirrors(gm.h))
            for got, ref_, fill in ((o, full["occupancy"], -7.0), (i8, full["inflate"], 9), (d, full["distance"], -5.0)):
                g3, r3 = got.reshape(om.nvox), ref_.reshape(om.nvox)
                assert np.array_equal(g3[sl], r3[sl])
                outside = np.ones(om.nvox, dtype=bool)
                outside[sl] = False
                assert np.all(g3[outside] == fill), "bytes outside the box were touched"
            results.append((o, i8, d))
        for a, b in zip(*results):
            assert np.array_equal(a, b)
    gm.close()


# ------------------------------------------------------------------------------------------------
# reference_order: the reference's own cell order (BFS), sequential means, in-order VoxelGrid sums --
# against the LITERAL oracle (canonical_order = False), which is the mode pinned to the real reference
# ------------------------------------------------------------------------------------------------
def _assert_exact_clusters(of, gf, which=0, filtered=False):
    ca, cb = of.clusters(which), gf.clusters(which)
    assert len(ca) == len(cb)
    for k in range(len(ca)):
        assert np.array_equal(ca[k], cb[k]), "cluster %d: cells differ or are in a different order" % k
        for x, y in zip(of.cluster_info(which, k), gf.clusterInfo(which, k)):
            assert np.array_equal(np.asarray(x), np.asarray(y)), "cluster %d: average_/box not bit-equal" % k
        if filtered:
            fa_, fb_ = of.filtered(which, k), gf.filtered(which, k)
            assert fa_.shape == fb_.shape and len(fa_) > 0
            assert np.array_equal(fa_.astype(np.float32), fb_), "cluster %d: filtered_cells_ differ" % k
    return len(ca)


def test_reference_order_cells_and_means_incremental(fa):
    """searchFrontiers over incremental rounds with reference_order: every cluster lists its cells exactly in
    expandFrontier's order (frontier_finder.cpp:123-164) and average_ is the sequential f64 sum (:374-390)."""
    map_size = (20.0, 20.0, 5.0)
    org = (-10.0, -10.0, -1.0)
    box = ((org[0] + 1, org[1] + 1, 0.0), (9.0, 9.0, 3.0))
    om = fo.OracleMap(map_size, *box)
    gm = fa.SDFMap(map_size, *box)
    truth = om.fixture_world(42, 60)
    of = fo.OracleFrontier(om, 100)
    gf = fa.FrontierFinder(gm, cluster_min=100, reference_order=True)
    k = 0
    total = 0
    for r in range(4):
        for _ in range(12):
            pose = om.fixture_camera(truth, 7, k, 60, 0.7)
            k += 1
            pts = om.fixture_render(truth, pose, 160, 120, 2, 2)
            om.input_points(pts, pose[:3])
            gm.inputPointCloud(pts, pose[:3])
        assert of.search() == gf.searchFrontiers()
        total += _assert_exact_clusters(of, gf)
        assert np.array_equal(of.flags, gf.flags())
        of.commit(r == 2)
        gf.commit(r == 2)
        for which in (1, 2):
            _assert_exact_clusters(of, gf, which)
    assert total > 5
    gm.close()


def test_reference_order_with_low_z_seeds(fa):
    """clusters started by a seed below min_z / on the box face: the seed is cells_[0], its member neighbours
    follow in allNeighbors order (:848-860), several components may hang off one seed"""
    map_size = (8.0, 6.0, 4.0)
    box = ((-2.0, -1.5, -0.5), (1.0, 2.0, 1.0))
    om = fo.OracleMap(map_size, *box)
    truth = om.fixture_world(5, 6)
    om.fixture_known_state(truth, 5, 6, 1.0, 2.2)
    gm = fa.SDFMap(map_size, *box)
    gm.uploadOccupancy(om.occ)
    n = 0
    for cmin in (0, 5, 60):
        of = fo.OracleFrontier(om, cmin)
        gf = fa.FrontierFinder(gm, cluster_min=cmin, reference_order=True)
        om.set_updated_box((-1.0, -1.0, 0.2), (0.5, 1.0, 0.8))
        gm.setUpdatedBox((-1.0, -1.0, 0.2), (0.5, 1.0, 0.8))
        assert of.search() == gf.searchFrontiers()
        n += _assert_exact_clusters(of, gf)
        gf.close()
    assert n > 3
    gm.close()


@pytest.mark.parametrize("seed,size_xy", [(42, 2.0), (7, 1.2), (11, 3.0)])
def test_reference_order_split_pieces_exact(fa, seed, size_xy):
    """splitLargeFrontiers with reference_order against the literal oracle: same pieces, cells in the same order,
    bit-equal average_ / boxes / filtered_cells_ (VoxelGrid float sums in BFS order)"""
    om, truth, frames, box = helpers.explored_oracle_map((16.0, 14.0, 4.0), 30, 28, seed=seed)
    gm = fa.SDFMap(tuple(om.cfg.map_size), box[0], box[1])
    gm.uploadOccupancy(om.occ)
    ub = om.get_updated_box(reset=False)
    gm.setUpdatedBox(*ub)
    of = fo.OracleFrontier(om, cluster_min=60, cluster_size_xy=size_xy, down_sample=3, split=True)
    gf = fa.FrontierFinder(gm, cluster_min=60, cluster_size_xy=size_xy, down_sample=3, split=True,
                           reference_order=True)
    n1, n2 = of.search(), gf.searchFrontiers()
    assert n1 == n2 > 0
    assert _assert_exact_clusters(of, gf, filtered=True) == n1
    gf.commit()
    of.commit()
    _assert_exact_clusters(of, gf, 1, filtered=True)
    gf.close()
    gm.close()


def test_reference_order_split_with_seed_clusters(fa):
    om, truth, frames, box = helpers.explored_oracle_map((12.0, 12.0, 4.0), 16, 22, seed=5, extent=0.8)
    gm = fa.SDFMap(tuple(om.cfg.map_size), box[0], box[1])
    gm.uploadOccupancy(om.occ)
    ub = om.get_updated_box(reset=False)
    gm.setUpdatedBox(*ub)
    of = fo.OracleFrontier(om, cluster_min=20, cluster_size_xy=1.0, down_sample=3, split=True)
    gf = fa.FrontierFinder(gm, cluster_min=20, cluster_size_xy=1.0, down_sample=3, split=True, reference_order=True)
    n1, n2 = of.search(), gf.searchFrontiers()
    assert n1 == n2 > 0
    _assert_exact_clusters(of, gf, filtered=True)
    gf.close()
    gm.close()


@pytest.mark.parametrize("seed,size_xy", [(42, 2.0), (7, 1.2)])
def test_reference_order_viewpoints_exact(fa, seed, size_xy):
    """computeFrontiersToVisit with reference_order against the literal oracle: same partition, per cluster the
    same viewpoints in the same order, identical coverage counts and bit-equal positions (the sample centre is
    average_); yaws to 1e-9 rad (device libm)"""
    om, truth, frames, box = helpers.explored_oracle_map((16.0, 14.0, 4.0), 30, 28, seed=seed)
    om.inflate_local()
    gm = fa.SDFMap(tuple(om.cfg.map_size), box[0], box[1])
    gm.uploadOccupancy(om.occ)
    gm.setLocalBound(*om.get_local_bound())
    gm.clearAndInflateLocalMap()
    ub = om.get_updated_box(reset=False)
    gm.setUpdatedBox(*ub)
    of = fo.OracleFrontier(om, cluster_min=60, cluster_size_xy=size_xy, down_sample=3, split=True)
    of.set_viewpoint_cfg(fo.viewpoint_cfg(min_visib_num=5))
    gf = fa.FrontierFinder(gm, cluster_min=60, cluster_size_xy=size_xy, down_sample=3, split=True, reference_order=True)
    gf.setViewpointConfig(gf.viewpointConfig(min_visib_num=5))
    assert of.search() == gf.searchFrontiers() > 0
    of.compute_to_visit()
    na, nd = gf.computeFrontiersToVisit()
    assert na == len(of.clusters(1)) > 0 and nd == len(of.clusters(2))
    total = 0
    for k in range(na):
        (pa, va), (pb, vb) = of.viewpoints(1, k), gf.viewpoints(1, k)
        assert np.array_equal(va, vb), "coverage counts of cluster %d differ" % k
        assert np.array_equal(pa[:, :3], pb[:, :3])
        dyaw = np.abs(pa[:, 3] - pb[:, 3])
        assert np.minimum(dyaw, 2 * np.pi - dyaw).max() <= 1e-9
        total += len(va)
    assert total > 20
    for which in (1, 2):
        _assert_exact_clusters(of, gf, which, filtered=True)
    gf.close()
    gm.close()


# ------------------------------------------------------------------------------------------------
# depth frames read where they lie (device memory, registered host memory) and the C++ streaming loop
# ------------------------------------------------------------------------------------------------
def _stream_frames(n=12, width=160, height=120):
    from fuel_amd import synth
    map_size = (10.0, 8.0, 4.0)
    w = synth.World.for_map_size(map_size)
    truth = w.world(3, 14)
    frames = []
    for k in range(n):
        pose = w.camera(truth, 5, k, n, 0.9)
        frames.append((w.depth_image(truth, pose, width, height, max_range=7.0), pose[:3].copy(),
                       synth.World.pose_quaternion(pose)))
    return map_size, ((-4.0, -3.0, 0.0), (4.0, 3.0, 2.2)), frames


@pytest.mark.parametrize("where", ["device", "registered"])
def test_depth_frames_read_in_place_give_the_same_map(fa, where):
    """fuelmi_map_input_depth with the image in device memory / in a registered host ring (no staging copy: the
    fusion kernels read it where it lies) == the pageable path == the oracle, bit for bit"""
    from fuel_amd._lib import check
    map_size, box, frames = _stream_frames()
    s = 160 / 640.0
    cfg_kw = dict(fx=387.229248046875 * s, fy=387.229248046875 * s, cx=321.04638671875 * s, cy=243.44969177246094 * s)
    om = fo.OracleMap(map_size, *box)
    gm = fa.SDFMap(map_size, *box)
    gcfg, ocfg = gm.depthConfig(**cfg_kw), fo.depth_cfg(**cfg_kw)
    stack = np.ascontiguousarray(np.stack([f[0] for f in frames]).astype(np.uint16))
    rows, cols = stack.shape[1:]
    fb = rows * cols * 2
    if where == "device":
        dev = fa.DeviceBuffer(stack)
        base = dev.ptr
    else:
        ring = fa.RegisteredHostBuffer(stack)
        base = ring.ptr
    try:
        for k, (img, pos, q) in enumerate(frames):
            pts = fo.project_depth(img, pos, q, ocfg)
            om.input_points(pts, pos)
            assert gm.inputDepthImageAt(base + k * fb, rows, cols, pos, q, gcfg) == len(pts)
            assert om.get_local_bound() == gm.getLocalBound()
        gm.synchronize()
    finally:
        if where == "registered":
            ring.close()
    assert np.array_equal(gm.syncHost(occupancy=True)["occupancy"], om.occ)
    gm.close()


def test_cpp_streaming_loop_equals_the_call_sequence(fa):
    """fuelmi_bench_stream (the measurement driver bench.py times) leaves the same map, clusters and costs as
    the same frames pushed through the individual C-ABI calls"""
    import bench
    from fuel_amd import synth
    map_size, n_obs, _ = bench.WORKLOADS["G200"]
    box = bench.exploration_box(map_size)
    frames = bench.streaming_frames(map_size, n_obs, 10, seed=5)
    rng = np.random.default_rng(3)
    ctrl = bench.make_trajectories(rng, 8, 32, np.array(box[0]) + 0.5, np.array(box[1]) - 0.5)
    out = []
    for native in (False, True):
        cyc = bench.GpuStreamCycle(map_size, box, frames, ctrl, device=0)
        if native:
            cyc.run_native(len(frames))
        else:
            for _ in frames:
                cyc.step()
        cyc.finish()
        cost, _ = cyc.dev_problem.download()
        out.append((cyc.map.syncHost(occupancy=True, distance=True), [c.copy() for c in cyc.ff.clusters(1)], cost.copy(),
                    cyc.n_clusters))
        cyc.close()  # (also undoes the registration of the host frame ring -- round 4: this test used to close the
        #              objects one by one and left the ring registered; its freed memory then poisoned whichever later
        #              test's numpy array the allocator placed there: "hipMemcpyAsync invalid argument", 1 run in 8)
    a, b = out
    assert np.array_equal(a[0]["occupancy"], b[0]["occupancy"])
    assert np.array_equal(a[0]["distance"], b[0]["distance"])
    assert len(a[1]) == len(b[1]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))
    assert np.array_equal(a[2], b[2]) and a[3] == b[3]


def test_device_helpers_and_triad(fa):
    """fuelmi_device_alloc / _upload / _free round trip through a kernel that reads the buffer (a depth frame), and
    the STREAM-triad figure bench.py reports is a plausible HBM bandwidth"""
    import ctypes as C
    from fuel_amd._lib import check, lib
    L = lib()
    t = C.c_double()
    check(L.fuelmi_hbm_triad(0, 256 << 20, 2, C.byref(t)))
    assert 500.0 < t.value < 20000.0, t.value
    buf = fa.DeviceBuffer(np.arange(1024, dtype=np.uint16))
    assert buf.ptr and buf.nbytes == 2048
    buf.close()
    assert buf.ptr is None
