"""The cloud extraction without a device: every scene of tests/map_cloud_cases.py sits on the edge it is drawn for (its
predicate holds under the restatement, tests/map_cloud_ref.py), the restatement's vectorised form equals its literal
loops, its point expression is the one the header states, and fuelmi_cloud_plan (host only) reports the geometry at its
edges."""
import math

import numpy as np
import pytest

import map_cloud_cases as mc
import map_cloud_ref as mr


@pytest.fixture(scope="module")
def clouds():
    """tag -> {kind: the restatement's cloud}"""
    return {sc["tag"]: {k: mc.restate(sc, k) for k in mr.KINDS} for sc in mc.scenes()}


def test_maps_have_the_sizes_they_are_drawn_for():
    for name in mc.MAPS:
        m = mc.spec(name)
        assert m.initmap_nvox() == m.nvox, name
        assert m.step == 2
    a = mc.spec("a")
    assert a.nvox[2] % 2 == 1 and math.gcd(a.nvox[2], 64) == 1
    starts = {((x * a.nvox[1] + y) * a.nvox[2]) % 64 for x in range(a.nvox[0]) for y in range(a.nvox[1])}
    assert starts == set(range(64))  # the lines start at every bit offset
    assert mc.spec("b").nvox[2] == 2 * 64 + 2
    assert mc.spec("c1").nvox[2] == 64 and mc.spec("c2").nvox[2] == 128
    d = mc.spec("d")
    assert not np.any(np.float64(np.float32(mr.index_to_pos(d.P, (3, 4, 5)))) == mr.index_to_pos(d.P, (3, 4, 5)))


def test_thresholds_are_the_maps():
    """the constants of the cases are SDFMap::initMap's (fuelmi_map_create computes them the same way)"""
    assert mc.MIN_OCC == math.log(0.80 / (1 - 0.80)) and mc.CLAMP_MIN == math.log(0.12 / (1 - 0.12))
    assert mc.V_UNKNOWN < mc.THR < mc.V_FREE < mc.MIN_OCC < mc.V_OCC


@pytest.mark.parametrize("tag", [sc["tag"] for sc in mc.scenes()])
def test_scene_sits_on_its_edge(tag, clouds):
    sc = next(s for s in mc.scenes() if s["tag"] == tag)
    occ, _ = mc.spec(sc["map"]).state(sc["state"])
    if sc["state"] != mc.DEVIATION_STATE:
        assert mc.state_is_off_threshold(occ)
        assert np.array_equal(mc.restate(sc, mr.KNOWN), mc.restate(sc, mr.KNOWN, known_as="plane"))
    assert sc["pred"](sc, clouds[tag]), tag


def test_vectorised_restatement_equals_the_literal_loops():
    for tag in ("one_voxel", "one_line", "part_line_b", "face_z1_d", "leak_occ", "thr", "thr_exact", "zboth_d", "zcrossed_a",
                "znan_high_a", "items_63"):
        sc = next(s for s in mc.scenes() if s["tag"] == tag)
        m = mc.spec(sc["map"])
        occ, infl = m.state(sc["state"])
        for kind in mr.KINDS:
            for known_as in ("reference", "plane"):
                a = mr.extract(m.P, occ, infl, kind, sc["lo"], sc["hi"], sc["z_low"], sc["z_high"], known_as)
                b = mr.extract_loop(m.P, occ, infl, kind, sc["lo"], sc["hi"], sc["z_low"], sc["z_high"], known_as)
                assert a.tobytes() == b.tobytes(), (tag, kind)


def test_point_expression():
    """each coordinate is the f64 expression (i + 0.5) * resolution + origin rounded once to float"""
    for name in ("a", "d"):
        m = mc.spec(name)
        occ, infl = m.state("fresh")
        pts = mr.extract(m.P, occ, infl, mr.UNKNOWN, *mc.full_box(m.nvox))
        idx = np.argwhere(np.ones(m.nvox, dtype=bool))
        for a in range(3):
            want = np.array([np.float32((i + 0.5) * m.res + m.origin[a]) for i in idx[:, a].tolist()], dtype=np.float32)
            assert pts[:, a].tobytes() == want.tobytes()


def test_fresh_map_is_the_order_test(clouds):
    sc = next(s for s in mc.scenes() if s["tag"] == "fresh_part_a")
    pts = clouds["fresh_part_a"][mr.UNKNOWN]
    m = mc.spec("a")
    lo, hi = sc["lo"], sc["hi"]
    adr = [(x * m.nvox[1] + y) * m.nvox[2] + z for x in range(lo[0], hi[0] + 1) for y in range(lo[1], hi[1] + 1)
           for z in range(lo[2], hi[2] + 1)]
    assert adr == sorted(adr) and len(adr) == len(pts)  # ascending voxel address


def test_cloud_plan_edges():
    """fails on the parent commit: the symbol does not exist"""
    p0 = mc.plan((8, 8, 8), (0, 0, 0), (7, 7, 7))
    wg, sw = p0["items_per_workgroup"], p0["scan_width"]
    assert wg >= 64 and wg % 64 == 0 and sw >= 64 and sw % 64 == 0
    # items per line: 64-bit chunks of the z extent
    for zlen, cpl in ((1, 1), (64, 1), (65, 2), (128, 2), (130, 3)):
        p = mc.plan((4, 4, 130), (1, 0, 0), (2, 3, zlen - 1))
        assert (p["items_per_line"], p["lines"], p["voxels"]) == (cpl, 8, 8 * zlen)
        q = mc.plan((4, 4, 130), (1, 0, 130 - zlen), (2, 3, 129))  # the same extent from any start
        assert q == p
    # workgroups around the workgroup's items, rounds around the scan's width
    for lines, nwg in ((1, 1), (wg - 1, 1), (wg, 1), (wg + 1, 2), (2 * wg, 2), (2 * wg + 1, 3)):
        p = mc.plan((lines + 2, 2, 3), (1, 1, 0), (lines, 1, 2))
        assert (p["lines"], p["workgroups"], p["scan_rounds"]) == (lines, nwg, 1)
    for nwg, rounds in ((sw - 1, 1), (sw, 1), (sw + 1, 2), (2 * sw, 2), (2 * sw + 1, 3)):
        p = mc.plan((nwg, wg, 2), (0, 0, 0), (nwg - 1, wg - 1, 1))
        assert (p["workgroups"], p["scan_rounds"]) == (nwg, rounds)
        assert p["scratch_bytes"] >= 4 * nwg + 4
    e = mc.map_e()
    p = mc.plan(e.nvox, *mc.full_box(e.nvox))
    assert p["scan_rounds"] == 2 and sw < p["workgroups"] <= sw + 64 and e.initmap_nvox() == e.nvox
    # an empty box: nothing to do; a box that leaves the map, an impossible map: refused
    for lo, hi in mc.EMPTY_BOXES:
        p = mc.plan(mc.spec("a").nvox, lo, hi)
        assert (p["items_per_line"], p["lines"], p["workgroups"], p["scan_rounds"], p["voxels"]) == (0, 0, 0, 0, 0)
    import fuel_amd
    for lo, hi in mc.BAD_BOXES:
        with pytest.raises(fuel_amd.FuelmiError):
            mc.plan(mc.spec("a").nvox, lo, hi)
    for dims in ((0, 4, 4), (4, 4, 256), (4096, 4096, 255)):
        with pytest.raises(fuel_amd.FuelmiError):
            mc.plan(dims, (0, 0, 0), (0, 0, 0))


def test_empty_and_bad_boxes_are_what_they_claim():
    nv = mc.spec("a").nvox
    for k, (lo, hi) in enumerate(mc.EMPTY_BOXES):
        assert any(lo[a] > hi[a] for a in range(3))
        if k < 3:
            assert lo[k] > hi[k] and all(0 <= lo[a] <= hi[a] < nv[a] for a in range(3) if a != k)
    for lo, hi in mc.BAD_BOXES:
        assert all(lo[a] <= hi[a] for a in range(3)) and any(lo[a] < 0 or hi[a] >= nv[a] for a in range(3))


def test_python_mirror_exports_the_calls():
    """fails on the parent commit"""
    import fuel_amd
    from fuel_amd import _lib
    assert hasattr(fuel_amd.SDFMap, "extract_cloud") and hasattr(fuel_amd.SDFMap, "count_voxels")
    assert (_lib.CLOUD_OCCUPIED, _lib.CLOUD_UNKNOWN, _lib.CLOUD_KNOWN, _lib.CLOUD_INFLATED) == mr.KINDS
    assert hasattr(fuel_amd.lib(), "fuelmi_map_extract_cloud")
