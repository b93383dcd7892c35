"""fuelmi_map_extract_cloud on the device against the restatement (tests/map_cloud_ref.py) on the scenes of
tests/map_cloud_cases.py, every scene with every kind.

Everything is compared BIT FOR BIT -- counts, order, float bit patterns, the untouched tail of a capped buffer: the step is
integer selection plus one f64 expression rounded once, compiled without FMA contraction, so there is no tolerance to
measure.  The restatement is evaluated on the occupancy and inflate arrays read back from the device (syncHost), which are
also compared with the uploaded log-odds and their numpy inflation.  Then the cap, the empty boxes and refusals, the cloud
behind every mutator of the planes, repeated calls on one map, map E (two rounds of the scan) and the facade driver with
every mirror off."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import map_cloud_cases as mc
import map_cloud_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SENTINEL = 0xA5A5A5A5


def new_map(m):
    import fuel_amd
    gm = fuel_amd.SDFMap(m.map_size, device=0, **m.kw)
    assert gm.nvox == m.nvox and np.array_equal(gm.origin, m.origin)
    assert gm.info.min_occupancy_log == mc.MIN_OCC and gm.info.clamp_min_log == mc.CLAMP_MIN
    assert gm.info.inflate_step == m.step
    return gm


def params(gm):
    return mr.Params(gm.res, gm.origin, gm.info.min_occupancy_log, gm.info.clamp_min_log)


def read_back(gm):
    h = gm.syncHost(occupancy=True, inflate=True)
    return h["occupancy"].reshape(gm.nvox), h["inflate"].reshape(gm.nvox)


def load_state(gm, m, state):
    """upload the state's log-odds, inflate the whole map; -> the arrays read back (and compared with what went in)"""
    occ, infl = m.state(state) if isinstance(state, str) else state
    gm.uploadOccupancy(occ.reshape(-1))
    gm.setLocalBound(*mc.full_box(gm.nvox))
    gm.clearAndInflateLocalMap()
    o, i = read_back(gm)
    assert o.tobytes() == occ.tobytes()
    if infl is not None:
        assert np.array_equal(i, infl)
    return o, i


def check(gm, o, i, kind, lo, hi, z_low=-np.inf, z_high=np.inf, known_as="reference", tag=""):
    want = mr.extract(params(gm), o, i, kind, lo, hi, z_low, z_high, known_as)
    got = gm.extract_cloud(kind, lo, hi, z_low, z_high)
    assert got.dtype == np.float32 and got.shape == want.shape, (tag, kind, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), (tag, kind)
    assert gm.count_voxels(kind, lo, hi, z_low, z_high) == len(want), (tag, kind)
    return got


@pytest.mark.parametrize("name", sorted(mc.MAPS))
def test_scenes(name):
    m = mc.spec(name)
    mine = [sc for sc in mc.scenes() if sc["map"] == name]
    gm = new_map(m)
    try:
        # the fresh map first: as created, nothing uploaded, nothing inflated
        o, i = read_back(gm)
        assert o.tobytes() == m.state("fresh")[0].tobytes() and not i.any()
        for sc in [s for s in mine if s["state"] == "fresh"]:
            for kind in mr.KINDS:
                check(gm, o, i, kind, sc["lo"], sc["hi"], sc["z_low"], sc["z_high"], tag=sc["tag"])
        for state in sorted({sc["state"] for sc in mine} - {"fresh"}):
            o, i = load_state(gm, m, state)
            for sc in [s for s in mine if s["state"] == state]:
                for kind in mr.KINDS:
                    if state == mc.DEVIATION_STATE and kind == mr.KNOWN:
                        # the documented deviation: a value ON the threshold is known to the plane's complement
                        got = check(gm, o, i, kind, sc["lo"], sc["hi"], sc["z_low"], sc["z_high"], "plane", sc["tag"])
                        assert len(got) == len(mc.restate(sc, kind)) + int((o == mc.THR).sum())
                    else:
                        check(gm, o, i, kind, sc["lo"], sc["hi"], sc["z_low"], sc["z_high"], tag=sc["tag"])
    finally:
        gm.close()


def raw_call(gm, kind, lo, hi, cap, rows, null=False, z_low=-np.inf, z_high=np.inf):
    """the C call on a buffer of `rows` points filled with the sentinel -> (status, n_total, buffer as uint32 [rows, 3])"""
    from fuel_amd import _lib
    buf = np.full((rows, 3), SENTINEL, dtype=np.uint32)
    n = C.c_int(-77)
    cfg = _lib.CloudCfg(int(kind), (C.c_int * 3)(*lo), (C.c_int * 3)(*hi), float(z_low), float(z_high))
    rc = gm.L.fuelmi_map_extract_cloud(gm.h, C.byref(cfg), None if null else buf.ctypes.data, int(cap), C.byref(n))
    return rc, n.value, buf


def test_cap_and_refusals():
    from fuel_amd import _lib
    m = mc.spec("a")
    gm = new_map(m)
    try:
        o, i = load_state(gm, m, "random")
        sc = next(s for s in mc.scenes() if s["tag"] == mc.CAP_SCENE)
        for kind in mr.KINDS:
            want = mr.extract(params(gm), o, i, kind, sc["lo"], sc["hi"]).view(np.uint32)
            n = len(want)
            assert n > 2
            for label, f in mc.CAPS:
                cap = f(n)
                rc, tot, buf = raw_call(gm, kind, sc["lo"], sc["hi"], cap, cap + 8)
                k = min(cap, n)
                assert rc == (0 if n <= cap else _lib.ELIMIT), (kind, label)
                assert tot == n and np.array_equal(buf[:k], want[:k]) and (buf[k:] == SENTINEL).all(), (kind, label)
                pts, tot2 = gm.extract_cloud(kind, sc["lo"], sc["hi"], cap=cap)
                assert tot2 == n and pts.view(np.uint32).tobytes() == want[:k].tobytes()
            rc, tot, buf = raw_call(gm, kind, sc["lo"], sc["hi"], 0, 4, null=True)  # count only
            assert (rc, tot) == (0, n) and (buf == SENTINEL).all()
        # empty boxes: the loops do not run
        for lo, hi in mc.EMPTY_BOXES:
            for kind in mr.KINDS:
                rc, tot, buf = raw_call(gm, kind, lo, hi, 4, 4)
                assert (rc, tot) == (0, 0) and (buf == SENTINEL).all()
                assert gm.count_voxels(kind, lo, hi) == 0 and gm.extract_cloud(kind, lo, hi).shape == (0, 3)
        # refusals: nothing is written
        for lo, hi in mc.BAD_BOXES:
            rc, tot, buf = raw_call(gm, mr.UNKNOWN, lo, hi, 4, 4)
            assert (rc, tot) == (_lib.EINVAL, -77) and (buf == SENTINEL).all()
        for kind in mc.BAD_KINDS:
            rc, tot, buf = raw_call(gm, kind, (0, 0, 0), (3, 3, 3), 4, 4)
            assert (rc, tot) == (_lib.EINVAL, -77) and (buf == SENTINEL).all()
        rc, tot, buf = raw_call(gm, mr.UNKNOWN, (0, 0, 0), (3, 3, 3), 4, 4, null=True)  # room promised, no buffer
        assert (rc, tot) == (_lib.EINVAL, -77)
        rc, tot, buf = raw_call(gm, mr.UNKNOWN, (0, 0, 0), (3, 3, 3), -1, 4)
        assert (rc, tot) == (_lib.EINVAL, -77) and (buf == SENTINEL).all()
    finally:
        gm.close()


def test_cloud_follows_every_mutator():
    """each mutator of the planes, then the cloud at once (no synchronise in between), then the arrays it must equal"""
    m = mc.spec("a")
    gm = new_map(m)
    box = mc.full_box(m.nvox)

    def clouds_then_arrays(tag, kinds=mr.KINDS):
        got = {k: gm.extract_cloud(k, *box) for k in kinds}
        o, i = read_back(gm)
        for k in kinds:
            assert got[k].tobytes() == mr.extract(params(gm), o, i, k, *box).tobytes(), (tag, k)
        return o, i

    try:
        occ = m.state("random")[0]
        gm.uploadOccupancy(occ.reshape(-1))
        o, _ = clouds_then_arrays("upload")
        assert o.tobytes() == occ.tobytes()
        # one small depth-like point cloud from inside the map
        ang = np.linspace(0.0, 2 * np.pi, 40, endpoint=False)
        pts = np.stack([0.7 * np.cos(ang), 0.6 * np.sin(ang), 0.3 + 0.2 * np.sin(3 * ang)], axis=1).astype(np.float32)
        gm.inputPointCloud(pts, (0.02, -0.03, 0.25))
        o1, _ = clouds_then_arrays("inputPointCloud")
        assert o1.tobytes() != o.tobytes()
        gm.setLocalBound((2, 3, 1), (20, 15, 22))
        gm.clearAndInflateLocalMap()
        _, i1 = clouds_then_arrays("clearAndInflateLocalMap", (mr.INFLATED,))
        assert i1.any()
        # resetBuffer clears the inflated plane (and the distances) of a box, as the reference's does (sdf_map.cpp:95-115)
        lo_p, hi_p = mr.index_to_pos(m.P, (4, 5, 6)), mr.index_to_pos(m.P, (15, 12, 20))
        gm.resetBuffer(lo_p, hi_p)
        o2, i2 = clouds_then_arrays("resetBuffer box")
        assert i1[4:16, 5:13, 6:21].any() and not i2[4:16, 5:13, 6:21].any() and i2.any()
        assert o2.tobytes() == o1.tobytes()
        gm.resetBuffer()
        _, i3 = clouds_then_arrays("resetBuffer all")
        assert not i3.any() and len(gm.extract_cloud(mr.INFLATED, *box)) == 0
    finally:
        gm.close()


def test_repeated_calls_leave_nothing_behind():
    """growing, then shrinking boxes on one map give the bytes of fresh maps: the grow-only scratch holds no stale counts"""
    m = mc.spec("a")
    tags = ("one_voxel", "items_63", "face_z1_a", "whole_a", "items_255", "one_line", "items_1", "whole_a", "one_voxel")
    seq = [next(s for s in mc.scenes() if s["tag"] == t) for t in tags]
    gm = new_map(m)
    try:
        load_state(gm, m, "random")
        got = [[gm.extract_cloud(k, sc["lo"], sc["hi"]) for k in (mr.OCCUPIED, mr.KNOWN)] for sc in seq]
        cnt = [[gm.count_voxels(k, sc["lo"], sc["hi"]) for k in (mr.OCCUPIED, mr.KNOWN)] for sc in seq]
    finally:
        gm.close()
    for sc, g, c in zip(seq, got, cnt):
        fm = new_map(m)
        try:
            load_state(fm, m, "random")
            for j, k in enumerate((mr.OCCUPIED, mr.KNOWN)):
                fresh = fm.extract_cloud(k, sc["lo"], sc["hi"])
                assert fresh.tobytes() == g[j].tobytes() and len(fresh) == c[j], (sc["tag"], k)
        finally:
            fm.close()


def test_map_e_takes_two_rounds_of_the_scan():
    e = mc.map_e()
    p = mc.plan(e.nvox, *mc.full_box(e.nvox))
    assert p["scan_rounds"] == 2
    gm = new_map(e)
    try:
        o, i = load_state(gm, e, (mc.e_state(e), None))
        for kind in mr.KINDS:
            check(gm, o, i, kind, *mc.full_box(e.nvox), tag="map_e")
    finally:
        gm.close()


def test_facade_driver_with_every_mirror_off():
    exe = os.path.join(ROOT, "fuel_amd", "facade", "facade_cloud")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(out.stdout)
    assert r["mirrors"] == [0, 0, 0]
    for name in ("publishMapLocal", "publishMapAll", "publishUnknown"):
        assert r[name]["byte_equal"] is True and r[name]["n_device"] == r[name]["n_host"] > 0, name
    assert r["publishMapAll"]["known_device"] == r["publishMapAll"]["known_host"] > 0
