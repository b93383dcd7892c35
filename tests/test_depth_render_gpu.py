"""fuelmi_render_depth on the device against the restatement (tests/depth_render_ref.py) on the scenes of
tests/depth_render_cases.py, every scene in every model it is drawn for.

Everything is compared BIT FOR BIT -- the metres frames (tobytes()), the raw frames, stats: the step is integer selection
plus expressions rounded at fixed points, compiled without FMA contraction, and the minimum makes every schedule give the
same bytes, so there is no tolerance to measure.  Then: the cloud's order does not matter; one renderer reused for
larger and smaller calls equals fresh renderers; clouds given by host and by device pointer; the refusals that need a
renderer; the closed loop into the map's fusion through the device pointer; the facade driver."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import depth_render_cases as dc
import depth_render_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SCENES = dc.scenes()


def renderer(sc, model, max_poses=None):
    import fuel_amd
    return fuel_amd.DepthRenderer(sc["rows"], sc["cols"], *sc["intr"], model=model, range=sc["range"],
                                  max_poses=max_poses or sc["max_poses"], device=0)


def poses_of(sc):
    return np.stack([T for T, _ in sc["poses"]]), np.stack([p for _, p in sc["poses"]])


def render_scene(r, sc, cloud=None):
    r.set_cloud(sc["cloud"] if cloud is None else cloud)
    return r.render(*poses_of(sc), scaling=sc["k"])


def assert_equals_restatement(got, sc, model, cloud=None):
    metres, raw, stats = got
    cam = dc.cam_of(sc, model)
    assert metres.dtype == np.float32 and raw.dtype == np.uint16 and stats.dtype == np.int32
    assert metres.shape == raw.shape == (len(sc["poses"]), sc["rows"], sc["cols"]) and stats.shape == (len(sc["poses"]), 4)
    for j, (T, p) in enumerate(sc["poses"]):
        wm, wr, ws = rr.render(cam, sc["cloud"] if cloud is None else cloud, T, p, sc["k"])
        assert metres[j].tobytes() == wm.tobytes(), (sc["tag"], model, j, int((metres[j] != wm).sum()))
        assert raw[j].tobytes() == wr.tobytes(), (sc["tag"], model, j)
        assert stats[j].tolist() == ws.tolist(), (sc["tag"], model, j)


@pytest.mark.parametrize("tag", [sc["tag"] for sc in SCENES])
def test_scenes(tag):
    sc = dc.by_tag(tag)
    for model in sc["models"]:
        r = renderer(sc, model)
        try:
            assert_equals_restatement(render_scene(r, sc), sc, model)
            t = r.times()
            assert t.shape == (3,) and (t >= 0).all()
        finally:
            r.close()


@pytest.mark.parametrize("tag", ["general_70x50", "general_160x120", "plan_threshold", "overlap_many_near_last"])
def test_cloud_order_does_not_matter(tag):
    sc = dc.by_tag(tag)
    for model in sc["models"]:
        r = renderer(sc, model)
        try:
            first = render_scene(r, sc)
            assert_equals_restatement(first, sc, model)
            for seed in (1, 2, 3):
                perm = np.random.default_rng(seed).permutation(len(sc["cloud"]))
                again = render_scene(r, sc, sc["cloud"][perm])
                for a, b in zip(first, again):
                    assert a.tobytes() == b.tobytes(), (tag, model, seed)
        finally:
            r.close()


def test_reuse_equals_fresh_renderers():
    """a larger call, a smaller one, the first again on ONE renderer: a key image that is not back to empty, or records
    left in the grown scratch, would show"""
    big, small = dc.by_tag("batch_max_poses"), dc.by_tag("count_63")
    like = lambda sc, **kw: dict(sc, range=big["range"], **kw)  # noqa: E731  one renderer: one range
    other = like(dc.by_tag("count_257"), poses=big["poses"][:3])
    seq = [big, like(small), big, other, like(small, cloud=small["cloud"][:0]), big]
    for model in rr.MODELS:
        r = renderer(big, model)
        try:
            got = [render_scene(r, sc) for sc in seq]
        finally:
            r.close()
        for sc, g in zip(seq, got):
            assert_equals_restatement(g, sc, model)
            f = renderer(sc, model, max_poses=len(sc["poses"]))
            try:
                fresh = render_scene(f, sc)
            finally:
                f.close()
            for a, b in zip(g, fresh):
                assert a.tobytes() == b.tobytes(), (sc["tag"], model)
        assert (got[4][0] == 0).all() and (got[4][1] == 0).all() and not got[4][2].any()  # the empty cloud: all-zero frames


def test_set_cloud_twice_and_by_device_pointer():
    import fuel_amd
    a, b = dc.by_tag("general_70x50"), dc.by_tag("count_65")
    for model in rr.MODELS:
        r = renderer(a, model)
        buf = fuel_amd.DeviceBuffer(a["cloud"], device=0)
        try:
            r.set_cloud(b["cloud"])
            r.set_cloud(a["cloud"])  # replaces the first
            host = r.render(*poses_of(a), scaling=a["k"])
            assert_equals_restatement(host, a, model)
            r.set_cloud(b["cloud"])
            assert_equals_restatement(r.render(*poses_of(a), scaling=a["k"]), dict(a, cloud=b["cloud"]), model)
            r.set_cloud(buf.ptr, len(a["cloud"]))
            dev = r.render(*poses_of(a), scaling=a["k"])
            for x, y in zip(host, dev):
                assert x.tobytes() == y.tobytes()
            only_stats = r.render(*poses_of(a), scaling=a["k"], metres=False, raw=False)
            assert only_stats[0] is None and only_stats[1] is None and np.array_equal(only_stats[2], host[2])
        finally:
            buf.close()
            r.close()


def test_refusals_that_need_a_renderer():
    import fuel_amd
    from fuel_amd import _lib
    sc = dc.by_tag("batch_3")
    T, p = poses_of(sc)
    L = fuel_amd.lib()
    r = renderer(sc, rr.HOST_NODE)
    try:
        with pytest.raises(fuel_amd.FuelmiError, match="no cloud"):
            r.render(T, p)
        r.set_cloud(sc["cloud"][:0])  # an empty cloud is legal
        m, raw, st = r.render(T, p)
        assert not m.any() and not raw.any() and not st.any()
        r.set_cloud(sc["cloud"])
        want = r.render(T, p)
        stats = np.full((4, 4), -7, dtype=np.int32)

        def rc_of(n_pose, k, TT=T, pp=p):
            return L.fuelmi_render_depth(r._h, n_pose, TT.ctypes.data_as(C.POINTER(C.c_double)),
                                         pp.ctypes.data_as(C.POINTER(C.c_double)), k, None, None,
                                         stats.ctypes.data_as(C.POINTER(C.c_int)))
        assert rc_of(0, 1000.0) == _lib.EINVAL and rc_of(-1, 1000.0) == _lib.EINVAL and rc_of(4, 1000.0) == _lib.ELIMIT
        for k in (0.0, -1.0, float("nan"), float("inf")):
            assert rc_of(3, k) == _lib.EINVAL
        bad = T.copy()
        bad[1, 2, 3] = np.nan
        assert rc_of(3, 1000.0, TT=bad) == _lib.EINVAL
        badp = p.copy()
        badp[2, 0] = np.inf
        assert rc_of(3, 1000.0, pp=badp) == _lib.EINVAL
        assert (stats == -7).all()  # nothing was written
        assert L.fuelmi_render_set_cloud(r._h, None, 5) == _lib.EINVAL and L.fuelmi_render_set_cloud(r._h, None, -1) == _lib.EINVAL
        with pytest.raises(fuel_amd.FuelmiError):
            r.frame_raw_ptr(3)
        with pytest.raises(fuel_amd.FuelmiError):
            r.frame_raw_ptr(-1)
        again = r.render(T, p)  # the refusals left the renderer as it was
        for a, b in zip(want, again):
            assert a.tobytes() == b.tobytes()
        h = C.c_void_p(r._h.value)
        r.close()
        # used after destroy: refused, not followed
        assert L.fuelmi_render_depth(h, 3, T.ctypes.data_as(C.POINTER(C.c_double)), p.ctypes.data_as(C.POINTER(C.c_double)),
                                     1000.0, None, None, None) == _lib.EINVAL
        assert L.fuelmi_render_set_cloud(h, None, 0) == _lib.EINVAL and L.fuelmi_render_destroy(h) == _lib.EINVAL
        assert not L.fuelmi_render_frame_raw(h, 0)
    finally:
        r.close()


def test_closed_loop_into_the_fusion():
    """six frames of smoke()'s world and camera path rendered in one call; frame k into map A by its device pointer, into
    map B from the host copy: the same maps"""
    import fuel_amd
    from fuel_amd import synth
    map_size, bmin, bmax = (10.0, 8.0, 4.0), (-4.0, -3.0, 0.0), (4.0, 3.0, 2.2)
    w = synth.World.for_map_size(map_size)
    truth = w.world(3, 14)
    idx = np.argwhere(truth.reshape(w.nvox) != 0)
    assert len(idx) > 1000
    origin = np.array([-map_size[0] / 2, -map_size[1] / 2, -1.0])
    cloud = ((idx + 0.5) * 0.1 + origin).astype(np.float32)  # the centres of the truth voxels
    s = 160 / 640.0
    kw = dict(fx=387.229248046875 * s, fy=387.229248046875 * s, cx=321.04638671875 * s, cy=243.44969177246094 * s)
    poses = [w.camera(truth, 5, k, 6, 0.6) for k in range(6)]
    quats = [synth.World.pose_quaternion(p) for p in poses]
    tp = [fuel_amd.DepthRenderer.pose_transform(p[:3], q) for p, q in zip(poses, quats)]
    r = fuel_amd.DepthRenderer(120, 160, kw["fx"], kw["fy"], kw["cx"], kw["cy"], model=rr.HOST_NODE, range=5.0, max_poses=6)
    ga = fuel_amd.SDFMap(map_size, bmin, bmax, device=0)
    gb = fuel_amd.SDFMap(map_size, bmin, bmax, device=0)
    try:
        r.set_cloud(cloud)
        metres, raw, stats = r.render(np.stack([t for t, _ in tp]), np.stack([c for _, c in tp]))
        cam = rr.Cam(120, 160, kw["fx"], kw["fy"], kw["cx"], kw["cy"], rr.HOST_NODE, 5.0)
        wm, wr, ws = rr.render(cam, cloud, *tp[2])
        assert metres[2].tobytes() == wm.tobytes() and raw[2].tobytes() == wr.tobytes() and stats[2].tolist() == ws.tolist()
        cfg = ga.depthConfig(**kw)
        na = [ga.inputDepthImageAt(r.frame_raw_ptr(k), 120, 160, poses[k][:3], quats[k], cfg) for k in range(6)]
        nb = [gb.inputDepthImage(raw[k], poses[k][:3], quats[k], cfg) for k in range(6)]
        assert na == nb and min(na) >= 0 and sum(na) > 0
        ga.clearAndInflateLocalMap()
        gb.clearAndInflateLocalMap()
        ha, hb = ga.syncHost(occupancy=True, inflate=True), gb.syncHost(occupancy=True, inflate=True)
        assert ha["occupancy"].tobytes() == hb["occupancy"].tobytes() and ha["inflate"].tobytes() == hb["inflate"].tobytes()
        assert ha["inflate"].any()
    finally:
        r.close()
        ga.close()
        gb.close()


def test_facade_driver_with_every_mirror_off():
    exe = os.path.join(ROOT, "fuel_amd", "facade", "facade_render")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout)
    assert res["mirrors"] == [0, 0, 0] and res["frames"] >= 4
    for m in ("host_node", "cuda_node"):
        assert res[m]["pixels_with_return"] > 0
        assert res[m]["fused_device_pointer"] == res[m]["fused_host_copy"] and sum(res[m]["fused_device_pointer"]) > 0
        assert res[m]["occupancy_byte_equal"] is True and res[m]["inflate_byte_equal"] is True
        assert res[m]["occupied_voxels"] > 0
