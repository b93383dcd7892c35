"""The depth renderer without a device: the two forms of the restatement (tests/depth_render_ref.py) agree byte for byte
on every scene of tests/depth_render_cases.py except the one drawn for deviation 1, where they provably differ; every
scene sits on the edge it is drawn for; fuelmi_render_plan (host only) reports the geometry the scenes aim at; the symbols
exist; every refusal that needs no device."""
import ctypes as C

import numpy as np
import pytest

import depth_render_cases as dc
import depth_render_ref as rr

SCENES = dc.scenes()
RUNS = [(sc["tag"], m) for sc in SCENES for m in sc["models"]]


@pytest.fixture(scope="module")
def restated():
    """(tag, model) -> (D, out), computed once"""
    return {(sc["tag"], m): dc.restate(sc, m) for sc in SCENES for m in sc["models"]}


def test_tags_are_unique_and_both_models_are_drawn():
    tags = [sc["tag"] for sc in SCENES]
    assert len(tags) == len(set(tags))
    assert sum(rr.HOST_NODE in sc["models"] for sc in SCENES) > 30 and sum(rr.CUDA_NODE in sc["models"] for sc in SCENES) > 25


@pytest.mark.parametrize("tag,model", RUNS)
def test_literal_loop_equals_minimum_over_windows(tag, model, restated):
    sc = dc.by_tag(tag)
    cam = dc.cam_of(sc, model)
    _, out = restated[(tag, model)]
    for (T, p), (metres, raw, stats) in zip(sc["poses"], out):
        lit = rr.literal(cam, sc["cloud"], T, p)
        assert lit.dtype == np.float32 and metres.dtype == np.float32 and raw.dtype == np.uint16
        if tag == dc.DEVIATION_SCENE:
            # the near point comes last and lowers every pixel of the literal loop (HOST_NODE: to 9e-4; CUDA_NODE: to
            # 1 mm, published as 0.001f); without it the forms agree
            assert lit.tobytes() != metres.tobytes() and (lit <= np.float32(1e-3)).all() and (lit > 0).all()
            assert (metres == 0).any() and (metres[metres != 0] >= 1.0).all()
            assert rr.literal(cam, sc["cloud"][:-1], T, p).tobytes() == metres.tobytes()
        else:
            assert lit.tobytes() == metres.tobytes()


@pytest.mark.parametrize("tag,model", RUNS)
def test_scene_sits_on_its_edge(tag, model, restated):
    sc = dc.by_tag(tag)
    D, out = restated[(tag, model)]
    assert len(D) == len(sc["poses"]) <= sc["max_poses"]
    assert sc["pred"](model, D, out), (tag, model)
    if sc["general"]:
        metres = out[0][0]
        assert (metres != 0).sum() >= 0.1 * metres.size and len(np.unique(metres[metres != 0])) >= 2
    for d, (metres, raw, stats) in zip(D, out):
        k = d["why"] == rr.KEPT  # every window lies in the image: what the kernel's stores rely on
        assert (d["x0"][k] >= 0).all() and (d["x0"][k] <= d["x1"][k]).all() and (d["x1"][k] < sc["cols"]).all()
        assert (d["y0"][k] >= 0).all() and (d["y0"][k] <= d["y1"][k]).all() and (d["y1"][k] < sc["rows"]).all()
        assert stats[0] == k.sum() and stats[3] == 0 and stats[2] == (metres != 0).sum()


def test_deviation_scene_without_the_near_point_is_order_free():
    """with no point nearer than 1e-3 in view the sequential update is the minimum: any order, the same bytes"""
    sc = dc.by_tag("general_70x50")
    for model in rr.MODELS:
        cam = dc.cam_of(sc, model)
        T, p = sc["poses"][0]
        a = rr.literal(cam, sc["cloud"], T, p)
        b = rr.literal(cam, sc["cloud"][::-1], T, p)
        assert a.tobytes() == b.tobytes()


def test_raw_rule():
    m = np.array([0.0, 0.0005, 0.0015, 0.0025, 1.0, 65.5345, 65.535, 65.5355, 70.0, np.inf], dtype=np.float32)
    r = rr.raw_from_metres(m, 1000.0)
    assert r[0] == 0 and r[4] == 1000 and r[-1] == 65535 and r[-2] == 65535
    for v, got in zip(m[:-1].tolist(), r[:-1].tolist()):
        x = float(np.float32(v) * np.float32(1000.0))
        lo = np.floor(x)
        want = lo + (1 if x - lo > 0.5 or (x - lo == 0.5 and lo % 2 == 1) else 0)
        assert got == min(want, 65535)


def plan(rows, cols, n_points, max_poses=1, fx=32.0, fy=32.0, model=rr.HOST_NODE, range=5.0):
    import fuel_amd
    return fuel_amd.DepthRenderer.plan_for(fuel_amd.DepthRenderer.config(rows, cols, fx, fy, cols / 2.0, rows / 2.0, model,
                                                                         range, max_poses), n_points)


def test_render_plan_is_what_the_scenes_aim_at():
    """fails on the parent commit: the symbol does not exist"""
    p = plan(50, 70, 300)
    assert p["project_points"] == dc.PROJECT_POINTS and p["wave_min_size"] == dc.WAVE_MIN
    assert p["segment_lanes"] == 16 and p["wave_min_size"] == p["segment_lanes"] + 1  # a small window fits 16 x 16
    assert 70 % p["segment_lanes"] and 70 % 64 and 50 % p["segment_lanes"]
    for n, wg in ((0, 0), (1, 1), (256, 1), (257, 2), (512, 2), (513, 3)):
        assert plan(50, 70, n)["project_workgroups"] == wg
    assert plan(50, 70, dc.PROJECT_POINTS + 1)["project_workgroups"] == 2  # scene count_257: more than one workgroup
    for npix_rows, cols, wg in ((1, 1, 1), (1, 1024, 1), (1, 1025, 2), (120, 160, 19), (50, 70, 4)):
        assert plan(npix_rows, cols, 10)["convert_workgroups"] == wg
    assert plan(50, 70, 0)["splat_workgroups"] == 1 and plan(50, 70, 64 * 5 + 1)["splat_workgroups"] == 6
    assert plan(50, 70, 1 << 20)["splat_workgroups"] == 1024
    # the records: 20 bytes per (pose, point), padded to 256
    assert plan(50, 70, 1000, 6)["scratch_bytes"] == -(-6 * 1000 * 20 // 256) * 256
    assert plan(50, 70, 1 << 27, 2)["scratch_bytes"] == 2 * (1 << 27) * 20  # past 2^31: both words of the plan
    for sc in SCENES:  # every scene is renderable
        assert plan(sc["rows"], sc["cols"], len(sc["cloud"]), sc["max_poses"], *sc["intr"][:2])["convert_workgroups"] >= 1


def test_refusals_that_need_no_device():
    """fails on the parent commit"""
    import fuel_amd
    from fuel_amd import _lib
    L = fuel_amd.lib()
    out = (C.c_int * 8)()

    def rc_of(n_points=10, cfg_is_bad=True, **kw):
        a = dict(rows=50, cols=70, fx=32.0, fy=32.0, cx=35.0, cy=25.0, model=rr.HOST_NODE, range=5.0, max_poses=2)
        a.update(kw)
        cfg = fuel_amd.DepthRenderer.config(**a)
        rc = L.fuelmi_render_plan(C.byref(cfg), n_points, out)
        if rc and cfg_is_bad:  # fuelmi_render_create makes the same checks of cfg, before any device is looked for
            h = C.c_void_p()
            assert L.fuelmi_render_create(C.byref(cfg), C.byref(h)) == rc and not h
        return rc

    assert rc_of() == 0
    nan, inf = float("nan"), float("inf")
    for kw in (dict(rows=0), dict(cols=0), dict(rows=-3), dict(fx=0.0), dict(fy=-1.0), dict(fx=nan), dict(fy=inf), dict(cx=nan),
               dict(cy=inf), dict(model=2), dict(model=-1), dict(range=-1.0), dict(range=nan), dict(max_poses=0)):
        assert rc_of(**kw) == _lib.EINVAL, kw
        assert L.fuelmi_last_error()
    for kw in (dict(rows=4097, cols=4096), dict(fx=(2.0 ** 31 - 1) / 57.3), dict(fy=1e9), dict(max_poses=4097),
               dict(rows=4096, cols=4096, max_poses=17)):
        assert rc_of(**kw) == _lib.ELIMIT, kw
    assert rc_of(rows=4096, cols=4096, max_poses=16) == 0 and rc_of(fx=3.7e7) == 0 and rc_of(range=inf) == 0
    assert rc_of(model=rr.CUDA_NODE, range=nan) == 0  # CUDA_NODE ignores the range
    assert rc_of(n_points=-1, cfg_is_bad=False) == _lib.EINVAL and rc_of(n_points=(1 << 27) + 1, cfg_is_bad=False) == _lib.ELIMIT
    assert rc_of(n_points=1 << 27) == 0 and rc_of(n_points=(1 << 27), cfg_is_bad=False, max_poses=3) == _lib.ELIMIT
    # a null renderer is refused everywhere
    assert L.fuelmi_render_set_cloud(None, None, 0) == _lib.EINVAL and L.fuelmi_render_destroy(None) == _lib.EINVAL
    assert L.fuelmi_render_depth(None, 1, None, None, 1000.0, None, None, None) == _lib.EINVAL
    assert L.fuelmi_render_times(None, None) == _lib.EINVAL
    assert not L.fuelmi_render_frame_raw(None, 0) and not L.fuelmi_render_frame_metres(None, 0)


def test_python_mirror_exports_the_calls():
    """fails on the parent commit"""
    import fuel_amd
    from fuel_amd import _lib
    L = fuel_amd.lib()
    for name in ("fuelmi_render_create", "fuelmi_render_destroy", "fuelmi_render_set_cloud", "fuelmi_render_depth",
                 "fuelmi_render_frame_raw", "fuelmi_render_frame_metres", "fuelmi_render_plan", "fuelmi_render_times"):
        assert getattr(L, name) is not None and name in _lib.SYMBOLS
    assert (_lib.RENDER_HOST_NODE, _lib.RENDER_CUDA_NODE) == rr.MODELS
    for name in ("set_cloud", "render", "frame_raw_ptr", "plan", "times", "close", "pose_transform"):
        assert hasattr(fuel_amd.DepthRenderer, name)


def test_pose_transform_is_the_inverse_of_the_camera_pose():
    import fuel_amd
    from fuel_amd import synth
    pose = [0.4, -0.3, 1.2, 0.7, -0.2]
    q = synth.World.pose_quaternion(pose)
    T, pos = fuel_amd.DepthRenderer.pose_transform(pose[:3], q)
    assert T.shape == (3, 4) and np.array_equal(pos, pose[:3])
    fwd = np.array([np.cos(0.7) * np.cos(-0.2), np.sin(0.7) * np.cos(-0.2), np.sin(-0.2)])
    pc = T[:, :3] @ (pos + 2.0 * fwd) + T[:, 3]  # two metres ahead: on the optical axis
    assert np.abs(pc - [0, 0, 2.0]).max() < 1e-12
    assert np.abs(T[:, :3] @ pos + T[:, 3]).max() < 1e-12
