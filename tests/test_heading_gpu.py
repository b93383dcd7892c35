"""fuelmi_map_info_gains / fuelmi_map_yaw_paths on the device against the restatement (tests/heading_ref.py) on the scenes
of tests/heading_cases.py.

The maps are uploaded as log-odds (unknown = clamp_min_log - 0.01) and the device derives its own unknown and occupied
planes.  Integers and UNIFORM gains equal the restatement; a NON_UNIFORM gain lies within heading_ref.parity_tolerance of
the restatement's sum in the device's order (the C library's exp against the device's); path, path_vertex and g_value are
compared BIT FOR BIT with the restatement's recurrence run on the gains the device returned, and with given gains with the
restatement outright.  Then packing, reversal, strides, repetition, the memo (n_rays), a map that changes between two
calls, and the error paths."""
import os
import sys

import numpy as np
import pytest

import heading_cases as hc
import heading_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
GAINS = hc.gain_scenes()
PATHS = hc.path_scenes()
CFG_KEYS = ("weight_type", "in_box", "factor", "far", "top_ang", "left_ang", "right_ang", "lambda1", "lambda2")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def device_map(name):
    import fuel_amd
    m = hc.spec(name)
    gm = fuel_amd.SDFMap(m.map_size, m.box_min, m.box_max, device=0, **m.kw)
    assert gm.nvox == m.nvox and tuple(gm.origin) == m.origin
    assert abs(gm.info.clamp_min_log - hc.L_FREE) < 1e-12
    gm.uploadOccupancy(m.log_odds())
    return gm


@pytest.fixture(scope="module")
def maps():
    """name -> (device map, the restatement's map with the device's resolution_inv), made on first use"""
    made = {}

    def get(name):
        if name not in made:
            gm = device_map(name)
            made[name] = (gm, hc.spec(name).ref(gm.info.resolution_inv))
            assert made[name][1].box_min == tuple(gm.info.box_min) and made[name][1].box_max == tuple(gm.info.box_max)
        return made[name]
    yield get
    for gm, _ in made.values():
        gm.close()


def grun(gm, scs, **kw):
    """one call for gain scenes that share their map and configuration"""
    c0 = scs[0]["cfg"]
    assert all(s["cfg"] == c0 for s in scs)
    ctrl = None
    if c0["weight_type"] == hr.NON_UNIFORM:
        ctrl = [s["ctrl"] for s in scs]
        kw.setdefault("path_of", list(range(len(scs))))
    return gm.info_gains([s["pos"] for s in scs], [s["yaws"] for s in scs], ctrl=ctrl, **dict(c0, **kw))


def gassert(out, b, sc, want=None):
    r = want if want is not None else hc.restate(sc)
    k = len(sc["yaws"])
    tag = sc["tag"]
    assert out["status"][b] == 0, tag
    assert list(out["n_cand"][b][:k]) == r["n_cand"], (tag, out["n_cand"][b][:k], r["n_cand"])
    assert list(out["n_visible"][b][:k]) == r["n_visible"], (tag, out["n_visible"][b][:k], r["n_visible"])
    assert out["n_rays"][b] == r["n_rays"], (tag, out["n_rays"][b], r["n_rays"])
    if sc["cfg"]["weight_type"] == hr.UNIFORM:
        assert list(out["gain"][b][:k]) == r["gain"], tag
    else:
        tol = hr.parity_tolerance()[1]
        for g, w in zip(out["gain"][b][:k], r["gain"]):
            assert abs(g - w) <= tol * abs(w), (tag, g, w, tol)
    assert not out["gain"][b][k:].any() and not out["n_cand"][b][k:].any(), tag  # what is not written is zero


def ggroups(scenes):
    g = {}
    for sc in scenes:
        g.setdefault((sc["map"],) + tuple(sc["cfg"][k] for k in CFG_KEYS), []).append(sc)
    return g


def prun(gm, scs, **kw):
    """one call for path scenes that share their map and configuration"""
    s0 = scs[0]
    key = ("cfg", "h", "yaw_diff", "max_yaw_rate", "w")
    assert all(all(s[k] == s0[k] for k in key) and (s["gains_in"] is None) == (s0["gains_in"] is None) for s in scs)
    ctrl = [s["ctrl"] for s in scs] if s0["ctrl"] is not None else None
    gin = [s["gains_in"] for s in scs] if s0["gains_in"] is not None else None
    return gm.yaw_paths([s["pts"] for s in scs], [s["yaws"] for s in scs], [s["dt"] for s in scs], ctrl=ctrl, gains_in=gin,
                        half_vert_num=s0["h"], yaw_diff=s0["yaw_diff"], max_yaw_rate=s0["max_yaw_rate"], w=s0["w"],
                        **dict(s0["cfg"], **kw))


def passert(out, b, sc):
    tag, L, nv = sc["tag"], len(sc["yaws"]), 2 * sc["h"] + 1
    r = hc.restate(sc)
    assert out["status"][b] == 0, tag
    assert list(out["n_rays"][b][:L]) == r["n_rays"], (tag, out["n_rays"][b][:L], r["n_rays"])
    got = out["gains"][b][:L, :nv]
    if sc["gains_in"] is not None:
        assert _bits(got[1:L - 1]) == _bits(sc["gains_in"][1:L - 1]), tag
    elif sc["cfg"]["weight_type"] == hr.UNIFORM:
        assert _bits(got) == _bits(r["gains"]), tag
    else:
        tol = hr.parity_tolerance()[1]
        assert np.all(np.abs(got - np.array(r["gains"])) <= tol * np.abs(np.array(r["gains"]))), tag
    # the recurrence on the gains the device returned
    s = hr.search(hr.layers_of(sc["yaws"], got, sc["h"], sc["yaw_diff"]), sc["dt"], sc["w"], sc["max_yaw_rate"])
    assert list(out["path_vertex"][b][:L]) == s["path_vertex"], (tag, out["path_vertex"][b][:L], s["path_vertex"])
    assert _bits(out["path"][b][:L]) == _bits(s["path"]), tag
    for i in range(L):
        row = s["g_value"][i]
        assert _bits(out["g_value"][b][i][:len(row)]) == _bits(row), (tag, i, out["g_value"][b][i], row)
        assert not out["g_value"][b][i][len(row):].any(), tag
    assert not out["path"][b][L:].any() and not out["g_value"][b][L:].any(), tag
    if sc["gains_in"] is not None or sc["cfg"]["weight_type"] == hr.UNIFORM or sc["assert_path"]:
        assert s["path_vertex"] == r["path_vertex"], tag
    for k, v in sc["expect"].items():
        assert list(out[k][b][:L]) == v, (tag, k)


# ---- 1. every scene -----------------------------------------------------------------------------------------------------------
def test_every_gain_scene(maps):
    seen = 0
    for key, scs in ggroups(GAINS).items():
        gm, _ = maps(key[0])
        out = grun(gm, scs)
        assert not out["limit"]
        for b, sc in enumerate(scs):
            gassert(out, b, sc)
            for k, v in sc["expect"].items():
                if k != "cells":
                    got = out[k][b]
                    assert (list(got[:len(v)]) if isinstance(v, list) else got) == v, (sc["tag"], k)
            seen += 1
    assert seen == len(GAINS) >= 30


def test_every_path_scene(maps):
    for sc in PATHS:
        gm, _ = maps(sc["map"])
        passert(prun(gm, [sc]), 0, sc)


def test_mid_scale_defaults(maps):
    sc = hc.mid_scene()
    gm, _ = maps(sc["map"])
    out = prun(gm, [sc])
    passert(out, 0, sc)
    assert min(out["n_rays"][0][1:6]) > 500  # a few thousand cells, several hundred rays a way-point


# ---- 2. packing, reversal, strides, repetition ---------------------------------------------------------------------------------
def test_gain_packing_reversal_strides_and_repetition(maps):
    gm, _ = maps("open")
    for wt in (hr.UNIFORM, hr.NON_UNIFORM):  # the largest call of either weight type: groups of 1, 2, 3 and 11 yaws
        main = max((g for k, g in ggroups(GAINS).items() if k[:2] == ("open", wt)), key=len)
        assert len(main) >= 3 and len({len(s["yaws"]) for s in main}) >= 2
        fwd, again, rev = grun(gm, main), grun(gm, main), grun(gm, main[::-1])
        wide = grun(gm, main, max_yaw=hr.MAX_YAW, max_ctrl=17)
        n = len(main)
        for b, sc in enumerate(main):
            alone = grun(gm, [sc])
            k = len(sc["yaws"])
            for key in ("gain", "n_cand", "n_visible"):
                want = _bits(fwd[key][b][:k])
                assert want == _bits(again[key][b][:k]), (sc["tag"], key)
                assert want == _bits(rev[key][n - 1 - b][:k]), (sc["tag"], key)
                assert want == _bits(alone[key][0][:k]), (sc["tag"], key)
                assert want == _bits(wide[key][b][:k]), (sc["tag"], key)
            assert fwd["n_rays"][b] == rev["n_rays"][n - 1 - b] == alone["n_rays"][0] == wide["n_rays"][b]
    assert gm.info_gains(np.zeros((0, 3)), [])["status"].shape == (0,)  # n_group = 0


def test_path_packing_reversal_and_strides(maps):
    gm, _ = maps("wall")
    base = next(s for s in PATHS if s["tag"] == "layers_3")
    pts, yaws = hc._line(7), [0.0, 0.2, 0.1, -0.3, 0.4, 0.0, 0.1]
    batch = [base] + [dict(base, tag="layers_3/%d" % k, pts=np.array(pts[:k]), yaws=yaws[:k], expect={})
                      for k in (5, 1, 7, 2)]  # problems of different depth share a call
    fwd, rev = prun(gm, batch), prun(gm, batch[::-1])
    wide = prun(gm, batch, max_layer=hr.MAX_LAYER)
    for b, sc in enumerate(batch):
        passert(fwd, b, sc)
        passert(rev, len(batch) - 1 - b, sc)
        passert(wide, b, sc)
    nu = next(s for s in PATHS if s["tag"] == "nu_layers_5")
    a, b2 = prun(gm, [nu, nu]), prun(gm, [nu], max_ctrl=40)
    for key in ("gains", "g_value", "path"):
        assert _bits(a[key][0]) == _bits(a[key][1]) == _bits(b2[key][0]), key
    assert gm.yaw_paths([], [], [])["status"].shape == (0,)


# ---- 3. the memo ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["open_11", "wall_11", "nu_wall_11", "open_cap", "count_129_3"])
def test_k_yaws_equal_k_groups_of_one(maps, tag):
    """bit for bit, NON_UNIFORM included; and a group's rays are the distinct cells that need one, not K times them"""
    sc = next(s for s in GAINS if s["tag"] == tag)
    gm, m = maps(sc["map"])
    k = len(sc["yaws"])
    whole = grun(gm, [sc])
    split = gm.info_gains([sc["pos"]] * k, [[y] for y in sc["yaws"]], ctrl=None if sc["ctrl"] is None else [sc["ctrl"]],
                          **sc["cfg"])  # (every group weighs with array 0)
    for key in ("gain", "n_cand", "n_visible"):
        assert _bits(whole[key][0][:k]) == _bits(split[key][:, 0]), key
    cells = set()
    for y in sc["yaws"]:
        cells |= {c[0] for c in hr.view(m, sc["cfg"], sc["pos"], y)}
    assert whole["n_rays"][0] == len(cells) < int(split["n_rays"].sum())
    assert list(split["n_rays"]) == [int(v) for v in whole["n_cand"][0][:k]]


# ---- 4. the map changes between two calls ---------------------------------------------------------------------------------------
def test_sees_the_planes_a_fused_frame_leaves():
    """the call runs behind the fusion on the map's stream and reads the planes it rewrote: no host mirror in between"""
    gm = device_map("open")
    sc = next(s for s in GAINS if s["tag"] == "open_11")
    before = grun(gm, [sc])
    gassert(before, 0, sc)
    # a disc of points 0.9 m in front of the camera: the fusion marks their cells occupied and the rays to them free
    ys, zs = np.meshgrid(np.arange(-0.5, 0.5, 0.04), np.arange(-0.3, 0.7, 0.04), indexing="ij")
    pts = np.stack([np.full(ys.size, 0.92), ys.ravel() + 0.03, zs.ravel()], axis=1)
    for _ in range(8):  # (log-odds: several hits until a cell counts as occupied)
        gm.inputPointCloud(pts, hc.CAM)
    after = grun(gm, [sc])
    occ = gm.syncHost(occupancy=True)["occupancy"].reshape(gm.nvox)
    unk, hit = occ < gm.info.clamp_min_log - 1e-3, occ > gm.info.min_occupancy_log
    assert hit.any() and (~unk).sum() > hit.sum()
    m = hc.spec("open")
    ref = hr.Map(m.origin, hc.RES, unk, hit, m.box_min, m.box_max, gm.info.resolution_inv)
    want = hr.info_gains(ref, sc["cfg"], sc["pos"], sc["yaws"])
    gassert(after, 0, sc, want)
    assert list(after["n_visible"][0]) != list(before["n_visible"][0])
    gm.close()


# ---- 5. the limits and the refusals ---------------------------------------------------------------------------------------------
def test_over_the_cell_cap_among_good_neighbours(maps):
    import fuel_amd
    gm, m = maps("mid")
    plan = fuel_amd.yawpath_plan()
    assert plan["max_cells"] == hr.MAX_CELLS and plan["max_yaw"] == hr.MAX_YAW and plan["max_layer"] == hr.MAX_LAYER
    cfg = hr.gain_cfg(far=4.5, factor=2)
    good = ((-2.0, 5.9, 0.3), [1.5]), ((5.9, -1.0, 0.3), [0.0, 0.2])  # looking out of the map: small boxes
    over = ((0.5, 0.5, 0.3), [0.0, 2.0])
    groups = [good[0], over, good[1]]
    want = [hr.info_gains(m, cfg, p, y) for p, y in groups]
    assert want[1]["cells"] > hr.MAX_CELLS >= max(want[0]["cells"], want[2]["cells"]) > 0
    with pytest.raises(fuel_amd.FuelmiError, match="error -5"):
        gm.info_gains([g[0] for g in groups], [g[1] for g in groups], **cfg)
    out = gm.info_gains([g[0] for g in groups], [g[1] for g in groups], allow_limit=True, **cfg)
    assert out["limit"] and list(out["status"]) == [0, -1, 0]
    assert not out["gain"][1].any() and not out["n_cand"][1].any() and out["n_rays"][1] == 0
    for b in (0, 2):
        k = len(groups[b][1])
        assert list(out["n_cand"][b][:k]) == want[b]["n_cand"] and list(out["gain"][b][:k]) == want[b]["gain"]
        assert out["n_rays"][b] == want[b]["n_rays"]
    # the search: the problem with such a layer is -1, its neighbours complete
    ok = dict(hc.mid_scene(), cfg=dict(cfg, weight_type=hr.UNIFORM, far=1.5), ctrl=None, tag="mid_small", h=1)
    big = dict(ok, cfg=dict(cfg, weight_type=hr.UNIFORM, far=4.5), tag="mid_big")
    kw = dict(half_vert_num=1, yaw_diff=ok["yaw_diff"], max_yaw_rate=ok["max_yaw_rate"], w=ok["w"], allow_limit=True)
    o = gm.yaw_paths([ok["pts"], big["pts"], ok["pts"]], [ok["yaws"]] * 3, [ok["dt"]] * 3, **dict(big["cfg"], **kw))
    assert o["limit"] and list(o["status"]) == [-1, -1, -1]  # one configuration, far = 4.5 for all three
    o = gm.yaw_paths([ok["pts"], ok["pts"]], [ok["yaws"]] * 2, [ok["dt"]] * 2, **dict(ok["cfg"], **kw))
    assert not o["limit"] and list(o["status"]) == [0, 0]
    far_pts = np.array(ok["pts"]) + (6.0, 0.0, 0.0)  # way-points at the map's edge: small boxes at far = 4.5
    r_small = hr.search_path_of_yaw(m, big["cfg"], far_pts, ok["yaws"], ok["dt"], None, 1, ok["yaw_diff"], ok["max_yaw_rate"],
                                    ok["w"])
    assert not r_small["over"] and hr.search_path_of_yaw(m, big["cfg"], big["pts"], ok["yaws"], ok["dt"], None, 1,
                                                         ok["yaw_diff"], ok["max_yaw_rate"], ok["w"])["over"]
    o = gm.yaw_paths([far_pts, big["pts"], far_pts], [ok["yaws"]] * 3, [ok["dt"]] * 3, **dict(big["cfg"], **kw))
    assert o["limit"] and list(o["status"]) == [0, -1, 0]
    assert not o["path"][1].any() and not o["g_value"][1].any() and not o["gains"][1].any() and not o["n_rays"][1].any()
    for b in (0, 2):
        assert list(o["path_vertex"][b]) == r_small["path_vertex"] and _bits(o["g_value"][b][1]) == _bits(r_small["g_value"][1])


def test_refusals(maps):
    import fuel_amd
    gm, _ = maps("open")
    sc = GAINS[0]

    def refused(code, f, *a, **kw):
        with pytest.raises(fuel_amd.FuelmiError, match="error %d" % code):
            f(*a, **kw)
    nan = (0.0, float("nan"), 0.0)
    refused(-1, gm.info_gains, [nan], [[0.0]])
    refused(-1, gm.info_gains, [sc["pos"]], [[float("inf")]])
    refused(-1, gm.info_gains, [sc["pos"]], [[0.0]], weight_type=2)
    refused(-1, gm.info_gains, [sc["pos"]], [[0.0]], factor=0)
    refused(-1, gm.info_gains, [sc["pos"]], [[0.0]], far=float("nan"))
    refused(-1, gm.info_gains, [sc["pos"]], [[0.0]], weight_type=hr.NON_UNIFORM)  # no control points
    refused(-1, gm.info_gains, [sc["pos"]], [[0.0]], weight_type=hr.NON_UNIFORM, ctrl=[[nan]])
    refused(-1, gm.info_gains, [sc["pos"]], [[0.0]], weight_type=hr.NON_UNIFORM, ctrl=[[(0, 0, 0)]], path_of=[1])
    refused(-5, gm.info_gains, [sc["pos"]], [[0.0] * (hr.MAX_YAW + 1)])
    pts, yaws = [[(0, 0, 0)] * 3], [[0.0] * 3]
    uni = dict(weight_type=hr.UNIFORM)
    refused(-1, gm.yaw_paths, [np.zeros((0, 3))], [[]], [0.5], max_layer=3, **uni)      # n_layer = 0
    refused(-1, gm.yaw_paths, pts, yaws, [0.0], **uni)                                  # dt
    refused(-1, gm.yaw_paths, pts, [[0.0, float("nan"), 0.0]], [0.5], **uni)
    refused(-1, gm.yaw_paths, pts, yaws, [0.5], w=float("inf"), **uni)
    refused(-1, gm.yaw_paths, pts, yaws, [0.5], gains_in=[np.full((3, 7), np.nan)], **uni)
    refused(-1, gm.yaw_paths, pts, yaws, [0.5], half_vert_num=-1, **uni)
    refused(-5, gm.yaw_paths, pts, yaws, [0.5], half_vert_num=(hr.MAX_YAW + 1) // 2, **uni)
    refused(-5, gm.yaw_paths, pts, yaws, [0.5], max_layer=hr.MAX_LAYER + 1, **uni)
    gassert(grun(gm, [sc]), 0, sc)  # the map still answers
