"""fuelmi_map_topo_paths on the device.  The field is built through the map's own calls (occupancy upload, inflation,
updateESDF3d), read back, and first checked to lie within 2 ulp (f32) of res * sqrt(k) of the scene.  Then
  (A) against the restatement (tests/topo_ref.py, which tests/test_topo_path_cpu.py pins to the reference's own code) in
      `cut` mode on the device's own field: every output and counter bit for bit;
  (B) against the recorded results of the reference itself (tests/golden/topo/*.npz): every discrete output and every
      point that no gradient push produced equal, a pushed point (and a path length behind one) within 100 x the
      disagreement tests/test_topo_path_cpu.py measures for the scene under -2 .. +2 ulp of the f32 field
      (topo_cases.robustness; at most 3.3e-8 m, so 3.3e-6 m);
batch independence, the pool's size over a repeated call, and the refusal that needs the map's resolution."""
import os
import sys

import numpy as np
import pytest

import topo_cases as tc
import topo_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "topo")
SCENES = tc.scenes()
_maps, _refs = {}, {}


def _device_map(blocks):
    """(the device map of the blocks, its distance field as an [nx, ny, nz] f64 array)"""
    import fuel_amd
    key = repr(blocks)
    if key not in _maps:
        gm = fuel_amd.SDFMap(tc.MAP_SIZE, device=0)
        assert gm.nvox == tc.NVOX and np.array_equal(gm.origin, tc.ORIGIN) and gm.res == tc.RES
        gm.uploadOccupancy(tc.occupancy(blocks))
        gm.setLocalBound((0, 0, 0), tuple(v - 1 for v in tc.NVOX))
        gm.clearAndInflateLocalMap()
        gm.updateESDF3d()
        h = gm.syncHost(inflate=True, distance=True)
        assert np.array_equal(h["inflate"].reshape(tc.NVOX) == 1, tc.sources(blocks))
        dist = h["distance"].reshape(tc.NVOX)
        k = tc.squared_distance(tc.sources(blocks))
        if (k < 0).all():
            assert (dist > 1e30).all()
        else:
            want = tc.RES * np.sqrt(k.astype(np.float64))
            with np.errstate(over="ignore"):
                d32 = dist.astype(np.float32)
            assert np.array_equal(d32.astype(np.float64), dist)  # the mirror holds the device's f32 values
            assert np.all(np.abs(dist - want) <= 2 * np.spacing(want.astype(np.float32)).astype(np.float64))
        _maps[key] = (gm, dist)
    return _maps[key]


@pytest.fixture(scope="module", autouse=True)
def _close_maps():
    yield
    for gm, _ in _maps.values():
        gm.close()
    _maps.clear()


def _cfg(sc):
    return {k: v for k, v in sc["cfg"].items() if k != "max_sample_num"}


def _run(gm, sc, probs=None, **kw):
    probs = sc["probs"] if probs is None else probs
    return gm.topo_paths([p["start"] for p in probs], [p["end"] for p in probs], [sc["samples"]] * len(probs),
                         [p["start_pts"] or None for p in probs], [p["end_pts"] or None for p in probs],
                         **dict(_cfg(sc), **kw))


def _restated(name):
    if name not in _refs:
        sc = SCENES[name]
        _refs[name] = tc.run_ref(sc, "cut", _device_map(sc["blocks"])[1])
    return _refs[name]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def _assert_equal(out, b, r, cfg):
    """problem b of a device result against a result of the restatement, bit for bit"""
    mpp, maxn = cfg["max_path_points"], cfg["max_nodes"]
    over = any(len(p) > mpp for k in ("raw", "filt", "sel") for p in r[k]) or len(r["nodes"]) > maxn
    assert out["status"][b] == (-1 if over and r["status"] in (tr.OK, tr.NO_PATH) else r["status"])
    assert list(out["counts"][b]) == list(r["counts"]) and list(out["events"][b]) == list(r["events"])
    assert out["n_nodes"][b] == len(r["nodes"])
    for got, want in zip(out["nodes"][b], r["nodes"][:maxn]):
        assert (got[0], got[1]) == (want[0], want[1]) and _bits(got[2]) == _bits(want[2]) and list(got[3]) == list(want[3])
    for key in ("raw", "filt", "sel"):
        lens = [int(v) for v in out[key + "_len"][b] if v > 0]
        assert lens == [len(p) for p in r[key]], key
        for got, want in zip(out[key][b], r[key]):
            assert _bits(got) == _bits(want[:mpp]), key
    assert _bits(out["sel_length"][b][:len(r["sel"])]) == _bits(r["sel_length"])


@pytest.mark.parametrize("name", list(SCENES))
def test_device_equals_the_restatement_on_its_own_field(name):
    sc = SCENES[name]
    gm, _ = _device_map(sc["blocks"])
    out = _run(gm, sc, allow_limit=True)
    assert out["limit"] == (name == "overflow")
    for b, r in enumerate(_restated(name)):
        _assert_equal(out, b, r, sc["cfg"])
    if name == "overflow":  # the graph is complete although the paths are cut
        assert out["n_nodes"][0] == len(_restated(name)[0]["nodes"]) == len(out["nodes"][0])


@pytest.mark.parametrize("name", [n for n in SCENES if n not in tc.NOT_RECORDED])
def test_device_against_the_recorded_reference(name):
    sc = SCENES[name]
    gm, _ = _device_map(sc["blocks"])
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    ok, measured = tc.robustness(name)
    tol = 100 * measured
    print("%s: measured disagreement %.3e, tolerance of a pushed point %.3e" % (name, measured, tol))
    assert ok
    out = _run(gm, sc)
    for b, r in enumerate(_restated(name)):
        assert out["n_nodes"][b] == len(z["node_id%d" % b])
        assert [n[0] for n in out["nodes"][b]] == list(z["node_id%d" % b])
        assert [n[1] for n in out["nodes"][b]] == list(z["node_type%d" % b])
        assert _bits([n[2] for n in out["nodes"][b]]) == _bits(z["node_pos%d" % b])
        assert [i for n in out["nodes"][b] for i in n[3]] == list(z["nb_ids%d" % b])
        flags = dict(raw=[[False] * len(p) for p in r["raw"]], filt=r["filt_pushed"], sel=r["sel_pushed"])
        for key in ("raw", "filt", "sel"):
            lens = [int(v) for v in out[key + "_len"][b] if v > 0]
            assert lens == list(z[key + "_len%d" % b]), key
            pts = z[key + "_pts%d" % b]
            at = 0
            for got, fl in zip(out[key][b], flags[key]):
                want = pts[at:at + len(got)]
                at += len(got)
                for q, w, pushed in zip(got, want, fl):
                    if pushed:
                        assert np.max(np.abs(q - w)) <= tol, key
                    else:
                        assert _bits(q) == _bits(w), key
        for got, want, fl in zip(out["sel_length"][b], z["sel_length%d" % b], r["sel_pushed"]):
            assert abs(got - want) <= (2 * len(fl) * tol if any(fl) else 0.0)
        assert (out["status"][b] == tr.NO_PATH) == (len(z["sel_len%d" % b]) == 0)


def test_a_result_does_not_depend_on_the_place_in_the_batch():
    sc = SCENES["two_pillars"]
    gm, _ = _device_map(sc["blocks"])
    p = sc["probs"][0]
    others = [dict(p, start=(-2.0, -0.6, 0.0), end=(2.0, 0.7, 0.2)), dict(p, start=(-2.4, 1.0, 0.3), end=(1.0, -2.0, 0.0)),
              dict(p, start=(0.0, 0.0, -0.5), end=(0.0, 0.0, 0.9))]
    out = _run(gm, sc, probs=[p] + others + [p])
    assert out["status"][3] == tr.UNDEFINED and out["status"][0] == tr.OK
    r = _restated("two_pillars")[0]
    _assert_equal(out, 0, r, sc["cfg"])
    _assert_equal(out, 4, r, sc["cfg"])


def test_a_repeated_call_allocates_nothing():
    sc = SCENES["pillar"]
    gm, _ = _device_map(sc["blocks"])
    _run(gm, sc, probs=sc["probs"] * 3)
    size = gm.topo_pool_bytes()
    assert size > 0
    for n in (3, 1, 2):
        _run(gm, sc, probs=sc["probs"] * n)
        assert gm.topo_pool_bytes() == size


def test_start_and_end_within_a_resolution_are_refused():
    import fuel_amd
    sc = SCENES["free"]
    gm, _ = _device_map(sc["blocks"])
    with pytest.raises(fuel_amd.FuelmiError):
        _run(gm, sc, probs=[dict(sc["probs"][0], start=(0.0, 0.0, 0.0), end=(0.1, 0.0, 0.0))])
    out = _run(gm, sc, probs=[dict(sc["probs"][0], start=(0.0, 0.0, 0.0), end=(0.11, 0.0, 0.0))])
    assert out["status"][0] in (tr.OK, tr.NO_PATH, tr.UNDEFINED)
