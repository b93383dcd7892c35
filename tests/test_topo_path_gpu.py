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
import topo_device as td
import topo_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "topo")
SCENES = tc.scenes()
_refs = {}
_device_map, _run, _bits, _assert_equal = td.device_map, td.run, td.bits, td.assert_equal


@pytest.fixture(scope="module", autouse=True)
def _close_maps():
    yield
    td.close_maps()


def _restated(name):
    if name not in _refs:
        sc = SCENES[name]
        _refs[name] = tc.run_ref(sc, "cut", _device_map(sc["blocks"])[1])
    return _refs[name]


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
