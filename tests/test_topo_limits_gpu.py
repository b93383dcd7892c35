"""fuelmi_map_topo_paths on the device at its lane-window, stride and cap edges: every scene of topo_cases.edge_scenes()
and the batches round the large graphs `forest10` / `forest14`, each problem against the restatement (tests/topo_ref.py)
in `cut` mode on the device's own read-back field, every output, count and event bit for bit (rule (A) of
tests/test_topo_path_gpu.py, which also holds the two forests against their recorded fixtures).  What a scene is there to
reach is asserted again here from the witness trace of the restatement on the device's field
(tests/test_topo_limits_cpu.py asserts it on the f32 rounding of the scene's field): a scene that has drifted off its edge
fails, it does not pass unnoticed."""
import os
import sys

import pytest

import topo_cases as tc
import topo_device as td
import topo_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
SCENES, EDGE = tc.scenes(), tc.edge_scenes()
_refs = {}


@pytest.fixture(scope="module", autouse=True)
def _close_maps():
    yield
    td.close_maps()


def _restated(key, sc):
    """(results, traces) of the restatement on the device's field of the scene's map"""
    if key not in _refs:
        traces = []
        _refs[key] = (tc.run_ref(sc, "cut", td.device_map(sc["blocks"])[1], traces), traces)
    return _refs[key]


@pytest.mark.parametrize("name", list(EDGE))
def test_edge_scene_equals_the_restatement(name):
    sc = EDGE[name]
    gm, _ = td.device_map(sc["blocks"])
    res, traces = _restated(name, sc)
    tc.check_edge_claims(name, sc, res, traces)
    out = td.run(gm, sc, allow_limit=True)
    cfg = sc["cfg"]
    over = [r["status"] == -1 or any(len(p) > cfg["max_path_points"] for k in ("raw", "filt", "sel") for p in r[k])
            for r in res]
    assert out["limit"] == any(over)
    assert over == dict(rows_one_less=[True], cap256=[False, True], cap4096=[False, True]).get(name, [False] * len(res))
    for b, r in enumerate(res):
        td.assert_equal(out, b, r, cfg)


def _forest10():
    return _restated("forest10", SCENES["forest10"])


def test_max_nodes_at_the_graph_and_under_it():
    sc = SCENES["forest10"]
    gm, _ = td.device_map(sc["blocks"])
    res, traces = _forest10()
    tc.check_forest_claims("forest10", sc, res, traces)
    n = len(res[0]["nodes"])
    one_less, two = tc.FOREST10_MAX_NODES
    assert one_less == n - 1 and sum(len(x[3]) for x in res[0]["nodes"][:two]) > 4 * two
    for maxn in (n, one_less, two):
        out = td.run(gm, sc, allow_limit=True, max_nodes=maxn)
        assert out["limit"] == (maxn < n) and out["status"][0] == (-1 if maxn < n else res[0]["status"])
        assert out["n_nodes"][0] == n and len(out["nodes"][0]) == min(n, maxn)
        td.assert_equal(out, 0, res[0], dict(sc["cfg"], max_nodes=maxn))
    # (two rows of over 8 ids: the ids stop at their 8 slots, and nb_off with them)
    assert sum(len(x[3]) for x in out["nodes"][0]) == 4 * two


def test_a_batch_round_the_large_graphs():
    """[the large graph, a problem over the 256-point cap, an undefined problem, the large graph again, another large
    graph]: each equals the restatement of it alone -- a workspace slice carved with the wrong stride shows here"""
    sc = SCENES["forest10"]
    gm, _ = td.device_map(sc["blocks"])
    p = sc["probs"][0]
    probs = [p, dict(p, start_pts=((-2.0 - tc.CAP256_D[1], 0.033, 0.0),)), dict(p, start=(0.0, 0.0, -0.5), end=(0.0, 0.0, 0.9)),
             p, dict(p, start=(-2.0, -0.45, 0.0), end=(2.0, 0.55, 0.1))]
    res, traces = _restated("forest10 batch", dict(sc, probs=[probs[1], probs[2], probs[4]]))
    res = [_forest10()[0][0], res[0], res[1], _forest10()[0][0], res[2]]
    assert [r["status"] for r in res] == [tr.OK, -1, tr.UNDEFINED, tr.OK, tr.OK]
    # the second large graph is another graph, and large; the capped problem got as far as its last select path
    assert len(res[4]["nodes"]) >= 32 and tc.discrete(res[4]) != tc.discrete(res[0]) and res[4]["counts"][3] >= 2
    assert res[1]["counts"][0] == res[0]["counts"][0] and res[1]["counts"][1:] == [0, 0, 0]
    assert max(q["committed"] for q in traces[0]["shortcut"]) == tr.MAX_PATH_POINTS - 2
    out = td.run(gm, sc, probs=probs, allow_limit=True)
    assert out["limit"]
    for b, r in enumerate(res):
        td.assert_equal(out, b, r, sc["cfg"])


def test_the_other_forest_in_a_batch_of_its_own():
    """forest14 (four prune rounds, max_raw_path2 cutting a length bucket) twice round another problem of its map"""
    sc = SCENES["forest14"]
    gm, _ = td.device_map(sc["blocks"])
    res, traces = _restated("forest14", sc)
    tc.check_forest_claims("forest14", sc, res, traces)
    p = sc["probs"][0]
    other = dict(p, start=(0.0, 0.0, -0.5), end=(0.0, 0.0, 0.9))
    out = td.run(gm, sc, probs=[p, other, p])
    assert out["status"][1] == tr.UNDEFINED
    td.assert_equal(out, 0, res[0], sc["cfg"])
    td.assert_equal(out, 2, res[0], sc["cfg"])
