"""The topological path search at its lane-window, stride and cap edges, on the CPU: what the scenes of
topo_cases.edge_scenes() (hand-placed samples, restatement only) and the recorded large graphs `forest10` / `forest14` of
topo_cases.scenes() reach, asserted from the witness trace of the restatement (tests/topo_ref.py), so that a scene that
stops reaching its edge fails here and not silently on the device; the trace changes no result; pruneGraph in the kernel's
synchronous rounds (topo_ref.prune_rounds) leaves the survivors, their order and their neighbours' order of the
reference's restart after every erase, on every graph of these scenes and on some three hundred small random graphs.  The edge scenes run
in `cut` mode on the f32 rounding of their field, the mode the device is compared in (tests/test_topo_limits_gpu.py asserts
the same claims again on the device's own field); the forests in `f64` mode, the mode their fixtures are compared in
(tests/test_topo_path_cpu.py: restatement against fixture, robustness, the kernel's text on the host).

Out of scope, because no scene in this map reaches them:
  the 64-neighbour cap   the densest graph found has 14 neighbours at a node (forests at spacings 8, 10 and 14, 8000
                         samples); the forests here reach 11 and 15
  the 100-node raw path  the longest raw path found has 35 nodes
  the merge cap          nsp + len + nep > 256 needs a shortened path of over 128 points; the longest found has 33
A sameTopoPath call of needConnection compares two paths of three points: in a map of 6.4 x 6.4 x 2.4 m they are under
18.8 m, so pt_num stays under 189 there; the scene `same_long` reaches 202 in pruneEquivalent instead, over two select
paths that share a start point 16 m outside the map."""
import numpy as np
import pytest

import topo_cases as tc
import topo_ref as tr

SCENES, EDGE = tc.scenes(), tc.edge_scenes()
FORESTS = ("forest10", "forest14")
_edge, _forest = {}, {}


def _edge_run(name):
    """(results, traces) of an edge scene in `cut` mode on the f32 rounding of its field"""
    if name not in _edge:
        traces = []
        res = tc.run_ref(EDGE[name], "cut", tc.as_field_array(tc.f32_field(EDGE[name]["blocks"])), traces)
        _edge[name] = (res, traces)
    return _edge[name]


def _forest_run(name):
    if name not in _forest:
        traces = []
        _forest[name] = (tc.run_ref(SCENES[name], traces=traces), traces)
    return _forest[name]


@pytest.mark.parametrize("name", list(EDGE))
def test_edge_scenes_reach_their_edges(name):
    res, traces = _edge_run(name)
    for b, t in enumerate(traces):
        print(name, b, "status", res[b]["status"], "passes", [(p["nd"], [w[1:] for w in p["windows"]][:5], p["committed"])
                                                             for p in t["shortcut"]][:3],
              "sameTopoPath", [(c["pt_num"], c["first_invisible"]) for c in t["same_topo"]][:6])
    tc.check_edge_claims(name, EDGE[name], res, traces)


def test_every_edge_has_its_scene():
    """the claims of check_edge_claims, read across the scenes: every window, stride and cap edge is somewhere"""
    windows = [w for name in EDGE for t in _edge_run(name)[1] for p in t["shortcut"] for w in p["windows"]]
    assert any(w[1:] == (tr.LANES, tr.LANES - 1) for w in windows)        # the last lane
    assert any(w[1] < tr.LANES and w[2] is not None for w in windows)      # a block under lanes that are past nd
    assert any(w[1] == 1 for w in windows)                                # a window of one live lane
    pt = sorted(c["pt_num"] for name in EDGE for t in _edge_run(name)[1] for c in t["same_topo"])
    assert {64, 65, 128, 129} <= set(pt) and pt[0] <= 63 and pt[-1] >= 193
    committed = [p["committed"] for name in EDGE for t in _edge_run(name)[1] for p in t["shortcut"]]
    assert max(committed) == tr.MAX_PATH_POINTS - 2
    nd = [p["nd"] for name in EDGE for t in _edge_run(name)[1] for p in t["shortcut"]]
    assert tr.MAX_DIS_POINTS in nd and tr.MAX_DIS_POINTS + 1 in nd


@pytest.mark.parametrize("name", FORESTS)
def test_forests_reach_their_edges(name):
    res, traces = _forest_run(name)
    g, s = traces[0]["graph"][0], traces[0]["search"][0]
    print(name, {k: v for k, v in g.items() if k != "before"}, s, "lengths", [len(p) for p in res[0]["raw"]],
          [len(p) for p in res[0]["sel"]])
    tc.check_forest_claims(name, SCENES[name], res, traces)
    if name == "forest10":
        # max_raw_path stops the search in its middle: without it the same graph gives more raw paths
        free = tc.run_ref(dict(SCENES[name], cfg=dict(SCENES[name]["cfg"], max_raw_path=300)))[0]
        assert free["counts"][0] > SCENES[name]["cfg"]["max_raw_path"]
        # the max_nodes the host build and the device test cut the graph at: one under it, and where nb_off is clamped
        one_less, two = tc.FOREST10_MAX_NODES
        assert one_less == len(res[0]["nodes"]) - 1
        assert sum(len(n[3]) for n in res[0]["nodes"][:two]) > 4 * two


def test_the_trace_changes_no_result():
    for name, sc in list(EDGE.items()) + [("pillar", SCENES["pillar"]), ("dfs_cap", SCENES["dfs_cap"])]:
        d = tc.as_field_array(tc.f32_field(sc["blocks"]))
        plain = tc.run_ref(sc, "cut", d)
        traced = _edge_run(name)[0] if name in EDGE else tc.run_ref(sc, "cut", d, [])
        for a, b in zip(plain, traced):
            assert tc.discrete(a) == tc.discrete(b) and a["far_visible"] == b["far_visible"], name
            assert repr((a["nodes"], a["raw"], a["filt"], a["sel"], a["sel_length"])) == \
                   repr((b["nodes"], b["raw"], b["filt"], b["sel"], b["sel_length"])), name


def _same_graph(before):
    nodes = [(i, nb) for i, _, nb in before]
    restart = tr.prune_restart(nodes)
    in_rounds, rounds = tr.prune_rounds(nodes)
    assert in_rounds == restart
    return restart, rounds


def test_prune_in_rounds_equals_the_restart_on_the_scenes():
    seen = 0
    for name in list(EDGE) + list(FORESTS):
        res, traces = _edge_run(name) if name in EDGE else _forest_run(name)
        for r, t in zip(res, traces):
            for g in t["graph"]:
                pruned, n = _same_graph(g["before"])
                assert n == g["rounds"]
                # ... and both are what createGraph's own pruneGraph left
                assert pruned == [(i, nb) for i, _, _, nb in r["nodes"]], name
                seen += 1
    assert seen >= len(EDGE) + len(FORESTS)


def test_prune_in_rounds_equals_the_restart_on_random_graphs():
    """graphs as createGraph makes them: guards, and connectors that join two guards each, every list in push_back order;
    every graph holds a guard without a neighbour and a guard with one"""
    rng = np.random.default_rng(20)
    most = graphs = 0
    for _ in range(400):
        n = int(rng.integers(6, 40))
        kinds = [tr.GUARD, tr.GUARD] + [tr.GUARD if rng.random() < 0.45 else tr.CONNECTOR for _ in range(n - 2)]
        nb = [[] for _ in range(n)]
        for i in range(2, n):
            guards = [j for j in range(i) if kinds[j] == tr.GUARD]
            if kinds[i] == tr.CONNECTOR:
                a, b = (int(v) for v in rng.choice(guards, 2, replace=False))
                nb[a].append(i), nb[b].append(i), nb[i].extend((a, b))
        lonely = [i for i in range(2, n) if kinds[i] == tr.GUARD and not nb[i]]
        if len(lonely) < 2:
            continue
        # one of the guards without a neighbour gets one connector, to the start or the end
        kinds.append(tr.CONNECTOR)
        far = int(rng.integers(0, 2))
        nb.append([lonely[0], far])
        nb[lonely[0]].append(n), nb[far].append(n)
        counts = [len(nb[i]) for i in range(2, n) if kinds[i] == tr.GUARD]
        assert 0 in counts and 1 in counts
        _, rounds = _same_graph([(i, kinds[i], nb[i]) for i in range(n + 1)])
        most, graphs = max(most, rounds), graphs + 1
    print("graphs", graphs, "most rounds", most)
    assert graphs >= 200 and most >= 3  # chains that a single round does not take down
