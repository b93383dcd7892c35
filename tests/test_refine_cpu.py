"""CPU checks of the local tour refinement: the C-ABI declares and exports fuelmi_map_refine_tours, its struct matches
ctypes, bad arguments and the size limits are refused before the map is touched, and the restatement
(tests/refine_ref.py) -- literal Dijkstra against the layer pass, and every rule of the reference by hand."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import refine_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fuelmi.h")
VM, YD, WDIR = 2.0, 60 * 3.1415926 / 180.0, 1.5


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import fuel_amd
    return fuel_amd


def test_header_declares_refine_and_library_exports_it(built):
    src = open(HEADER).read()
    assert re.search(r"typedef struct \{\s*fuelmi_path_cfg path;[^}]*double vm, yd, w_dir;[^}]*double tour_lattice_res;"
                     r"[^}]*int max_tour_points;[^}]*int flags;[^}]*\} fuelmi_refine_cfg;", src)
    assert "int fuelmi_map_refine_tours(fuelmi_map* m, const fuelmi_refine_cfg* cfg, int n_prob," in src
    assert "#define FUELMI_REFINE_LAST_ARGMIN 1" in src
    out = subprocess.check_output(["nm", "-D", "--defined-only", built.LIB_PATH]).decode()
    assert re.search(r" T fuelmi_map_refine_tours$", out, flags=re.M)


def test_refine_cfg_layout_matches_c(built, tmp_path):
    from fuel_amd import _lib
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fuelmi.h"\n'
                    'int main(){printf("%zu %zu %zu %zu %zu %d %d %d\\n", sizeof(fuelmi_refine_cfg), '
                    'offsetof(fuelmi_refine_cfg, vm), offsetof(fuelmi_refine_cfg, tour_lattice_res), '
                    'offsetof(fuelmi_refine_cfg, max_tour_points), offsetof(fuelmi_refine_cfg, flags), '
                    'FUELMI_REFINE_LAST_ARGMIN, FUELMI_REFINE_MAX_LAYERS, FUELMI_REFINE_MAX_NODES);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    R = _lib.RefineCfg
    assert got == [C.sizeof(R), R.vm.offset, R.tour_lattice_res.offset, R.max_tour_points.offset, R.flags.offset,
                   _lib.REFINE_LAST_ARGMIN, _lib.REFINE_MAX_LAYERS, _lib.REFINE_MAX_NODES]


def _call(L, cfg, layer_sizes_per_problem, m=None, nodes=None):
    """fuelmi_map_refine_tours on a NULL map (nothing is touched before the checks pass)"""
    B = len(layer_sizes_per_problem)
    start = np.zeros((B, 7))
    lp, npt = [0], [0]
    for sizes in layer_sizes_per_problem:
        for k in sizes:
            npt.append(npt[-1] + k)
        lp.append(lp[-1] + len(sizes))
    lp = np.array(lp, dtype=np.int32)
    npt = np.array(npt, dtype=np.int32)
    if nodes is None:
        nodes = np.zeros((max(npt[-1], 1), 4))
    choice = np.zeros(max(lp[-1], 1), dtype=np.int32)
    cost = np.zeros(B)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731
    return L.fuelmi_map_refine_tours(m, None if cfg is None else C.byref(cfg), B, dp(start), ip(lp), ip(npt), dp(nodes),
                                     ip(choice), dp(cost), None, None)


def _cfg(vm=VM, yd=YD, flags=0):
    from fuel_amd import _lib
    return _lib.RefineCfg(_lib.PathCfg(0.4, 0.1, 1000.0, 0), vm, yd, WDIR, 0.0, 0, flags)


def test_refusals_before_the_map(built):
    L = built.lib()
    assert _call(L, None, [[3]]) == -1                       # no configuration
    assert _call(L, _cfg(), [[3]]) == -1                     # NULL map, once everything else passed
    assert _call(L, _cfg(vm=0.0), [[3]]) == -1               # vm > 0
    assert _call(L, _cfg(yd=-1.0), [[3]]) == -1              # yd > 0
    assert _call(L, _cfg(), [[3, 0, 2]]) == -1               # an empty layer
    assert _call(L, _cfg(), [[2], []]) == -1                 # a problem without layers
    assert _call(L, _cfg(), [[2] * 65]) == -5                # layers per problem
    assert _call(L, _cfg(), [[2, 257]]) == -5                # nodes per layer
    assert _call(L, _cfg(), [[2] * 64]) == -1                # at the limit: only the NULL map is left
    assert _call(L, _cfg(), [[256, 256]]) == -1
    bad = np.zeros((3, 4))
    bad[1, 2] = 2e7                                          # |coordinate| < 1e7, as path costs
    assert _call(L, _cfg(), [[3]], nodes=bad) == -1
    bad[1, 2] = np.nan
    assert _call(L, _cfg(), [[3]], nodes=bad) == -1


def test_edge_count_limit_before_reading_nodes(built):
    # 64 layers of 256 nodes with the argmin flag: 256 + 63 * 65 536 edges a problem; 521 problems pass 2^31 - 1.
    # The node array is never read (one row suffices): the limit is decided on the two index arrays alone
    L = built.lib()
    sizes = [[256] * 64] * 521
    assert _call(L, _cfg(flags=1), sizes, nodes=np.zeros((1, 4))) == -5
    assert "edges" in L.fuelmi_last_error().decode()


# ---- the restatement ------------------------------------------------------------------------------------------------
def _random_graph(rng, n_layers, width, argmin=False, quantum=None):
    pos = rng.normal(size=3)
    vel = rng.normal(size=3) * (rng.random() < 0.7)
    layers = [np.concatenate([rng.normal(scale=3.0, size=(k, 3)), rng.uniform(-math.pi, math.pi, (k, 1))], axis=1)
              for k in rng.integers(1, width + 1, n_layers)]
    g = rr.Graph(pos, vel, rng.uniform(-math.pi, math.pi), layers, last_argmin=argmin)
    lengths = {}
    for (u, v) in g.edge_pairs():
        d = rr.norm3(*(g.pts[v] - g.pts[u]))
        lengths[(u, v)] = d * (1.0 + 2.0 * rng.random()) if rng.random() < 0.8 else 1000.0
    return g, lengths


def test_literal_dijkstra_equals_layer_pass():
    rng = np.random.default_rng(1)
    n_done = 0
    for trial in range(3000):
        g, lengths = _random_graph(rng, int(rng.integers(1, 6)), 5)
        cost = g.costs(lengths, VM, YD, WDIR)
        a, ca = rr.dijkstra(g, cost)
        b, cb = rr.layer_dp(g, cost)
        assert a == b and ca == cb, trial
        n_done += a is not None
    assert n_done > 2500


def test_single_layer_argmin_is_the_single_destination_branch():
    rng = np.random.default_rng(2)
    for trial in range(500):
        g, lengths = _random_graph(rng, 1, 8, argmin=True)
        cost = g.costs(lengths, VM, YD, WDIR)
        ch, c = rr.layer_dp(g, cost)
        ids = g.layer_ids[0]
        i, ci = rr.single_destination(g.pts[0], g.vel, g.yaws[0], [g.pts[v] for v in ids], [g.yaws[v] for v in ids],
                                      [lengths[(0, v)] for v in ids], VM, YD, WDIR)
        assert (ch[0] if ch else -1) == i and (c if ch else rr.ARGMIN_INIT) == ci, trial


def _one_layer(points, yaws, pos=(0.0, 0.0, 1.0), vel=(0.0, 0.0, 0.0), yaw=0.0, argmin=False, lengths=None):
    layer = np.concatenate([np.asarray(points, dtype=float), np.asarray(yaws, dtype=float)[:, None]], axis=1)
    g = rr.Graph(pos, vel, yaw, [layer], last_argmin=argmin)
    if lengths is None:
        lengths = {(u, v): rr.norm3(*(g.pts[v] - g.pts[u])) for (u, v) in g.edge_pairs()}
    return g, g.costs(lengths, VM, YD, WDIR)


def test_rules_by_hand():
    # ties: the first index of the cheapest (nodes 1 and 2 at distance 1, node 0 at 2)
    pts = [(2.0, 0.0, 1.0), (0.0, 1.0, 1.0), (-1.0, 0.0, 1.0)]
    g, c = _one_layer(pts, [0.0, 0.0, 0.0], argmin=True)
    assert rr.layer_dp(g, c) == ([1], 0.5)
    g, c = _one_layer(pts, [0.0, 0.0, 0.0])  # without the flag only node 0 is kept
    assert rr.layer_dp(g, c) == ([0], 1.0) and len(g.layer_ids[0]) == 1
    # |v| <= 1e-3: no direction term; just above: a term
    g, c = _one_layer([(-1.0, 0.0, 1.0)], [0.0], vel=(1e-3, 0.0, 0.0))
    assert c[(0, 1)] == 0.5
    g, c = _one_layer([(-1.0, 0.0, 1.0)], [0.0], vel=(2e-3, 0.0, 0.0))
    assert c[(0, 1)] == 0.5 + WDIR * math.pi
    # a viewpoint at the start: real Eigen's normalized() leaves the zero vector, acos(0) = pi / 2
    g, c = _one_layer([(0.0, 0.0, 1.0)], [0.0], vel=(0.3, 0.0, 0.0))
    assert c[(0, 1)] == WDIR * (math.pi / 2)
    # yaw wrap across +-pi: 3.1 -> -3.1 is 2 pi - 6.2
    g, c = _one_layer([(0.05, 0.0, 1.0)], [-3.1], yaw=3.1)
    assert c[(0, 1)] == (2 * math.pi - 6.2) / YD
    # a sealed viewpoint: searchPath's 1000
    g, c = _one_layer([(1.0, 0.0, 1.0)], [0.0], lengths={(0, 1): 1000.0})
    assert c[(0, 1)] == 1000.0 / VM
    # a best total >= 1e6 stays unreached (g starts at 1e6, strict <)
    g, c = _one_layer([(1.0, 0.0, 1.0)], [0.0], lengths={(0, 1): 2e6})
    assert rr.layer_dp(g, c) == (None, math.inf) and rr.dijkstra(g, c) == (None, math.inf)
    # argmin: strict < from 1e5
    g, c = _one_layer([(1.0, 0.0, 1.0)], [0.0], lengths={(0, 1): 2.5e5}, argmin=True)
    assert rr.layer_dp(g, c) == (None, math.inf)


def nan_edge(rng, max_len=None):
    """a start velocity v and an offset d = p2 - p1 (d a multiple of v) with v^ . d^ rounding above 1"""
    for _ in range(100000):
        v = rng.normal(size=3)
        d = v * rng.uniform(0.5, 3.0)
        nv, nd = rr.norm3(*v), rr.norm3(*d)
        if max_len is not None and nd > max_len:
            continue
        vd, dd = [v[k] / nv for k in range(3)], [d[k] / nd for k in range(3)]
        if vd[0] * dd[0] + vd[1] * dd[1] + vd[2] * dd[2] > 1.0:
            return v, d
    raise AssertionError("no NaN edge found")


def test_nan_edge_is_never_taken():
    rng = np.random.default_rng(4)
    v, d = nan_edge(rng)
    pos = np.array([0.0, 0.0, 1.0])
    perp = np.array([d[1], -d[0], 0.0])
    far = pos + perp * (4.0 * rr.norm3(*d) / rr.norm3(*perp))  # sideways and farther: the dearer one without the NaN
    g, c = _one_layer([pos + d, far], [0.0, 0.0], pos=pos, vel=v, argmin=True)
    assert math.isnan(c[(0, 1)]) and not math.isnan(c[(0, 2)])
    assert rr.layer_dp(g, c)[0] == [1]
    g0, c0 = _one_layer([pos + d, far], [0.0, 0.0], pos=pos, vel=(0.0, 0.0, 0.0), argmin=True)
    assert rr.layer_dp(g0, c0)[0] == [0]  # without the direction term the near one wins: the NaN flips the choice
    g, c = _one_layer([pos + d], [0.0], pos=pos, vel=v)
    assert rr.layer_dp(g, c) == (None, math.inf) and rr.dijkstra(g, c) == (None, math.inf)


def test_polyline_assembly():
    cur = np.array([0.0, 0.0, 1.0])
    pts = [np.array([1.0, 0.0, 1.0]), np.array([1.0, 0.0, 1.0]), np.array([2.0, 1.0, 1.0])]
    legs = [(1.0, np.array([cur, pts[0]])), (0.0, np.array([pts[0], pts[1]])),
            (1000.0, np.array([pts[1], pts[2]]))]
    out = rr.polyline(cur, pts, legs)
    assert np.array_equal(out, [cur, cur, pts[0], pts[1], pts[1], pts[2]])


def test_viewpoints_info():
    fr = {0: [((0.0, 0.0, 1.0), 0.1, 100), ((3.0, 0.0, 1.0), 0.2, 90), ((4.0, 0.0, 1.0), 0.3, 81),
              ((5.0, 0.0, 1.0), 0.4, 80), ((6.0, 0.0, 1.0), 0.5, 79)],
          1: [((0.1, 0.0, 1.0), 0.6, 10), ((0.2, 0.0, 1.0), 0.7, 9)]}
    P, Y = rr.viewpoints_info((0.0, 0.0, 1.0), fr, [0, 1], 15, 0.8, 0.75)
    assert [list(map(tuple, p)) for p in P] == [[(3.0, 0.0, 1.0), (4.0, 0.0, 1.0)], [(0.1, 0.0, 1.0), (0.2, 0.0, 1.0)]]
    assert Y == [[0.2, 0.3], [0.6, 0.7]]
    P, _ = rr.viewpoints_info((0.0, 0.0, 1.0), fr, [0], 1, 0.8, 0.75)
    assert len(P[0]) == 1
