"""CPU checks of the viewpoint path costs: the C-ABI declares and exports fuelmi_map_path_costs, bad arguments are
refused before any device work, and the CPU restatement (tests/path_cost_ref.py) gives the hand-worked answers."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import path_cost_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fuelmi.h")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import fuel_amd
    return fuel_amd


def test_header_declares_path_costs_and_library_exports_it(built):
    src = open(HEADER).read()
    assert re.search(r"typedef struct \{\s*double lattice_res;[^}]*double edge_step;[^}]*double no_path_cost;"
                     r"[^}]*int max_path_points;[^}]*\} fuelmi_path_cfg;", src)
    assert "int fuelmi_map_path_costs(fuelmi_map* m, const fuelmi_path_cfg* cfg, int n," in src
    out = subprocess.check_output(["nm", "-D", "--defined-only", built.LIB_PATH]).decode()
    assert re.search(r" T fuelmi_map_path_costs$", out, flags=re.M)


def test_path_cfg_layout_matches_c(built, tmp_path):
    from fuel_amd import _lib
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fuelmi.h"\n'
                    'int main(){printf("%zu %zu\\n", sizeof(fuelmi_path_cfg), '
                    'offsetof(fuelmi_path_cfg, max_path_points));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_lib.PathCfg), _lib.PathCfg.max_path_points.offset]


def test_null_map_or_config_is_einval(built):
    from fuel_amd import _lib
    L = built.lib()
    cfg = _lib.PathCfg(0.4, 0.1, 1000.0, 16)
    p = np.zeros(3)
    out_d = np.zeros(1)
    out_i = np.zeros(1, dtype=np.int32)
    dp = p.ctypes.data_as(C.POINTER(C.c_double))
    od = out_d.ctypes.data_as(C.POINTER(C.c_double))
    oi = out_i.ctypes.data_as(C.POINTER(C.c_int))
    assert L.fuelmi_map_path_costs(None, C.byref(cfg), 1, dp, dp, od, oi, oi, None) == -1
    assert L.fuelmi_map_path_costs(C.c_void_p(0), None, 1, dp, dp, od, oi, oi, None) == -1


# ---- the restatement on hand-worked maps ---------------------------------------------------------------------------
# 8 x 8 x 4 m at 0.1 m (origin (-4, -4, -1)); the box's z range (0.9, 1.1) leaves one lattice layer for sources at
# z = 1: the cases are planar and can be worked by hand

def _world(wall=None, door=None, unknown_voxels=()):
    from oracle import fuel_oracle as fo
    om = fo.OracleMap((8.0, 8.0, 4.0), (-3.9, -3.9, 0.9), (3.9, 3.9, 1.1))
    om.occ[:] = om.l_min  # all free
    om.infl[:] = 0
    infl = om.infl.reshape(om.nvox)
    if wall is not None:  # inflated voxels x in [-0.1, 0.1), every y (but the door's) and z
        infl[39:41, :, :] = 1
        if door is not None:
            infl[39:41, door[0]:door[1], :] = 0
    occ = om.occ.reshape(om.nvox)
    for v in unknown_voxels:
        occ[v] = om.unknown_value
    return om, pr.PathMap.from_oracle(om)


def test_open_straight_line():
    om, pm = _world()
    p1, p2 = (-2.0, 0.05, 1.0), (2.0, 0.33, 1.02)
    kind, length, path = pr.search_path(pm, om, p1, p2)
    assert kind == 0
    assert length == math.sqrt(4.0 * 4.0 + 0.28 * 0.28 + 0.02 * 0.02) or length == np.linalg.norm(np.subtract(p1, p2))
    assert np.array_equal(path, [p1, p2])


def test_one_door_wall_detour():
    # door: y in [1.5, 2.5) (voxels 55..64).  Lattice from (-1, 0): x = -1 + 0.4 i, y = 0.4 j; the wall can only be
    # crossed inside the door, the lowest crossing being (-0.2, 1.6) -> (0.2, 1.6).  Start -> (-0.2, 1.6): 2 diagonal
    # + 2 straight steps; the crossing: 0.4; (0.2, 1.6) -> p2 = (1, 0) costs again 2 diagonal + 2 straight steps to
    # the goal (1.0, 0.0) (or an equal-length split through (0.6, 0.4) / (1.0, 0.4) and a last straight leg)
    om, pm = _world(wall=True, door=(55, 65))
    p1, p2 = (-1.0, 0.0, 1.0), (1.0, 0.0, 1.0)
    assert not pr.straight_line_safe(pm, om, p1, p2)
    kind, length, path = pr.search_path(pm, om, p1, p2)
    assert kind == 1
    assert abs(length - (4 * math.sqrt(0.32) + 2.0)) < 1e-12
    assert length == pr.path_length(path)
    assert np.array_equal(path[0], p1) and np.array_equal(path[-1], p2)
    for a, b in zip(path[1:-2], path[2:-1]):
        assert pr.edge_ok(pm, a, b)
    assert any(abs(q[0] + 0.2) < 1e-9 and 1.5 <= q[1] < 2.5 for q in path)  # through the door


def test_sealed_room_costs_1000():
    om, pm = _world(wall=True)
    p1, p2 = (-1.0, 0.0, 1.0), (1.0, 0.0, 1.0)
    kind, length, path = pr.search_path(pm, om, p1, p2)
    assert (kind, length) == (2, 1000.0)
    assert np.array_equal(path, [p1, p2])


def test_start_inside_goal_neighbourhood_behind_unknown():
    # one unknown voxel (x 31, y 40, z 20) between p1 (voxel 30) and p2 (voxel 32): the line is blocked, the start
    # itself is a goal node (lattice index 7 vs p2's 8) and no other goal is closer than d + |p2 - node| = 0.25
    om, pm = _world(unknown_voxels=[(31, 40, 20)])
    p1, p2 = (-1.0, 0.0, 1.0), (-0.75, 0.0, 1.0)
    assert not pr.straight_line_safe(pm, om, p1, p2)
    kind, length, path = pr.search_path(pm, om, p1, p2)
    assert kind == 1
    assert length == 0.25
    assert np.array_equal(path, [p1, p2])


def test_heapq_and_csgraph_distances_agree():
    om, pm = _world(wall=True, door=(55, 65))
    lat = pr.Lattice(pm, (-1.0, 0.0, 1.0))
    d1, d2 = lat.dijkstra(), lat.csgraph_dist()
    assert np.array_equal(np.isinf(d1), np.isinf(d2))
    assert np.array_equal(d1[np.isfinite(d1)], d2[np.isfinite(d2)])
