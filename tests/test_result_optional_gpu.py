"""The optional result arrays of the staged batch calls: a call without one of them returns every other output bit for
bit as the call with all of them does, at 1 and 2 problems.  host.py passes the topological search's arrays always, and
the yaw planner's and the kinodynamic search's only all together, so the library's function is wrapped here and the
chosen arguments go in as null pointers; the array host.py allocated for one stays as it was made, zero.  Maps, scenes
and configurations are the smallest of each stage's own test file."""
import contextlib
import os
import sys

import numpy as np
import pytest

import kino_ref as kr
import topo_cases as tc
import topo_device as td
import yaw_plan_ref as yr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _close_maps():
    yield
    td.close_maps()


class _Nulled:
    """the library with the arguments at `positions` of function `name` replaced by null pointers"""

    def __init__(self, lib, name, positions):
        self._lib, self._name, self._positions = lib, name, positions

    def __getattr__(self, attr):
        fn = getattr(self._lib, attr)
        if attr != self._name:
            return fn

        def call(*args):
            args = list(args)
            for p in self._positions:
                assert args[p] is not None
                args[p] = None
            return fn(*args)
        return call


@contextlib.contextmanager
def nulled(gm, name, positions):
    lib = gm.L
    gm.L = _Nulled(lib, name, positions)
    try:
        yield
    finally:
        gm.L = lib


def _flat(v):
    if isinstance(v, np.ndarray):
        return v.dtype.str.encode() + v.tobytes()
    if isinstance(v, (list, tuple)):
        return b"[" + b",".join(_flat(x) for x in v) + b"]"
    return repr(v).encode()


def assert_others_same(full, part, dropped):
    """every output but the dropped ones bit for bit; a dropped one was not written"""
    assert set(full) == set(part)
    for k in full:
        if k in dropped:
            assert not np.any(part[k]), k
            assert np.any(full[k]), "%s of the full call is empty: the scene does not exercise it" % k
        else:
            assert _flat(full[k]) == _flat(part[k]), k


# ---- the topological path search: everything behind status, counts, events -------------------------------------------------
# (position in fuelmi_map_topo_paths, the keys of host.py's dict that are made from it)
TOPO_OPTIONAL = {"n_nodes": (15, ("n_nodes", "nodes")), "node_id": (16, ("nodes",)), "node_type": (17, ("nodes",)),
                 "node_xyz": (18, ("nodes",)), "nb_off": (19, ("nodes",)), "nb_ids": (20, ("nodes",)),
                 "raw_paths": (21, ("raw",)), "raw_len": (22, ("raw_len", "raw")), "filt_paths": (23, ("filt",)),
                 "filt_len": (24, ("filt_len", "filt")), "sel_paths": (25, ("sel",)), "sel_len": (26, ("sel_len", "sel")),
                 "sel_length": (27, ("sel_length",))}


@pytest.mark.parametrize("n_prob", [1, 2])
def test_topo_paths_without_optional_arrays(n_prob):
    sc = tc.scenes()["two_pillars_reserve"]  # (leaves a filtered path behind the selection)
    gm, _ = td.device_map(sc["blocks"])
    p0 = sc["probs"][0]
    probs = [p0, dict(p0, start=(-2.0, -0.6, 0.0), end=(2.0, 0.7, 0.2))][:n_prob]
    full = td.run(gm, sc, probs=probs)
    assert full["status"][0] == gm.TOPO_OK and not full["limit"]
    for name, (pos, keys) in TOPO_OPTIONAL.items():
        with nulled(gm, "fuelmi_map_topo_paths", [pos]):
            part = td.run(gm, sc, probs=probs)
        # host.py's lists are cut from several arrays: compared below through the arrays the call did fill
        loose = {"nodes", "raw", "filt", "sel"} & set(keys)
        assert_others_same({k: v for k, v in full.items() if k not in loose},
                           {k: v for k, v in part.items() if k not in loose}, set(keys) - loose)
        if name in ("node_id", "node_type", "node_xyz", "nb_ids"):  # one column of the node tuples
            col = dict(node_id=0, node_type=1, node_xyz=2, nb_ids=3)[name]
            for b in range(n_prob):
                assert len(part["nodes"][b]) == len(full["nodes"][b]) > 0
                for got, want in zip(part["nodes"][b], full["nodes"][b]):
                    for c in range(4):
                        if c == col:
                            assert not np.any(got[c])
                        else:
                            assert _flat(got[c]) == _flat(want[c]), (name, c)
        elif name.endswith("_paths"):  # the lengths stay, the points are not written
            key = name[:-len("_paths")]
            for b in range(n_prob):
                assert [len(p) for p in part[key][b]] == [len(p) for p in full[key][b]]
                assert not any(np.any(p) for p in part[key][b])
    with nulled(gm, "fuelmi_map_topo_paths", [pos for pos, _ in TOPO_OPTIONAL.values()]):
        bare = td.run(gm, sc, probs=probs)
    for k in ("status", "counts", "events", "limit"):
        assert _flat(bare[k]) == _flat(full[k]), k
    assert not bare["n_nodes"].any() and not bare["sel_length"].any() and not bare["raw_len"].any()


# ---- the yaw planner: the control points of the two derivatives, each on its own ------------------------------------------
@pytest.mark.parametrize("n_prob", [1, 2])
def test_plan_yaws_without_derivative_arrays(n_prob):
    import fuel_amd
    gm = fuel_amd.SDFMap((10.0, 8.0, 4.0), (-4.0, -3.0, 0.0), (4.0, 3.0, 2.2), device=0)
    try:
        prs = [yr.problem(yr.curve(12, 3), 0.3, (0.4, 0.1, -0.05), 1.2),
               yr.problem(yr.curve(9, 4), 0.25, (-0.2, 0.0, 0.1), -0.7)][:n_prob]

        def run():
            return gm.plan_yaws([p["ctrl"] for p in prs], [p["dt"] for p in prs], [p["start"] for p in prs],
                                [p["end"] for p in prs], relax_time=0.5)
        full = run()
        assert not full["status"].any()
        for dropped, positions in ((("yawdot_ctrl",), [-2]), (("yawddot_ctrl",), [-1]),
                                   (("yawdot_ctrl", "yawddot_ctrl"), [-2, -1])):
            with nulled(gm, "fuelmi_map_plan_yaws", positions):
                assert_others_same(full, run(), set(dropped))
    finally:
        gm.close()


# ---- the kinodynamic search: the three node arrays, each on its own ---------------------------------------------------------
@pytest.mark.parametrize("n_prob", [1, 2])
def test_kino_paths_without_node_arrays(n_prob):
    import fuel_amd
    sc, near = kr.scenes()["open"], kr.scenes()["near_start"]
    gm = fuel_amd.SDFMap(kr.MAP_SIZE, kr.BOX[0], kr.BOX[1], device=0)
    try:
        gm.uploadOccupancy(kr.occupancy((), ()))
        gm.setLocalBound((0, 0, 0), tuple(v - 1 for v in gm.nvox))
        gm.clearAndInflateLocalMap()
        probs = (sc["probs"] + near["probs"])[:n_prob]

        def run():
            return gm.kino_paths([p["start"] for p in probs], [p["vel"] for p in probs], [p["acc"] for p in probs],
                                 [p["goal"] for p in probs], [p["goal_vel"] for p in probs], **kr.DEFAULTS)
        full = run()
        assert full["n_nodes"][0] > 1 and not full["limit"]
        for key, pos in (("node_state", 13), ("node_input", 14), ("node_duration", 15)):
            with nulled(gm, "fuelmi_map_kino_paths", [pos]):
                part = run()
            assert set(part) == set(full)
            for k in full:
                if k == key:
                    assert [len(v) for v in part[k]] == [len(v) for v in full[k]] and not any(np.any(v) for v in part[k])
                    assert any(np.any(v) for v in full[k])
                else:
                    assert _flat(full[k]) == _flat(part[k]), k
    finally:
        gm.close()
