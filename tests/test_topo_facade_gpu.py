"""The facade's TopologyPRM (fuel_amd/facade/path_searching/topo_prm.h) through its driver facade_topo against the C-ABI on
the `pillar` scene with a fixed topo_prm/seed: the class draws from its own default_random_engine the stream
topo_cases.sample_stream restates, so the graph it rebuilds, the three path sets and pathLength must equal
fuelmi_map_topo_paths' outputs on the same map bit for bit; pathToGuidePts against the restatement's
discretizePath(path, pt_num)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import topo_cases as tc
import topo_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
GUIDE_NUM = 9


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def _hex(tokens):
    return np.array([float.fromhex(t) for t in tokens], dtype=np.float64).reshape(-1, 3)


def test_facade_find_topo_paths(tmp_path):
    import fuel_amd
    sc = tc.scenes()["pillar"]
    cfg, p = sc["cfg"], sc["probs"][0]
    gm = fuel_amd.SDFMap(tc.MAP_SIZE, device=0)
    try:
        gm.uploadOccupancy(tc.occupancy(sc["blocks"]))
        gm.setLocalBound((0, 0, 0), tuple(v - 1 for v in tc.NVOX))
        gm.clearAndInflateLocalMap()
        gm.updateESDF3d()
        kw = {k: v for k, v in cfg.items() if k not in ("max_sample_num", "max_path_points", "max_nodes")}
        out = gm.topo_paths([p["start"]], [p["end"]], [sc["samples"]], max_path_points=256,
                            max_nodes=cfg["max_sample_num"] + 2, **kw)
    finally:
        gm.close()
    assert out["status"][0] == tr.OK and len(out["sel"][0]) >= 2
    scen = str(tmp_path / "scen.bin")
    with open(scen, "wb") as f:
        hdr = list(tc.MAP_SIZE) + list(cfg["sample_inflate"]) + [cfg["clearance"], cfg["ratio_to_short"], cfg["max_sample_num"],
                                                                 cfg["max_raw_path"], cfg["max_raw_path2"], cfg["reserve_num"],
                                                                 sc["seed"], GUIDE_NUM, 0.0]
        np.array(hdr, dtype=np.float64).tofile(f)
        tc.occupancy(sc["blocks"]).reshape(-1).tofile(f)
        np.array(list(p["start"]) + list(p["end"]), dtype=np.float64).tofile(f)
    exe = os.path.join(ROOT, "fuel_amd", "facade", "facade_topo")
    run = subprocess.run([exe, scen], check=True, capture_output=True, text=True, timeout=120)
    got = dict(node=[], raw=[], filt=[], sel=[], length=[], guide=[])
    for line in run.stdout.splitlines():
        t = line.split()
        if t[0] == "call":
            got["call"] = (int(t[2]), int(t[3]), float(t[4]))
        elif t[0] == "node":
            got["node"].append((int(t[2]), int(t[3]), _hex(t[4:7])[0], [int(v) for v in t[8:8 + int(t[7])]]))
        elif t[0] == "length":
            got["length"].append(float.fromhex(t[2]))
        elif t[0] in got:
            pts = _hex(t[3:])
            assert len(pts) == int(t[2])
            got[t[0]].append(pts)
    assert got["call"] == (0, tr.OK, cfg["clearance"])
    assert len(got["node"]) == out["n_nodes"][0] == len(out["nodes"][0])
    for a, b in zip(got["node"], out["nodes"][0]):
        assert (a[0], a[1]) == (b[0], b[1]) and _bits(a[2]) == _bits(b[2]) and a[3] == list(b[3])
    for key in ("raw", "filt", "sel"):
        assert len(got[key]) == len(out[key][0]), key
        for a, b in zip(got[key], out[key][0]):
            assert _bits(a) == _bits(b), key
    assert _bits(got["length"]) == _bits(out["sel_length"][0][:len(got["sel"])])
    ref = tr.TopoPRM(tr.Field(tc.ORIGIN, tc.RES, np.zeros(tc.NVOX)), {})
    assert len(got["guide"]) == len(got["sel"])
    for g, path in zip(got["guide"], got["sel"]):
        want = ref.discretize_n([list(q) for q in path], GUIDE_NUM)
        assert len(g) == GUIDE_NUM and _bits(g) == _bits(want)
