"""The restatement of the topological path search (tests/topo_ref.py) pinned to the reference's own code, and the host
side of the new calls: the recorded results of the reference's TopologyPRM (tests/golden/topo/*.npz, written by
tests/golden/make_topo_golden.py) equal the restatement's in `f64` mode bit for bit; the scenes hold what they claim;
with the field replaced by its f32 rounding nudged by -2 .. +2 ulp the restatement in `cut` mode keeps every discrete
output of every scene (the largest position disagreement is printed: the GPU test takes 100 x that as the tolerance of a
pushed point); the new symbols, fuelmi_topo_plan and the host refusals.  The scenes `undefined` and `overflow` stand alone:
the reference cannot express them (topo_cases.NOT_RECORDED)."""
import ctypes as C
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import topo_cases as tc
import topo_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "topo")
NEW_SYMBOLS = ("fuelmi_map_topo_paths", "fuelmi_topo_plan")
SCENES = tc.scenes()
_runs = {}


def _ref(name):
    if name not in _runs:
        _runs[name] = tc.run_ref(SCENES[name])
    return _runs[name]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def test_fixtures_cover_the_scenes():
    have = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))
    assert have == sorted(n for n in SCENES if n not in tc.NOT_RECORDED)
    for p in glob.glob(os.path.join(GOLDEN, "*.npz")):
        assert os.path.getsize(p) < 64 * 1024, p


@pytest.mark.parametrize("name", [n for n in SCENES if n not in tc.NOT_RECORDED])
def test_restatement_equals_the_reference(name):
    z, sc = np.load(os.path.join(GOLDEN, name + ".npz")), SCENES[name]
    # the fixture's inputs are the scene's: the sources, the parameters, the stream the reference's engine gave
    n = int(np.prod(tc.NVOX))
    assert np.array_equal(np.unpackbits(z["source_bits"])[:n].reshape(tc.NVOX).astype(bool), tc.sources(sc["blocks"]))
    cfg = dict(zip([str(k) for k in z["cfg_keys"]], [float(v) for v in z["cfg_vals"]]))
    assert all(float(sc["cfg"][k]) == v for k, v in cfg.items())
    assert _bits(z["sample_inflate"]) == _bits(sc["cfg"]["sample_inflate"])
    assert _bits(z["samples"]) == _bits(sc["samples"])
    assert int(z["n_prob"]) == len(sc["probs"])
    for b, r in enumerate(_ref(name)):
        assert r["status"] in (tr.OK, tr.NO_PATH)
        assert [x[0] for x in r["nodes"]] == list(z["node_id%d" % b])
        assert [x[1] for x in r["nodes"]] == list(z["node_type%d" % b])
        assert _bits([x[2] for x in r["nodes"]]) == _bits(z["node_pos%d" % b])
        assert [i for x in r["nodes"] for i in x[3]] == list(z["nb_ids%d" % b])
        assert list(np.cumsum([0] + [len(x[3]) for x in r["nodes"]])) == list(z["nb_off%d" % b])
        for key in ("raw", "filt", "sel"):
            assert [len(p) for p in r[key]] == list(z[key + "_len%d" % b]), key
            assert _bits([q for p in r[key] for q in p]) == _bits(z[key + "_pts%d" % b]), key
        assert _bits(r["sel_length"]) == _bits(z["sel_length%d" % b])
        # (selectShortPaths erases what it takes from the filtered set the caller gets back)
        assert r["counts"][1] == len(z["raw_len%d" % b]) and r["counts"][3] == len(z["sel_len%d" % b])
        assert r["counts"][2] >= len(z["filt_len%d" % b]) + r["counts"][3]
        assert (r["status"] == tr.NO_PATH) == (len(z["sel_len%d" % b]) == 0)


def test_scenes_hold_what_they_claim():
    ev = lambda name: dict(zip(tr.EVENTS, _ref(name)[0]["events"]))
    r = _ref("free")[0]
    assert r["counts"] == [1, 1, 1, 1] and ev("free")["connectors"] == 1 and ev("free")["guards"] == 0
    assert len(r["sel"][0]) == 2  # the straight line
    r = _ref("pillar")[0]
    assert r["counts"][2] >= 2 and r["counts"][3] >= 2  # two classes survive both prunes
    r = _ref("two_pillars")[0]
    assert r["counts"][2] == 3 and r["counts"][3] == 3 and r["counts"][1] > r["counts"][2]
    assert _ref("two_pillars_reserve")[0]["counts"][2:] == [3, 2]  # reserve_num cuts one
    assert _ref("two_pillars_ratio")[0]["counts"][2:] == [3, 1]    # ratio_to_short cuts two
    r = _ref("blocked")[0]
    assert r["status"] == tr.NO_PATH and r["counts"] == [0, 0, 0, 0]
    chunk = 64
    r = _ref("comb")[0]
    assert 2 + ev("comb")["guards"] > chunk + 3 and r["far_visible"] > 0  # a visible guard past the first chunk
    assert ev("moved")["moved"] > 0
    assert ev("rollback")["rollbacks"] > 0 and sum(map(sum, _ref("rollback")[0]["sel_pushed"])) > 0
    # adjacent: decisions on values equal to their thresholds, k = 1 (res) and k = kmax(clearance) = 4
    sc = SCENES["adjacent"]
    f = tr.Field(tc.ORIGIN, tc.RES, tc.field_of(sc["blocks"]))
    p = sc["probs"][0]
    tr.find_topo_paths(f, sc["cfg"], p["start"], p["end"], sc["samples"])
    assert tr.kmax(tc.RES, tc.RES) == 1 and tr.kmax(tc.RES, sc["cfg"]["clearance"]) == 4 and tr.kmax(tc.RES, 0.0) == 0
    assert f.at_thresh.get(tc.RES, 0) > 0 and f.at_thresh.get(sc["cfg"]["clearance"], 0) > 0
    # ... which the device's widened f32 values would decide the other way without the cut
    assert float(np.float32(tc.RES)) > tc.RES
    sc = SCENES["dfs_cap"]
    r = _ref("dfs_cap")[0]
    free_run = tc.run_ref(dict(sc, cfg=dict(sc["cfg"], max_raw_path=300, max_raw_path2=25)))[0]
    assert r["counts"][0] == sc["cfg"]["max_raw_path"] < free_run["counts"][0]
    assert r["counts"][1] == sc["cfg"]["max_raw_path2"] < r["counts"][0]
    r = _ref("merge")[0]
    p = SCENES["merge"]["probs"][0]
    # (a path's last point is discretizeLine's p1 + dir * n / n: the end point within an ulp or two)
    assert all(_bits(s[0]) == _bits(p["start_pts"][0]) and np.allclose(s[-1], p["end_pts"][-1], rtol=0, atol=1e-12)
               for s in r["sel"])
    assert sum(map(sum, r["sel_pushed"])) > 0
    assert _ref("undefined")[0]["status"] == tr.UNDEFINED
    r = _ref("overflow")[0]
    assert r["status"] == tr.OK and max(len(s) for s in r["sel"]) > SCENES["overflow"]["cfg"]["max_path_points"]


@pytest.mark.parametrize("name", list(SCENES))
def test_every_scene_is_robust(name):
    ok, worst = tc.robustness(name)
    print("%s: largest position disagreement under -2 .. +2 ulp of the f32 field: %.3e" % (name, worst))
    assert ok, name


def test_plan_call_and_refusals():
    import fuel_amd
    from fuel_amd.host import topo_cfg
    L = fuel_amd.lib()
    plan = fuel_amd.SDFMap.topo_plan()
    assert plan["lanes"] == 64 and plan["guard_chunk"] == 64 and 0 < plan["lds_bytes"] <= 64 * 1024
    assert (plan["max_path_points"], plan["max_dis_points"], plan["max_neighbors"], plan["undefined_raw_nodes"]) == \
           (tr.MAX_PATH_POINTS, tr.MAX_DIS_POINTS, tr.MAX_NEIGHBORS, tr.RAW_NODES)
    small = fuel_amd.SDFMap.topo_plan(max_sample_num=300)
    assert 0 < small["workspace_bytes"] < plan["workspace_bytes"] < 1 << 20
    out = (C.c_longlong * 12)()
    for over in (dict(max_sample_num=8191), dict(max_raw_path=4097), dict(max_raw_path2=4097), dict(reserve_num=4097),
                 dict(max_path_points=257), dict(max_nodes=8193)):
        assert L.fuelmi_topo_plan(C.byref(topo_cfg(**over)), out) == -5, over
    for bad in (dict(clearance=-0.1), dict(clearance=float("nan")), dict(sample_inflate=(1.0, float("inf"), 1.0)),
                dict(sample_inflate=(1e7, 1.0, 1.0)), dict(max_raw_path=0), dict(max_raw_path2=0), dict(reserve_num=0),
                dict(max_path_points=0), dict(max_nodes=1), dict(max_sample_num=-1), dict(ratio_to_short=float("nan"))):
        assert L.fuelmi_topo_plan(C.byref(topo_cfg(**bad)), out) == -1, bad
    assert L.fuelmi_topo_plan(None, out) == -1
    # refusals before the map is touched
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    n = 3
    st, en, smp = np.zeros((n, 3)), np.ones((n, 3)), np.zeros((n, 4, 3))
    iv = [np.zeros(n * 6, dtype=np.int32) for _ in range(3)]
    cfg = topo_cfg(max_sample_num=4)

    def call(n_prob=n, st=st, en=en, smp=smp, cfg=cfg, ms=0, nsp=None, sp=None):
        return L.fuelmi_map_topo_paths(None, C.byref(cfg), n_prob, dp(st), dp(en), ms, nsp, sp, 0, None, None, dp(smp),
                                       ip(iv[0]), ip(iv[1]), ip(iv[2]), *([None] * 13))
    assert call(n_prob=0) == 0
    assert call(n_prob=-1) == -1
    assert call(cfg=topo_cfg(max_sample_num=4, max_raw_path=5000)) == -5
    assert call(ms=65) == -5
    for v in (np.nan, np.inf, 1e7, -1e7):
        bad = st.copy()
        bad[1, 2] = v
        assert call(st=bad) == -1 and call(en=bad) == -1, v
    for v in (1.0, -1.0000001, np.nan):
        bad = smp.copy()
        bad[2, 3, 1] = v
        assert call(smp=bad) == -1, v
    nsp, sp = np.array([1, 2, 1], dtype=np.int32), np.zeros((n, 1, 3))
    assert call(ms=1, nsp=ip(nsp), sp=dp(sp)) == -1          # a count over the stride
    # the workspace bound, refused before the map is looked at: one problem of the largest path caps takes over 50 MB, so
    # 200 of them are over FUELMI_TOPO_MAX_WORKSPACE and 100 are not (those go on to the missing map)
    big = topo_cfg(max_sample_num=4, max_raw_path=4096, max_raw_path2=4096, reserve_num=4096)
    per = fuel_amd.SDFMap.topo_plan(max_sample_num=4, max_raw_path=4096, max_raw_path2=4096, reserve_num=4096)
    assert 100 * per["workspace_bytes"] <= per["max_workspace"] < 200 * per["workspace_bytes"]
    for nb, want in ((200, -5), (100, -1)):
        zs, ze, zsmp = np.zeros((nb, 3)), np.ones((nb, 3)), np.zeros((nb, 4, 3))
        ziv = [np.zeros(nb * 6, dtype=np.int32) for _ in range(3)]
        assert L.fuelmi_map_topo_paths(None, C.byref(big), nb, dp(zs), dp(ze), 0, None, None, 0, None, None, dp(zsmp),
                                       ip(ziv[0]), ip(ziv[1]), ip(ziv[2]), *([None] * 13)) == want, nb
    # everything valid but the map: still an argument error, nothing dereferenced
    assert call() == -1


def test_new_symbols_exported_and_declared(tmp_path):
    import fuel_amd
    from fuel_amd import _lib
    header = open(os.path.join(ROOT, "include", "fuelmi.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", fuel_amd.LIB_PATH], check=True, capture_output=True,
                              text=True).stdout
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert re.search(r"\bT %s\b" % name, exported), name
    for word, val in (("FUELMI_TOPO_OK", 0), ("FUELMI_TOPO_NO_PATH", 1), ("FUELMI_TOPO_UNDEFINED", 2),
                      ("FUELMI_TOPO_MAX_PATH_POINTS", tr.MAX_PATH_POINTS), ("FUELMI_TOPO_MAX_DIS_POINTS", tr.MAX_DIS_POINTS),
                      ("FUELMI_TOPO_MAX_NEIGHBORS", tr.MAX_NEIGHBORS)):
        m = re.search(r"#define %s (\d+)" % word, header)
        assert m and int(m.group(1)) == val, word
    assert (_lib.TOPO_OK, _lib.TOPO_NO_PATH, _lib.TOPO_UNDEFINED) == (tr.OK, tr.NO_PATH, tr.UNDEFINED) == (0, 1, 2)
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fuelmi.h"\n'
                    'int main(){printf("%zu %zu %zu %zu\\n", sizeof(fuelmi_topo_cfg), offsetof(fuelmi_topo_cfg, clearance), '
                    'offsetof(fuelmi_topo_cfg, max_sample_num), offsetof(fuelmi_topo_cfg, max_nodes));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_lib.TopoCfg), _lib.TopoCfg.clearance.offset, _lib.TopoCfg.max_sample_num.offset,
                   _lib.TopoCfg.max_nodes.offset] == [64, 24, 40, 60]


def test_kernel_text_on_the_host_under_the_sanitizers():
    """tests/golden/check_topo_host_build.py as a child process: k_topo_path's own text, a thread per lane, under the address
    and undefined-behaviour sanitizers, equals the restatement in `cut` mode on every scene and every edge scene
    (topo_cases.edge_scenes), on the f32 field and on it moved by +2 ulp, and on `forest10` cut at two more max_nodes (the
    only check of the kernel's barriers that needs no device)"""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "check_topo_host_build.py")],
                       capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    lines = p.stdout.splitlines()
    want = 2 * (len(SCENES) + len(tc.edge_scenes())) + len(tc.FOREST10_MAX_NODES)
    assert len(lines) == want and all(l.endswith("identical") for l in lines), lines
