"""The restatement of the kinodynamic search (tests/kino_ref.py) pinned to the reference's own code, and the host side of
the new calls: the recorded results of the reference's KinodynamicAstar (tests/golden/kino/*.npz, written by
tests/golden/make_kino_golden.py) equal the restatement's bit for bit; every scene tests/test_kino_path_gpu.py uses keeps
its discrete outputs when every libm result is nudged by -4 .. +4 ulp (the largest disagreement of each continuous output
is printed: the GPU test takes 100 x that as its tolerance); the two heap routines equal std::push_heap / std::pop_heap on
keys that are changed in place; the scenes hold what they claim; the host refusals and fuelmi_kino_plan."""
import ctypes as C
import glob
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import kino_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NEW_SYMBOLS = ("fuelmi_map_kino_paths", "fuelmi_bspline_dev_load_kino", "fuelmi_kino_plan")
INT_KEYS = ("allocate_num", "check_num", "optimistic", "min_seg", "seg_num", "max_path_nodes", "max_samples")


def _fixture(path):
    z = np.load(path)
    cfg = dict(zip([str(k) for k in z["cfg_keys"]], [float(v) for v in z["cfg_vals"]]))
    for k in INT_KEYS:
        cfg[k] = int(cfg[k])
    nv = tuple(int(v) for v in z["nvox"])
    n = nv[0] * nv[1] * nv[2]
    km = kr.KMap(z["origin"], kr.MAP_RES, nv, z["map_size"], z["box_mind"], z["box_maxd"],
                 np.unpackbits(z["infl_bits"])[:n], np.unpackbits(z["unk_bits"])[:n])
    probs = [dict(start=p[0], vel=p[1], acc=p[2], goal=p[3], goal_vel=p[4]) for p in z["probs"]]
    return z, km, cfg, probs


FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "kino", "*.npz")))


def test_fixtures_cover_the_scenes():
    names = {os.path.basename(f)[:-4] for f in FIXTURES}
    # forced_seg changes getSamples' rule, which the reference does not have: the restatement stands alone there
    assert names == set(kr.scenes()) - {"forced_seg"}
    for f in FIXTURES:
        assert os.path.getsize(f) < 64 * 1024


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_restatement_equals_the_reference(path):
    z, km, cfg, probs = _fixture(path)
    name = os.path.basename(path)[:-4]
    sc = kr.scenes()[name]
    # the fixture's inputs are the scene's (a drift of either fails here, not on the device)
    ref_map = kr.scene_map(sc)
    assert np.array_equal(ref_map.infl, km.infl) and np.array_equal(ref_map.unk, km.unk)
    assert np.array_equal(ref_map.box_maxd, km.box_maxd)
    assert [tuple(np.asarray(p[k], dtype=float)) for p in sc["probs"] for k in ("start", "vel", "acc", "goal", "goal_vel")] == \
           [tuple(p[k]) for p in probs for k in ("start", "vel", "acc", "goal", "goal_vel")]
    for b, p in enumerate(probs):
        r = kr.solve(km, p, cfg)
        if r["status"] == kr.CLOSE_GOAL:
            continue  # the manager's refusal; the fixture holds what the search itself would have done
        assert [int(v) for v in z["head%d" % b]] == [r["status"], r["which"], r["iter_num"], r["use_node_num"]], (name, b)
        if r["status"] == kr.NO_PATH:
            continue
        nodes = r["nodes"]
        assert np.array_equal(z["index%d" % b], np.array([n["index"] for n in nodes]))
        assert np.array_equal(z["state%d" % b], np.array([n["state"] for n in nodes]))
        assert np.array_equal(z["input%d" % b], np.array([n["input"] for n in nodes]))
        assert np.array_equal(z["duration%d" % b], np.array([n["duration"] for n in nodes]))
        assert int(z["shot%d" % b][0]) == r["shot"]
        assert z["t_shot%d" % b][0] == r["t_shot"] and np.array_equal(z["coef%d" % b], r["coef"])
        assert z["ts%d" % b][0] == r["ts"]
        assert np.array_equal(z["samples%d" % b], r["samples"]) and np.array_equal(z["derivs%d" % b], r["derivs"])


@pytest.mark.parametrize("name", sorted(kr.scenes()))
def test_every_gpu_scene_is_robust(name):
    for b, (r, robust, worst) in enumerate(kr.scene_results(name)):
        print("%s problem %d: status %d, %d pops, %d nodes; plain vs nudged: %s" %
              (name, b, r["status"], r["iter_num"], r["use_node_num"], worst))
        assert robust, (name, b)
        assert all(math.isfinite(v) and v < 1e-9 for v in worst.values()), worst
        # every problem has a start velocity and a goal offset with three distinct non-zero components
        p = kr.scenes()[name]["probs"][b]
        off = np.abs(np.array(p["goal"]) - np.array(p["start"]))
        vel = np.abs(np.array(p["vel"]))
        assert len(set(off.tolist())) == 3 and off.min() > 0 and len(set(vel.tolist())) == 3 and vel.min() > 0


def _assert_robust(tag, probs, results):
    assert len(probs) == len(results) > 0
    for b, (p, (r, robust, worst)) in enumerate(zip(probs, results)):
        print("%s problem %d: status %d, %d pops, %d nodes; plain vs nudged: %s" %
              (tag, b, r["status"], r["iter_num"], r["use_node_num"], worst))
        assert robust, (tag, b)
        assert all(math.isfinite(v) and v < 1e-9 for v in worst.values()), worst
        off = np.abs(np.array(p["goal"]) - np.array(p["start"]))
        vel = np.abs(np.array(p["vel"]))
        assert len(set(off.tolist())) == 3 and off.min() > 0 and len(set(vel.tolist())) == 3 and vel.min() > 0


def test_every_other_gpu_problem_is_robust():
    """the GPU test's problems that are not a scene's: the batch of 65, both loads of the device chain (seg_num forced),
    the facade's MID problem -- every one of them, and what the GPU test says about them holds on the restatement"""
    probs = kr.batch65()
    assert len(probs) == 65 and probs[0] == probs[64] == kr.scenes()["open"]["probs"][0]
    assert len({repr(p) for p in probs}) == 8
    res = kr.problem_results("open", probs)
    _assert_robust("batch65", probs, res)
    assert {r["status"] for r, _, _ in res} == {kr.REACH_END}
    pa, pb = kr.load_problems()
    cfg = dict(seg_num=kr.LOAD_SEG)
    ra, rb = kr.problem_results(kr.LOAD_SCENE, pa, cfg), kr.problem_results(kr.LOAD_SCENE, pb, cfg)
    _assert_robust("load, first", pa, ra)
    _assert_robust("load, second", pb, rb)
    assert all(r["status"] in (kr.REACH_END, kr.NEAR_END, kr.REACH_HORIZON) and r["n_samples"] == kr.LOAD_SEG + 1
               for r, _, _ in ra)
    assert [r["status"] for r, _, _ in rb][1::2] == [kr.NO_PATH, kr.CLOSE_GOAL]
    assert all(r["n_samples"] == kr.LOAD_SEG + 1 for r, _, _ in rb[0::2])
    fp = [kr.facade_problem()]
    rf = kr.problem_results(kr.FACADE_SCENE, fp)
    _assert_robust("facade", fp, rf)
    assert rf[0][0]["status"] in (kr.REACH_END, kr.NEAR_END, kr.REACH_HORIZON)
    d = np.array(fp[0]["goal"]) - np.array(fp[0]["start"])
    assert 1.5 < math.sqrt(d @ d) < 5.0  # a MID problem when the straight path is free


def test_scenes_hold_what_they_claim():
    res = {name: [r for r, _, _ in kr.scene_results(name)] for name in kr.scenes()}
    one = {k: v[0] for k, v in res.items()}
    assert one["open"]["status"] == kr.REACH_END and one["open"]["shot"] == 1 and one["open"]["n_nodes"] > 2
    init_d, inputs, durs = kr.primitives(kr.DEFAULTS)
    assert (len(init_d), len(inputs), len(durs)) == (20, 125, 1)  # 1 x 20, then 125 x 1
    assert one["near_start"]["status"] == kr.REACH_END and one["near_start"]["n_nodes"] == 1
    shot_acc = 2 * one["near_start"]["coef"][:, 2]
    assert np.array_equal(one["near_start"]["derivs"][2], shot_acc)  # start_acc from the shot
    assert (one["pillar_start"]["status"], one["pillar_start"]["which"], one["pillar_start"]["iter_num"]) == (kr.NO_PATH, 1, 0)
    assert one["near_end"]["status"] == kr.NEAR_END and one["near_end"]["shot"] == 0 and one["near_end"]["n_nodes"] > 1
    # the no-shot branch: end_vel is the START node's velocity
    assert np.array_equal(one["near_end"]["derivs"][1], one["near_end"]["nodes"][0]["state"][3:])
    assert one["horizon"]["status"] == kr.REACH_HORIZON and one["horizon"]["shot"] == 0
    assert one["enclosed"]["status"] == kr.NO_PATH and one["enclosed"]["which"] == 1
    assert one["enclosed"]["iter_num"] == one["enclosed"]["use_node_num"] < 100  # the open set ran empty
    at, over = one["alloc_at"], one["alloc_over"]
    assert at["status"] == kr.NO_PATH and at["use_node_num"] == 173 and over["status"] == kr.REACH_END
    assert over["use_node_num"] == 173 == one["open"]["use_node_num"]
    assert one["unknown_pess"]["status"] == one["unknown_opt"]["status"] == kr.REACH_END
    assert one["unknown_pess"]["iter_num"] > one["unknown_opt"]["iter_num"]
    assert one["face_in"]["use_node_num"] == one["face_on"]["use_node_num"] + 1
    assert res["close_goal"][0]["status"] == kr.CLOSE_GOAL and res["close_goal"][1]["status"] == kr.REACH_END
    d = [np.array(p["goal"]) - np.array(p["start"]) for p in kr.scenes()["close_goal"]["probs"]]
    assert math.sqrt(d[0] @ d[0]) < 1e-2 < math.sqrt(d[1] @ d[1]) < 1.02e-2
    assert [r["n_samples"] for r in res["forced_seg"]] == [13, 13]
    # the bookkeeping scene: all three order-dependent events occur
    sc = kr.scenes()["bookkeeping"]
    counts = kr.solve(kr.scene_map(sc), sc["probs"][0], sc.get("cfg"), count=True)["counts"]
    print("bookkeeping scene: %s" % counts)
    assert counts["sibling_f"] > 0 and counts["open_g"] > 0 and counts["stale_pop"] > 0
    # map sizes and searches stay small
    assert max(r["iter_num"] for v in res.values() for r in v) <= 300


def test_heap_routines_are_libstdcxx(tmp_path):
    """push_heap / pop_heap on random keys, with keys changed in place between the operations (the heap is then no
    heap any more: both implementations must still move the same elements)"""
    src = tmp_path / "heap_probe.cpp"
    src.write_text(r'''
#include <algorithm>
#include <cstdio>
#include <vector>
struct N { double f; int id; };
struct Cmp { bool operator()(const N* a, const N* b) const { return a->f > b->f; } };
int main() {
  std::vector<N> pool(4096);
  std::vector<N*> heap;
  int used = 0, op, id;
  double f;
  while (std::scanf("%d %d %lf", &op, &id, &f) == 3) {
    if (op == 0) { pool[used].f = f; pool[used].id = used; heap.push_back(&pool[used]); ++used;
                   std::push_heap(heap.begin(), heap.end(), Cmp()); }
    else if (op == 1) { std::printf("%d\n", heap.front()->id); std::pop_heap(heap.begin(), heap.end(), Cmp()); heap.pop_back(); }
    else pool[id].f = f;
  }
  for (N* n : heap) std::printf("%d\n", n->id);
  return 0;
}
''')
    exe = tmp_path / "heap_probe"
    subprocess.check_call(["g++", "-O1", "-std=c++14", str(src), "-o", str(exe)])
    rng = np.random.default_rng(5)
    for trial in range(4):
        ops, heap, nodes, got = [], [], [], []
        for _ in range(900):
            u = rng.random()
            if u < 0.5 or not heap:
                f = float(rng.integers(0, 40)) if trial % 2 else float(rng.random())  # (many equal keys / none)
                n = kr.Node()
                n.f, n.serial = f, len(nodes)
                nodes.append(n)
                kr.heap_push(heap, n)
                ops.append("0 0 %r" % f)
            elif u < 0.75:
                got.append(heap[0].serial)
                kr.heap_pop(heap)
                ops.append("1 0 0")
            else:
                n = heap[int(rng.integers(0, len(heap)))]
                n.f = float(rng.integers(0, 40)) if trial % 2 else float(rng.random())
                ops.append("2 %d %r" % (n.serial, n.f))
        got += [n.serial for n in heap]
        out = subprocess.run([str(exe)], input="\n".join(ops) + "\n", capture_output=True, text=True, check=True).stdout
        assert [int(v) for v in out.split()] == got, trial


def test_plan_call_and_refusals():
    import fuel_amd
    from fuel_amd.host import kino_cfg
    L = fuel_amd.lib()
    plan = fuel_amd.SDFMap.kino_plan()
    assert plan["lanes"] in (128, 256) and 0 < plan["lds_bytes"] <= 64 * 1024
    assert (plan["n_init"], plan["n_regular"], plan["max_prims"]) == (20, 125, kr.MAX_PRIMS == 256 and 256)
    # 100000 nodes of 128 B plus heap and hash: about 14 MB
    assert plan["hash_slots"] >= 2 * 100000 and plan["hash_slots"] & (plan["hash_slots"] - 1) == 0
    assert plan["workspace_bytes"] == 100000 * 132 + 4 * plan["hash_slots"] and 13e6 < plan["workspace_bytes"] < 15e6
    small = fuel_amd.SDFMap.kino_plan(allocate_num=4096)
    assert small["workspace_bytes"] == 4096 * 132 + 4 * 8192
    out = (C.c_longlong * 8)()
    assert L.fuelmi_kino_plan(C.byref(kino_cfg(time_res_init=1 / 257.0)), out) == -5      # 257 init primitives
    assert L.fuelmi_kino_plan(C.byref(kino_cfg(time_res_init=1 / 256.0)), out) == 0 and out[3] == 256
    assert L.fuelmi_kino_plan(C.byref(kino_cfg(res=1 / 3.0)), out) == -5                  # 7^3 regular primitives
    assert L.fuelmi_kino_plan(C.byref(kino_cfg(time_res=1 / 2.0)), out) == 0 and out[4] == 250
    assert L.fuelmi_kino_plan(C.byref(kino_cfg(time_res=1 / 3.0)), out) == -5             # 125 x 3
    assert L.fuelmi_kino_plan(C.byref(kino_cfg(allocate_num=(1 << 22) + 1)), out) == -5
    for bad in (dict(check_num=0), dict(allocate_num=1), dict(max_tau=0.0), dict(resolution=float("inf")),
                dict(lambda_heu=float("nan")), dict(min_seg=0), dict(seg_num=-1), dict(max_samples=0)):
        assert L.fuelmi_kino_plan(C.byref(kino_cfg(**bad)), out) == -1, bad
    assert L.fuelmi_kino_plan(None, out) == -1
    # a voxel index of any admitted coordinate (|c| < 1e7) must fit an int: 2e7 / resolution < 2^31
    assert L.fuelmi_kino_plan(C.byref(kino_cfg(resolution=0.0094)), out) == 0
    assert L.fuelmi_kino_plan(C.byref(kino_cfg(resolution=0.0093)), out) == -1
    # the primitive lists of the restatement are the host's
    for kw in (dict(), dict(time_res=1 / 2.0), dict(max_acc=1.7, res=1 / 2.0), dict(init_max_tau=0.63, time_res_init=1 / 7.0)):
        assert L.fuelmi_kino_plan(C.byref(kino_cfg(**kw)), out) == 0
        init_d, inputs, durs = kr.primitives(dict(kr.DEFAULTS, **kw))
        assert (out[3], out[4]) == (len(init_d), len(inputs) * len(durs)), kw
    # refusals that need no device: before the map is touched
    args = [None] * 22
    assert L.fuelmi_map_kino_paths(None, C.byref(kino_cfg()), 0, *args) == 0                          # n_prob = 0
    assert L.fuelmi_map_kino_paths(None, C.byref(kino_cfg(time_res_init=1 / 257.0)), 0, *args) == -5
    assert L.fuelmi_map_kino_paths(None, C.byref(kino_cfg(check_num=0)), 0, *args) == -1
    z = np.zeros((300, 3))
    g = z + 1.0
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ins = [dp(z), dp(z), dp(z), dp(g), dp(z)]
    rest = [None] * 17
    # n_prob x workspace over the bound (8 GiB): 300 x 2^22 nodes
    assert L.fuelmi_map_kino_paths(None, C.byref(kino_cfg(allocate_num=1 << 22)), 300, *ins, *rest) == -5
    bad = z.copy()
    bad[7, 1] = np.nan
    assert L.fuelmi_map_kino_paths(None, C.byref(kino_cfg()), 300, dp(bad), dp(z), dp(z), dp(g), dp(z), *rest) == -1
    bad[7, 1] = 1e7
    assert L.fuelmi_map_kino_paths(None, C.byref(kino_cfg()), 300, dp(z), dp(z), dp(z), dp(bad), dp(z), *rest) == -1
    # everything valid but the outputs / the map: still an argument error, nothing dereferenced
    assert L.fuelmi_map_kino_paths(None, C.byref(kino_cfg()), 300, *ins, *rest) == -1


def test_new_symbols_exported_and_declared(tmp_path):
    import fuel_amd
    header = open(os.path.join(ROOT, "include", "fuelmi.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", fuel_amd.LIB_PATH], check=True, capture_output=True,
                              text=True).stdout
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert re.search(r"\bT %s\b" % name, exported), name
    for word, val in (("FUELMI_KINO_REACH_HORIZON", 1), ("FUELMI_KINO_REACH_END", 2), ("FUELMI_KINO_NO_PATH", 3),
                      ("FUELMI_KINO_NEAR_END", 4), ("FUELMI_KINO_CLOSE_GOAL", 5), ("FUELMI_KINO_MAX_PRIMS", 256)):
        m = re.search(r"#define %s (\d+)" % word, header)
        assert m and int(m.group(1)) == val, word
    assert (kr.REACH_HORIZON, kr.REACH_END, kr.NO_PATH, kr.NEAR_END, kr.CLOSE_GOAL) == (1, 2, 3, 4, 5)
    from fuel_amd import _lib
    assert (_lib.KINO_REACH_HORIZON, _lib.KINO_REACH_END, _lib.KINO_NO_PATH, _lib.KINO_NEAR_END, _lib.KINO_CLOSE_GOAL) == \
           (1, 2, 3, 4, 5)
    # the ctypes mirror has the C layout
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fuelmi.h"\n'
                    'int main(){printf("%zu %zu %zu %zu\\n", sizeof(fuelmi_kino_cfg), offsetof(fuelmi_kino_cfg, ts), '
                    'offsetof(fuelmi_kino_cfg, allocate_num), offsetof(fuelmi_kino_cfg, max_samples));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_lib.KinoCfg), _lib.KinoCfg.ts.offset, _lib.KinoCfg.allocate_num.offset,
                   _lib.KinoCfg.max_samples.offset] == [128, 88, 96, 120]
