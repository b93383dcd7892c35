"""The restatement of the kinodynamic search (tests/kino_ref.py) pinned to the reference's own code, and the host side of
the new calls: the recorded results of the reference's KinodynamicAstar (tests/golden/kino/*.npz, written by
tests/golden/make_kino_golden.py) equal the restatement's bit for bit; every scene tests/test_kino_path_gpu.py uses keeps
its discrete outputs when every libm result is nudged by -4 .. +4 ulp (the largest disagreement of each continuous output
is printed: the GPU test takes 100 x that as its tolerance); the two heap routines equal std::push_heap / std::pop_heap on
keys that are changed in place; the scenes hold what they claim -- the edge scenes on the restatement's counters (the
init and regular lists at their wave and workgroup edges, tables that collide and wrap, a pool that runs out in a
four-wave expansion, starts and goals the search refuses, getSamples at its sample-count edges), fixtures by rule; the host
refusals and fuelmi_kino_plan."""
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
    # by rule: a scene that changes what the reference holds constant -- res, time_res, time_res_init of search(), seg_num
    # (getSamples has no such argument) and min_seg (a literal 8 in getSamples) -- has no fixture, the restatement
    # stands alone there; every other scene has one
    assert kr.NOT_IN_REFERENCE == ("res", "time_res", "time_res_init", "seg_num", "min_seg")
    sc = kr.scenes()
    assert names == {n for n in sc if not any(k in sc[n].get("cfg", {}) for k in kr.NOT_IN_REFERENCE)}
    assert names >= {"tight_near_end", "tight16", "tight2", "tight8", "tight9", "check1", "ts_long_shot", "ts_long_noshot"}
    assert names >= set(kr.REFUSED) and "forced_seg" not in names and len(names) == 26
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


# ---- the edges: lanes and waves, the hash table, the pool, getSamples -----------------------------------------------------
_counted = {}


def _counts(name):
    """(result, counters) of a scene's first problem, run once more with the counters on"""
    if name not in _counted:
        sc = kr.scenes()[name]
        r = kr.solve(kr.scene_map(sc), sc["probs"][0], sc.get("cfg"), count=True)
        plain = kr.scene_results(name)[0][0]
        # the counters and the table model change nothing: the same result bit for bit
        assert kr.discrete(r) == kr.discrete(plain) and all(v == 0.0 for v in kr.disagreement(r, plain).values()), name
        _counted[name] = (r, r["counts"])
    return _counted[name]


def test_table_model_is_the_kernels_table():
    """the hash in 32-bit unsigned arithmetic (negative indices included), the table size against fuelmi_kino_plan, and
    linear probing with its wrap on a table filled by hand"""
    import fuel_amd
    rng = np.random.default_rng(3)
    keys = np.concatenate([rng.integers(-2000, 2000, (200, 3)), [[-1, -1, -1], [0, 0, 0], [-44, 25, 10], [2 ** 31 - 1, -2 ** 31, 7]]])
    with np.errstate(over="ignore"):
        u = keys.astype(np.int64).astype(np.uint32)
        want = (u[:, 0] * np.uint32(73856093)) ^ (u[:, 1] * np.uint32(19349663)) ^ (u[:, 2] * np.uint32(83492791))
    assert [kr.voxel_hash(tuple(k)) for k in keys] == [int(v) for v in want]
    for alloc in (2, 8, 9, 16, 17, 200, 256, 257, 512, 1024, 2029, 2040, 2048, 2049, 4096):
        assert kr.table_slots(alloc) == fuel_amd.SDFMap.kino_plan(allocate_num=alloc)["hash_slots"], alloc
    assert [kr.table_slots(a) for a in (2, 8, 9, 16, 200, 2040)] == [16, 16, 32, 32, 512, 4096]
    # three keys with the last slot as their home: the second wraps to slot 0, the third to slot 1
    t = kr.TableModel(8)
    home = [k for k in ((x, y, 0) for x in range(-40, 40) for y in range(-40, 40)) if kr.voxel_hash(k) & 15 == 15][:3]
    nodes = []
    for k in home:
        n = kr.Node()
        n.index, n.closed = k, len(nodes) == 1
        nodes.append(n)
        t.insert(n)
    assert [t.slot[15], t.slot[0], t.slot[1]] == nodes
    assert (t.c["displaced"], t.c["longest_probe"], t.c["wraps"]) == (2, 2, 2)
    assert [t.lookup(k) for k in home] == nodes and t.lookup((1000, 1000, 1000)) in (None,)
    assert (t.c["found_closed_displaced"], t.c["found_open_displaced"], t.c["lookup_wraps"]) == (1, 1, 2)


def test_init_lists_reach_their_wave_edges():
    book = _counts("bookkeeping")[0]
    for n in kr.INIT_LISTS:
        name = "init%d" % n
        sc = kr.scenes()[name]
        r, c = _counts(name)
        w = c["waves"]["init"]
        print("%s: %d pops, %d nodes, init expansion %s" % (name, r["iter_num"], r["use_node_num"], w))
        assert len(kr.primitives(dict(kr.DEFAULTS, **sc["cfg"]))[0]) == n
        assert sc["probs"] == kr.scenes()["bookkeeping"]["probs"] and sc["blocks"] == kr.scenes()["bookkeeping"]["blocks"]
        assert r["status"] == kr.REACH_END and 353 <= r["use_node_num"] <= 387 and r["n_nodes"] == book["n_nodes"]
        if n in (64, 65, 256):
            assert 368 <= r["use_node_num"] <= 387
        last = (n - 1) // kr.WAVE
        assert all(v == 0 for v in w["sibling_f"][last + 1:]) and w["open_g"] == [0, 0, 0, 0]
        assert w["sibling_f_cross"][0] == 0
        if n > 1:
            assert w["sibling_f"][last] > 0  # the list's last wave takes part
        for k in range(1, last + 1):     # and in every wave past the first a sibling's first lane is in an earlier wave
            assert w["sibling_f_cross"][k] >= 1, (name, k)
    assert sum(_counts("init256")[1]["waves"]["init"]["sibling_f"]) == 252
    assert _counts("init1")[1]["waves"]["init"]["sibling_f"] == [0, 0, 0, 0]


def test_regular_lists_reach_their_wave_edges():
    import fuel_amd
    for name, (n, cfg) in kr.REG_LISTS.items():
        sc = kr.scenes()[name]
        assert sc["cfg"] == cfg
        _, inputs, durs = kr.primitives(dict(kr.DEFAULTS, **cfg))
        plan_cfg = {k: v for k, v in cfg.items() if k != "allocate_num"}
        assert len(inputs) * len(durs) == n == fuel_amd.SDFMap.kino_plan(**plan_cfg)["n_regular"], name
        r, c = _counts(name)
        w = c["waves"]["reg"]
        print("%s: status %d, search %d, %d pops, %d nodes, regular expansions %s, tables %s" %
              (name, r["status"], r["which"], r["iter_num"], r["use_node_num"], w, c["tables"]))
        last = (n - 1) // kr.WAVE
        assert all(v == 0 for k in w for v in w[k][last + 1:])
    assert [len(kr.primitives(dict(kr.DEFAULTS, **kr.REG_LISTS[k][1]))[2]) for k in ("reg1x8", "reg27x2")] == [8, 2]
    head = lambda name: tuple(_counts(name)[0][k] for k in ("status", "which", "iter_num", "use_node_num"))  # noqa: E731
    assert head("reg64") == (kr.REACH_END, 0, 70, 523) and head("reg216") == (kr.REACH_END, 0, 117, kr.REG216_NODES)
    assert head("reg256_open") == (kr.REACH_END, 0, 3, 276)
    # full pool, deep heap: both searches of these run until the pool of 1024 is used up
    for name in ("reg128", "reg250", "reg256"):
        r, c = _counts(name)
        assert (r["status"], r["which"], r["use_node_num"]) == (kr.NO_PATH, 1, 1024) and r["iter_num"] > 100
        assert [t["inserts"] for t in c["tables"]] == [1024, 1024]
    # both order-dependent events occur for primitives in the last wave the list reaches.  With one duration of 0.8 s
    # and inputs 0.8 m/s^2 apart two primitives of reg216 end 0.256 m apart, never in one voxel: it has no sibling_f at
    # all, and its last wave (the largest x input) finds no open node with a larger g on the way out.  reg216_back (the
    # way back: that wave brakes) has the open_g events, reg216_tau (durations of 0.4 s) both kinds.
    for name in ("reg128", "reg216_tau", "reg250", "reg256"):
        w = _counts(name)[1]["waves"]["reg"]
        last = (kr.REG_LISTS[name][0] - 1) // kr.WAVE
        assert w["sibling_f"][last] > 0 and w["open_g"][last] > 0, (name, w)
        assert w["sibling_f_cross"][last] > 0, (name, w)
    assert _counts("reg216_back")[1]["waves"]["reg"]["open_g"][3] > 0
    assert _counts("reg216")[1]["waves"]["reg"]["sibling_f"] == [0, 0, 0, 0]
    assert _counts("reg216")[1]["waves"]["reg"]["open_g"][2] > 0
    w = _counts("reg256_open")[1]["waves"]["reg"]
    assert all(v > 0 for v in w["sibling_f"]) and w["sibling_f_cross"][3] > 0
    # the pool runs out in the middle of a later four-wave expansion, and one node later it does not
    at, over, full = _counts("reg216_at"), _counts("reg216_over")[0], _counts("reg216")[0]
    assert at[1]["tables"][0]["inserts"] == kr.REG216_NODES and at[0]["which"] == 1
    assert kr.scenes()["reg216_at"]["cfg"]["allocate_num"] + 1 == kr.scenes()["reg216_over"]["cfg"]["allocate_num"]
    assert kr.discrete(over) == kr.discrete(full) and over["use_node_num"] == kr.REG216_NODES


def test_tight_tables_collide_and_wrap():
    tab = {}
    for name in kr.TIGHT:
        r, c = _counts(name)
        tab[name] = c["tables"]
        print("%s: status %d, search %d, %d nodes, tables %s" % (name, r["status"], r["which"], r["use_node_num"], c["tables"]))
    t, = tab["tight216"]
    assert (t["slots"], t["inserts"], t["displaced"], t["longest_probe"], t["wraps"]) == (4096, kr.REG216_NODES, 502, 22, 1)
    assert t["wraps"] >= 1 and t["longest_probe"] >= 8 and t["displaced"] > 0.1 * t["inserts"]
    assert kr.REG216_NODES < kr.scenes()["tight216"]["cfg"]["allocate_num"] <= 2048
    t, = tab["tight_near_end"]
    assert (t["slots"], t["inserts"], t["displaced"], t["longest_probe"]) == (512, 143, 37, 3)
    assert 144 <= kr.scenes()["tight_near_end"]["cfg"]["allocate_num"] <= 256
    first, retry = tab["tight16"]
    assert (retry["slots"], retry["inserts"], retry["displaced"], retry["longest_probe"], retry["wraps"]) == (32, 16, 4, 3, 1)
    for a, slots in ((2, 16), (8, 16), (9, 32), (16, 32)):  # fewer slots than lanes; the pool runs out in the first expansion
        r = _counts("tight%d" % a)[0]
        assert (r["status"], r["which"], r["iter_num"], r["use_node_num"]) == (kr.NO_PATH, 1, 1, a)
        assert [t["slots"] for t in tab["tight%d" % a]] == [slots, slots] and slots < kr.LANES
        assert [t["inserts"] for t in tab["tight%d" % a]] == [a, a]
    # the retry finds a path on a table shorter than the workgroup that the first search had filled to its pool's end
    r = _counts("retry_short_table")[0]
    first, retry = tab["retry_short_table"]
    assert (r["status"], r["which"], r["shot"]) == (kr.REACH_END, 1, 1) and r["n_nodes"] >= 4
    assert first["slots"] == 128 < kr.LANES and first["inserts"] == 64 and 32 < retry["inserts"] == r["use_node_num"] < 64
    assert retry["displaced"] >= 4 and retry["longest_probe"] >= 4
    closed = sum(t["found_closed_displaced"] for v in tab.values() for t in v)
    opened = sum(t["found_open_displaced"] for v in tab.values() for t in v)
    print("lookups through a displaced slot in the tight scenes: %d find a closed node, %d an open one" % (closed, opened))
    assert closed >= 1 and opened >= 1
    # (what the scenes from before hold, for the record)
    old = [t for n in ("open", "near_end", "bookkeeping", "alloc_at") for t in _counts(n)[1]["tables"]]
    print("open, near_end, bookkeeping, alloc_at: longest probe %d, %d wraps" %
          (max(t["longest_probe"] for t in old), sum(t["wraps"] for t in old)))
    assert sum(t["wraps"] for t in old) == 0


def test_refused_starts_and_goals():
    res = {n: _counts(n) for n in kr.REFUSED}
    org_x = -kr.MAP_SIZE[0] / 2.0
    r, c = res["start_out_of_box"]   # no primitive survives, twice
    assert (r["status"], r["which"], r["iter_num"], r["use_node_num"]) == (kr.NO_PATH, 1, 1, 1)
    assert c["tables"][0]["lookups"] == 0  # the init list: every primitive ends outside the box
    p = kr.scenes()["start_out_of_box"]["probs"][0]
    assert org_x < p["start"][0] < kr.BOX[0][0]
    r, c = res["start_out_of_map"]   # negative voxel indices in the table and on the path
    p = kr.scenes()["start_out_of_map"]
    assert p["box"][0][0] < p["probs"][0]["start"][0] < org_x
    assert r["status"] == kr.REACH_END and r["nodes"][0]["index"][0] < 0 <= r["nodes"][1]["index"][0]
    assert c["tables"][0]["lookups"] > 0 and c["tables"][0]["negative"] > 1  # the start and nodes of the init expansion
    r, _ = res["goal_out_of_map"]    # below the origin no shot passes
    assert kr.scenes()["goal_out_of_map"]["probs"][0]["goal"][0] < org_x
    assert (r["status"], r["shot"]) == (kr.NEAR_END, 0)
    r, _ = res["goal_past_size"]     # past the far face, below the SIZE: the reference lets the shot pass
    assert -org_x < kr.scenes()["goal_past_size"]["probs"][0]["goal"][0] < kr.MAP_SIZE[0]
    assert (r["status"], r["shot"]) == (kr.REACH_END, 1)
    r, _ = res["check1"]             # only the primitive's end is tested: the path crosses the wall
    assert r["status"] == kr.REACH_END and r["iter_num"] < _counts("bookkeeping")[0]["iter_num"]
    sc = kr.scenes()["check1"]
    km = kr.scene_map(sc)
    hit = False
    for a, b in zip(r["nodes"][:-1], r["nodes"][1:]):
        dt = np.linspace(0.0, b["duration"], 41)
        hit |= bool(km.inflated(kr.Search.transit(a["state"], np.repeat(b["input"][None, :], 41, axis=0), dt)[:, :3]).any())
    assert hit


def test_get_samples_edges():
    for w, base in (("shot", "bookkeeping"), ("noshot", "near_end")):
        full = kr.scene_results(base)[0][0]
        assert full["shot"] == (w == "shot") and full["n_nodes"] >= 4
        dur = [n["duration"] for n in full["nodes"]]
        res = {k: kr.scene_results("%s_%s" % (k, w))[0][0] for k in
               ("seg1", "seg2", "seg1000_at", "seg1000_over", "minseg_above", "minseg_below", "ts_long")}
        for k, r in res.items():  # the search is the same; only the sampling differs
            assert kr.discrete(r)[1:5] == kr.discrete(full)[1:5] and r["T_sum"] == full["T_sum"], (k, w)
        assert (res["seg1"]["seg_num"], res["seg1"]["n_samples"]) == (1, 2)
        assert (res["seg2"]["seg_num"], res["seg2"]["n_samples"]) == (2, 3)
        # one sample spans several path nodes: the step is longer than two whole nodes and the shot, so the time stays
        # negative after one node's duration is added; with two segments it is longer than the last node and the shot
        assert res["seg1"]["ts"] == full["T_sum"] > dur[-1] + dur[-2] + full["t_shot"] + 0.5
        assert res["seg2"]["ts"] > dur[-1] + full["t_shot"] + 0.4
        at, over = res["seg1000_at"], res["seg1000_over"]
        assert (at["status"], at["n_samples"]) == (full["status"], 1001) and at["ts"] * 3 < min(dur[1:])  # many samples a node
        assert (over["status"], over["n_samples"], over["seg_num"]) == (kr.OVER, 1001, 1000)
        assert np.array_equal(over["samples"], at["samples"])
        q = math.floor(full["T_sum"] / kr.DEFAULTS["ts"])
        above, below = res["minseg_above"], res["minseg_below"]
        assert kr.scenes()["minseg_below_" + w]["cfg"]["min_seg"] < q < kr.scenes()["minseg_above_" + w]["cfg"]["min_seg"]
        assert above["seg_num"] == 40 and below["seg_num"] == q == full["seg_num"]
        assert res["ts_long"]["seg_num"] == 8 > math.floor(full["T_sum"] / 1.0)  # the reference's own 8 decides
        print("getSamples, %s: T_sum %.4f, durations %s, t_shot %.4f, floor(T_sum / ts) %d" % (w, full["T_sum"], dur, full["t_shot"], q))


def test_outcome_batch_has_every_outcome():
    names, probs = kr.outcome_problems()
    res = kr.problem_results(kr.OUTCOME_SCENE, probs, kr.OUTCOME_CFG)
    _assert_robust("outcomes", probs, res)
    st = {n: (r["status"], r["which"]) for n, (r, _, _) in zip(names, res)}
    print(st)
    assert st["book"] == st["left"] == st["short"] == (kr.REACH_END, 0) and st["back"] == (kr.OVER, 0)
    assert st["behind_wall"] == (kr.NEAR_END, 0) and st["horizon_far"] == st["horizon_out"] == (kr.REACH_HORIZON, 0)
    assert st["in_inflation"] == st["across_wall"] == (kr.NO_PATH, 1) and st["close"] == (kr.CLOSE_GOAL, 0)
    over = [n for n, (r, _, _) in zip(names, res) if r["n_samples"] > kr.OUTCOME_CFG["max_samples"]]
    assert over == ["back"] and res[1][0]["shot"] == 1 and res[8][0]["n_nodes"] == 1
    bn, bp = kr.outcome_batch()
    assert len(bp) == 72 > 64 and set(bn) == set(names) and bn[64:] == names[4:10] + names[:2]


def test_load_sizes_and_layout_calls():
    """what the GPU test's other chain sizes and its calls of changing layout rely on"""
    pa, _ = kr.load_problems()
    assert {n - d for d, n in kr.LOAD_SIZES} == {1, kr.LOAD_SEG} and {d for d, _ in kr.LOAD_SIZES} == {3, 4, 5}
    for seg in sorted({n - d for d, n in kr.LOAD_SIZES}):
        res = kr.problem_results(kr.LOAD_SCENE, pa, dict(seg_num=seg))
        _assert_robust("load, %d segments" % seg, pa, res)
        assert all(r["n_samples"] == seg + 1 and r["n_nodes"] > 1 for r, _, _ in res)
    names, probs = kr.outcome_problems()
    km = kr.scene_map(kr.scenes()[kr.OUTCOME_SCENE])
    first = [kr.solve(km, p, dict(allocate_num=4096))["status"] for p in probs[:3]]
    assert set(first) == {kr.REACH_END, kr.NEAR_END}
    small = [kr.solve(km, p, dict(allocate_num=16)) for p in probs]
    assert {r["status"] for r in small} <= {kr.NO_PATH, kr.CLOSE_GOAL, kr.REACH_END}
    assert {r["use_node_num"] for r in small} >= {0, 1, 16}


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
