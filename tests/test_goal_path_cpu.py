"""fuelmi_map_goal_paths without a GPU: the restatement (tests/goal_path_ref.py) states that shortenPath's literal loop
and the first-push form the device kernel uses agree on every scene the GPU tests run, and that those scenes are what
they claim -- conditions on the inputs, asserted on the restatement alone, so that a GPU test cannot pass by comparing
nothing.  The binding: the header declares the call, fuel_amd._lib binds it with the C layout."""
import collections
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import goal_path_ref as gr
import path_cost_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _both_forms(pm, om, case, results, runs=None):
    cfg = dict(gr.DEFAULTS, **case.get("cfg", {}))
    n = 0
    for r in results:
        if r["status"] in (gr.NO_PATH, gr.RAW_OVER):
            continue
        fp = gr.first_push_shorten(pm, om, r["raw"], cfg["shorten_dist"], cfg["end_eps"], runs)
        assert _same(fp, r["short"])
        n += 1
    return n


@pytest.fixture(scope="module")
def door():
    om, pm, size, box, case = gr.door_scene()
    logs = []
    sources = {}
    res = []
    for s, g in zip(case["starts"], case["goals"]):
        key = s.tobytes()
        if key not in sources:
            sources[key] = gr.Source(pm, s)
        logs.append([])
        res.append(gr.solve(pm, om, sources[key], g, log=logs[-1], **gr.DEFAULTS))
    return om, pm, case, res, logs


def test_door_scene_both_forms_and_coverage(door):
    om, pm, case, res, logs = door
    assert len(res) >= 80 + 2 and len({s.tobytes() for s in case["starts"]}) >= 2
    assert _both_forms(pm, om, case, res) >= 70
    st = collections.Counter(r["status"] for r in res)
    assert min(st[gr.CLOSE], st[gr.MID], st[gr.FAR], st[gr.NO_PATH]) >= 1, st
    assert 10 * st[gr.NO_PATH] <= len(res), st
    kinds = collections.Counter(k for log in logs for k, _ in log)
    assert kinds["dist"] >= 1 and kinds["ray"] >= 1, kinds
    far = [r for r in res if r["status"] == gr.FAR]
    assert any(r["dropped"] > 0 for r in far) and any(r["dropped"] == 0 for r in far)
    for r in far:  # the truncation ends on a way-point of the shortened path and keeps a prefix of it
        assert _same(r["way"], r["short"][:len(r["way"])]) and np.array_equal(r["next_goal"], r["way"][-1])
    # start = goal: the raw path {p, p} comes out as the single point; the near goal: two points and their mid-point
    single, near = res[-2], res[-1]
    assert single["raw_len"] == 2 and len(single["way"]) == 1 and single["status"] == gr.CLOSE
    assert single["length"] == 0.0
    assert len(near["way"]) == 3 and np.array_equal(near["way"][1], 0.5 * (near["way"][0] + near["way"][2]))
    assert len(gr.shorten_loop(pm, om, near["raw"])) == 1


def test_window_scene_runs_and_lengths():
    om, pm = gr.corridor_map()
    cases, src = gr.window_cases(pm)
    sources = {(gr.CORRIDOR_START.tobytes(), gr.CORRIDOR_RES, 0.1): src}
    seen_runs = set()
    for case in cases:
        res = gr.solve_case(pm, om, case, sources)
        runs = []
        assert _both_forms(pm, om, case, res, runs) == len(res)
        if "run" in case:
            assert runs[0] == case["run"], (case["run"], runs)
            seen_runs.add(runs[0])
        else:
            assert tuple(r["raw_len"] for r in res) == case["points"]
    W = gr.WINDOW
    assert seen_runs == {W - 1, W, W + 1, 2 * W + 1}
    # the kernel's window is what the scene was built for
    src_txt = open(os.path.join(ROOT, "fuel_amd", "csrc", "goal_path.hip")).read()
    assert re.search(r"constexpr int GS_WIN = %d;" % W, src_txt)


def test_face_scene_leaves_the_map_and_ends_in_unknown():
    om, pm = gr.face_map()
    case = gr.face_case()
    res = gr.solve_case(pm, om, case)
    assert _both_forms(pm, om, case, res) == 2
    out, unk = res
    assert out["status"] != gr.NO_PATH and out["raw_len"] >= 3
    raw = out["raw"]
    outside = [v for i in range(1, len(raw) - 1) for v in pr.ray_voxels(om, raw[0], raw[i + 1])
               if not all(0 <= v[k] < pm.nvox[k] for k in range(3))]
    assert outside, "no ray of the scene leaves the map"
    # the goal's voxel is unknown, the search reaches its neighbourhood, and the last ray stops before it
    g = case["goals"][1]
    assert pm.blocked(g[None])[0] and unk["status"] != gr.NO_PATH
    gv = tuple(int(v) for v in np.floor((g - pm.origin) * pm.res_inv))
    assert gv == gr.FACE_UNKNOWN
    last_anchor = gr.shorten_loop(pm, om, unk["raw"])[-1]
    assert gv not in pr.ray_voxels(om, last_anchor, g)
    assert np.array_equal(unk["way"][-1], g)


def test_threshold_cases_flip_at_the_value(door):
    om, pm, case, res, _ = door
    b = next(i for i, r in enumerate(res) if r["status"] == gr.MID and r["raw_len"] >= 12)
    cases, src = gr.threshold_cases(pm, om, case["starts"][b], case["goals"][b])
    sources = {(case["starts"][b].tobytes(), 0.2, 0.1): src}
    got = {}
    for name, v, three in cases:
        got[name] = [gr.solve_case(pm, om, c, sources)[0] for c in three]
        for c, r in zip(three, got[name]):
            assert _both_forms(pm, om, c, [r]) == 1
    lo, at, hi = got["radius_close"]
    assert (lo["status"], at["status"], hi["status"]) == (gr.MID, gr.MID, gr.CLOSE)
    lo, at, hi = got["radius_far"]
    assert (lo["status"], at["status"], hi["status"]) == (gr.FAR, gr.MID, gr.MID)
    lo, at, hi = got["shorten_dist"]  # strictly greater pushes: only the value below does
    assert not _same(lo["short"], at["short"]) and _same(at["short"], hi["short"])
    lo, at, hi = got["end_eps"]
    goal = case["goals"][b]  # strictly greater pushes the goal: only the value below does
    assert np.array_equal(lo["short"][-1], goal) and not np.array_equal(at["short"][-1], goal)
    assert _same(at["short"], hi["short"])


def test_header_declares_and_python_binds_the_call():
    hdr = open(os.path.join(ROOT, "include", "fuelmi.h")).read()
    assert re.search(r"\bint fuelmi_map_goal_paths\(", hdr)
    for name in ("FUELMI_GOAL_CLOSE", "FUELMI_GOAL_MID", "FUELMI_GOAL_FAR", "FUELMI_GOAL_NO_PATH", "fuelmi_goal_cfg"):
        assert name in hdr, name
    from fuel_amd import _lib
    assert "fuelmi_map_goal_paths" in _lib.SYMBOLS
    assert (_lib.GOAL_CLOSE, _lib.GOAL_MID, _lib.GOAL_FAR, _lib.GOAL_NO_PATH) == (gr.CLOSE, gr.MID, gr.FAR, gr.NO_PATH)
    from fuel_amd import host
    assert callable(getattr(host.SDFMap, "goal_paths"))


def test_goal_cfg_layout_matches_c(tmp_path):
    from fuel_amd import _lib
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fuelmi.h"\n'
                    'int main(){printf("%zu %zu %zu %zu %d %d %d %d\\n", sizeof(fuelmi_goal_cfg), '
                    'offsetof(fuelmi_goal_cfg, shorten_dist), offsetof(fuelmi_goal_cfg, max_way_points), '
                    'sizeof(fuelmi_path_cfg), FUELMI_GOAL_CLOSE, FUELMI_GOAL_MID, FUELMI_GOAL_FAR, '
                    'FUELMI_GOAL_NO_PATH);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_lib.GoalCfg), _lib.GoalCfg.shorten_dist.offset, _lib.GoalCfg.max_way_points.offset,
                   C.sizeof(_lib.PathCfg), 0, 1, 2, 3]
