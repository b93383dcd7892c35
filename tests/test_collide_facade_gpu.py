"""The facade's TopologyPRM::findCollisionRange / guidePoints (fuel_amd/facade/path_searching/topo_prm.h) through the
driver facade_collide, which runs the collide branch of topoReplan end to end with every host mirror of the map switched
off: collision ranges, findTopoPaths, guide points of every select path.  On the `pillar` map of tests/topo_cases.py with
a fixed topo_prm/seed; the printed results against the restatement (tests/collide_ref.py in `cut` mode on the field read
back from an equal map) and the C-ABI's topological search on the same sample stream, bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

import collide_cases as cc
import collide_ref as cr
import topo_cases as tcs
import topo_ref as tpr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
CTRL_PT_DIST = 0.5


def _bits(a):
    a = np.ascontiguousarray(a, dtype=np.float64).copy()
    a[np.isnan(a)] = np.nan
    return a.tobytes()


def _hex(tokens):
    return np.array([float.fromhex(t) for t in tokens], dtype=np.float64).reshape(-1, 3)


def problems():
    """(tag, degree, dt, ctrl): through the pillar (degrees 3 and 4), past it, into it"""
    return [("through", 3, 0.5, cc.flight((-2.5, 0.0, 0.0), (1, 0, 0), 0.02, 12.5)),
            ("through_deg4", 4, 0.5, cc.flight((-2.5, 0.1, 0.1), (1, 0, 0), 0.02, 12.5, 4)),
            ("past", 3, 0.5, cc.flight((-2.5, 2.0, 0.0), (1, 0, 0), 0.02, 12.5)),
            ("into", 3, 0.5, cc.flight((-2.5, 0.0, 0.0), (1, 0, 0), 0.02, 6.0))]


def test_facade_collide_chain(tmp_path):
    import fuel_amd
    sc = tcs.scenes()["pillar"]
    cfg = sc["cfg"]
    probs = problems()
    scen = str(tmp_path / "scen.bin")
    with open(scen, "wb") as f:
        hdr = list(tcs.MAP_SIZE) + [tcs.RES, tcs.GROUND] + list(cfg["sample_inflate"]) + \
            [cfg["clearance"], cfg["ratio_to_short"], cfg["max_sample_num"], cfg["max_raw_path"], cfg["max_raw_path2"],
             cfg["reserve_num"], sc["seed"], CTRL_PT_DIST]
        np.array(hdr, dtype=np.float64).tofile(f)
        tcs.occupancy(sc["blocks"]).reshape(-1).tofile(f)
        for _, degree, dt, ctrl in probs:
            np.concatenate([[degree, len(ctrl), dt], ctrl.reshape(-1)]).tofile(f)
    exe = os.path.join(ROOT, "fuel_amd", "facade", "facade_collide")
    run = subprocess.run([exe, scen], check=True, capture_output=True, text=True, timeout=120)
    got = [dict(sel=[], guide=[], guide_info=[]) for _ in probs]
    for line in run.stdout.splitlines():
        t = line.split()
        if t[0] not in ("range", "call", "colli_start", "colli_end", "start_pts", "end_pts", "sel", "guide", "guide_info"):
            continue
        g = got[int(t[1])]
        if t[0] == "range":
            g["range"] = (int(t[2]), float(t[3]))
        elif t[0] == "call":
            g["call"] = (int(t[2]), int(t[3]))
        elif t[0] == "guide_info":
            g["guide_info"].append((int(t[2]), int(t[3]), float.fromhex(t[4]), int(t[5]), float.fromhex(t[6])))
        else:
            pts = _hex(t[3:])
            assert len(pts) == int(t[2])
            if t[0] in ("sel", "guide"):
                g[t[0]].append(pts)
            else:
                g[t[0]] = pts

    gm = fuel_amd.SDFMap(tcs.MAP_SIZE, device=0)
    try:
        gm.uploadOccupancy(tcs.occupancy(sc["blocks"]))
        gm.setLocalBound((0, 0, 0), tuple(v - 1 for v in tcs.NVOX))
        gm.clearAndInflateLocalMap()
        gm.updateESDF3d()
        dist = gm.syncHost(distance=True)["distance"].reshape(tcs.NVOX)
        field = cr.Field(tcs.ORIGIN, tcs.RES, dist, "cut", gm.info.resolution_inv)
        statuses = []
        for g, (tag, degree, dt, ctrl) in zip(got, probs):
            want = cr.collision_ranges(field, ctrl, degree, dt, cfg["clearance"], 64, 64)
            statuses.append(want["status"])
            assert g["range"] == (want["status"], cfg["clearance"]), tag
            for key in ("colli_start", "colli_end", "start_pts", "end_pts"):
                assert _bits(g[key]) == _bits(np.array(want[key], dtype=np.float64).reshape(-1, 3)), (tag, key)
            if want["status"] != cr.OK:
                assert "call" not in g and not g["sel"], tag
                continue
            kw = {k: v for k, v in cfg.items() if k not in ("max_sample_num", "max_path_points", "max_nodes")}
            out = gm.topo_paths([want["first_start"]], [want["last_end"]], [sc["samples"]], [want["start_pts"]],
                                [want["end_pts"]], max_path_points=256, max_nodes=cfg["max_sample_num"] + 2, **kw)
            assert g["call"] == (0, out["status"][0]) and out["status"][0] == tpr.OK, tag
            assert len(g["sel"]) == len(out["sel"][0]) >= 1, tag
            duration = (len(ctrl) - degree) * dt
            for path, want_path, info, guide in zip(g["sel"], out["sel"][0], g["guide_info"], g["guide"]):
                assert _bits(path) == _bits(want_path), tag
                w = cr.guide_points(path, duration, CTRL_PT_DIST, degree, 1024)
                assert info[:2] == (w["status"], w["seg_num"]) and info[3] == w["n_ctrl"] and w["status"] == cr.G_OK, tag
                assert _bits(info[2]) == _bits(w["dt"]) and _bits(info[4]) == _bits(duration), tag
                assert len(guide) == w["n_guide"] == w["n_ctrl"] - (8 if degree == 4 else 6), tag
                assert _bits(guide) == _bits(np.array(w["guide_pts"], dtype=np.float64).reshape(-1, 3)), tag
        assert statuses == [cr.OK, cr.OK, cr.NO_COLLISION, cr.ENDS_IN_OBSTACLE]
    finally:
        gm.close()
