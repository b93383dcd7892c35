"""The facade's BsplineOptimizer::paramLocalTraj / reparamLocalTraj (fuel_amd/facade/bspline_opt/bspline_optimizer.h)
through the driver facade_localseg, with every host mirror of the map switched off: one paramLocalTraj per SPHERE problem,
ONE reparamLocalTraj for the guide paths' dt of a state.  The printed results against the restatement
(tests/localseg_ref.py) and against the Python route (SDFMap.local_segments with the facade's strides) on an equal map,
bit for bit, control points included."""
import os
import subprocess
import sys

import numpy as np
import pytest

import localseg_cases as lc
import localseg_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
MAP_SIZE, BMIN, BMAX, RES, GROUND = (10.0, 8.0, 4.0), (-4.0, -3.0, 0.0), (4.0, 3.0, 2.2), 0.1, -1.0
MAX_POINTS = 1024  # FUELMI_LOCALSEG_MAX_POINTS: the facade's stride


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def _hex(tokens, cols=3):
    return np.array([float.fromhex(t) for t in tokens], dtype=np.float64).reshape(-1, cols)


def scenario():
    """(state, problems): a SPHERE problem first, then the dt of three guide paths on the sphere's duration (one
    reparamLocalTraj), then a start at the trajectory's end (DEGENERATE)"""
    out = []
    for st in (lc.tour(), lc.with_local(lc.tour(), degree=4), lc.line(degree=5), lc.with_local(lc.tour(), degree=5)):
        sphere = (lr.SPHERE, 0.5, 3.0, 0.45)
        duration = lr.solve(st, *sphere)["duration"]
        probs = [sphere] + [(lr.DURATION, 0.5, duration, duration / k) for k in (6, 9, 14)] + \
            [(lr.SPHERE, st.global_duration - 5e-4, 3.0, 0.45), (lr.DURATION, 0.25, 1.0, 0.125)]
        out.append((st, probs))
    return out


def test_facade_local_segments(tmp_path):
    import fuel_amd
    scen = scenario()
    path = str(tmp_path / "scen.bin")
    with open(path, "wb") as f:
        np.array(list(MAP_SIZE) + list(BMIN) + list(BMAX) + [RES, GROUND, len(scen)], dtype=np.float64).tofile(f)
        for st, probs in scen:
            nl = 0 if st.local_ctrl is None else len(st.local_ctrl)
            np.array([st.degree, len(st.seg_times), st.global_duration, nl, st.local_knot_span, st.local_ts, st.local_te,
                      st.time_change, st.last_time_inc, len(probs)], dtype=np.float64).tofile(f)
            np.array(st.seg_times, dtype=np.float64).tofile(f)
            np.array(st.coef, dtype=np.float64).reshape(-1).tofile(f)
            if nl:
                np.array(st.local_ctrl, dtype=np.float64).reshape(-1).tofile(f)
            np.array(probs, dtype=np.float64).reshape(-1).tofile(f)
    exe = os.path.join(ROOT, "fuel_amd", "facade", "facade_localseg")
    run = subprocess.run([exe, path], check=True, capture_output=True, text=True, timeout=120)
    got, calls = {}, []
    for line in run.stdout.splitlines():
        t = line.split()
        if t[0] == "call":
            calls.append(tuple(int(v) for v in t[1:]))
        elif t[0] == "seg":
            got[int(t[1]), int(t[2])] = dict(status=int(t[3]), n_steps=int(t[4]), seg_num=int(t[5]),
                                             segment_len=float.fromhex(t[6]), dt=float.fromhex(t[7]),
                                             duration=float.fromhex(t[8]), n_ctrl=int(t[9]), n_points=int(t[10]),
                                             n_der=int(t[11]))
        elif t[0] in ("ctrl", "points", "derivs"):
            got[int(t[1]), int(t[2])][t[0]] = _hex(t[3:])
    # one call per SPHERE problem, ONE for the three guide paths, every call accepted
    assert calls == [c for s in range(len(scen)) for c in ((s, 0, 1, 1), (s, 1, 3, 1), (s, 4, 1, 1), (s, 5, 1, 1))]
    gm = fuel_amd.SDFMap(MAP_SIZE, BMIN, BMAX, device=0)
    try:
        for s, (st, probs) in enumerate(scen):
            out = gm.local_segments([st.as_dict()], [(0,) + p for p in probs], degree=st.degree, max_points=MAX_POINTS)
            assert out["status"].tolist() == [0, 0, 0, 0, lr.DEGENERATE, 0]
            for b, p in enumerate(probs):
                g, r = got[s, b], lr.solve(st, *p, max_points=MAX_POINTS)
                tag = (s, b)
                for k in ("status", "n_steps", "seg_num", "n_points", "n_ctrl"):
                    assert g[k] == r[k] == out[k][b], (tag, k)
                for k in ("segment_len", "dt", "duration"):
                    assert _bits(g[k]) == _bits(r[k]) == _bits(out[k][b]), (tag, k)
                assert _bits(g["points"]) == _bits(np.array(r["points"]).reshape(-1, 3)), tag
                assert _bits(g["ctrl"]) == _bits(out["ctrl"][b][:r["n_ctrl"]]), tag
                if r["status"] == lr.OK:
                    assert g["n_der"] == 4 and _bits(g["derivs"]) == _bits(r["derivs"]) == _bits(out["derivs"][b]), tag
                    assert len(g["ctrl"]) == r["n_points"] + st.degree - 1
                else:
                    assert g["n_der"] == 0 and g["n_ctrl"] == 0
        # the three guide paths of a state have three different point counts
        assert len({got[0, b]["n_points"] for b in (1, 2, 3)}) == 3
    finally:
        gm.close()
