"""The facade's HeadingPlanner (fuel_amd/facade/active_perception/heading_planner.h) through the driver facade_heading,
which calls searchPathOfYaw / searchPathsOfYaw and calcInfoGain / calcInfoGains with every host mirror of the map switched
off.  On the `wall` map of tests/heading_cases.py; the printed results against the C-ABI's on an equal map, bit for bit,
and against the restatement (tests/heading_ref.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import heading_cases as hc
import heading_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
H, YAW_DIFF, RATE, W, FAR, L1, L2 = 2, 0.25, 0.9, 0.37, 1.6, 2.0, 1.0


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def problems():
    """(pts, yaws, dt, ctrl): trajectories of 5, 3, 2 and 1 way-points"""
    line = hc._line(8, step=(0.2, 0.03, 0.0))
    full = (hc._line(5), [0.0, 0.1, 0.0, -0.1, 0.0], 0.5, line)
    return [full, (hc._line(3), [0.3, -0.2, 0.1], 0.4, line[:3]), (hc._line(2), [0.3, 0.5], 0.5, line[:1]),
            (hc._line(1), [0.7], 0.5, line[:2])]


def poses():
    return [(hc.CAM, 0.0), (hc.CAM, 0.45), ((-0.5, 0.3, 0.4), -0.3), ((3.0, 3.0, 1.3), -3 * hc.PI / 4)]


@pytest.mark.parametrize("weight_type", [hr.NON_UNIFORM, hr.UNIFORM])
def test_facade_heading(tmp_path, weight_type):
    import fuel_amd
    m = hc.spec("wall")
    probs, ps = problems(), poses()
    scen = str(tmp_path / "scen.bin")
    with open(scen, "wb") as f:
        hdr = list(m.map_size) + list(m.box_min) + list(m.box_max) + [H, YAW_DIFF, RATE, W, weight_type, L1, L2, FAR,
                                                                       len(probs), len(ps)]
        np.array(hdr, dtype=np.float64).tofile(f)
        m.log_odds().reshape(-1).tofile(f)
        for pts, yaws, dt, ctrl in probs:
            np.concatenate([[len(yaws), dt, len(ctrl)], np.array(pts).reshape(-1), yaws, np.array(ctrl).reshape(-1)]).tofile(f)
        for p, y in ps:
            np.array(list(p) + [y], dtype=np.float64).tofile(f)
    exe = os.path.join(ROOT, "fuel_amd", "facade", "facade_heading")
    run = subprocess.run([exe, scen], check=True, capture_output=True, text=True, timeout=120)
    got = {}
    for line in run.stdout.splitlines():
        t = line.split()
        if t[0] in ("call", "batch_call", "batch_gain_call"):
            got.setdefault(t[0], []).append([int(v) for v in t[1:]])
        elif t[0] in ("path", "gains", "g_value", "batch_path", "gain", "batch_gain"):
            v = np.array([float.fromhex(x) for x in t[3:]], dtype=np.float64)
            assert len(v) == int(t[2])
            got.setdefault(t[0], {})[int(t[1])] = v
    assert got["call"] == [[b, 0, 0] for b in range(len(probs))] and got["batch_call"] == [[0]] and got["batch_gain_call"] == [[0]]

    gm = fuel_amd.SDFMap(m.map_size, m.box_min, m.box_max, device=0, **m.kw)
    gm.uploadOccupancy(m.log_odds())
    ref = m.ref(gm.info.resolution_inv)
    gcfg = hr.gain_cfg(weight_type=weight_type, far=FAR, lambda1=L1, lambda2=L2)
    out = gm.yaw_paths([p[0] for p in probs], [p[1] for p in probs], [p[2] for p in probs], ctrl=[p[3] for p in probs],
                       half_vert_num=H, yaw_diff=YAW_DIFF, max_yaw_rate=RATE, w=W, **gcfg)
    nv = 2 * H + 1
    tol = hr.parity_tolerance()[1]
    for b, (pts, yaws, dt, ctrl) in enumerate(probs):
        L = len(yaws)
        assert _bits(got["path"][b]) == _bits(out["path"][b][:L]) == _bits(got["batch_path"][b]), b
        if L:
            assert _bits(got["gains"][b]) == _bits(out["gains"][b][:L]) and _bits(got["g_value"][b]) == _bits(out["g_value"][b][:L]), b
        r = hr.search_path_of_yaw(ref, gcfg, np.array(pts), yaws, dt, np.array(ctrl), H, YAW_DIFF, RATE, W)
        assert np.all(np.abs(got["gains"][b].reshape(L, nv) - np.array(r["gains"])) <= tol * np.abs(np.array(r["gains"]))), b
        assert _bits(got["path"][b]) == _bits(r["path"]), b
    # calcInfoGain: UNIFORM, no isInBox, whatever heading_planner/weight_type says
    cfg1 = hr.gain_cfg(weight_type=hr.UNIFORM, in_box=False, far=FAR)
    g = gm.info_gains([p for p, _ in ps], [[y] for _, y in ps], **cfg1)
    for b, (p, y) in enumerate(ps):
        want = hr.info_gains(ref, cfg1, tuple(p), [y])
        assert got["gain"][b][0] == g["gain"][b][0] == got["batch_gain"][0][b] == want["gain"][0] == want["n_visible"][0], b
    assert g["gain"][:, 0].max() > 0
    gm.close()
