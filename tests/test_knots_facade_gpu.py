"""facade_knots in a child process: BsplineOptimizer::adjustTime, then checkTrajCollision, evaluateCommand, replanState and
planYaw on the knots it returned (the overloads that take an Eigen::VectorXd where the knot span stood), against the
direct calls SDFMap.adjust_trajs -> check_trajs / sample_trajs / plan_yaws(knots=...) on the same problems.  Both routes
end in the same device entries, so every number is compared bit for bit (the driver prints 17 significant digits)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import knots_cases as kc
import traj_adjust_ref as ar
import traj_check_cases as tc
import traj_sample_ref as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

LIMITS = dict(limit_vel=0.8, limit_acc=0.6)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def test_facade_knots_equals_the_direct_calls(tmp_path):
    import fuel_amd
    m = tc.spec(kc.MAP)
    problems = [(3, kc.flight(9, 401), 0.3, 0.0), (3, kc.flight(31, 402), 0.1, 0.4), (4, kc.flight(14, 403), 0.2, 0.1),
                (5, kc.flight(17, 404), 0.15, 0.0), (3, kc.flight(4, 405, x0=0.4, span=0.6), 0.5, 0.0)]
    times = [np.concatenate([[-0.1, 0.0], np.linspace(0.05, d * (len(c) - p) * 1.6, 70)]) for p, c, d, _ in problems]
    scen = str(tmp_path / "scen.bin")
    with open(scen, "wb") as f:
        np.array(list(m.map_size) + list(m.origin) + list(m.origin + np.array(m.map_size)) + [m.res, m.kw["ground_height"]],
                 dtype=np.float64).tofile(f)
        m.occ3.reshape(-1).tofile(f)
        for (p, c, d, now), t in zip(problems, times):
            np.concatenate([[p, len(c), d, now, len(t), LIMITS["limit_vel"], LIMITS["limit_acc"]], c.reshape(-1), t]).tofile(f)
    exe = os.path.join(ROOT, "fuel_amd", "facade", "facade_knots")
    out = subprocess.run([exe, scen], check=True, capture_output=True, text=True, timeout=300)
    res = json.loads(out.stdout[out.stdout.index("{"):])["problems"]
    assert len(res) == len(problems)

    gm = fuel_amd.SDFMap(m.map_size, device=0, **m.kw)
    gm.uploadOccupancy(m.occ3.reshape(-1))
    gm.setLocalBound(*helpers.full_box(gm.nvox))
    gm.clearAndInflateLocalMap()
    moved = unsafe = 0
    for got, (p, c, d, now), t in zip(res, problems, times):
        adj = gm.adjust_trajs([c], [d], ops=ar.LENGTHEN | ar.REALLOC, degree=p, **LIMITS)
        u = adj["knots_out"][0][:len(c) + p + 1]
        assert _bits(got["knots"]) == _bits(u) and got["iters"] == adj["iters"][0]
        assert _bits(got["duration"]) == _bits(adj["duration_out"][0])
        moved += int(adj["iters"][0] > 0)
        chk = gm.check_trajs([c], None, [now], knots=[u], degree=p)
        assert got["safe"] == chk["safe"][0]
        assert _bits(got["distance"]) == _bits(chk["distance"][0] if not chk["safe"][0] else -7.0)
        unsafe += 1 - got["safe"]
        smp = gm.sample_trajs([c], None, [t], flight=np.zeros((1, 8)), knots=[u], degree=p)
        assert got["status"] == smp["status"][0].tolist()
        for k in ("pos", "vel", "acc", "jerk"):
            assert _bits(got[k]) == _bits(smp[k][0]), k
        assert _bits(got["flight"]) == _bits(smp["flight"][0])
        st = gm.sample_trajs([c], None, [[t[len(t) // 2]]], knots=[u], mode=ts.STATE, degree=p)
        assert _bits(got["state"]) == _bits(np.concatenate([st["pos"][0, 0], st["vel"][0, 0], st["acc"][0, 0]]))
        yaw = gm.plan_yaws([c], None, [(0.3, 0.1, 0.0)], None, knots=[u], mode=1, pos_degree=p, seg_num=0, relax_time=0.0)
        assert got["yaw_status"] == yaw["status"][0] == 0
        n = yaw["seg_num"][0] + 3
        assert _bits(got["dt_yaw"]) == _bits(yaw["dt_yaw"][0]) and _bits(got["yaw_ctrl"]) == _bits(yaw["yaw_ctrl"][0, :n])
        assert _bits(got["path_yaw"]) == _bits(yaw["waypts"][0, :yaw["n_waypt"][0]])
    assert moved >= 3 and 0 < unsafe < len(problems)  # the knots really moved; both answers of the safety check occur
    gm.close()
