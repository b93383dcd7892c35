"""The scenes of the trajectory-sampling tests (tests/test_traj_sample_cpu.py, tests/test_traj_sample_gpu.py): the smallest
shapes at which the kernel can still go wrong.  A scene is a dict: tag, mode, degree, ctrl [n, 3], dt, t [n_t], yaw (None
or dict ctrl / degree / dt), t_stop (None or a number).  Scenes of one (mode, degree, yaw degree) share a call."""
import math

import numpy as np

import traj_sample_ref as sr

WIN = 64   # samples per window (traj_sample.hip TS_WIN)
PACK = 3   # problems per workgroup (traj_sample.hip TS_WAVES)
_REF = {}


def wiggle(n, seed, start=(0.5, -1.0, 1.0), step=0.25, amp=0.08):
    """a forward-moving path with noise: n control points"""
    rng = np.random.default_rng(seed)
    d = np.array([1.0, 0.4, 0.1]) / np.linalg.norm([1.0, 0.4, 0.1])
    return np.array(start) + np.arange(n)[:, None] * step * d + rng.normal(scale=amp, size=(n, 3))


def yaw_wiggle(n, seed):
    rng = np.random.default_rng(seed)
    return np.cumsum(rng.normal(scale=0.3, size=n))


def duration_of(n, p, dt):
    u = sr.knots(n, p, dt)
    return u[n] - u[p]


def edge_times(n, p, dt, T=None, extra=()):
    """0; the accumulated knots u[i] - u[p] and the products k * dt (they differ in the last bit); nextafter(T, 0), T and
    beyond; a time below 0"""
    u = sr.knots(n, p, dt)
    D = u[n] - u[p]
    T = D if T is None else T
    acc = [u[i] - u[p] for i in range(p, n + 1)]
    prod = [k * dt for k in range(n - p + 1)]
    t = [0.0] + acc + prod + [math.nextafter(T, 0.0), T, math.nextafter(T, math.inf), T + 0.3, D, D + 1.0, -0.05, 0.5 * dt]
    return np.array(t + list(extra), dtype=np.float64)


def tape(count, tick=0.01, start=0.0):
    """a 100 Hz tape: start + k * tick"""
    return start + tick * np.arange(count, dtype=np.float64)


def scene(tag, mode, degree, ctrl, dt, t, yaw=None, t_stop=None):
    return dict(tag=tag, mode=mode, degree=degree, ctrl=np.ascontiguousarray(ctrl, dtype=np.float64), dt=float(dt),
                t=np.ascontiguousarray(t, dtype=np.float64), yaw=yaw, t_stop=t_stop)


def yaw_of(ctrl, degree, dt):
    return dict(ctrl=np.ascontiguousarray(ctrl, dtype=np.float64), degree=degree, dt=float(dt))


def slow_line(n=8, dt=0.4, speed=6e-5):
    """a straight constant-speed cubic: control points speed * dt apart.  Sampled every 0.01 s successive positions are
    0.6e-6 apart: below the record's 1e-6 against the previous sample, above it against the last pushed one about every
    other sample"""
    return np.array([1.0, 2.0, 0.5]) + np.arange(n)[:, None] * (speed * dt) * np.array([1.0, 0.0, 0.0])


def quick_scenes():
    out = []
    seed = 0
    for p, py in ((3, 3), (4, 3), (5, 5)):
        sizes = (p + 1, p + 2, 9, 40)
        for n in sizes:
            seed += 1
            dt = (0.31, 0.2, 0.4, 0.17)[seed % 4]
            D = duration_of(n, p, dt)
            # yaw: absent / the minimum / 12 segments of D / 12 (its duration differs from D by rounding) / planYaw's
            if n == p + 1:
                yaw = None
            elif n == p + 2:
                yaw = yaw_of(yaw_wiggle(py + 1, seed), py, D / 1.0)
            elif n == 9:
                yaw = yaw_of(yaw_wiggle(12 + py, seed), py, D / 12)
            else:
                yaw = yaw_of(yaw_wiggle(n, seed), py, dt)
            out.append(scene("cmd_p%d_n%d" % (p, n), sr.COMMAND, p, wiggle(n, seed), dt, edge_times(n, p, dt), yaw))
            # t_stop below, equal to and above D; once below 0 ([T, 0) is PAST: the reference's order of tests)
            for name, ts in (("below", 0.6 * D), ("equal", D), ("above", D + 0.4)) + ((("neg", -0.2),) if n == 9 else ()):
                if n in (p + 2, 9) or name == "below":
                    T = min(ts, D)
                    out.append(scene("stop_%s_p%d_n%d" % (name, p, n), sr.COMMAND, p, wiggle(n, seed), dt,
                                     edge_times(n, p, dt, T, extra=(-0.1, -0.3)), yaw, t_stop=ts))
            # STATE: the clamp below 0 and beyond D
            out.append(scene("state_p%d_n%d" % (p, n), sr.STATE, p, wiggle(n, seed), dt,
                             edge_times(n, p, dt, extra=(-2.0, D + 5.0)), yaw))
        # window edges: n_t = 1, 63, 64, 65, 129 and 0, on a tape that runs past the end
        for n_t in (0, 1, WIN - 1, WIN, WIN + 1, 2 * WIN + 1):
            seed += 1
            n, dt = 7 + p, 0.05
            yaw = yaw_of(yaw_wiggle(12 + py, seed), py, duration_of(n, p, dt) / 12)
            out.append(scene("tape_p%d_nt%d" % (p, n_t), sr.COMMAND, p, wiggle(n, seed), dt, tape(n_t, 0.01, -0.02), yaw))
        out.append(scene("state_tape_p%d" % p, sr.STATE, p, wiggle(9, seed), 0.05, tape(WIN + 1, 0.01, -0.1), None))
    # the record's chain: 6e-5 m/s at 100 Hz; with an INVALID sample in the middle; running past T
    line = slow_line()
    out.append(scene("record_slow", sr.COMMAND, 3, line, 0.4, tape(2 * WIN + 1)))
    mid = tape(WIN + 6)
    mid[WIN // 2] = -1.0
    mid[WIN + 2] = -0.5
    out.append(scene("record_invalid_mid", sr.COMMAND, 3, line, 0.4, mid))
    D = duration_of(len(line), 3, 0.4)
    out.append(scene("record_past_end", sr.COMMAND, 3, wiggle(8, 77), 0.4, tape(WIN + 9, 0.01, D - 0.295)))
    return out


def big_scenes():
    """max_ctrl = 1024 with a neighbour of p + 1 points in the same workgroup (one call, stride 1024)"""
    n, p, dt = sr.MAX_CTRL, 3, 0.05
    D = duration_of(n, p, dt)
    t = np.concatenate([np.linspace(0.0, D, WIN - 3), [math.nextafter(D, 0.0), D + 0.1, (n - p - 1) * dt, -1.0]])
    big = scene("big_n1024", sr.COMMAND, p, wiggle(n, 901, step=0.01, amp=0.004), dt, t,
                yaw_of(yaw_wiggle(n, 902), 3, dt))
    small = scene("big_neighbour_n4", sr.COMMAND, p, wiggle(4, 903), 0.3, edge_times(4, 3, 0.3), None)
    return [big, small, dict(small, tag="big_neighbour_again")]


def key(sc):
    """scenes with the same key share a call"""
    return (sc["mode"], sc["degree"], max([sc["yaw"]["degree"]] if sc["yaw"] else [0]))


def groups(scenes):
    """key -> scenes; a scene without yaw joins any yaw degree of its (mode, degree)"""
    g = {}
    for sc in scenes:
        g.setdefault(key(sc), []).append(sc)
    for (mode, deg, py) in [k for k in g if k[2] == 0]:
        host = [k for k in g if k[:2] == (mode, deg) and k[2] != 0]
        if host:
            g[host[0]].extend(g.pop((mode, deg, 0)))
    return g


def restate(sc):
    """sample() of a scene, and for COMMAND the record from zeros (windowed form), computed once"""
    if id(sc) not in _REF:
        y = sc["yaw"]
        s = sr.sample(sc["mode"], sc["ctrl"], sc["degree"], sc["dt"], sc["t"], y["ctrl"] if y else None,
                      y["degree"] if y else 3, y["dt"] if y else None, sc["t_stop"])
        s["flight"] = sr.record_windowed([0.0] * 8, sc["t"], s, WIN) if sc["mode"] == sr.COMMAND else None
        _REF[id(sc)] = (sc, s)
    return _REF[id(sc)][1]
