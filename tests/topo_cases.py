"""The scenes of the topological path search (tests/test_topo_path_cpu.py, tests/test_topo_path_gpu.py,
tests/golden/make_topo_golden.py): a 64 x 64 x 24 map at 0.1 m, occupied index blocks, the problems, and per problem a
fixed sample stream.  The stream is what std::default_random_engine (minstd_rand0) seeded with the scene's seed gives
through std::uniform_real_distribution<double>(-1, 1) -- the numbers TopologyPRM::getSample draws -- restated here so that
the fixtures of the reference's own code and the scenes hold the same numbers."""
import math

import numpy as np

import topo_ref as tr

NVOX = (64, 64, 24)
RES, GROUND, INFL_STEP = 0.1, -1.0, 2
MAP_SIZE = (6.4, 6.4, 2.4)
ORIGIN = (-3.2, -3.2, GROUND)
L_FREE, L_OCC = math.log(0.12 / 0.88), math.log(0.9 / 0.1)


def sample_stream(seed, count):
    """[count, 3] numbers of uniform_real_distribution<double>(-1, 1) over minstd_rand0(seed) (libstdc++:
    generate_canonical<double, 53> takes two draws)"""
    x = seed % 2147483647 or 1
    r = 2147483646.0
    out = np.empty(3 * count)
    for i in range(3 * count):
        x = x * 16807 % 2147483647
        s = float(x - 1) * 1.0
        x = x * 16807 % 2147483647
        s += float(x - 1) * r
        v = s / float(2147483646 ** 2)
        if v >= 1.0:
            v = math.nextafter(1.0, 0.0)
        out[i] = v * 2.0 + -1.0
    return out.reshape(count, 3)


def occupancy(blocks):
    occ = np.full(NVOX, L_FREE)
    for (x0, x1), (y0, y1), (z0, z1) in blocks:
        occ[x0:x1, y0:y1, z0:z1] = L_OCC
    return occ


def sources(blocks):
    """the voxels the ESDF starts from: the occupied blocks inflated by a cube of INFL_STEP voxels.
    clearAndInflateLocalMap keeps an inflated voxel by its address alone, so a cube that leaves the map in y or z comes
    back in the neighbouring row; the blocks stay INFL_STEP voxels inside the map, where no cube leaves it"""
    src = np.zeros(NVOX, dtype=bool)
    s = INFL_STEP
    for b in blocks:
        assert all(s <= lo < hi <= n - s for (lo, hi), n in zip(b, NVOX)), b
        (x0, x1), (y0, y1), (z0, z1) = b
        src[x0 - s:x1 + s, y0 - s:y1 + s, z0 - s:z1 + s] = True
    return src


_k_cache = {}


def squared_distance(src):
    """k: the exact squared voxel distance to the nearest source (-1: no source at all)"""
    key = src.tobytes()
    if key not in _k_cache:
        _k_cache[key] = _squared_distance(src)
    return _k_cache[key]


def _squared_distance(src):
    if not src.any():
        return np.full(src.shape, -1, dtype=np.int64)
    big = 1 << 40
    d = np.where(src, 0, big).astype(np.int64)
    for ax in range(3):
        n = d.shape[ax]
        i = np.arange(n)
        off = (i[:, None] - i[None, :]) ** 2  # [to, from]
        m = np.moveaxis(d, ax, -1)
        m = (m[..., None, :] + off).min(axis=-1)
        d = np.moveaxis(m, -1, ax)
    return d


def field_of(blocks):
    """the reference's distance_buffer_ of the scene: res * sqrt(k), without a source res * sqrt(DBL_MAX)"""
    k = squared_distance(sources(blocks))
    return np.where(k < 0, RES * math.sqrt(tr.NO_SOURCE), RES * np.sqrt(np.maximum(k, 0).astype(np.float64)))


# (the blocks end INFL_STEP voxels inside the map: inflated they reach its faces)
PILLAR = [((30, 34), (30, 34), (2, 22))]
TWO = [((30, 34), (20, 24), (2, 22)), ((30, 34), (40, 44), (2, 22))]
WALL = [((30, 34), (2, 62), (2, 22))]
# slabs one voxel thick every 8 voxels in x: between two inflated slabs one column of voxels at k = 4 with a column at
# k = 1 on either side.  With clearance 0 a sample in a k = 1 voxel is kept, and its own voxel blocks every ray from it:
# it becomes a guard
COMB = [((8 * i, 8 * i + 1), (2, 62), (2, 22)) for i in range(1, 8)]

S0, E0 = (-2.0, 0.0, 0.0), (2.0, 0.0, 0.0)


def scenes():
    """name -> dict(blocks, seed, cfg, probs = [dict(start, end, start_pts, end_pts)])"""
    p0 = dict(start=S0, end=E0, start_pts=(), end_pts=())
    sc = {
        "free": dict(blocks=[], seed=1, cfg={}, probs=[p0]),
        "pillar": dict(blocks=PILLAR, seed=2, cfg={}, probs=[p0]),
        "two_pillars": dict(blocks=TWO, seed=3, cfg={}, probs=[p0]),
        "two_pillars_reserve": dict(blocks=TWO, seed=3, cfg=dict(reserve_num=2), probs=[p0]),
        "two_pillars_ratio": dict(blocks=TWO, seed=3, cfg=dict(ratio_to_short=1.02), probs=[p0]),
        "blocked": dict(blocks=WALL, seed=4, cfg={}, probs=[p0]),
        "comb": dict(blocks=COMB, seed=53, cfg=dict(clearance=0.0, sample_inflate=(1.2, 3.0, 1.0)),
                     probs=[dict(p0, start=(-1.95, 0.0, 0.0), end=(2.05, 0.0, 0.0))]),
        "moved": dict(blocks=PILLAR, seed=6, cfg={}, probs=[p0]),
        "rollback": dict(blocks=TWO, seed=7, cfg={}, probs=[dict(p0, start=(-2.0, -0.6, 0.0), end=(2.0, 0.7, 0.2))]),
        "adjacent": dict(blocks=PILLAR, seed=8, cfg={}, probs=[dict(p0, start=(-2.0, 0.55, 0.0), end=(2.0, 0.55, 0.0))]),
        "dfs_cap": dict(blocks=TWO, seed=9, cfg=dict(max_raw_path=3, max_raw_path2=2), probs=[p0]),
        "merge": dict(blocks=PILLAR, seed=10, cfg={},
                      probs=[dict(p0, start_pts=((-2.6, 0.3, 0.1), (-2.3, 0.2, 0.0)), end_pts=((2.3, -0.2, 0.0), (2.6, -0.3, 0.1)))]),
        "undefined": dict(blocks=[], seed=11, cfg={}, probs=[dict(p0, start=(0.0, 0.0, -0.5), end=(0.0, 0.0, 0.9))]),
        "overflow": dict(blocks=PILLAR, seed=2, cfg=dict(max_path_points=2), probs=[p0]),
    }
    for s in sc.values():
        s["cfg"] = dict(tr.DEFAULTS, **s["cfg"])
        s["samples"] = sample_stream(s["seed"], s["cfg"]["max_sample_num"])
    return sc


# the reference cannot express these: `undefined` is undefined behaviour there, `overflow` is about this library's strides
NOT_RECORDED = ("undefined", "overflow")


def run_ref(sc, mode="f64", dist=None):
    """the restatement on a scene: one result per problem"""
    f = tr.Field(ORIGIN, RES, field_of(sc["blocks"]) if dist is None else dist, mode)
    return [tr.find_topo_paths(f, sc["cfg"], p["start"], p["end"], sc["samples"], p["start_pts"], p["end_pts"])
            for p in sc["probs"]]


def f32_field(blocks, ulp=0, rng=None):
    """what a device holds for the scene: the f32 rounding of res * sqrt(k) (f32 product of f32 factors), every finite
    positive value moved by `ulp` f32 steps (rng: by a step drawn per voxel from -|ulp| .. |ulp|); +inf without a source"""
    k = squared_distance(sources(blocks))
    with np.errstate(invalid="ignore"):
        d = (np.float32(RES) * np.sqrt(np.maximum(k, 0).astype(np.float32))).astype(np.float32)
    step = np.full(d.shape, ulp, dtype=np.int32) if rng is None else rng.integers(-abs(ulp), abs(ulp) + 1, size=d.shape).astype(np.int32)
    bits = d.view(np.int32) + np.where(d > 0, step, 0)
    d = bits.view(np.float32).copy()
    d[k < 0] = np.inf
    return d


def as_field_array(d32):
    """an f32 field as the f64 array fuelmi_map_sync_host returns (inf: the reference's res * sqrt(DBL_MAX))"""
    return np.where(np.isinf(d32), RES * math.sqrt(tr.NO_SOURCE), d32.astype(np.float64))


def discrete(r):
    """everything of a result but positions"""
    return (r["status"], tuple(r["counts"]), tuple(r["events"]), tuple((n[0], n[1], tuple(n[3])) for n in r["nodes"]),
            tuple(len(p) for p in r["raw"]), tuple(len(p) for p in r["filt"]), tuple(len(p) for p in r["sel"]),
            tuple(tuple(f) for f in r["filt_pushed"]), tuple(tuple(f) for f in r["sel_pushed"]))


def disagreement(a, b):
    """the largest |difference| of a position between two results with the same discrete outputs"""
    worst = 0.0
    for na, nb in zip(a["nodes"], b["nodes"]):
        worst = max(worst, float(np.max(np.abs(np.array(na[2]) - np.array(nb[2])))))
    for key in ("raw", "filt", "sel"):
        for pa, pb in zip(a[key], b[key]):
            worst = max(worst, float(np.max(np.abs(np.array(pa) - np.array(pb)))))
    for la, lb in zip(a["sel_length"], b["sel_length"]):
        worst = max(worst, abs(la - lb))
    return worst


_robust = {}


def robustness(name):
    """(every nudged `cut` run keeps the discrete outputs of the f64 run, the largest position disagreement) of a scene:
    the field replaced by its f32 rounding, as it is, moved by -2 and by +2 ulp, and by -2 .. +2 ulp per voxel at random"""
    if name not in _robust:
        sc = scenes()[name]
        base = run_ref(sc)
        ok, worst = True, 0.0
        fields = [f32_field(sc["blocks"], u) for u in (-2, 0, 2)] + [f32_field(sc["blocks"], 2, np.random.default_rng(7))]
        for d32 in fields:
            got = run_ref(sc, "cut", as_field_array(d32))
            for a, b in zip(base, got):
                if discrete(a) != discrete(b):
                    ok = False
                else:
                    worst = max(worst, disagreement(a, b))
        _robust[name] = (ok, worst)
    return _robust[name]
