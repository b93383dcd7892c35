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


def forest(step):
    """pillars of one voxel every `step` voxels in x and y: with clearance 0 most samples see no guard and become one, so
    the graph runs to hundreds of nodes, which pruneGraph takes down to a mesh of some sixty"""
    return [((x, x + 1), (y, y + 1), (2, 22)) for x in range(6, 60, step) for y in range(6, 60, step)]


FOREST = dict(clearance=0.0, sample_inflate=(1.0, 3.0, 0.3), max_sample_num=1500)
FOREST10_MAX_NODES = (64, 2)  # one under forest10's pruned graph of 65 nodes; the first two rows alone hold over 8 ids
FOREST_PROB = dict(start=(-2.0, 0.02, 0.0), end=(2.0, 0.03, 0.0), start_pts=(), end_pts=())

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
        # the large graphs (tests/test_topo_limits_cpu.py holds what each reaches)
        "forest10": dict(blocks=forest(10), seed=5, cfg=dict(FOREST, max_raw_path=50, max_raw_path2=5), probs=[FOREST_PROB]),
        "forest14": dict(blocks=forest(14), seed=5, cfg=dict(FOREST), probs=[FOREST_PROB]),
    }
    for s in sc.values():
        s["cfg"] = dict(tr.DEFAULTS, **s["cfg"])
        s["samples"] = sample_stream(s["seed"], s["cfg"]["max_sample_num"])
    return sc


# the reference cannot express these: `undefined` is undefined behaviour there, `overflow` is about this library's strides
NOT_RECORDED = ("undefined", "overflow")


def sample_at(start, end, sample_inflate, pt):
    """getSample (:240-250) inverted: the three numbers of the stream that put a sample at pt"""
    s, e, pt = (np.array(v, dtype=np.float64) for v in (start, end, pt))
    mid = 0.5 * (s + e)
    x = (e - mid) / np.linalg.norm(e - mid)
    y = np.cross(x, (0.0, 0.0, -1.0))
    y /= np.linalg.norm(y)
    z = np.cross(x, y)
    r = (0.5 * np.linalg.norm(e - s) + sample_inflate[0], sample_inflate[1], sample_inflate[2])
    out = [float((pt - mid) @ a) / b for a, b in zip((x, y, z), r)]
    assert all(-1.0 <= v < 1.0 for v in out), out
    return out


def zigzag(n, span, y0, last_x=None):
    """n points that swing between x = span and x = -span, 1 cm further in y each (last_x: the last point's x)"""
    pts = [((-span if i % 2 else span), y0 + 0.01 * i, 0.0) for i in range(n)]
    if last_x is not None:
        pts[-1] = (last_x,) + pts[-1][1:]
    return tuple(pts)


# the hand-placed edge scenes' numbers (tests/test_topo_limits_cpu.py asserts from the witness trace what each reaches)
CAP256_D = (26.65, 26.75)         # metres the outside point lies before the start: 254 blocked points, and 255
CAP4096_SPAN = 1.55               # the zig-zags' half width: 32 points a swing
CAP4096_LAST_X = (-0.05, -0.15)      # x of the last end point: nd = 4096, and 4097
SAME_Y = (2.45, 2.5, 2.62, 2.69)  # the second sample's y: pt_num = 64, 65 between S0 and E0, 128, 129 between the corners
CORNER_S, CORNER_E = (-3.0, -3.0, 0.0), (3.0, -3.0, 0.0)
WIN_S = (-3.0, -1.0, 0.0)


def edge_scenes():
    """name -> a scene as scenes() gives it, every problem with its own hand-placed `samples` (but `reserve_over_raw2`).
    None is recorded from the reference: they are about the kernel's lane windows, strides, caps and rows"""
    def prob(start, end, pts, infl=tr.DEFAULTS["sample_inflate"], start_pts=(), end_pts=()):
        return dict(start=start, end=end, start_pts=tuple(start_pts), end_pts=tuple(end_pts),
                    samples=np.array([sample_at(start, end, infl, q) for q in pts]).reshape(-1, 3))

    one = dict(max_sample_num=1)
    lane63 = prob(WIN_S, (2.9, -1.0, 0.0), [(1.5, 2.4, 0.0)])
    wide = (1.0, 6.0, 1.0)
    low = (0.0, 0.05, 0.0)
    ok4096, over4096 = (prob(S0, E0, [(0.0, 0.3, 0.0)], start_pts=zigzag(64, CAP4096_SPAN, 1.0),
                             end_pts=zigzag(64, CAP4096_SPAN, -2.0, x)) for x in CAP4096_LAST_X)
    sc = {
        # shortcutPath's windows, round the pillar: one connector, one raw path
        "win_lane63": dict(blocks=PILLAR, cfg=one, probs=[lane63]),
        "win_clear_then_0": dict(blocks=PILLAR, cfg=one, probs=[prob(WIN_S, (2.9, -1.0, 0.0), [(1.6, 2.4, 0.0)])]),
        "win_62_then_0": dict(blocks=PILLAR, cfg=one, probs=[prob(WIN_S, (2.9, 0.5, 0.0), [(1.5, 2.3, 0.0)])]),
        "win_nd65": dict(blocks=PILLAR, cfg=one, probs=[prob((-3.0, -2.5, 0.0), (3.0, -2.5, 0.0), [(0.0, -1.4, 0.0)])]),
        "win_nd66": dict(blocks=PILLAR, cfg=one, probs=[prob((-3.0, -2.5, 0.0), (3.0, -2.5, 0.0), [(0.05, -1.3, 0.0)])]),
        # the rows of the path outputs cut at the longest path of the result, and one point before it
        "rows_exact": dict(blocks=PILLAR, cfg=dict(one, max_path_points=6), probs=[lane63]),
        "rows_one_less": dict(blocks=PILLAR, cfg=dict(one, max_path_points=5), probs=[lane63]),
        # sameTopoPath's strides: the first sample makes the connector, needConnection compares the second with it
        "same_strides": dict(blocks=[], cfg=dict(max_sample_num=2, sample_inflate=wide), probs=[
            prob(S0, E0, [low, (0.0, SAME_Y[0], 0.0)], wide), prob(S0, E0, [low, (0.0, SAME_Y[1], 0.0)], wide),
            prob(CORNER_S, CORNER_E, [(0.0, -2.95, 0.0), (0.0, SAME_Y[2], 0.0)], wide),
            prob(CORNER_S, CORNER_E, [(0.0, -2.95, 0.0), (0.0, SAME_Y[3], 0.0)], wide),
            prob((-0.75, 0.0, 0.0), (0.75, 0.0, 0.0), [low, (0.0, 0.5, 0.0)], wide)]),
        # two select paths that share 16 m from a point outside the map (a pass from there commits a point a step, comes
        # out longer and is rolled back: the paths keep the point)
        "same_long": dict(blocks=PILLAR, cfg=dict(max_sample_num=2, max_path_points=256), probs=[
            prob(S0, E0, [(0.0, 1.5, 0.0), (0.0, -1.5, 0.0)], start_pts=[(-18.0, 0.013, 0.0)])]),
        # on + 2 > 256: a ray from outside the map is blocked in its own voxel, where the gradient is zero
        "cap256": dict(blocks=[], cfg=one, probs=[prob(S0, E0, [(0.0, 0.3, 0.0)], start_pts=[(-2.0 - d, 0.013, 0.0)])
                                                  for d in CAP256_D]),
        # nd + count > 4096
        "cap4096": dict(blocks=[], cfg=one, probs=[ok4096, over4096]),
        # n_start / n_end of 0, 64 and 1 under one stride
        "stride_batch": dict(blocks=[], cfg=one, probs=[
            prob(S0, E0, [(0.0, 0.3, 0.0)]), ok4096,
            prob(S0, E0, [(0.0, -0.4, 0.0)], start_pts=[(-2.5, 0.4, 0.1)], end_pts=[(2.5, -0.4, 0.1)])]),
        # exist_paths_id is carved by max(max_raw_path2, reserve_num)
        "reserve_over_raw2": dict(blocks=TWO, cfg=dict(max_raw_path2=2, reserve_num=6), samples=sample_stream(9, 300), probs=[
            dict(start=S0, end=E0, start_pts=(), end_pts=()),
            dict(start=(-2.0, -0.6, 0.0), end=(2.0, 0.7, 0.2), start_pts=(), end_pts=()),
            dict(start=(-2.4, 1.0, 0.3), end=(1.0, -2.0, 0.0), start_pts=((-2.6, 1.2, 0.3),), end_pts=())]),
    }
    for s in sc.values():
        s["cfg"] = dict(tr.DEFAULTS, **s["cfg"])
        s.setdefault("seed", 0)
        s.setdefault("samples", None)
    return sc


def samples_of(sc, p):
    """a problem's sample stream: its own, or the scene's"""
    return p["samples"] if "samples" in p else sc["samples"]


def run_ref(sc, mode="f64", dist=None, traces=None):
    """the restatement on a scene: one result per problem (traces: a list that takes one witness trace per problem)"""
    f = tr.Field(ORIGIN, RES, field_of(sc["blocks"]) if dist is None else dist, mode)
    out = []
    for p in sc["probs"]:
        trace = None
        if traces is not None:
            trace = {}
            traces.append(trace)
        out.append(tr.find_topo_paths(f, sc["cfg"], p["start"], p["end"], samples_of(sc, p), p["start_pts"], p["end_pts"],
                                      trace=trace))
    return out


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


def _passes(trace):
    return [(p["nd"], [w[1:] for w in p["windows"]], p["committed"], p["rolled_back"]) for p in trace["shortcut"]]


def check_edge_claims(name, sc, results, traces):
    """what the edge scene `name` was made to reach, asserted from the witness traces of its problems (one per problem,
    of the restatement on whatever field the caller compares on): a scene that stops reaching its edge fails here"""
    first = _passes(traces[0])[0]
    longest = max([len(p) for k in ("raw", "filt", "sel") for p in results[0][k]] + [0])
    status = [r["status"] for r in results]
    if name == "win_lane63":  # the first blocked point in the last lane; then a block in a window that nd cuts to 30 lanes
        assert first[0] == 95 and first[1][:3] == [(64, 63), (30, 14), (15, 3)] and first[2] == 3, first
    elif name == "win_clear_then_0":  # a clear window, then the block in lane 0 of the next
        assert first[0] == 96 and first[1][:4] == [(64, None), (31, 0), (30, 14), (15, 1)] and first[2] == 3, first
        assert traces[0]["shortcut"][0]["windows"][1][0] == 65
    elif name == "win_62_then_0":  # two commits in a row, the second from the new back
        assert first[0] == 80 and first[1][:2] == [(64, 62), (16, 0)] and first[2] == 2, first
    elif name == "win_nd65":  # one full window and no other
        assert first[:2] == (65, [(64, None)]), first
    elif name == "win_nd66":  # a second window of one live lane
        assert first[:2] == (66, [(64, None), (1, None)]), first
    elif name == "rows_exact":
        assert status == [tr.OK] and longest == sc["cfg"]["max_path_points"], longest
    elif name == "rows_one_less":
        assert status == [tr.OK] and longest == sc["cfg"]["max_path_points"] + 1, longest
    elif name == "same_strides":  # needConnection's one comparison per problem
        assert [[c["pt_num"] for c in t["same_topo"]] for t in traces[:4]] == [[64], [65], [128], [129]]
        assert [c["pt_num"] <= 63 for c in traces[4]["same_topo"]] == [True]
        assert all(c["first_invisible"] is None for t in traces for c in t["same_topo"])
    elif name == "same_long":
        assert status == [tr.OK] and max(c["pt_num"] for c in traces[0]["same_topo"]) >= 3 * tr.LANES + 1
    elif name == "cap256":
        ok, over = _passes(traces[0])[-1], _passes(traces[1])[-1]
        # 254 blocked points and dis_path.back() fill the 256 slots; the pass comes out longer and is rolled back
        assert status[0] == tr.OK and ok[2] == tr.MAX_PATH_POINTS - 2 and ok[3] and results[0]["events"][5] == 1, ok
        assert [len(p) for p in results[0]["sel"]] == [3]
        # the 255th blocked point ends the problem
        assert status[1] == -1 and over[2] == tr.MAX_PATH_POINTS - 2 and not over[3], over
        assert sum(traces[1]["shortcut"][-1]["blocked"]) == tr.MAX_PATH_POINTS - 1
        assert results[1]["counts"][1:] == [0, 0, 0] and not (results[1]["raw"] or results[1]["filt"] or results[1]["sel"])
    elif name == "cap4096":
        assert status == [tr.OK, -1]
        assert tr.MAX_DIS_POINTS in [p[0] for p in _passes(traces[0])]
        assert _passes(traces[1])[-1][0] == tr.MAX_DIS_POINTS + 1
        assert results[1]["counts"][1:] == [0, 0, 0] and not (results[1]["raw"] or results[1]["filt"] or results[1]["sel"])
        assert all(len(p["start_pts"]) == len(p["end_pts"]) == 64 for p in sc["probs"])
    elif name == "stride_batch":
        assert [(len(p["start_pts"]), len(p["end_pts"])) for p in sc["probs"]] == [(0, 0), (64, 64), (1, 1)]
        assert status == [tr.OK] * 3 and tr.MAX_DIS_POINTS in [p[0] for p in _passes(traces[1])]
    elif name == "reserve_over_raw2":
        assert sc["cfg"]["reserve_num"] > sc["cfg"]["max_raw_path2"] and len(sc["probs"]) == 3
        assert all(r["counts"][1] == sc["cfg"]["max_raw_path2"] < r["counts"][0] and r["counts"][3] >= 1 for r in results)
    else:
        raise KeyError(name)


def check_forest_claims(name, sc, results, traces):
    """what the recorded large graphs reach, from the witness trace of their one problem"""
    g, s, cfg = traces[0]["graph"][0], traces[0]["search"][0], sc["cfg"]
    assert results[0]["status"] == tr.OK
    assert g["survivors"] == len(results[0]["nodes"]) and g["guards"] == 2 + results[0]["events"][1]
    if name == "forest10":
        assert g["nodes"] > 256 and g["survivors"] >= tr.LANES and g["rounds"] >= 2, g
        assert g["guards"] > 2 * tr.LANES and g["far_place"] >= 2 * tr.LANES, g  # a visible guard in the third chunk
        assert s["depth"] >= 15 and max(n for n, _, kept in s["buckets"] if kept) >= 15, s
        assert s["found"] == cfg["max_raw_path"] == results[0]["counts"][0]  # (the caller shows that a free search finds more)
        # a sameTopoPath call that only a later stride can decide
        assert max(c["first_invisible"] for c in traces[0]["same_topo"] if c["first_invisible"] is not None) >= tr.LANES
        assert max(c["pt_num"] for c in traces[0]["same_topo"]) > 2 * tr.LANES
    elif name == "forest14":
        assert g["rounds"] >= 3 and g["nodes"] > 2 * tr.LANES, g
        assert s["depth"] >= 15, s
        assert any(0 < kept < total for _, total, kept in s["buckets"]), s  # max_raw_path2 cuts inside a length bucket
        assert sum(kept for _, _, kept in s["buckets"]) == cfg["max_raw_path2"]
    else:
        raise KeyError(name)
