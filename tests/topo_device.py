"""What the device tests of the topological path search share (tests/test_topo_path_gpu.py,
tests/test_topo_limits_gpu.py): the device map of a scene with its distance field read back, a call of
fuelmi_map_topo_paths over a scene's problems, and the bit-for-bit comparison of a device result with a result of the
restatement (tests/topo_ref.py)."""
import numpy as np

import topo_cases as tc
import topo_ref as tr

_maps = {}


def device_map(blocks):
    """(the device map of the blocks, its distance field as an [nx, ny, nz] f64 array)"""
    import fuel_amd
    key = repr(blocks)
    if key not in _maps:
        gm = fuel_amd.SDFMap(tc.MAP_SIZE, device=0)
        assert gm.nvox == tc.NVOX and np.array_equal(gm.origin, tc.ORIGIN) and gm.res == tc.RES
        gm.uploadOccupancy(tc.occupancy(blocks))
        gm.setLocalBound((0, 0, 0), tuple(v - 1 for v in tc.NVOX))
        gm.clearAndInflateLocalMap()
        gm.updateESDF3d()
        h = gm.syncHost(inflate=True, distance=True)
        assert np.array_equal(h["inflate"].reshape(tc.NVOX) == 1, tc.sources(blocks))
        dist = h["distance"].reshape(tc.NVOX)
        k = tc.squared_distance(tc.sources(blocks))
        if (k < 0).all():
            assert (dist > 1e30).all()
        else:
            want = tc.RES * np.sqrt(k.astype(np.float64))
            with np.errstate(over="ignore"):
                d32 = dist.astype(np.float32)
            assert np.array_equal(d32.astype(np.float64), dist)  # the mirror holds the device's f32 values
            assert np.all(np.abs(dist - want) <= 2 * np.spacing(want.astype(np.float32)).astype(np.float64))
        _maps[key] = (gm, dist)
    return _maps[key]


def close_maps():
    for gm, _ in _maps.values():
        gm.close()
    _maps.clear()


def cfg_of(sc):
    return {k: v for k, v in sc["cfg"].items() if k != "max_sample_num"}


def run(gm, sc, probs=None, **kw):
    probs = sc["probs"] if probs is None else probs
    return gm.topo_paths([p["start"] for p in probs], [p["end"] for p in probs], [tc.samples_of(sc, p) for p in probs],
                         [p["start_pts"] or None for p in probs], [p["end_pts"] or None for p in probs],
                         **dict(cfg_of(sc), **kw))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def assert_equal(out, b, r, cfg):
    """problem b of a device result against a result of the restatement, bit for bit.  Past max_nodes the graph's rows
    stop (n_nodes does not), and the neighbour ids stop at their 4 max_nodes slots: nb_off is clamped there"""
    mpp, maxn = cfg["max_path_points"], cfg["max_nodes"]
    over = any(len(p) > mpp for k in ("raw", "filt", "sel") for p in r[k]) or len(r["nodes"]) > maxn
    assert out["status"][b] == (-1 if over and r["status"] in (tr.OK, tr.NO_PATH) else r["status"])
    assert list(out["counts"][b]) == list(r["counts"]) and list(out["events"][b]) == list(r["events"])
    assert out["n_nodes"][b] == len(r["nodes"])
    assert len(out["nodes"][b]) == min(len(r["nodes"]), maxn)
    flat = [i for n in r["nodes"] for i in n[3]]
    off = np.minimum(np.cumsum([0] + [len(n[3]) for n in r["nodes"]]), 4 * maxn)
    for at, (got, want) in enumerate(zip(out["nodes"][b], r["nodes"][:maxn])):
        assert (got[0], got[1]) == (want[0], want[1]) and bits(got[2]) == bits(want[2])
        assert list(got[3]) == flat[off[at]:off[at + 1]]
    for key in ("raw", "filt", "sel"):
        lens = [int(v) for v in out[key + "_len"][b] if v > 0]
        assert lens == [len(p) for p in r[key]], key
        assert [int(v) for v in out[key + "_len"][b][len(lens):]] == [0] * (len(out[key + "_len"][b]) - len(lens)), key
        for got, want in zip(out[key][b], r[key]):
            assert bits(got) == bits(want[:mpp]), key
    assert bits(out["sel_length"][b][:len(r["sel"])]) == bits(r["sel_length"])
    assert not np.any(out["sel_length"][b][len(r["sel"]):])
