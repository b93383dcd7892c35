"""fuelmi_tsp_solve on the device against the restatement (tests/tsp_ref.py): the exact method and the local search
bit for bit, the default configuration on FUEL-like matrices, batching invariance, the headline G400 cycle, the
refusals, and the facade (FrontierFinder::findGlobalTour and the drop-in solveTSPLKH of libfuelmi_lkh.so)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import tsp_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


def _solver(**kw):
    import fuel_amd
    return fuel_amd.TourSolver(device=0, **kw)


def _edge_matrices(rng, d):
    """random, all-equal, all-zero, negative, and entries near 2^31 / d (int32 sums would overflow)"""
    big = (2 ** 31 - 1) // max(1, d)
    return [rng.integers(0, 1000, (d, d)), np.full((d, d), 7), np.zeros((d, d), np.int64),
            rng.integers(-1000, 1000, (d, d)), rng.integers(big - 50, big, (d, d)),
            rng.integers(0, 3, (d, d))]  # many ties


def _check_tour(c, o, cost):
    d = len(c)
    assert o[0] == 0 and sorted(o.tolist()) == list(range(d))
    assert int(cost) == tr.tour_cost(c, o.tolist())


# ---- 1. the exact method, bit for bit ------------------------------------------------------------------------------------
def test_exact_bit_for_bit():
    rng = np.random.default_rng(11)
    mats = []
    for d in range(1, 14):
        mats += _edge_matrices(rng, d)
    ts = _solver(exact_max=12)
    orders, costs, methods = ts.solve(mats)
    for c, o, v, m in zip(mats, orders, costs, methods):
        assert m == 0
        ro, rv = tr.held_karp(c)
        assert o.tolist() == ro and int(v) == rv, (len(c), o, ro, v, rv)
    # all-equal / all-zero: the lexicographically smallest optimal order is the identity
    for c, o in zip(mats, orders):
        if (c == c.flat[0]).all():
            assert o.tolist() == list(range(len(c)))
    ts.close()
    # exact_max at the cap: d = 17 (16 non-start nodes, an 8 MiB table each), a batch of them
    ts = _solver(exact_max=16)
    mats = _edge_matrices(rng, 17)[:4] + [rng.integers(0, 100, (d, d)) for d in (14, 15, 16)]
    orders, costs, methods = ts.solve(mats)
    for c, o, v, m in zip(mats, orders, costs, methods):
        assert m == 0
        ro, rv = tr.held_karp(c)
        assert o.tolist() == ro and int(v) == rv, len(c)
    ts.close()


# ---- 2. the heuristic, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [20, 60, 150])
def test_heuristic_bit_for_bit(d):
    rng = np.random.default_rng(d)
    mats = [rng.integers(0, 1000, (d, d)), rng.integers(-500, 500, (d, d)), rng.integers(0, 4, (d, d))]
    for seed in (0, 12345):
        ts = _solver(restarts=3, kicks=5, seed=seed)
        orders, costs, methods = ts.solve(mats)
        ts.close()
        for c, o, v, m in zip(mats, orders, costs, methods):
            assert m == 1
            ro, rv = tr.ils(c, 3, 5, seed)
            assert int(v) == rv and o.tolist() == ro, (d, seed, int(v), rv)


# ---- 3. the default configuration on FUEL-like matrices -----------------------------------------------------------------
def test_default_config_fuel_like():
    import fuel_amd
    rng = np.random.default_rng(5)
    mats = [fuel_amd.tour_matrix(tr.fuel_like_matrix(rng, n)) for n in (20, 60, 120)]
    ts = _solver()
    a = ts.solve(mats)
    b = ts.solve(mats)
    ts.close()
    for c, o, v, m in zip(mats, *a):
        assert m == 1
        _check_tour(c, o, v)
        assert tr.local_optimum_violations(c, o.tolist()) == []
    for x, y in zip(a[0], b[0]):
        assert x.tobytes() == y.tobytes()
    assert a[1].tobytes() == b[1].tobytes()


# ---- 4. batching invariance --------------------------------------------------------------------------------------------
def test_batching_invariance():
    rng = np.random.default_rng(9)
    dims = [1, 2, 3, 5, 9, 13, 14, 20, 33, 7, 48, 12, 64, 4, 90, 25]
    mats = [rng.integers(0, 1000, (d, d)) for d in dims]
    ts = _solver(restarts=8, kicks=6, seed=77)
    ob, cb, mb = ts.solve(mats)
    assert set(mb.tolist()) == {0, 1}
    for k, c in enumerate(mats):
        o1, c1, m1 = ts.solve([c])
        assert o1[0].tobytes() == ob[k].tobytes() and c1[0] == cb[k] and m1[0] == mb[k], k
    ts.close()


# ---- 5. the headline cycle -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g400_matrix():
    return tr.cycle_matrix("G400")


def test_headline_cycle(g400_matrix):
    import fuel_amd
    m = g400_matrix
    assert m.shape[0] >= 250, m.shape
    c = fuel_amd.tour_matrix(m)
    assert np.array_equal(c, np.array(tr.ref_int_matrix(m)))
    ts = _solver()
    (o,), (v,), (meth,) = ts.solve([c])
    (o2,), (v2,), _ = ts.solve([c])
    ts.close()
    assert meth == 1
    _check_tour(c, o, v)
    assert tr.local_optimum_violations(c, o.tolist()) == []
    assert o.tobytes() == o2.tobytes() and v == v2
    # a 13-node sub-matrix (the current state and 12 clusters): exact = the restatement; the heuristic forced on it
    # costs no less than the optimum
    sub = c[np.ix_(range(13), range(13))]
    ts = _solver()
    (oe,), (ve,), (me,) = ts.solve([sub])
    ts.close()
    ro, rv = tr.held_karp(sub)
    assert me == 0 and oe.tolist() == ro and int(ve) == rv
    ts = _solver(exact_max=3)
    (oh,), (vh,), (mh,) = ts.solve([sub])
    ts.close()
    assert mh == 1 and vh >= ve
    _check_tour(sub, oh, vh)
    print("G400: %d nodes, tour cost %d; 13-node sub-matrix: heuristic / optimum = %.4f" % (len(c), v, vh / max(1, ve)))


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals():
    import fuel_amd
    from fuel_amd import _lib
    L = fuel_amd.lib()
    EINVAL, ELIMIT = -1, -5
    for cfg in ((0, 5, 12), (4, -1, 12), (4, 5, 2), (4, 5, 17)):
        h = C.c_void_p(1234)
        assert L.fuelmi_tsp_create(0, C.byref(_lib.TspCfg(*cfg, 0)), C.byref(h)) == EINVAL, cfg
        assert h.value == 1234
    h = C.c_void_p()
    assert L.fuelmi_tsp_create(0, C.byref(_lib.TspCfg(4, 3, 12, 0)), C.byref(h)) == 0
    costs = np.arange(64, dtype=np.int32)
    order = np.full(64, -7, dtype=np.int32)
    cost = np.full(8, -9, dtype=np.int64)
    meth = np.full(8, -11, dtype=np.int32)

    def call(dim_ptr, n):
        dp = np.asarray(dim_ptr, dtype=np.int32)
        return L.fuelmi_tsp_solve(h, n, dp.ctypes.data_as(C.POINTER(C.c_int)),
                                  costs.ctypes.data_as(C.POINTER(C.c_int32)), order.ctypes.data_as(C.POINTER(C.c_int)),
                                  cost.ctypes.data_as(C.POINTER(C.c_int64)), meth.ctypes.data_as(C.POINTER(C.c_int)))
    cases = [([0, 2, 2], 2, EINVAL),            # a problem of dimension 0
             ([0, 3, 1], 2, EINVAL),            # negative dimension
             ([1, 3], 1, EINVAL),               # dim_ptr[0] != 0
             ([0, 1025], 1, ELIMIT),            # d > FUELMI_TSP_MAX_DIM
             (np.arange(2049) * 1024, 2048, ELIMIT)]  # 2^31 matrix entries (refused before any is read)
    for dp, n, rc in cases:
        assert call(dp, n) == rc, (dp, n)
        assert (order == -7).all() and (cost == -9).all() and (meth == -11).all()
    # still usable
    c = np.random.default_rng(1).integers(0, 100, (8, 8)).astype(np.int32)
    costs[:64] = c.reshape(-1)
    assert call([0, 8], 1) == 0
    ro, rv = tr.held_karp(c)
    assert order[:8].tolist() == ro and cost[0] == rv and meth[0] == 0
    L.fuelmi_tsp_destroy(h)


# ---- 7. the facade: findGlobalTour and the drop-in solveTSPLKH ------------------------------------------------------------
def _driver(*args):
    exe = os.path.join(ROOT, "fuel_amd", "facade", "facade_tsp")
    out = subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True, timeout=600).stdout
    res = {"row": []}
    for line in out.splitlines():
        f = line.split()
        if not f:
            continue
        if f[0] == "row":
            res["row"].append([float(v) for v in f[1:]])
        else:
            res[f[0]] = [int(v) for v in f[1:]]
    return res


def test_facade_global_tour_g400(tmp_path):
    import bench
    import fuel_amd
    map_size, box, occ, _, _ = bench.build_inputs("G400", seed=42)
    scen = tmp_path / "scen.bin"
    with open(scen, "wb") as f:
        np.array(list(map_size) + list(box[0]) + list(box[1]), dtype=np.float64).tofile(f)
        np.ascontiguousarray(occ, dtype=np.float64).tofile(f)
    del occ
    res = _driver(scen, tmp_path)
    mat = np.array(res["row"])
    n = res["clusters"][0]
    assert n >= 250 and mat.shape == (n + 1, n + 1)
    assert (mat[:, 0] == 0).all()
    # the Python route on the matrix the facade solved
    ts = fuel_amd.TourSolver(device=0)
    (o,), _, (meth,) = ts.solve([fuel_amd.tour_matrix(mat)])
    ts.close()
    want = (o[1:] - 1).tolist()
    assert meth == 1 and res["indices"] == want
    assert res["tour_points"][0] >= n + 1
    # the drop-in route: the reference's files, solveTSPLKH, the reference's parse
    assert (tmp_path / "single.tsp").read_text() == tr.write_tsp(mat)
    assert res["lkh_rc"] == [0] and res["lkh"] == want
    assert tr.read_tour((tmp_path / "single.txt").read_text()) == want


def test_facade_lkh_malformed_leaves_no_tour(tmp_path):
    res = _driver("--malformed", tmp_path)
    assert res["lkh_rc"][0] != 0 and res["tour_file"] == [0]
    assert not (tmp_path / "single.txt").exists()
