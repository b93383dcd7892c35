"""fuelmi_tsp_solve at its size limits against the restatement (tests/tsp_ref.py): the heuristic bit for bit at
d = 5 .. 1024 (two chunk positions per lane in ils_prefix past 512, the float row split of ils_descend near 7 d^2
moves, more than one candidate per lane in the nearest-neighbour start), entries near +-2^31 / d, Held-Karp across
table chunks, and batching invariance at the largest sizes.  The large instances are tr.planted_matrix: a random
1024-node matrix needs hundreds of improving moves from the nearest-neighbour start, too many to restate; the planted
ones need 10 to 30 of every kind (tests/test_tour_limits_cpu.py)."""
import numpy as np
import pytest

import tsp_ref as tr

pytestmark = pytest.mark.gpu

SMALL = (5, 6)
LARGE = (511, 512, 513, 1000, 1023, 1024)
SEEDS = (0, 12345)
RESTARTS = 2


def kicks_for(d):
    """two kicks (a rejected kick returns to the best tour) up to 600; one beyond, to keep the restatement short"""
    return 2 if d <= 600 else 1


def heuristic_matrix(d):
    if d < 64:
        return np.random.default_rng(d).integers(0, 1000, (d, d)).astype(np.int64)
    return tr.planted_matrix(d, d)[0]


def extreme(c, d):
    """c mapped affinely onto [-(2^31-1)//d, (2^31-1)//d]: every move keeps d edges, so the moves are c's"""
    big = (2 ** 31 - 1) // d
    lo, hi = int(c.min()), int(c.max())
    a = (2 * big) // max(1, hi - lo)
    out = -big + (c - lo) * a
    assert out.min() >= -big and out.max() <= big
    return out


def _solver(**kw):
    import fuel_amd
    return fuel_amd.TourSolver(device=0, **kw)


def _starts(mats):
    return [tr.local_search(c, tr.nearest_neighbour(c)) for c in mats]


@pytest.fixture(scope="module")
def heuristic_refs():
    """{d: (matrix, {seed: (order, cost)})} with restarts 2 and kicks_for(d); the start is shared by both seeds"""
    out = {}
    for d in SMALL + LARGE:
        c = heuristic_matrix(d)
        (start,) = _starts([c])
        out[d] = (c, {s: tr.ils(c, RESTARTS, kicks_for(d), s, start=start) for s in SEEDS})
    return out


# ---- 1. the heuristic bit for bit up to FUELMI_TSP_MAX_DIM ---------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_heuristic_bit_for_bit_large_d(heuristic_refs, seed):
    for k in sorted({kicks_for(d) for d in heuristic_refs}):
        dims = [d for d in heuristic_refs if kicks_for(d) == k]
        mats = [heuristic_refs[d][0] for d in dims]
        ts = _solver(restarts=RESTARTS, kicks=k, exact_max=3, seed=seed)
        orders, costs, methods = ts.solve(mats)
        ts.close()
        for d, c, o, v, m in zip(dims, mats, orders, costs, methods):
            ro, rv = heuristic_refs[d][1][seed]
            assert m == 1
            assert int(v) == rv and o.tolist() == ro, (d, seed, int(v), rv)
            assert rv == tr.tour_cost(c, ro)


# ---- 2. entries near +-2^31 / d ------------------------------------------------------------------------------------------
def test_heuristic_extreme_entries():
    rng = np.random.default_rng(31)
    big20 = (2 ** 31 - 1) // 20
    mats = [rng.integers(-big20, big20 + 1, (20, 20)).astype(np.int64),
            extreme(tr.planted_matrix(600, 600)[0], 600),
            np.full((600, 600), (2 ** 31 - 1) // 600, dtype=np.int64)]
    assert mats[1].min() < -(2 ** 31 - 1) // 600 + 5000 and mats[1].max() > (2 ** 31 - 1) // 600 - 5000
    starts = _starts(mats)
    for seed in SEEDS:
        ts = _solver(restarts=RESTARTS, kicks=2, exact_max=3, seed=seed)
        orders, costs, methods = ts.solve(mats)
        ts.close()
        for c, st, o, v, m in zip(mats, starts, orders, costs, methods):
            ro, rv = tr.ils(c, RESTARTS, 2, seed, start=st)
            assert m == 1 and int(v) == rv and o.tolist() == ro, (len(c), seed, int(v), rv)
    # all equal: nothing improves on the nearest-neighbour start, the identity
    assert orders[2].tolist() == list(range(600)) and int(costs[2]) == 600 * ((2 ** 31 - 1) // 600)


# ---- 3. Held-Karp across table chunks -------------------------------------------------------------------------------------
def test_exact_across_table_chunks():
    rng = np.random.default_rng(17)
    d17 = [rng.integers(0, 1000, (17, 17)) for _ in range(17)]
    others = {1: rng.integers(0, 9, (1, 1)), 2: rng.integers(0, 1000, (2, 2)), 14: rng.integers(0, 1000, (14, 14)),
              16: rng.integers(-500, 500, (16, 16)), 20: rng.integers(0, 1000, (20, 20)),
              40: rng.integers(0, 1000, (40, 40))}
    # the ninth d = 17 table opens the second 64 MiB chunk; the small ones and the heuristic ones fall in between
    mats = d17[:3] + [others[1]] + d17[3:6] + [others[20], others[14]] + d17[6:9] + [others[2]] + d17[9:13] + \
        [others[40], others[16]] + d17[13:]
    ts = _solver(restarts=2, kicks=2, exact_max=16, seed=5)
    orders, costs, methods = ts.solve(mats)
    for c, o, v, m in zip(mats, orders, costs, methods):
        if len(c) <= 17:
            ro, rv = tr.held_karp(c)
            assert m == 0 and o.tolist() == ro and int(v) == rv, len(c)
        else:
            assert m == 1
        o1, v1, m1 = ts.solve([c])
        assert o1[0].tobytes() == o.tobytes() and v1[0] == v and m1[0] == m, len(c)
    # exactly eight d = 17 tables fill one chunk (the limit is >, not >=)
    eight = d17[9:17]
    orders, costs, methods = ts.solve(eight)
    ts.close()
    for c, o, v, m in zip(eight, orders, costs, methods):
        ro, rv = tr.held_karp(c)
        assert m == 0 and o.tolist() == ro and int(v) == rv


# ---- 4. batching invariance at the top ----------------------------------------------------------------------------------
def test_batching_invariance_at_the_top(heuristic_refs):
    rng = np.random.default_rng(4)
    mats = [heuristic_refs[1024][0], heuristic_refs[513][0], rng.integers(0, 1000, (17, 17)),
            rng.integers(0, 1000, (1024, 1024))]
    ts = _solver(restarts=3, kicks=2, exact_max=16, seed=9)
    ob, cb, mb = ts.solve(mats)
    assert mb.tolist() == [1, 1, 0, 1]
    for k, c in enumerate(mats):
        o1, c1, m1 = ts.solve([c])
        assert o1[0].tobytes() == ob[k].tobytes() and c1[0] == cb[k] and m1[0] == mb[k], k
        assert int(cb[k]) == tr.tour_cost(c, ob[k].tolist())
    ts.close()
    # the random 1024-node answer is a local optimum of both neighbourhoods
    assert tr.local_optimum_violations(mats[3], ob[3].tolist()) == []
