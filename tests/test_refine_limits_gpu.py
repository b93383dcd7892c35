"""fuelmi_map_refine_tours at FUELMI_REFINE_MAX_NODES (256 nodes a layer: four predecessor strides per lane, 64 nodes
per wave, byte parents up to 255) and FUELMI_REFINE_MAX_LAYERS (64: the last parent row), against the restatement
(tests/refine_ref.py) fed with the device's own path lengths, on an open map where every edge is a straight line."""
import numpy as np
import pytest

import refine_ref as rr
from test_refine_gpu import SMALL, VM, WDIR, YD, _assert_same, _device_world, _near_ties, _refine, _restated

pytestmark = pytest.mark.gpu
LO, HI = np.array([-3.5, -3.5, 0.3]), np.array([3.5, 3.5, 2.0])  # (higher, a ray may step past the box top)


@pytest.fixture(scope="module")
def open_map():
    gm = _device_world(*SMALL)
    yield gm
    gm.close()


def _layers(rng, sizes):
    return [np.concatenate([LO + (HI - LO) * rng.random((n, 3)), rng.uniform(-3.1, 3.1, (n, 1))], axis=1)
            for n in sizes]


def _wide(seed):
    rng = np.random.default_rng(seed)
    return (np.array([0.2, -0.1, 1.2]), np.array([0.4, 0.3, -0.1]), 0.7, _layers(rng, [256] * 4))


def _deep(seed):
    rng = np.random.default_rng(seed)
    return (np.array([-1.0, 0.5, 1.0]), np.array([0.0, -0.5, 0.2]), -1.2, _layers(rng, rng.integers(3, 9, 64)))


def _tie(mu, mv):
    """layer 0: 256 nodes, those from mu on at one point and yaw (every one of them the same total), the rest
    farther; layer 1 (the goal layer, argmin): the same split at mv.  The answer must be (mu, mv)."""
    near0, far0 = np.array([1.0, 0.5, 1.2, 0.3]), np.array([3.0, -3.0, 2.4, 0.3])
    near1, far1 = np.array([-1.5, 2.0, 0.8, -0.4]), np.array([-3.4, -3.4, 0.4, -0.4])
    l0 = np.array([far0 if i < mu else near0 for i in range(256)])
    l1 = np.array([far1 if i < mv else near1 for i in range(256)])
    return (np.array([0.0, 0.0, 1.0]), np.zeros(3), 0.3, [l0, l1])


TIES = [(0, 0), (63, 1), (64, 2), (127, 3), (128, 4), (191, 67), (192, 130), (255, 255)]


def _check_restated(gm, prob, argmin, exact):
    pos, vel, yaw, layers = prob
    g, cost, ch, c, kind = _restated(gm, pos, vel, yaw, layers, argmin)
    assert (kind == 0).all()
    if not exact:
        assert _near_ties(g, cost, ch) == []
    (dev_ch,), dev_c, _ = _refine(gm, [prob], last_argmin=argmin)
    _assert_same(dev_ch, dev_c[0], ch, c, exact=exact)
    return list(dev_ch)


# ---- 1. four layers of 256 nodes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("argmin", [False, True])
def test_four_full_layers(open_map, argmin):
    ch = _check_restated(open_map, _wide(1), argmin, exact=False)
    assert open_map.path_stats()["launches"] == 0  # straight lines only
    assert len(ch) == 4 and min(ch) >= 0


# ---- 2. 64 layers: the last parent row ----------------------------------------------------------------------------------
@pytest.mark.parametrize("argmin", [False, True])
def test_sixty_four_layers(open_map, argmin):
    ch = _check_restated(open_map, _deep(2), argmin, exact=False)
    assert len(ch) == 64 and min(ch) >= 0


# ---- 3. 64 x 256 (4.2 M edges): batching invariance, the chosen route's cost, the restated ends -----------------------
def test_sixty_four_full_layers(open_map):
    gm = open_map
    rng = np.random.default_rng(3)
    pos, vel, yaw = np.array([0.0, 0.0, 1.4]), np.zeros(3), 0.0  # no velocity: every edge cost is exact in f64
    layers = _layers(rng, [256] * 64)
    big = (pos, vel, yaw, layers)
    small = [_deep(5), _wide(6)]
    ch, c, _ = _refine(gm, [big] + small + [big], last_argmin=True)
    assert np.array_equal(ch[0], ch[3]) and c[0].tobytes() == c[3].tobytes()
    (ch1,), c1, _ = _refine(gm, [big], last_argmin=True)
    assert gm.path_stats()["launches"] == 0  # 4.2 M straight lines
    assert np.array_equal(ch[0], ch1) and c[0].tobytes() == c1[0].tobytes()
    for k, p in enumerate(small):
        (chk,), ck, _ = _refine(gm, [p], last_argmin=True)
        assert np.array_equal(ch[k + 1], chk) and c[k + 1].tobytes() == ck[0].tobytes()
    # the cost is the left-to-right sum of the chosen route's edges (lengths: the device's straight lines)
    route = [pos] + [layers[i][ch1[i], :3] for i in range(64)]
    yaws = [yaw] + [layers[i][ch1[i], 3] for i in range(64)]
    L, K, _ = gm.path_costs(np.array(route[:-1]), np.array(route[1:]), max_points=0)
    assert (K == 0).all()
    total = 0.0
    for i in range(64):
        total = total + rr.compute_cost(L[i], route[i], route[i + 1], yaws[i], yaws[i + 1], (0.0, 0.0, 0.0), VM, YD,
                                        WDIR)
    assert c1[0] == total
    assert max(ch1) >= 128
    # the reference cannot price 4.2 M edges here: its first 4 and its last 4 layers (from the chosen node of layer 59)
    # as problems of their own
    _check_restated(gm, (pos, vel, yaw, layers[:4]), True, exact=True)
    p59 = layers[59][ch1[59]]
    _check_restated(gm, (p59[:3], np.zeros(3), p59[3], layers[60:]), True, exact=True)
    (tail,), _, _ = _refine(gm, [(p59[:3], np.zeros(3), p59[3], layers[60:])], last_argmin=True)
    assert list(tail) == list(ch1[60:])  # Bellman: the best route's tail is the best route from its node


# ---- 4. ties across strides, lanes and waves -----------------------------------------------------------------------------
def test_full_width_ties(open_map):
    gm = open_map
    probs = [_tie(mu, mv) for mu, mv in TIES]
    ch, c, _ = _refine(gm, probs, last_argmin=True)
    for (mu, mv), p, chb, cb in zip(TIES, probs, ch, c):
        assert list(chb) == [mu, mv], (mu, mv, chb)
        g, cost, rch, rc, _ = _restated(gm, *p, argmin=True)
        assert rch == [mu, mv] and cb == rc
        # every near node of layer 0 gives layer 1's node the same total
        v = g.layer_ids[1][mv]
        tot = {cost[(0, u)] + cost[(u, v)] for u in g.layer_ids[0][mu:]}
        assert len(tot) == 1


# ---- 5. a mixed batch against each problem alone -------------------------------------------------------------------------
def test_mixed_batch(open_map):
    gm = open_map
    rng = np.random.default_rng(8)
    probs = [_wide(11), _deep(12), _tie(64, 2), _tie(255, 255)]
    probs += [(LO + (HI - LO) * rng.random(3), rng.normal(size=3), 0.1 * k, _layers(rng, rng.integers(1, 6, 3)))
              for k in range(4)]
    order = [0, 4, 1, 5, 2, 6, 3, 7]
    for argmin in (False, True):
        batch = [probs[k] for k in order]
        ch, c, _ = _refine(gm, batch, last_argmin=argmin)
        for j, p in enumerate(batch):
            (ch1,), c1, _ = _refine(gm, [p], last_argmin=argmin)
            assert np.array_equal(ch[j], ch1) and c[j].tobytes() == c1[0].tobytes(), (argmin, j)
