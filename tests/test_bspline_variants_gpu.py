"""All five B-spline solve kernels against the oracle at their edges (fuelmi_bspline_dev_optimize_timed and
fuelmi_bspline_optimize pick one from the variable count n and the candidate count C, test_bspline_plan_cpu pins that
table), and the cost kernel past the control-point counts the parity tests reach.

Every case first asserts the plan it runs under (BsplineOptimizer.optPlan): a detour to another kernel would still
match the oracle.  The core check is iterate agreement: on the distance-free objective the device and the oracle's
fo_bspline_optimize run the same box-projected L-BFGS with the same arithmetic apart from reduction order, so after k
evaluations they hold the same best point.  A wrong direction, a masked variable or a stale history pair still
optimises -- it fails here.  Whole solves on the full objective, bit-equality between the two call sites and across
batch sizes, the wall-clock cap and the LDS attribute shared by every caller complete the file."""
import numpy as np
import pytest

import helpers
from oracle import fuel_oracle as fo

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-4  # the combineCost bar of test_gpu_parity (ESDF terms: f32 distance field)
KS = (1, 2, 4, 8, 16)


@pytest.fixture(scope="module")
def fa():
    import fuel_amd
    assert fuel_amd.lib().fuelmi_device_count() > 0, "no GPU visible: the HIP path cannot run"
    return fuel_amd


@pytest.fixture(scope="module")
def env(fa):
    """the explored 20 x 20 x 5 map of test_gpu_parity with its ESDF, on both sides"""
    om, _, _, box = helpers.explored_oracle_map((20.0, 20.0, 5.0), 60, 40)
    gm = fa.SDFMap(tuple(om.cfg.map_size), box[0], box[1])
    gm.uploadOccupancy(om.occ)
    lo, hi = helpers.full_box(om.nvox)
    om.set_local_bound(lo, hi)
    gm.setLocalBound(lo, hi)
    om.inflate_local()
    om.update_esdf()
    gm.clearAndInflateLocalMap()
    gm.updateESDF3d()
    opt = fa.BsplineOptimizer()
    opt.setEnvironment(gm)
    yield om, gm, box, opt
    gm.close()


def dist_free(fa):
    return fa.SMOOTHNESS | fa.FEASIBILITY | fa.START | fa.END | fa.WAYPOINTS | fa.MINTIME


def yaw_flags(fa):
    return fa.SMOOTHNESS | fa.WAYPOINTS | fa.START | fa.END


class Prob:
    """One batch on both sides: the device problem and, per candidate, the oracle's arguments.

    dim 3: helpers.make_trajectories inside the box.  edges: every third candidate has three control points outside
    the shrunk box (the start clamp, then active bounds), candidates 1 / 2 start with knot spans 0.02 / 4.97.
    full: guide points and a view constraint as well (for the 0x1FF flag set).  dim 1: the yaw case of test_gpu_parity
    (unbounded variables, knot span 0.3, no MINTIME)."""

    def __init__(self, fa, box, dim, N, C, cf, seed, edges=False, full=False):
        rng = np.random.default_rng(seed)
        self.N, self.C, self.cf, self.dim = N, C, cf, dim
        widx = np.array([1, N // 2, N - 3], dtype=np.int32)
        self.wi = np.tile(widx, (C, 1))
        self.guide = self.view = None
        vargs = (None, None, None)
        if dim == 1:
            self.x = rng.normal(size=(C, N))
            self.ptd = np.array([fo.bspline_pt_dist(self.x[c].reshape(N, 1)) for c in range(C)])
            self.st = np.zeros((C, 3, 3))
            self.en = np.zeros((C, 3, 3))
            self.st[:, :, 0] = rng.normal(size=(C, 3))
            self.en[:, :, 0] = rng.normal(size=(C, 3))
            self.wp = np.zeros((C, 3, 3))
            self.wp[:, :, 0] = rng.normal(size=(C, 3))
            self.ks = 0.3
        else:
            lo, hi = np.array(box[0]), np.array(box[1])
            ctrl = helpers.make_trajectories(rng, C, N, lo + 0.5, hi - 0.5)
            if edges:
                for c in range(0, C, 3):
                    for j, i in enumerate((0, N // 2, N - 1)):
                        ax = (c + j) % 3
                        ctrl[c, i, ax] = hi[ax] + 0.3 if (c + j) % 2 else lo[ax] - 0.3
            mint = bool(cf & fa.MINTIME)
            self.x, self.ptd, self.st, self.en = helpers.bspline_inputs(ctrl, 0.175, mint)
            if mint and edges:
                self.x[1 % C, -1] = 0.02
                self.x[2 % C, -1] = 4.97
            self.wp = ctrl[:, widx + 1, :] + 0.2
            self.ks = 0.175
            if full:
                self.guide = ctrl[:, 3:N - 3, :] + 0.1
                vpt = ctrl[:, N // 2, :] + 0.5
                vdir = np.tile(np.array([0.5, 1.0, 0.2]), (C, 1))
                vidx = np.full(C, N // 2 + 1, dtype=np.int32)
                vargs = (vpt, vdir, vidx)
                self.view = vargs
        self.pb = fa.BsplineBatchProblem(self.x, N, cf, self.ptd, self.st, self.en, 3, dim, self.ks, None, self.guide,
                                         self.wp, self.wi, *vargs)

    def sub(self, fa, box, c0, c1):
        """the batch of candidates c0 .. c1-1 (same inputs)"""
        s = Prob.__new__(Prob)
        s.__dict__.update(self.__dict__)
        s.C = c1 - c0
        for k in ("x", "ptd", "st", "en", "wp", "wi"):
            setattr(s, k, getattr(self, k)[c0:c1])
        s.guide = None if self.guide is None else self.guide[c0:c1]
        s.view = None if self.view is None else tuple(v[c0:c1] for v in self.view)
        s.pb = fa.BsplineBatchProblem(s.x, s.N, s.cf, s.ptd, s.st, s.en, 3, s.dim, s.ks, None, s.guide, s.wp, s.wi,
                                      *(s.view or (None, None, None)))
        return s

    def _args(self, c, x):
        view = None if self.view is None else tuple(v[c] for v in self.view)
        guide = None if self.guide is None else self.guide[c]
        return (x, self.N, self.cf, self.ptd[c], self.st[c], self.en[c], 3, self.dim, self.ks, -1.0, guide,
                self.wp[c], self.wi[c], view)

    def cost_grad(self, om, c, x=None):
        return fo.bspline_cost_grad(om, *self._args(c, self.x[c] if x is None else x))

    def optimize(self, om, c, max_eval):
        return fo.bspline_optimize(om, *self._args(c, self.x[c]), max_eval=max_eval)


def rel(a, b):
    return abs(a - b) / max(1.0, abs(b))


# --------------------------------------------------------------------------------------------------------------------
# (a) the cost kernel past its tested range: loops over > 256 control points, the > 64 KiB attribute (N >= 303), the
# 160 KiB limit (N = 757 fits, 758 does not)
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [64, 65, 256, 257, 302, 303, 757])
def test_cost_kernel_at_large_point_counts(fa, env, N):
    om, gm, box, opt = env
    for name in ("dist_free", "NORMAL|MINTIME", "ALL"):
        cf = {"dist_free": dist_free(fa), "NORMAL|MINTIME": fa.NORMAL_PHASE | fa.MINTIME, "ALL": 0x1FF}[name]
        P = Prob(fa, box, 3, N, 3, cf, 1000 + N, full=(name == "ALL"))
        dev = opt.deviceProblem(P.pb)
        dev.eval()
        got = {"eval": dev.download()}
        dev.evalPinned(0)
        dev.evalPinned(1)
        got["pinned0"], got["pinned1"] = dev.collect(0), dev.collect(1)
        got["combineCost"] = opt.combineCost(P.pb)
        dev.close()
        worst = [0.0, 0.0]
        for c in range(P.C):
            co, go = P.cost_grad(om, c)
            for path, (cg, gg) in got.items():
                ec, eg = rel(cg[c], co), np.abs(gg[c] - go).max()
                worst = [max(worst[0], ec), max(worst[1], eg / max(1.0, np.abs(go).max()))]
                if name == "dist_free":  # no ESDF term: the same f64 arithmetic up to reduction order
                    assert ec <= 1e-9 and eg <= 1e-9 * max(1.0, np.abs(go).max()), (name, path, c, ec, eg)
                else:
                    assert ec <= 1e-6 and eg <= GRAD_TOL, (name, path, c, ec, eg)
        print("cost kernel N = %d %s: worst cost rel %.1e, gradient rel %.1e" % (N, name, *worst))


def test_cost_kernel_refuses_758_points_then_serves_again(fa, env):
    """N = 758 needs (27 N + 32) * 8 > 160 KiB: both paths refuse it on the host, before any launch
    (fuelmi_bspline_dev_create, bspline_oneshot); the same optimiser and map then serve an ordinary call."""
    om, gm, box, opt = env
    P = Prob(fa, box, 3, 758, 2, fa.NORMAL_PHASE | fa.MINTIME, 758)
    with pytest.raises(fa.FuelmiError, match="error -5: 758 control points"):
        opt.deviceProblem(P.pb)
    with pytest.raises(fa.FuelmiError, match="error -5: 758 control points"):
        opt.combineCost(P.pb)
    P = Prob(fa, box, 3, 32, 4, fa.NORMAL_PHASE | fa.MINTIME, 32)
    cg, gg = opt.combineCost(P.pb)
    dev = opt.deviceProblem(P.pb)
    dev.eval()
    cd, gd = dev.download()
    dev.close()
    for c in range(P.C):
        co, go = P.cost_grad(om, c)
        for a, b in ((cg, gg), (cd, gd)):
            assert rel(a[c], co) <= 1e-6 and np.abs(b[c] - go).max() <= GRAD_TOL


# --------------------------------------------------------------------------------------------------------------------
# (b) iterate agreement, every variant
# --------------------------------------------------------------------------------------------------------------------
# (id, dim, N, C, expected plan (npl, waves))
DIM3 = [
    ("r2x4-N42", 3, 42, 8, (2, 4)),
    ("r4x4-N43", 3, 43, 8, (4, 4)),
    ("r4x4-N85", 3, 85, 8, (4, 4)),
    ("r2x1-N42", 3, 42, 257, (2, 1)),
    ("r4x1-N85", 3, 85, 257, (4, 1)),
    ("lds-N86", 3, 86, 4, (0, 1)),
    ("lds-N86-C257", 3, 86, 257, (0, 1)),  # (many line searches: an Armijo decision near its threshold)
    ("lds-N101", 3, 101, 4, (0, 1)),
    ("lds-N252", 3, 252, 4, (0, 1)),
]
DIM1 = [("yaw-N%d-C%d" % (N, C), 1, N, C, ((2 if N <= 128 else 4 if N <= 256 else 0), (4 if N <= 256 and C <= 256
                                                                                             else 1)))
        for N in (128, 129, 256, 257) for C in (4, 257)]


def _plan(fa, P, want):
    npl, waves, lds = fa.BsplineOptimizer.optPlan(P.pb)
    assert (npl, waves) == want, (npl, waves, want)
    return lds


@pytest.mark.parametrize("case", DIM3 + DIM1, ids=[c[0] for c in DIM3 + DIM1])
def test_iterates_agree_with_the_oracle(fa, env, case):
    """after k = 1, 2, 4, 8, 16 evaluations: best cost, best x and evaluation count as the oracle's"""
    om, gm, box, opt = env
    tag, dim, N, C, want = case
    cf = dist_free(fa) if dim == 3 else yaw_flags(fa)
    P = Prob(fa, box, dim, N, C, cf, 77 + N + C, edges=True)
    _plan(fa, P, want)
    dev = opt.deviceProblem(P.pb)
    ec, ex, ee = (np.zeros((len(KS), C)) for _ in range(3))
    for j, k in enumerate(KS):
        xg, cg, eg = dev.optimize(max_eval=k)
        for c in range(C):
            xo, co, eo = P.optimize(om, c, k)
            ec[j, c] = rel(cg[c], co)
            ex[j, c] = np.abs(xg[c] - xo).max() / max(1.0, np.abs(xo).max())
            ee[j, c] = eg[c] - eo
    dev.close()
    print("iterates %s: worst (cost rel, x rel, evaluation difference) per k: %s" %
          (tag, "  ".join("%d: %.1e %.1e %d" % (k, ec[j].max(), ex[j].max(), np.abs(ee[j]).max())
                          for j, k in enumerate(KS))))
    assert (ee == 0).all(), ee
    assert ec[0].max() <= 1e-12
    assert ec[1:4].max() <= 1e-9 and ex[1:4].max() <= 1e-7
    assert ec[4].max() <= 1e-7 and ex[4].max() <= 1e-6  # (reduction order grows ~10x per 4 evaluations: r<2,4> 5e-11)


ARMIJO = [("yaw-N%d-C%d" % (N, C), N, C, want) for N, C, want in
          [(128, 4, (2, 4)), (128, 257, (2, 1)), (129, 4, (4, 4)), (129, 257, (4, 1)), (257, 4, (0, 1))]]


@pytest.mark.parametrize("case", ARMIJO, ids=[c[0] for c in ARMIJO])
def test_armijo_decision_at_its_threshold(fa, env, case):
    """With zero boundary states and waypoints the yaw objective is f = x.H.x / 2 (H read off the oracle's gradient),
    minimum at 0.  Started at s v, v a unit eigenvector (eigenvalue > 2), the first step -g / |g| lands on (s - 1) v
    with an Armijo ratio (f - fn) / (g.(x - xn)) of exactly 1 - 1 / (2 s): s is chosen for ratios 5e-4 (accepted with
    the constant 1e-4), 5e-5 (refused) and 0.2.  A wrong constant or a wrong sign flips a decision; the iterates part."""
    om, gm, box, opt = env
    tag, N, C, want = case
    P = Prob(fa, box, 1, N, C, yaw_flags(fa), 31 + N + C)
    for a in (P.st, P.en, P.wp):
        a[:] = 0.0
    P.ptd[:] = P.ptd[0]  # (pt_dist scales terms of H: one H for the batch)
    f0, b = P.cost_grad(om, 0, np.zeros(N))
    assert f0 == 0.0 and not b.any()
    H = np.empty((N, N))
    for i in range(N):
        e = np.zeros(N)
        e[i] = 1.0
        H[:, i] = P.cost_grad(om, 0, e)[1] - b
    H = 0.5 * (H + H.T)
    lam, V = np.linalg.eigh(H)
    z = np.random.default_rng(N).normal(size=N)  # (the objective really is that quadratic)
    assert rel(P.cost_grad(om, 0, z)[0], f0 + b @ z + 0.5 * z @ H @ z) <= 1e-9
    big = np.flatnonzero(lam > 2.5)
    assert len(big) >= 8
    for c in range(C):
        r = (5e-4, 5e-5, 0.2)[c % 3]
        P.x[c] = V[:, big[(c * 7) % len(big)]] / (2.0 * (1.0 - r))
    P.pb = fa.BsplineBatchProblem(P.x, N, P.cf, P.ptd, P.st, P.en, 3, 1, P.ks, None, None, P.wp, P.wi)
    _plan(fa, P, want)
    dev = opt.deviceProblem(P.pb)
    for k in (2, 3, 4, 8):
        xg, cg, eg = dev.optimize(max_eval=k)
        for c in range(C):
            xo, co, eo = P.optimize(om, c, k)
            assert eg[c] == eo and rel(cg[c], co) <= 1e-9, (tag, k, c, cg[c], co)
            assert np.abs(xg[c] - xo).max() <= 1e-7 * max(1.0, np.abs(xo).max()), (tag, k, c)
    dev.close()


# --------------------------------------------------------------------------------------------------------------------
# (c) whole solves and (d) the two call sites, every dim-3 variant
# --------------------------------------------------------------------------------------------------------------------
def _whole_solve_checks(fa, om, box, P, xg, cg, eg, max_eval=300):
    """the invariants of test_bspline_device_optimizer_against_oracle_lbfgs"""
    c0 = np.array([P.cost_grad(om, c)[0] for c in range(P.C)])
    assert eg.max() <= max_eval and eg.min() >= 1
    blo, bhi = np.array(box[0]) + 0.1, np.array(box[1]) - 0.1
    pts = xg[:, :-1].reshape(P.C, P.N, 3)
    assert (pts >= blo - 1e-12).all() and (pts <= bhi + 1e-12).all()
    assert (xg[:, -1] >= 0.0).all() and (xg[:, -1] <= 5.0).all()
    worse, gap = 0, 0.0
    for c in range(P.C):
        xo, co, eo = P.optimize(om, c, max_eval)
        assert cg[c] < 0.5 * c0[c] and co < 0.5 * c0[c], (c, cg[c], co, c0[c])
        chk, _ = P.cost_grad(om, c, xg[c])
        assert abs(chk - cg[c]) <= 1e-6 * max(1.0, abs(chk))
        gap = max(gap, cg[c] / co - 1.0)
        if cg[c] > co * 1.001 + 1e-9:
            worse += 1
    assert worse <= P.C // 8, (worse, P.C)
    return worse, gap


@pytest.mark.parametrize("case", DIM3, ids=[c[0] for c in DIM3])
def test_whole_solves_and_both_call_sites(fa, env, case):
    """NORMAL_PHASE | MINTIME, 300 evaluations: deviceProblem().optimize and the query-slot optimize run the same
    kernel from the same plan -- bit-equal results --, and both meet the whole-solve invariants against the oracle"""
    om, gm, box, opt = env
    tag, dim, N, C, want = case
    P = Prob(fa, box, 3, N, C, fa.NORMAL_PHASE | fa.MINTIME, 500 + N + C)
    _plan(fa, P, want)
    dev = opt.deviceProblem(P.pb)
    xg, cg, eg = dev.optimize(max_eval=300)
    dev.close()
    xq, cq, eq = opt.optimize(P.pb, max_eval=300)
    assert np.array_equal(xg, xq) and np.array_equal(cg, cq) and np.array_equal(eg, eq)
    worse, gap = _whole_solve_checks(fa, om, box, P, xg, cg, eg)
    print("whole solves %s: %d of %d above the oracle by > 0.1 %%, largest gap %.2e, mean evaluations %.1f" %
          (tag, worse, C, gap, eg.mean()))


@pytest.mark.parametrize("N, want", [(42, (2, 1)), (85, (4, 1))], ids=["r2x1", "r4x1"])
def test_narrow_kernels_give_a_candidate_the_same_answer_in_any_batch(fa, env, N, want):
    om, gm, box, opt = env
    P = Prob(fa, box, 3, N, 300, fa.NORMAL_PHASE | fa.MINTIME, 900 + N)
    Q = P.sub(fa, box, 0, 257)
    _plan(fa, P, want)
    _plan(fa, Q, want)
    res = []
    for R in (P, Q):
        dev = opt.deviceProblem(R.pb)
        res.append(dev.optimize(max_eval=300))
        dev.close()
    for a, b in zip(*res):
        assert np.array_equal(a[:257], b)


# --------------------------------------------------------------------------------------------------------------------
# (e) the wall-clock cap on the one-wave and LDS kernels (test_gpu_parity_r3's test for the four-wave one)
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N, C, want", [(42, 257, (2, 1)), (101, 16, (0, 1))], ids=["r2x1", "lds-N101"])
def test_wall_clock_cap(fa, env, N, C, want):
    om, gm, box, opt = env
    P = Prob(fa, box, 3, N, C, fa.NORMAL_PHASE | fa.MINTIME, 12 + N)
    _plan(fa, P, want)
    c0, _ = opt.combineCost(P.pb)
    dev = opt.deviceProblem(P.pb)
    x_full, c_full, e_full = dev.optimize(max_eval=300)
    x_gen, c_gen, e_gen = dev.optimize(max_eval=300, max_time=1.0)     # a generous cap changes nothing
    assert np.array_equal(x_gen, x_full) and np.array_equal(e_gen, e_full)
    x_cap, c_cap, e_cap = dev.optimize(max_eval=300, max_time=200e-6)
    dev.close()
    assert (e_cap >= 1).all() and (e_cap <= e_full).all() and e_cap.sum() < e_full.sum(), (e_cap, e_full)
    assert (c_cap <= c0 + 1e-9).all() and (c_cap >= c_full - 1e-9).all()
    for c in range(C):
        chk, _ = P.cost_grad(om, c, x_cap[c])
        assert abs(chk - c_cap[c]) <= 1e-6 * max(1.0, abs(chk))
    print("wall-clock cap %s: mean evaluations uncapped %.1f, capped at 200 us %.1f" % (N, e_full.mean(), e_cap.mean()))


# --------------------------------------------------------------------------------------------------------------------
# (f) the LDS kernel's attribute: a larger batch launches after smaller ones have run
# --------------------------------------------------------------------------------------------------------------------
def test_lds_kernel_attribute_does_not_follow_the_last_caller(fa, env):
    """batch A (N = 200, ~127 KiB), then batch B (N = 120, ~76 KiB), then a query-slot solve (N = 110, ~70 KiB), then
    A again: each caller used to set the attribute to its own size, so A's second launch ran under B's or the query's"""
    om, gm, box, opt = env
    cf = fa.NORMAL_PHASE | fa.MINTIME
    A = Prob(fa, box, 3, 200, 8, cf, 200)
    B = Prob(fa, box, 3, 120, 4, cf, 120)
    Q = Prob(fa, box, 3, 110, 4, cf, 110)
    la, lb, lq = (_plan(fa, P, (0, 1)) for P in (A, B, Q))
    assert la > lb > lq > 64 * 1024
    dev_a = opt.deviceProblem(A.pb)
    r_a1 = dev_a.optimize(max_eval=300)
    dev_b = opt.deviceProblem(B.pb)
    r_b = dev_b.optimize(max_eval=300)
    r_q = opt.optimize(Q.pb, max_eval=300)
    r_a2 = dev_a.optimize(max_eval=300)
    dev_a.close()
    dev_b.close()
    for u, v in zip(r_a1, r_a2):
        assert np.array_equal(u, v)
    for P, r in ((A, r_a1), (B, r_b), (Q, r_q)):
        _whole_solve_checks(fa, om, box, P, *r)


# --------------------------------------------------------------------------------------------------------------------
# (g) dim 2: cost and gradient only
# --------------------------------------------------------------------------------------------------------------------
def test_dim2_is_refused_by_both_optimise_calls(fa, env):
    """The reference sets up start point and bounds for 3 axes (bspline_optimizer.cpp:194-214; with dim 2 its bounds
    loop overruns a 2 N vector): both optimise calls refuse dim 2 before any launch; combineCost still serves it."""
    om, gm, box, opt = env
    rng = np.random.default_rng(2)
    C, N = 4, 20
    x = rng.normal(size=(C, 2 * N))
    ptd = np.array([fo.bspline_pt_dist(x[c].reshape(N, 2)) for c in range(C)])
    st = rng.normal(size=(C, 3, 3))
    en = rng.normal(size=(C, 3, 3))
    cf = fa.SMOOTHNESS | fa.START | fa.END
    pb = fa.BsplineBatchProblem(x, N, cf, ptd, st, en, 3, 2, 0.3)
    with pytest.raises(fa.FuelmiError, match="error -1: .*not 2"):
        opt.optimize(pb, max_eval=20)
    dev = opt.deviceProblem(pb)
    with pytest.raises(fa.FuelmiError, match="error -1: .*not 2"):
        dev.optimize(max_eval=20)
    dev.eval()
    cd, gd = dev.download()
    dev.close()
    cg, gg = opt.combineCost(pb)
    assert np.array_equal(cg, cd) and np.array_equal(gg, gd)
    for c in range(C):
        co, go = fo.bspline_cost_grad(om, x[c], N, cf, ptd[c], st[c], en[c], 3, 2, 0.3)
        assert rel(cg[c], co) <= 1e-9 and np.abs(gg[c] - go).max() <= 1e-9 * max(1.0, np.abs(go).max())
