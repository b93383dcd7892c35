"""The optimiser's dispatch plan (fuelmi_bspline_opt_plan, host only) at the edges of its table: which of the five solve
kernels a batch runs, with how much dynamic LDS, and where the LDS budget ends.  Both optimise calls launch from this
plan; test_bspline_variants_gpu asserts it before every case it runs."""
import numpy as np
import pytest

KIB = 1024
MINTIME = 1 << 8


@pytest.fixture(scope="module")
def fa():
    import __graft_entry__ as ge
    ge.build()
    import fuel_amd
    return fuel_amd


def plan(fa, N, dim=3, mintime=True, C=4):
    n = dim * N + (1 if mintime else 0)
    pb = fa.BsplineBatchProblem(np.zeros((C, n)), N, fa.NORMAL_PHASE | (MINTIME if mintime else 0), np.ones(C),
                                np.zeros((C, 3, 3)), np.zeros((C, 3, 3)), 3, dim, None if mintime else 0.2)
    return fa.BsplineOptimizer.optPlan(pb)


def reg_lds(N, n):
    return (27 * N + 32) * 8 + 2 * n * 8   # evaluation scratch + four-wave partials + variables and gradient


def lds_kernel_lds(N, n):
    return (15 * N + 24) * 8 + (22 * n + 16) * 8   # evaluation scratch + 6 + 2 x 8 work vectors + rho, alpha


@pytest.mark.parametrize("N, npl", [(42, 2), (43, 4), (85, 4), (86, 0)])
def test_dim3_mintime_kernel_edges(fa, N, npl):
    """n = 3 N + 1 = 127 / 130 / 256 / 259: the knot span lands in the last register slot at n = 256."""
    n = 3 * N + 1
    want = reg_lds(N, n) if npl else lds_kernel_lds(N, n)
    assert plan(fa, N) == (npl, 4 if npl else 1, want)


@pytest.mark.parametrize("N, npl", [(43, 4), (85, 4), (86, 0)])
def test_dim3_without_mintime_kernel_edges(fa, N, npl):
    n = 3 * N
    assert plan(fa, N, mintime=False)[:1] == (npl,)
    assert plan(fa, N, mintime=False)[2] == (reg_lds(N, n) if npl else lds_kernel_lds(N, n))


@pytest.mark.parametrize("N, npl", [(128, 2), (129, 4), (256, 4), (257, 0)])
def test_dim1_kernel_edges(fa, N, npl):
    assert plan(fa, N, dim=1, mintime=False) == (npl, 4 if npl else 1, reg_lds(N, N) if npl else lds_kernel_lds(N, N))


@pytest.mark.parametrize("N", [42, 85])
def test_waves_per_candidate_switch_at_256_candidates(fa, N):
    npl = 2 if N == 42 else 4
    assert plan(fa, N, C=256) == (npl, 4, reg_lds(N, 3 * N + 1))
    assert plan(fa, N, C=257) == (npl, 1, reg_lds(N, 3 * N + 1))
    assert plan(fa, 86, C=257)[:2] == (0, 1)


def test_lds_kernel_needs_the_attribute_from_101_points(fa):
    assert plan(fa, 100)[2] == lds_kernel_lds(100, 301) <= 64 * KIB
    assert plan(fa, 101)[2] == lds_kernel_lds(101, 304) > 64 * KIB
    assert max(plan(fa, N)[2] for N in (42, 85)) <= 64 * KIB and plan(fa, 256, dim=1, mintime=False)[2] <= 64 * KIB


def test_lds_kernel_budget_ends_at_253_points(fa):
    assert plan(fa, 252)[2] == lds_kernel_lds(252, 757) <= 160 * KIB
    with pytest.raises(fa.FuelmiError, match="error -5: 760 variables exceed the LDS budget"):
        plan(fa, 253)


def test_dim1_budget_ends_at_553_points(fa):
    assert plan(fa, 552, dim=1, mintime=False) == (0, 1, lds_kernel_lds(552, 552))
    with pytest.raises(fa.FuelmiError, match="error -5"):
        plan(fa, 553, dim=1, mintime=False)


def test_dim2_is_refused(fa):
    """The device clamped a dim-2 start point per axis i % 3 where the reference uses j, and the reference's bounds
    loop writes 3 N entries into a 2 N vector: neither optimise call takes dim 2."""
    with pytest.raises(fa.FuelmiError, match="error -1: .*not 2"):
        plan(fa, 20, dim=2)
