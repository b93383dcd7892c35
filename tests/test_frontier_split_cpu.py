"""The frontier split on axis-aligned clusters and at its table edges, CPU half (no GPU).

tests/split_cases.py draws the scenes; here the oracle's split trace proves that each sits on the edge it was drawn for,
and the direction rule itself is examined: splitHorizontally's first principal direction of a straight or square
cluster must not depend on the order in which the covariance is summed (the device sums it with f64 atomics in
schedule order), must cut plates and lines across their long axis, and must leave every well-conditioned direction as
it was, bit for bit.  The figures these tests print are the ones DESIGN.md derives the snap threshold from."""
import functools
import math
import os

import numpy as np
import pytest

import helpers
import split_cases as sc
from oracle import fuel_oracle as fo
from oracle.ref_build import ref
from reference_tape import Tape

T = sc.T
ORDERS = pytest.mark.parametrize("reference_order", [False, True], ids=["device_order", "reference_order"])
N_PERM = 100
ANGLE_TOL = 1e-9      # rad: a cut of a plate or line against the perpendicular of its long axis
# the control's directions are well conditioned, not snapped: another summation order moves the covariance by a few
# ulps (nf * 2^-53 relative) and the angle by that over the conditioning |a - d, 2b| / tr >= 0.4 -- below 1e-12 rad
CONTROL_TOL = 1e-12


def parent_rule(c00, c01, c10, c11):
    """the direction as it was before the axis and isotropic zones were snapped: v = normalise(b, lambda - a)"""
    a, b, d = c00, 0.5 * (c01 + c10), c11
    tr, det = a + d, a * d - b * b
    disc = math.sqrt(max(tr * tr / 4 - det, 0.0))
    lam = tr / 2 + disc
    vx, vy = b, lam - a
    if abs(vx) + abs(vy) < 1e-300:
        vx, vy = lam - d, b
    if abs(vx) + abs(vy) < 1e-300:
        vx, vy = 1.0, 0.0
    n = math.sqrt(vx * vx + vy * vy)
    return vx / n, vy / n


def seq_cov(terms):
    """the covariance of (dx, dy) terms summed one by one in the given order, as splitHorizontally sums it"""
    dx, dy = terms[:, 0], terms[:, 1]
    s = [np.add.accumulate(v)[-1] for v in (dx * dx, dx * dy, dy * dx, dy * dy)]
    nf = float(len(terms))
    return tuple(float(v) / nf for v in s)


@functools.lru_cache(maxsize=None)
def resummed(name, reference_order):
    """[(plate, trace record, [covariance per order])] of every split node of a scene: the oracle's order, address
    order (x-major, like voxel addresses) and N_PERM seeded permutations"""
    run = sc.oracle_run(name, reference_order)
    rng = np.random.default_rng(20240 + len(name))
    out = []
    for row in run.split_nodes:
        t = run.node_terms(row)
        orders = [np.arange(len(t)), np.lexsort((t[:, 1], t[:, 0]))] + [rng.permutation(len(t)) for _ in range(N_PERM)]
        out.append((run.plate_of(row), row, [seq_cov(t[o]) for o in orders]))
    return out


@ORDERS
@pytest.mark.parametrize("name", list(sc.SCENES))
def test_scene_sits_on_its_edge(name, reference_order):
    run = sc.oracle_run(name, reference_order)
    assert sc.SCENES[name].pred(run), "%s does not reach its edge" % name
    # the split is a partition of the region-grown clusters, whatever else it is
    assert np.array_equal(np.sort(np.concatenate(run.pieces)), np.sort(np.concatenate(run.roots)))
    assert sum(len(p) for p in run.pieces) == sc.SCENES[name].cells


def test_coverage_names_every_scene():
    named = set()
    for edge, names in sc.COVERAGE.items():
        assert names, edge
        for n in names:
            assert n in sc.SCENES, (edge, n)
        named.update(names)
    assert named == set(sc.SCENES)
    assert all(a <= b for a, b in zip(sc.MAP_SIZE, (16.0, 14.0, 3.0)))
    for n in ("sums_fallback", "stats_fallback", "pieces_255", "pieces_256", "pieces_257", "pieces_513"):
        assert sc.SCENES[n].finder["cluster_min"] == 0
    assert sorted({sc.SCENES[n].finder["down_sample"] for n in sc.DIRECTION}) == [1, 2, 3, 6]
    assert sc.SCENES[sc.LARGEST].cells > 40 * sc.SCENES[sc.SMALLEST].cells


def test_trace_changes_nothing_and_is_off_by_default():
    scene = sc.SCENES["odd_ds3"]
    run = sc.oracle_run("odd_ds3")
    of = fo.OracleFrontier(run.om, split=True, canonical_order=True, **scene.finder)
    run.om.set_updated_box(*helpers.vp_whole_map(run.om))
    assert of.search() == len(run.pieces)
    rec, terms = of.split_trace()
    assert len(rec) == 0 and len(terms) == 0
    for k, p in enumerate(run.pieces):
        assert np.array_equal(of.clusters(0)[k], p)
        for x, y in zip(of.cluster_info(0, k), run.of.cluster_info(0, k)):
            assert np.array_equal(x, y)
        assert np.array_equal(of.filtered(0, k), run.of.filtered(0, k))
    # one record per splitHorizontally call, the sums re-summed from the terms are the trace's own
    assert len(run.rec) == 2 * len(run.split_nodes) + len(run.roots)
    for row in run.split_nodes:
        c = seq_cov(run.node_terms(row))
        assert list(c) == [row[T[k]] / row[T["nf"]] for k in ("sxx", "sxy", "syx", "syy")]
        assert fo.principal_dir(*c) == (row[T["pc_x"]], row[T["pc_y"]])
        assert row[T["n_pos"]] + row[T["n_neg"]] == row[T["cells"]]


@ORDERS
@pytest.mark.parametrize("name", sc.DIRECTION)
def test_direction_does_not_depend_on_the_summation_order(name, reference_order):
    """plates, lines and squares: the same bits, sign included, in the oracle's order, in address order and in 100
    seeded permutations.  The control is not snapped: its direction moves with the last bits of the sums, by less than
    CONTROL_TOL, and never changes sign."""
    checked = 0
    for plate, row, covs in resummed(name, reference_order):
        dirs = [fo.principal_dir(*c) for c in covs]
        if plate.kind == "oblique":
            ang = np.array([math.atan2(v[1], v[0]) for v in dirs])
            assert np.abs(ang - ang[0]).max() <= CONTROL_TOL, (name, plate.rect, np.abs(ang - ang[0]).max())
            continue
        assert len(set(dirs)) == 1, "%s %s depth %d: %d directions over %d summation orders, e.g. %s" % (
            name, plate.rect, row[T["depth"]], len(set(dirs)), len(dirs), sorted(set(dirs))[:3])
        checked += 1
    assert checked > 0 or name == "controls"


@ORDERS
@pytest.mark.parametrize("name", [n for n in sc.DIRECTION if n != "controls"])
def test_plates_are_cut_across_their_long_axis(name, reference_order):
    """every cut of a plate or line is perpendicular to its long axis within 1e-9 rad, the "dot >= 0" half is the one
    further along the axis, and every piece spans the whole short side"""
    run = sc.oracle_run(name, reference_order)
    for row in run.split_nodes:
        p = run.plate_of(row)
        if p.kind not in ("x", "y"):
            continue
        along, across = (row[T["pc_x"]], row[T["pc_y"]]) if p.kind == "x" else (row[T["pc_y"]], row[T["pc_x"]])
        assert along > 0 and math.atan2(abs(across), along) <= ANGLE_TOL, (name, p.rect, row[T["pc_x"]], row[T["pc_y"]])
        assert abs(row[T["n_pos"]] - row[T["n_neg"]]) <= min(p.a, p.b), (name, p.rect)
    for piece in run.pieces:
        x, y = run.xy(piece)
        p = [q for q in run.scene.plates if q.holds(x[0], y[0])][0]
        if p.kind == "x":
            assert (y.min(), y.max()) == (p.y0, p.y0 + p.b - 1), (name, p.rect, "piece does not span the short side")
            assert len(piece) == p.b * (x.max() - x.min() + 1)
        elif p.kind == "y":
            assert (x.min(), x.max()) == (p.x0, p.x0 + p.a - 1), (name, p.rect, "piece does not span the short side")
            assert len(piece) == p.a * (y.max() - y.min() + 1)


def test_isotropic_squares_get_one_fixed_direction():
    seen = set()
    for ds in sc.DOWN_SAMPLES:
        for reference_order in (False, True):
            run = sc.oracle_run("square_ds%d" % ds, reference_order)
            for plate, row, covs in resummed("square_ds%d" % ds, reference_order):
                if row[T["depth"]] == 0:
                    seen.update(fo.principal_dir(*c) for c in covs)
            assert sorted(len(p) for p in run.pieces) == [16 * 16] * 8   # x cut, then y cuts: four quarters per square
    assert seen == {(1.0, 0.0)}, sorted(seen)[:5]
    assert fo.principal_dir(2.0, 0.0, 0.0, 2.0) == (1.0, 0.0) and fo.principal_dir(0.0, 0.0, 0.0, 0.0) == (1.0, 0.0)


def test_noise_and_snap_threshold():
    """the figures behind the threshold: the largest |b| / |a - d| any summation order gives on a plate or
    line and the largest disc / tr it gives on a square -- residue of the f64 sums and of the float centroids -- lie
    below SNAP_TAU, by about as much as the smallest ratio of the explored worlds lies above it"""
    axis, iso = 0.0, 0.0
    for name in sc.DIRECTION:
        for reference_order in (False, True):
            for plate, row, covs in resummed(name, reference_order):
                for c00, c01, c10, c11 in covs:
                    a, b, d = c00, 0.5 * (c01 + c10), c11
                    if plate.kind in ("x", "y"):
                        axis = max(axis, abs(b) / abs(a - d))
                    elif plate.kind == "square" and row[T["depth"]] == 0:
                        iso = max(iso, math.sqrt(max((a + d) ** 2 / 4 - (a * d - b * b), 0.0)) / (a + d))
    print("largest |b| / |a - d| on plates and lines: %.3e; largest disc / tr on squares: %.3e" % (axis, iso))
    # NOISE_MAX is the figure as it was measured when the threshold was derived; another permutation seed or scene
    # offset moves it by some per cent, so what is held here is the margin that matters: a decade below the threshold
    assert 0.0 < axis <= sc.SNAP_TAU / 10 and 0.0 < iso <= sc.SNAP_TAU / 10
    assert sc.NOISE_MAX < sc.SNAP_TAU < sc.WORLD_MIN
    assert abs(math.log10(sc.SNAP_TAU) - 0.5 * (math.log10(sc.NOISE_MAX) + math.log10(sc.WORLD_MIN))) < 0.01


def test_explored_world_stays_outside_the_snap_zones():
    """the split nodes of an explored world (the one with the smallest ratio of those the parity tests run) are all
    well conditioned: none comes nearer to a zone than WORLD_MIN, so none of their directions is touched"""
    om, truth, frames, box = helpers.explored_oracle_map((16.0, 14.0, 4.0), 30, 28, seed=7)
    of = fo.OracleFrontier(om, cluster_min=60, cluster_size_xy=1.2, down_sample=3, split=True, canonical_order=True)
    of.trace_splits()
    om.set_updated_box(*om.get_updated_box(reset=False))
    of.search()
    rec, terms = of.split_trace()
    sp = rec[rec[:, T["split"]] == 1]
    assert len(sp) > 50
    ratios = np.array([sc.cov_ratios(row) for row in sp])
    print("smallest |b| / |a - d| %.3e, smallest max(|a - d|, |b|) / tr %.3e" % (ratios[:, 0].min(), ratios[:, 1].min()))
    assert ratios.min() >= sc.WORLD_MIN   # (the oracle is deterministic: 1.034e-3, a hundred times the threshold)
    for row in sp:
        nf = row[T["nf"]]
        c = [row[T[k]] / nf for k in ("sxx", "sxy", "syx", "syy")]
        assert (row[T["pc_x"]], row[T["pc_y"]]) == parent_rule(*c)


@pytest.fixture
def tape(request):
    t = Tape(request.node.name, ref.available(), os.environ.get("FUELMI_RECORD_REFERENCE") == "1")
    yield t
    t.close()


@pytest.mark.parametrize("name", [n for n, s in sc.SCENES.items() if s.finder["down_sample"] == 3])
def test_real_frontier_finder_agrees_on_the_scenes(tape, name):
    """the reference's own frontier_finder.cpp (down_sample 3 is its constant) over compat/Eigen/Eigenvalues gives the
    oracle's pieces on the scenes: the same cells in the same order, bit-equal averages, boxes and filtered cells --
    the stand-in and the oracle carry the same direction rule.  Where oracle/_ref was never built, the observations
    stored under tests/golden/reference/ stand in for it (tests/reference_tape.py)."""
    run = sc.oracle_run(name, True)
    rf = None
    if tape.live:
        rm = helpers.vp_map(run.vp, ref.RefMap)
        rm.occ[:] = run.om.occ
        rm.set_local_bound(*helpers.full_box(run.om.nvox))
        rm.inflate_local()
        rm.set_updated_box(*helpers.vp_whole_map(run.om))
        rf = ref.RefFrontier(rm, cluster_min=run.scene.finder["cluster_min"],
                             cluster_size_xy=run.scene.finder["cluster_size_xy"])
    n = len(run.pieces)
    tape.equal(n, lambda: rf.search())
    tape.equal(np.concatenate(run.pieces), lambda: np.concatenate(rf.clusters(0)))
    tape.equal([len(p) for p in run.pieces], lambda: [len(p) for p in rf.clusters(0)])
    tape.equal(np.array([np.concatenate(run.of.cluster_info(0, k)) for k in range(n)]),
               lambda: np.array([np.concatenate(rf.cluster_info(0, k)) for k in range(n)]))
    tape.equal(np.concatenate([run.of.filtered(0, k) for k in range(n)]),
               lambda: np.concatenate([rf.filtered(0, k) for k in range(n)]))


def test_well_conditioned_directions_keep_their_bits():
    """outside the zones the expression is the parent's, bit for bit; just inside them the axis is exact"""
    rng = np.random.default_rng(11)
    tau = sc.SNAP_TAU
    for _ in range(2000):
        a, d = rng.uniform(0.01, 10.0, 2)
        b = rng.uniform(-1.0, 1.0) * math.sqrt(a * d)
        if abs(b) <= 2 * tau * abs(a - d) or max(abs(a - d), abs(b)) <= 2 * tau * (a + d):
            continue
        assert fo.principal_dir(a, b, b, d) == parent_rule(a, b, b, d)
    for a, d in ((3.0, 0.2), (0.2, 3.0), (5.0, 0.0), (0.0, 5.0)):
        gap = abs(a - d)
        want = (1.0, 0.0) if a > d else (0.0, 1.0)
        for s in (1.0, -1.0):
            assert fo.principal_dir(a, s * 0.99 * tau * gap, s * 0.99 * tau * gap, d) == want
            b = s * 1.01 * tau * gap
            assert fo.principal_dir(a, b, b, d) == parent_rule(a, b, b, d) != want
    a = 2.0
    for s in (1.0, -1.0):
        for gap, b in ((0.99, 0.0), (0.0, 0.99), (0.99, 0.99), (-0.99, 0.5)):
            assert fo.principal_dir(a, s * b * tau * 2 * a, s * b * tau * 2 * a, a - gap * tau * 2 * a) == (1.0, 0.0)
        d = a * (1 + 2.2 * tau)   # a < d by more than the isotropic zone, b = 0: the y axis
        assert fo.principal_dir(a, 0.0, 0.0, d) == (0.0, 1.0)
