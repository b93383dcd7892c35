"""The frontier split (fuel_amd/csrc/frontier_split.hip) on axis-aligned clusters and at its table edges (GPU).

Every scene of tests/split_cases.py runs on the device against the oracle, in the device's cell order by the rules of
test_gpu_parity._assert_split_equal (the same pieces in the same order, cells as sets, means and boxes bit-equal,
filtered cells bit-equal) and in the reference's order by those of test_gpu_parity_r2._assert_exact_clusters (cells in
the same order as well).  tests/test_frontier_split_cpu.py proves from the oracle's trace that each scene reaches the
edge it is named after: the block-local tables of k_sp_sums and k_sp_stats overflowing into global atomics, 255 to 513
final pieces around the regrouping's switch and k_sp_rank's tile, six levels of recursion, leaves of 1, 2, 3 and 6
voxels, and covariances whose cross term is nothing but the order in which the f64 atomics arrived."""
import numpy as np
import pytest

import helpers
import split_cases as sc

pytestmark = pytest.mark.gpu

ORDERS = pytest.mark.parametrize("reference_order", [False, True], ids=["device_order", "reference_order"])
REPEATS = 5


@pytest.fixture(scope="module")
def fa():
    import fuel_amd
    fuel_amd.lib()
    return fuel_amd


class Device:
    """the device twin of a scene's oracle map (painted and inflated), with one finder on it"""

    def __init__(self, fa, run, reference_order=False, finder=None):
        vp = run.vp
        self.run = run
        self.gm = fa.SDFMap(vp.map_size, *vp.box_args(), **vp.map_kw)
        assert tuple(self.gm.nvox) == tuple(run.om.nvox)
        self.gf = fa.FrontierFinder(self.gm, split=True, reference_order=reference_order,
                                    **(finder or run.scene.finder))
        self.load(run)

    def load(self, run):
        self.gm.uploadOccupancy(run.om.occ)
        self.gm.setLocalBound(*helpers.full_box(run.om.nvox))
        self.gm.clearAndInflateLocalMap()

    def search(self):
        """a search of the whole map as a fresh finder would run it (the scratch of earlier searches stays)"""
        self.gf.reset()
        self.gm.setUpdatedBox(*helpers.vp_whole_map(self.run.om))
        return self.gf.searchFrontiers()

    def result(self, n):
        """everything a search delivers, as bytes: cells, average_ / box, filtered cells of every piece"""
        gf = self.gf
        cl = gf.clusters(0)
        assert len(cl) == n
        return [(c.tobytes(), b"".join(np.asarray(v, dtype=np.float64).tobytes() for v in gf.clusterInfo(0, k)),
                 gf.filtered(0, k).tobytes()) for k, c in enumerate(cl)]

    def close(self):
        self.gf.close()
        self.gm.close()


def _same_pieces(run, gf, n, reference_order, tag):
    ca, cb = run.pieces, gf.clusters(0)
    assert len(ca) == len(cb) == n, "%s: %d pieces, the oracle's %d" % (tag, len(cb), len(ca))
    for k in range(n):
        want = ca[k] if reference_order else np.sort(ca[k])
        assert np.array_equal(want, cb[k]), "%s: piece %d differs" % (tag, k)
        for x, y in zip(run.of.cluster_info(0, k), gf.clusterInfo(0, k)):
            assert np.array_equal(np.asarray(x), np.asarray(y)), "%s: average_ / box of piece %d" % (tag, k)
        fa_, fb_ = run.of.filtered(0, k), gf.filtered(0, k)
        assert fa_.shape == fb_.shape and len(fa_) > 0, "%s: filtered cells of piece %d" % (tag, k)
        assert np.array_equal(fa_.astype(np.float32), fb_), "%s: filtered cells of piece %d" % (tag, k)


def _valid_split(run, gf, n, tag):
    """what holds wherever the on-the-cut column is put: the pieces partition the region-grown clusters, every piece
    obeys cluster_size_xy, and every piece of a plate is a rectangle over the plate's whole short side -- a column
    that sits on a cut goes whole to one side"""
    pieces = gf.clusters(0)
    assert len(pieces) == n
    cells = np.concatenate(pieces)
    assert len(np.unique(cells)) == len(cells), "%s: a cell is in two pieces" % tag
    assert np.array_equal(np.sort(cells), np.sort(np.concatenate(run.roots))), "%s: not a partition" % tag
    root_of = {}
    for r, root in enumerate(run.roots):
        root_of.update((int(a), r) for a in root)
    size_xy = run.scene.finder["cluster_size_xy"]
    for k, piece in enumerate(pieces):
        assert len({root_of[int(a)] for a in piece}) == 1, "%s: piece %d spans two clusters" % (tag, k)
        mean = np.asarray(gf.clusterInfo(0, k)[0])
        f = gf.filtered(0, k).astype(np.float64)
        dist = np.sqrt((f[:, 0] - mean[0]) ** 2 + (f[:, 1] - mean[1]) ** 2)
        assert dist.max() <= size_xy, "%s: piece %d reaches %.17g beyond its mean" % (tag, k, dist.max())
        x, y = run.xy(piece)
        p = [q for q in run.scene.plates if q.holds(x[0], y[0])][0]
        assert p.kind in ("x", "y")
        lo, hi, span = (y, p.y0, x) if p.kind == "x" else (x, p.x0, y)
        width = p.b if p.kind == "x" else p.a
        assert (lo.min(), lo.max()) == (hi, hi + width - 1), "%s: piece %d leaves part of a column behind" % (tag, k)
        assert len(piece) == width * (span.max() - span.min() + 1), "%s: piece %d is no rectangle" % (tag, k)


@ORDERS
@pytest.mark.parametrize("name", list(sc.SCENES))
def test_scene_matches_oracle(fa, name, reference_order):
    run = sc.oracle_run(name, reference_order)
    assert run.scene.pred(run), "%s does not reach its edge" % name
    dev = Device(fa, run, reference_order)
    try:
        n = dev.search()
        assert n == len(run.pieces), "%s: %d pieces, the oracle's %d" % (name, n, len(run.pieces))
        if name in sc.ODD and not reference_order:
            # the oracle's mean and the device's may put the column that sits on the cut on different sides: piece for
            # piece only in the reference's order
            _valid_split(run, dev.gf, n, name)
        else:
            _same_pieces(run, dev.gf, n, reference_order, name)
    finally:
        dev.close()


@ORDERS
@pytest.mark.parametrize("name", sc.DIRECTION)
def test_direction_scenes_repeat_bit_for_bit(fa, name, reference_order):
    """five searches on one finder: the covariance sums arrive in another order every time, the pieces, their order,
    means, boxes and filtered cells must not move by a bit"""
    run = sc.oracle_run(name, reference_order)
    dev = Device(fa, run, reference_order)
    try:
        first = None
        for r in range(REPEATS):
            n = dev.search()
            assert n == len(run.pieces), "%s: search %d found %d pieces, the oracle %d" % (name, r, n, len(run.pieces))
            got = dev.result(n)
            first = first or got
            assert got == first, "%s: search %d differs from the first" % (name, r)
    finally:
        dev.close()


@ORDERS
def test_one_finder_large_small_large(fa, reference_order):
    """the largest scene, the smallest, the largest again on one finder (the split's scratch, tables and counters are
    sized by the first and reused): each search delivers what a fresh finder delivers, and what the oracle does"""
    large = sc.oracle_run(sc.LARGEST, reference_order)
    small = sc.oracle_run_as(sc.SMALLEST, sc.LARGEST, reference_order)  # (one finder: the large scene's parameters)
    assert len(small.pieces) > len(small.roots) == 1
    finder = large.scene.finder
    dev = Device(fa, large, reference_order, finder=finder)
    try:
        for step, run in enumerate((large, small, large)):
            dev.run = run
            dev.load(run)
            n = dev.search()
            fresh = Device(fa, run, reference_order, finder=finder)
            try:
                nf = fresh.search()
                assert n == nf > 0, "step %d: %d pieces, a fresh finder's %d" % (step, n, nf)
                assert dev.result(n) == fresh.result(nf), "step %d differs from a fresh finder" % step
            finally:
                fresh.close()
            _same_pieces(run, dev.gf, n, reference_order, "step %d" % step)
    finally:
        dev.close()
