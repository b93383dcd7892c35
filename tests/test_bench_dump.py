"""bench.py --dump-outputs: two runs with the same arguments write the same files, float32 / float64 only, within the
64 MB cap, holding what the timed path computed (frontier cells, B-spline cost / gradient, the map buffers' sample)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_dump_outputs_are_identical_from_run_to_run(tmp_path):
    dirs, clusters = [], []
    for run in ("a", "b"):
        d = tmp_path / run
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "G100",
                            "--steps", "3", "--warmup", "1", "--regions", "1", "--no-cpu-baseline",
                            "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        dirs.append(d)
        clusters.append(json.loads(p.stdout.strip().splitlines()[-1])["config"]["frontier_clusters"])
    assert clusters[0] == clusters[1]
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1]))
    wants = ["bspline_cost.npy", "bspline_grad.npy", "map_distance.npy", "map_inflate.npy", "map_occupancy.npy"]
    if clusters[0] > 0:
        wants.append("frontier_tmp_frontiers_cells.npy")
    for want in wants:
        assert want in names, (want, names)
    assert sum(os.path.getsize(os.path.join(dirs[0], n)) for n in names) <= 64 << 20
    for n in names:
        a, b = np.load(os.path.join(dirs[0], n)), np.load(os.path.join(dirs[1], n))
        assert a.dtype in (np.float32, np.float64), (n, a.dtype)
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), n
    assert np.load(os.path.join(dirs[0], "bspline_cost.npy")).shape == (64,)


def test_dump_outputs_fit_the_budget_with_large_frontier_lists(tmp_path):
    """CPU: three frontier lists of 3M cells each and a 16M-voxel map still fit the budget given (the share of one
    rank): the voxel sample takes at most half of it, the cell lists are sampled in proportion to their lengths."""
    import bench

    class Map:
        N = 16 << 20

        def syncHost(self, **kw):
            (key,) = kw
            return {key: np.arange(self.N, dtype=np.int8 if key == "inflate" else np.float64)}

    class Finder:
        def clusters(self, which):
            return [np.arange(k << 20, (k + 1) << 20, dtype=np.int32) + which for k in range(3)]

    class Problem:
        def download(self):
            return np.zeros(64), np.ones((64, 97))

    class Cycle:
        map, ff, dev_problem = Map(), Finder(), Problem()

        def finish(self):
            pass

    for budget in (bench.DUMP_BYTES_MAX, bench.DUMP_BYTES_MAX // 4):
        out = tmp_path / str(budget)
        bench.dump_outputs(Cycle(), str(out), budget=budget)
        files = {n: np.load(os.path.join(out, n)) for n in os.listdir(out)}
        assert sum(a.nbytes for a in files.values()) <= budget
        assert sum(files[n].nbytes for n in files if n.startswith("map_")) <= budget // 2
        cells = [files["frontier_%s_cells.npy" % n] for n in ("tmp_frontiers", "frontiers", "dormant_frontiers")]
        assert len({len(c) for c in cells}) == 1 and len(cells[0]) > 0
        assert all(np.all(np.diff(c) > 0) for c in cells)  # a sample of the list, in its order
