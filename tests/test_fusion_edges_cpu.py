"""The scenarios of tests/fusion_edges.py without a GPU: (1) every scenario reaches the edge it is drawn for, asserted
from the numpy restatements of the ray set-up and the cube placement -- a scenario that drifts off its edge fails here
by name; (2) on every scenario the oracle equals the REAL reference bit for bit (occupancy, local bound, updated box at
the compare frames, and for the lane rays every walked cell), live where oracle/_ref is built and against the
observations stored under tests/golden/reference/ elsewhere (tests/reference_tape.py)."""
import os

import numpy as np
import pytest

import fusion_edges as fe
from oracle import fuel_oracle as fo
from oracle.ref_build import ref
from reference_tape import Tape

LIVE = ref.available()


@pytest.fixture
def tape(request):
    t = Tape(request.node.name, LIVE, os.environ.get("FUELMI_RECORD_REFERENCE") == "1")
    yield t
    t.close()


def oracle_map(sc):
    return fo.OracleMap(sc["map_size"], *fe.exploration_box(sc), **sc["map_kw"])


def bound_box(m):
    lo, hi = m.get_local_bound()
    return np.array(lo + hi)


# ---- the plan call ----
def test_insert_plan_is_host_only_and_consistent():
    import ctypes as C
    import fuel_amd
    p = fuel_amd.SDFMap.insertPlan()
    assert p == fe.PLAN and all(v > 0 for v in (fe.LANES, fe.RAY_SLOTS, fe.CLASSIFY_SLOTS) + tuple(fe.CUBE))
    assert fe.LANES * fe.RAY_SLOTS <= fe.CLASSIFY_SLOTS and fe.CLASSIFY_SLOTS % fe.RAY_SLOTS == 0
    assert fe.CUBE[0] == fe.CUBE[1] and fe.CUBE[2] <= 32  # (one 32-bit LDS word per line)
    assert fuel_amd.lib().fuelmi_map_insert_plan(None) == -1
    out = (C.c_int * 8)(*([7] * 8))
    assert fuel_amd.lib().fuelmi_map_insert_plan(out) == 0 and list(out)[6:] == [0, 0]


# ---- the numpy restatements are the oracle's ----
@pytest.mark.parametrize("grid", list(fe.B_GRIDS))
def test_ray_restatement_walks_the_oracles_cells(grid):
    map_size, kw, cam, rays = fe.lane_rays(grid)
    om = fo.OracleMap(map_size, **kw)
    g = fe.Geo(map_size, **kw)
    kept, end, _, _ = fe.classify(g, [p for _, p in rays], cam)
    assert kept.sum() >= 0.85 * len(rays)  # (end points on the bottom face of the map are clipped and dropped)
    for (name, _), k, e in zip(rays, kept, end):
        if not k:
            continue
        cells = fe.ray_walk(e, cam, g.res)["cells"]
        mine = np.array([[int(c[q] + 0.5 - g.org[q] / g.res) for q in range(3)] for c in cells]).reshape(-1, 3)
        assert np.array_equal(mine, om.raycast_cells(e, cam)), name


@pytest.mark.parametrize("name", ["C_cubes", "D_hit_miss", "D_counts", "E_unaligned"])
def test_classification_restatement_gives_the_oracles_boxes(name):
    """the end points numpy keeps span, with the camera, exactly the box the oracle reports for the frame"""
    sc = fe.SCENARIOS[name]()
    g = fe.Geo(sc["map_size"], **sc["map_kw"])
    om = oracle_map(sc)
    for k, (pts, cam) in enumerate(sc["frames"]):
        kept, end, _, _ = fe.classify(g, pts, cam)
        box = np.vstack([end[kept], cam[None, :]])
        om.input_points(pts, cam)
        lo, hi = om.get_updated_box(reset=True)
        assert np.array_equal(lo, box.min(axis=0)) and np.array_equal(hi, box.max(axis=0)), (name, k)


# ---- A: the counter ----
def test_counter_scenario_decides_at_the_wrap_frames():
    sc = fe.scenario_counter_directed()
    g = fe.Geo(sc["map_size"])
    om = oracle_map(sc)
    mid = {n: g.address(np.array(fe.counter_mid_cell(g, n))) for n in fe.A_VOXELS}
    once = min(max(om.l_occ + om.l_miss, om.l_min), om.l_max)
    seen = {}
    for k, (pts, cam) in enumerate(sc["frames"], start=1):
        assert 1 <= len(pts) <= 30
        om.input_points(pts, cam)
        seen[k] = {n: om.occ[a] for n, a in mid.items()}
    unknown = lambda v: v < om.l_min - 1e-3  # noqa: E731
    # frame 257: the voxel that ended a ray in frame 1 looks already cast -- its mid cell was missed once, not twice
    assert seen[1]["first_and_257"] == once and seen[257]["first_and_257"] == once and seen[300]["first_and_257"] == once
    # frame 255: the counter equals the initial flag -1 -- a voxel never ended before casts no ray
    assert unknown(seen[254]["first_in_255"]) and unknown(seen[255]["first_in_255"]) and unknown(seen[300]["first_in_255"])
    assert unknown(seen[255]["first_in_256"]) and seen[256]["first_in_256"] == once   # frame 256 (counter 0) casts
    assert unknown(seen[127]["first_in_128"]) and seen[128]["first_in_128"] == once   # frame 128 (counter -128) casts
    assert max(fe.A_COMPARE) == len(sc["frames"]) == 300
    # F: an all-dropped frame 255 still advances the counter -- the voxel that follows it now ends in frame 256 and casts
    scf = fe.scenario_counter_directed(dropped_at=255)
    kept = fe.classify(g, *scf["frames"][254])[0]
    assert len(kept) >= 10 and not kept.any()
    omf = oracle_map(scf)
    for pts, cam in scf["frames"]:
        omf.input_points(pts, cam)
    assert omf.occ[mid["first_in_255"]] == once
    assert omf.occ[mid["first_and_257"]] == min(max(once + om.l_miss, om.l_min), om.l_max)


# ---- B: the lane hand-over ----
@pytest.mark.parametrize("grid", list(fe.B_GRIDS))
def test_lane_rays_reach_the_hand_over_edges(grid):
    map_size, kw, cam, rays = fe.lane_rays(grid)
    g = fe.Geo(map_size, **kw)
    kept, end, hit, _ = fe.classify(g, [p for _, p in rays], cam)
    exact = two = three = clipped = 0
    octants, cells, moving, fixed_axes = set(), set(), set(), 0
    for (name, p), k, e, h in zip(rays, kept, end, hit):
        if not k:
            continue
        w = fe.ray_walk(e, cam, g.res)
        exact += bool(fe.handover_exact(w))
        two += any(t >= 2 for t in w["ties"])
        three += any(t == 3 for t in w["ties"])
        clipped += not h
        octants.add(w["octant"])
        cells.add(len(w["cells"]))
        moving.add(w["moving"])
        _, _, step, tmax, tdel = fe.ray_params(e, cam, g.res)
        fixed_axes += any(s == 0 and np.isinf(tmax[q]) and np.isnan(tdel[q]) for q, s in enumerate(step))
        d = [abs(a - b) for a, b in zip(*fe.ray_params(e, cam, g.res)[:2])]
        if name.startswith(("face", "centre", "mixed")) and h:
            assert all(v % fe.LANES == 0 for v in d), (name, d)
    print("%s: %d rays kept of %d; exact hand-over %d, two-axis ties %d, three-axis ties %d, clipped %d, octants %d, "
          "cell counts %s" % (grid, kept.sum(), len(rays), exact, two, three, clipped, len(octants), sorted(cells)[:6]))
    assert exact >= 24, "rays with a crossing exactly on j / %d: %d" % (fe.LANES, exact)
    assert two >= 8 and three >= 4, (two, three)
    assert {(a, b, c) for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)} <= octants, "an octant is missing"
    assert {0, 1, 2, 3} <= cells, "a ray of 0, 1, 2 or 3 cells is missing: %s" % sorted(cells)
    assert moving == {0, 1, 2, 3} and fixed_axes >= 12 and clipped >= 5
    assert any(np.array_equal(p, np.float32(cam)) for _, p in rays)
    lone = [p for n, p in rays if n == "cam_voxel"][0]
    assert np.array_equal(g.index(lone), g.index(cam)) and not np.array_equal(lone, np.float32(cam))


# ---- C: the cube ----
def test_cube_frames_take_every_branch_on_every_axis():
    g = fe.Geo(fe.C_MAP, **fe.C_KW)
    assert tuple(g.nv) == (160, 120, 48)
    table = {(k, b): [] for k in range(3) for b in fe.BRANCHES}
    by_label = {}
    for label, pts, cam in fe.cube_frames():
        assert len(pts) <= fe.CLASSIFY_SLOTS
        cubes = fe.frame_cubes(g, pts, cam)
        by_label[label] = cubes
        for c in cubes:
            if c["casts"]:
                for k in range(3):
                    table[(k, c["branch"][k])].append(label)
    print("branch table (frames per axis and branch):")
    for k in range(3):
        print("  %s: %s" % ("xyz"[k], {b: len(set(table[(k, b)])) for b in fe.BRANCHES}))
    missing = [(("xyz"[k]), b) for (k, b), v in table.items() if not v]
    assert not missing, "no casting workgroup takes %s" % missing
    cam_of = {label: cam for label, _, cam in fe.cube_frames()}
    for label, zc in (("z_below_0", 5), ("corner_first", 5)):   # the flush forms a negative address
        assert g.index(cam_of[label])[2] == zc
        assert all(c["origin"][2] == zc - fe.CUBE[2] // 2 < 0 and c["branch"][2] == "middle" for c in by_label[label])
    for label in ("z_over_top", "corner_last"):                    # the cube overhangs the top of the map
        assert g.index(cam_of[label])[2] == 40
        assert all(c["origin"][2] + fe.CUBE[2] > g.nv[2] and c["branch"][2] == "middle" for c in by_label[label])
    # the corner columns: rays that run inside the line (0, 0) / (nx - 1, ny - 1), a line of the cube whose 32-bit word
    # lies across two 64-bit words of the miss plane
    for label, line in (("corner_first", (0, 0)), ("corner_last", (g.nv[0] - 1, g.nv[1] - 1))):
        pts = [p for n, p, _ in fe.cube_frames() if n == label][0]
        cam = cam_of[label]
        assert tuple(g.index(cam)[:2]) == line
        kept, end, _, _ = fe.classify(g, pts, cam)
        inline = [e for e, k in zip(end, kept) if k and tuple(g.index(e)[:2]) == line]
        long_ = [e for e in inline if len(fe.ray_walk(e, cam, g.res)["cells"]) >= 8]
        assert len(long_) >= 6, label
        org = by_label[label][0]["origin"]
        assert 0 <= line[0] - org[0] < fe.CUBE[0] and 0 <= line[1] - org[1] < fe.CUBE[1]
        sh = int(g.address(np.array([line[0], line[1], org[2]]))) & 63
        assert sh > 64 - fe.CUBE[2], (label, sh)
    # slot coupling: the far point of the last slot puts the first ray workgroup on another branch than its own points
    pts, cam = [(p, c) for n, p, c in fe.cube_frames() if n == "slot_coupling"][0]
    assert len(pts) == fe.CLASSIFY_SLOTS
    own = fe.frame_cubes(g, pts, cam, box_slots=fe.RAY_SLOTS)[0]
    got = by_label["slot_coupling"][0]
    assert got["casts"] and own["branch"][0] == "fits" and got["branch"][0] == "middle" and own["origin"] != got["origin"]


# ---- D: counts ----
def test_count_scenarios_straddle_waves_and_workgroups():
    g = fe.Geo(fe.D_MAP)
    assert fe.D_COUNTS == (1, 63, 64, 65, 255, 256, 257, 513) and fe.D_REGROW == (10, 3000, 10, 5000)
    assert [len(p) for p, _ in fe.scenario_counts()["frames"]] == list(fe.D_COUNTS)
    assert [len(p) for p, _ in fe.scenario_regrow()["frames"]] == list(fe.D_REGROW)
    cloud = fe.run_cloud()
    assert len(cloud) == 300
    eq = np.all(cloud[1:] == cloud[:-1], axis=1)          # eq[i]: slots i and i + 1 hold the same point
    assert eq[fe.WAVE - 1] and eq[2 * fe.WAVE - 1] and eq[fe.CLASSIFY_SLOTS - 1]
    runs = np.diff(np.concatenate([[0], np.where(~eq)[0] + 1, [len(cloud)]]))
    assert list(runs[:-1]) == list(fe.D_RUNS[:-1]) and runs[-1] == 300 - sum(fe.D_RUNS[:-1])
    kept, _, hit, _ = fe.classify(g, cloud, fe.D_CAM)
    assert kept.all() and 100 <= hit.sum() <= 200
    # hit and clipped miss of one voxel in neighbouring slots
    hm = fe.hit_miss_cloud(g)
    kept, _, hit, adr = fe.classify(g, hm, fe.D_HM_CAM)
    assert kept.all() and hit[0::2].all() and not hit[1::2].any(), "a pair is not (hit, clipped miss)"
    assert np.array_equal(adr[0::2], adr[1::2]), "a clipped point left its partner's voxel"
    assert len(np.unique(adr)) >= 4 and len(hm) > 2 * fe.WAVE
    # many points of one voxel
    kept, _, hit, adr = fe.classify(g, fe.one_voxel_cloud(), fe.D_CAM)
    assert len(adr) == 513 and kept.all() and hit.all() and len(np.unique(adr)) == 1
    # NaN records where the de-duplication looks at its neighbour
    for dirty, clean, _ in fe.nan_frames():
        bad = np.isnan(dirty[:, 0])
        assert bad[0] and bad[-1] and bad[fe.WAVE - 1] and bad[fe.WAVE] and len(clean) == (~bad).sum()
        assert np.array_equal(dirty[~bad], clean)
    dirty = fe.nan_frames()[1][0]
    bad = np.isnan(dirty[:, 0])
    between = [i for i in np.where(bad)[0][1:-1] if np.array_equal(dirty[i - 1], dirty[i + 1]) and not bad[i - 1]]
    assert len(between) >= 3


# ---- E, F ----
def test_unaligned_and_dropped_scenarios_are_what_they_claim():
    g = fe.Geo(fe.E_MAP, **fe.E_KW)
    assert tuple(g.org) == (-5.025, -4.015, -0.97) and tuple(g.nv) == (101, 81, 41)
    assert all(abs(v / g.res - round(v / g.res)) > 0.1 for v in g.org)   # no multiple of the resolution
    sc = fe.scenario_unaligned()
    assert [len(p) for p, _ in sc["frames"][:8]] == [500] * 8 and len(sc["frames"]) == 11 and len(sc["frames"][-1][0]) == 1
    size = np.array(fe.E_MAP)
    for _, cam in sc["frames"][:8]:
        assert np.all(cam >= g.org + 0.2 * size) and np.all(cam <= g.org + 0.8 * size)
    (_, c1), (_, c2) = sc["frames"][8:10]
    assert c1[2] > g.maxb[2] and c2[1] > g.maxb[1]
    for pts, cam in sc["frames"][8:10]:
        kept, _, hit, _ = fe.classify(g, pts, cam)
        assert len(pts) > 100 and kept.all() and hit.all()
    # the walker's truncation and posToIndex's floor disagree on this origin: end points whose first ray cell is not
    # their own voxel (the update sweeps one voxel more than the end-point box for that reason)
    differ = 0
    for pts, cam in sc["frames"][:8]:
        kept, end, _, _ = fe.classify(g, pts, cam)
        c = np.floor(end[kept] / g.res)
        walker = (c + (0.5 - g.org / g.res)).astype(np.int64)
        differ += int(np.any(walker != g.index(end[kept]), axis=1).sum())
    print("E: %d end points whose walker cell differs from posToIndex" % differ)
    assert differ >= 50
    # F: every point of the dropped clouds is clipped and ends below z = 0.2
    scd = fe.scenario_unaligned(True)
    assert len(scd["frames"]) == 12
    assert not fe.classify(g, *scd["frames"][4])[0].any()
    first = fe.scenario_all_dropped_first()
    ga = fe.Geo(first["map_size"])
    assert not fe.classify(ga, *first["frames"][0])[0].any()
    om = oracle_map(first)
    before = om.occ.copy()
    om.input_points(*first["frames"][0])
    assert np.array_equal(om.occ, before)
    cam = first["frames"][0][1]
    lo, hi = om.get_local_bound()
    assert lo == tuple(ga.index(cam - [ga.inflate, ga.inflate, 0])) and hi == tuple(ga.index(cam + [ga.inflate, ga.inflate, 0]))
    assert all(np.array_equal(v, cam) for v in om.get_updated_box())


# ---- the oracle is the reference on every scenario ----
@pytest.mark.parametrize("name", list(fe.SCENARIOS))
def test_scenario_matches_reference(tape, name):
    sc = fe.SCENARIOS[name]()
    om = oracle_map(sc)
    rm = ref.RefMap(sc["map_size"], *fe.exploration_box(sc), **sc["map_kw"]) if LIVE else None
    touched = 0
    for k, (pts, cam) in enumerate(sc["frames"]):
        for m in (om, rm):
            if m is not None:
                m.input_points(pts, cam)
        if k in sc["compare"]:
            tape.equal(om.occ, lambda: rm.occ)
            tape.equal(bound_box(om), lambda: bound_box(rm))
            tape.equal(np.concatenate(om.get_updated_box()), lambda: np.concatenate(rm.get_updated_box()))
            touched = int((om.occ >= om.l_min - 1e-3).sum())
    print("%s: %d frames, %d compared, %d known voxels at the end" % (name, len(sc["frames"]), len(sc["compare"]), touched))
    assert touched > 0


@pytest.mark.parametrize("grid", list(fe.B_GRIDS))
def test_lane_rays_walk_matches_reference(tape, grid):
    map_size, kw, cam, rays = fe.lane_rays(grid)
    om = fo.OracleMap(map_size, **kw)
    rm = ref.RefMap(map_size, **kw) if LIVE else None
    g = fe.Geo(map_size, **kw)
    kept, end, _, _ = fe.classify(g, [p for _, p in rays], cam)
    for k, e in zip(kept, end):
        if k:
            tape.equal(om.raycast_cells(e, cam), lambda: rm.raycast_cells(e, cam))
