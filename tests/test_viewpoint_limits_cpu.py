"""The scenes of test_viewpoint_limits_gpu.py without a device: every oracle-only guard that a scene reaches the edge
it was drawn for (helpers.vp_guard_*), and the arithmetic the guards restate against the oracle's own results."""
import pytest

import helpers

ORDERS = pytest.mark.parametrize("reference_order", [False, True], ids=["device_order", "reference_order"])


def _clear_of_cells(scene, of):
    assert helpers.vp_min_cell_distance(of, scene.vcfg) > 1e-6


@ORDERS
def test_cells_per_cluster_classes(reference_order):
    scene = helpers.vp_scene_cells(1)
    _, of = helpers.vp_oracle(scene, reference_order)
    helpers.vp_guard_cells(of)
    _clear_of_cells(scene, of)
    for ds in (1, 3):  # (at 3 the strip of 5 x 13 cells has candidates above its own patch: rejected, not divided by)
        s = helpers.vp_scene_cells(ds)
        _clear_of_cells(s, helpers.vp_oracle(s, reference_order)[1])


@pytest.mark.parametrize("name", list(helpers.VP_CLEARANCES))
def test_clearance_specks_flip_their_candidates(name):
    scene, flips, stays = helpers.vp_scene_clearance(name)
    _, of = helpers.vp_guard_clearance(name, scene, flips, stays)
    _clear_of_cells(scene, of)


@ORDERS
def test_box_face_cases(reference_order):
    for face in ("x_min", "y_max"):
        got = []
        for ulps in (-1, 0, 1):
            scene, p, inside = helpers.vp_scene_box_face(face, ulps, reference_order)
            _, of = helpers.vp_oracle(scene, reference_order)
            assert (p in helpers.vp_positions(of)) == inside
            got.append(inside)
        assert got == ([True, False, False] if face == "x_min" else [False, False, True])


@ORDERS
def test_min_visib_and_max_dist_edges(reference_order):
    v, n = helpers.vp_min_visib_edge(reference_order=reference_order)
    helpers.vp_guard_min_visib(v, n, reference_order)
    for ds in (1, 3):
        base, p, edges = helpers.vp_max_dist_edges(ds, reference_order)
        helpers.vp_guard_max_dist(base, p, edges, reference_order)


def test_collinear_row_and_yaw_wrap():
    scene = helpers.vp_scene_collinear()
    _, of = helpers.vp_oracle(scene)
    helpers.vp_guard_collinear(scene, of)
    _clear_of_cells(scene, of)
    scene = helpers.vp_scene_yaw_wrap()
    got = helpers.vp_guard_yaw_wrap(helpers.vp_oracle(scene)[1])
    assert min(got[1], got["below"]) >= helpers.VP_YAW_MIN and got[-1] == got["above"] == 0  # the default table: one side ...
    scene.vcfg["dphi"] = helpers.VP_DPHI_ABOVE
    got = helpers.vp_guard_yaw_wrap(helpers.vp_oracle(scene)[1])
    assert min(got[1], got[-1], got["below"]) >= helpers.VP_YAW_MIN  # ... a pi rounded up: both
    scene = helpers.vp_scene_yaw_wrap("step")
    _, of = helpers.vp_oracle(scene)
    assert helpers.vp_guard_yaw_wrap(of)["above"] >= helpers.VP_YAW_MIN
    _clear_of_cells(scene, of)


@ORDERS
@pytest.mark.parametrize("family", ["patch", "room"])
def test_frustum_cuts_and_is_asymmetric(family, reference_order):
    scene = helpers.vp_scene_frustum(family)
    _, of = helpers.vp_oracle(scene, reference_order)
    helpers.vp_guard_frustum(family, of, reference_order)
    _clear_of_cells(scene, of)


@ORDERS
@pytest.mark.parametrize("grid", list(helpers.VP_GRIDS))
def test_pillars_stop_rays_at_every_grid(grid, reference_order):
    scene = helpers.vp_scene_occluded(grid)
    om, of = helpers.vp_oracle(scene, reference_order)
    helpers.vp_guard_occluded(grid, of, reference_order)
    _clear_of_cells(scene, of)
    assert max(om.nvox) <= 200 and om.nvox[2] <= 40


@pytest.mark.parametrize("beyond", [False, True])
def test_face_scene_reaches_outside_the_map(beyond):
    scene = helpers.vp_scene_faces(beyond)
    om, of = helpers.vp_oracle(scene)
    helpers.vp_guard_faces(om, of, scene.vcfg, beyond)
    _clear_of_cells(scene, of)


def test_floor_probe_candidates_stay_accepted():
    scene, hit = helpers.vp_scene_floor_probe()
    om, of = helpers.vp_oracle(scene)
    helpers.vp_guard_floor_probe(om, of, hit)
    _clear_of_cells(scene, of)


def test_candidate_table_sizes():
    ns = {}
    for name, kw in helpers.VP_TABLES.items():
        scene = helpers.vp_scene_occluded(**kw)
        _, of = helpers.vp_oracle(scene)
        ns[name] = helpers.vp_guard_tables(of, scene.vcfg)
        _clear_of_cells(scene, of)
    assert ns == helpers.VP_TABLE_NS and len(set(ns.values())) >= 5


def test_round_states_grow_shrink_and_leave_a_dormant_cluster():
    ns = len(helpers.vp_candidate_offsets(helpers.vp_scene_rounds(0).vcfg))
    need, dormant = [], 0
    for r in range(3):
        _, of = helpers.vp_oracle(helpers.vp_scene_rounds(r))
        views = helpers.vp_views(of)
        need.append(helpers.vp_stage_bytes(len(views), ns, sum(len(c) for *_, c in views)))
        dormant += len(of.clusters(2))
    helpers.vp_guard_stage_growth(need)
    assert dormant > 0
