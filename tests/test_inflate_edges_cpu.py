"""The scene table of the inflation edge tests (tests/inflate_cases.py), oracle only: a scene that misses the edge it is
drawn for is worthless, so every scene says what it is there for and this file checks it -- the address residues, the
zero funnel shifts (restated from nz, nyz, dy, dx), the word and workgroup counts (from the library's own launch plan,
fuelmi_map_inflate_plan, host only), the wrap, the surviving bits, the voxels that are no sources -- and that every value
of the table's four axes appears, every kernel with every geometry.  The launch plan itself is pinned here too: the
margins, the ranges of the benchmark's maps, and that no window load of the factored pair leaves a plane or reads a word
the call did not write."""
import numpy as np
import pytest

import inflate_cases as ic

AUTO, FUSED, FACTORED = ic.AUTO, ic.FUSED, ic.FACTORED


@pytest.fixture(scope="module")
def fa():
    import __graft_entry__ as ge
    ge.build()
    import fuel_amd
    return fuel_amd


def kernels_of(sc):
    """the kernels a scene runs over all its pins: fused<whole?>, yz2<whole?>, yz0<whole?>"""
    out = set()
    for lo, hi, pin in sc.calls:
        whole = (lo, hi) == ic.full_box(sc.dims)
        for p in sc.pins:
            k = sc.kernel_of(p, (lo, hi, pin))
            out.add(("fused" if k == FUSED else "yz2" if sc.step == 2 else "yz0", whole))
    return out


def test_every_axis_value_appears_and_every_kernel_meets_every_geometry():
    assert 40 <= len(ic.SCENES) <= 60
    assert {sc.step for sc in ic.SCENES} == set(ic.STEPS)
    assert {b for sc in ic.SCENES for b in sc.box} == set(ic.BOX_CLASSES)
    assert {c for sc in ic.SCENES for c in sc.content} == set(ic.CONTENT_CLASSES)
    for dims in ic.GEOMETRY:
        ks = {k for sc in ic.SCENES if sc.dims == dims for k, _ in kernels_of(sc)}
        assert ks == {"fused", "yz2", "yz0"}, (dims, ks)
    # both variants of every kernel: the whole map (no masking pass / <2, true>) and a sub-box (k_box_and / <2, false>)
    assert {k for sc in ic.SCENES for k in kernels_of(sc)} == {(k, w) for k in ("fused", "yz2", "yz0") for w in (True, False)}
    # step 31 both where the stamp is larger than the map and on the largest map
    assert any(sc.step == 31 and sc.full_by_reach for sc in ic.SCENES)
    assert any(sc.step == 31 and sc.dims == (33, 64, 64) for sc in ic.SCENES)
    assert max(sc.N for sc in ic.SCENES) == 135168
    # seeds stay sparse at step 31
    assert all(len(sc.occupied) <= 2 for sc in ic.SCENES if sc.step == 31)
    # a sequence large box -> small box -> another small box, for stale words of the two scratch planes
    assert any(len(sc.calls) >= 3 and sc.step == 2 for sc in ic.SCENES)
    assert any(len(sc.calls) >= 3 and sc.step != 2 for sc in ic.SCENES)


@pytest.mark.parametrize("sc", ic.SCENES, ids=repr)
def test_scene_hits_what_it_is_drawn_for(sc, fa):
    occ, planes, (l_min, l_max, l_occ) = ic.expected(sc)  # (asserts nvox and the step)
    assert sc.N == int(np.prod(sc.nvox)) and sc.W == (sc.N + 63) // 64
    dr = sc.drawn
    nz, nyz = sc.dims[2], sc.nyz
    # -- the classes the scene claims --
    for b in sc.box:
        boxes = [(lo, hi) for lo, hi, _ in sc.calls]
        if b == "whole":
            assert ic.full_box(sc.dims) in boxes
        elif b in ("voxel_mod0", "voxel_mod63"):
            r = 0 if b == "voxel_mod0" else 63
            assert any(lo == hi and ic.adr(sc.dims, *lo) % 64 == r and ic.adr(sc.dims, *lo) in sc.occupied for lo, hi in boxes)
        elif b == "flush_low":
            assert any(lo == (0, 0, 0) and (lo, hi) != ic.full_box(sc.dims) for lo, hi in boxes)
        elif b == "flush_high":
            assert any(hi == tuple(d - 1 for d in sc.dims) and (lo, hi) != ic.full_box(sc.dims) for lo, hi in boxes)
        elif b == "outside_neighbours":
            assert dr.get("not_a_source")
        elif b == "survive":
            assert dr.get("survive")
        elif b == "sequence":
            assert len(sc.calls) >= 2
    if "voxel_mod" in dr:
        got = {ic.adr(sc.dims, *lo) % 64 for lo, hi, _ in sc.calls if lo == hi}
        assert set(dr["voxel_mod"]) <= got
    # -- the named funnel shift is 0 --
    if "shift0" in dr:
        kind, d = dr["shift0"]
        if kind == "yz2":    # k_inflate_yz<2>: start = 64 w - dy nz - 2
            assert sc.step == 2 and abs(d) <= 2 and (-d * nz - 2) % 64 == 0
        elif kind == "yz0":  # k_inflate_yz<0>: start = 64 w - dy nz - step (plane_window's sh == 0 branch)
            assert sc.step != 2 and abs(d) <= sc.step and (-d * nz - sc.step) % 64 == 0
        elif kind == "x":    # k_inflate_x: plane_window(T, 64 w - dx nyz)
            assert 1 <= d <= sc.step and (d * nyz) % 64 == 0
        elif kind == "fused":  # k_inflate_fused: shx = (-dx nyz) & 63, sh = (shx - dy nz) & 63, all dx, dy
            assert sc.step == 2 and all((-dx * nyz - dy * nz) % 64 == 0 for dx in range(-2, 3) for dy in range(-2, 3))
    # -- word and workgroup counts, from the launch plan the library runs --
    for lo, hi, pin in sc.calls:
        for p in sc.pins:
            k = sc.kernel_of(p, (lo, hi, pin))
            plan = fa.SDFMap.inflatePlan(sc.dims, sc.step, lo, hi, k if pin is not None or p != AUTO else AUTO)
            assert plan["kernel"] == k and plan["W"] == sc.W
            assert plan["whole"] == ((lo, hi) == ic.full_box(sc.dims))
            check_reads_stay_inside(sc, plan)
    whole_plan = fa.SDFMap.inflatePlan(sc.dims, sc.step, *ic.full_box(sc.dims), FACTORED)
    if "W" in dr:
        assert sc.W == dr["W"]
    if "out_words" in dr:
        assert whole_plan["out"] == (0, dr["out_words"] - 1)
        assert fa.SDFMap.inflatePlan(sc.dims, 2, *ic.full_box(sc.dims), FUSED)["grids"]["fused"] == -(-dr["out_words"] // 256)
    if "x_blocks" in dr:
        assert ic.full_box(sc.dims) in [(lo, hi) for lo, hi, _ in sc.calls]
        assert -(-(whole_plan["out"][1] - whole_plan["out"][0] + 1) // 256) == dr["x_blocks"]
        assert whole_plan["grids"]["x"] == dr["x_grid"] and dr["x_grid"] % 8 == 0
    if dr.get("nx1"):
        assert sc.dims[0] == 1
    # -- content --
    last = planes[-1]
    if "wrap" in sc.content or dr.get("wrap"):
        # at least one bit a dilation clipped at the map faces would not set
        assert dr.get("wrap") and "wrap" in sc.content and len(sc.pre) == 0
        first = planes[0]
        clipped = ic.clipped_dilation(sc, sc.calls[0])
        assert np.all(first[clipped == 1] == 1)
        assert np.count_nonzero((first == 1) & (clipped == 0)) >= 1
    if "empty" in sc.content:
        assert len(sc.occupied) == 0 and len(sc.pre) > 0
        assert all(last[a] == (0 if any(sc.in_box(a, c) for c in sc.calls) else 1) for a in sc.pre)
    if "full" in sc.content:
        assert len(sc.occupied) == sc.N and sc.N % 64 != 0 and np.all(planes[0] == 1)
    if sc.full_by_reach:
        # the stamp is larger than every dimension: the reach covers the map and every voxel is set
        assert 2 * sc.step + 1 > max(sc.dims) and np.all(last == 1)
    for i, (call, plane) in enumerate(zip(sc.calls, planes)):
        a_lo, a_hi = sc.reach_range(call)
        inside = plane[a_lo:a_hi + 1]
        if not ("empty" in sc.content or "full" in sc.content or sc.full_by_reach):
            if inside.size > 1 and any(sc.in_box(a, call) for a in sc.occupied):
                assert 0 < inside.sum() < inside.size, (i, inside.sum(), inside.size)
    if "at_occ_threshold" in sc.content:
        # log-odds exactly min_occupancy_log: no source (the comparison is strict), and its stamp would have shown
        assert dr.get("thresholds") and all(occ[a] == l_occ for a in sc.at_occ_threshold)
        assert all(np.any(planes[0][sc.stamp(a)] == 0) for a in sc.at_occ_threshold)
    if "at_unknown_threshold" in sc.content:
        assert all(occ[a] == l_min - 1e-3 and not occ[a] < l_min - 1e-3 for a in sc.at_unknown_threshold)
        assert all(occ[a] < l_min - 1e-3 for a in sc.unknown) and len(sc.unknown) > 0
    if dr.get("survive"):
        # a bit set before the calls, outside the box of a call (and of the calls before it) but within the addresses the
        # call rewrites, that no stamp sets: it is still there after the call
        without = ic.expected(sc, with_pre=False)[1]
        kept = []
        for i, call in enumerate(sc.calls):
            a_lo, a_hi = sc.reach_range(call)
            kept += [a for a in sc.pre if not any(sc.in_box(a, c) for c in sc.calls[:i + 1]) and a_lo <= a <= a_hi
                     and planes[i][a] == 1 and without[i][a] == 0]
        assert kept, "no surviving bit within reach"
        # and a bit inside a box that the call clears
        assert any(sc.in_box(a, sc.calls[0]) and planes[0][a] == 0 for a in sc.pre)
    if dr.get("not_a_source"):
        call = sc.calls[0]
        lo, hi = call[0], call[1]
        faces = set()
        for a in sc.occupied:
            if sc.in_box(a, call):
                continue
            id3 = ic.idx(sc.dims, a)
            for k in range(3):
                rest_in = all(lo[j] <= id3[j] <= hi[j] for j in range(3) if j != k)
                if rest_in and id3[k] == lo[k] - 1:
                    faces.add((k, 0))
                if rest_in and id3[k] == hi[k] + 1:
                    faces.add((k, 1))
            # its stamp would have changed the result
            assert np.any(planes[0][sc.stamp(a)] == 0), a
        assert len(faces) >= (6 if "outside_neighbours" in sc.box and len(sc.occupied) >= 7 else 2), faces


def check_reads_stay_inside(sc, plan):
    """Restated from the kernels: the window loads of the factored pair.  k_inflate_yz reads S at the words of bit
    64 w - dy nz - step .. + 127 (the <2> form: three words from (start >> 6), unguarded) for w in t, k_inflate_x reads T
    at the words of bit 64 w - dx nyz .. + 63 for w in out.  Every plane holds the words [-margin, W + margin + 1]; S
    must have been written this call (s) unless it is the occupancy plane, T always (t)."""
    if plan["kernel"] != FACTORED:
        return
    m, W, step, nz, nyz = plan["margin_words"], plan["W"], sc.step, sc.dims[2], sc.nyz
    assert m == (max(step, 1) * (nyz + nz + 1) + 64) // 64 + 4
    t_lo, t_hi = plan["t"]
    s_lo, s_hi = plan["s"]
    o_lo, o_hi = plan["out"]
    x_min = o_lo + ((-step * nyz) >> 6)
    x_max = o_hi + ((step * nyz) >> 6) + 1
    assert t_lo <= x_min and x_max <= t_hi, "the x pass reads words of T the y/z pass did not write"
    yz_min = t_lo + ((-step * nz - step) >> 6)
    yz_max = t_hi + ((step * nz - step) >> 6) + 2
    assert -m <= yz_min and yz_max <= W + m + 1, "the y/z pass reads outside the plane"
    if not plan["whole"]:
        assert s_lo <= yz_min and yz_max <= s_hi, "the y/z pass reads words of S the masking pass did not write"
        assert plan["grids"]["box_and"] == -(-(s_hi - s_lo + 1) // 256)
    assert plan["grids"]["yz"] == -(-(t_hi - t_lo + 1) // 256)
    assert plan["grids"]["x"] == -(-(-(-(o_hi - o_lo + 1) // 256)) // 8) * 8 and plan["grids"]["fused"] == 0


def test_plan_of_the_benchmark_maps_is_unchanged(fa):
    """AUTO on the benchmark's maps: the same kernels with the same grids as before the ranges moved into one function"""
    p = fa.SDFMap.inflatePlan((400, 400, 100), 2, (0, 0, 0), (399, 399, 99))
    assert p == {"kernel": FUSED, "margin_words": 1258, "W": 250000, "out": (0, 249999), "t": (-1252, 251251),
                 "s": (-1258, 251257), "whole": True, "lds": 21520,
                 "grids": {"fused": 977, "box_and": 0, "yz": 0, "x": 0}}
    p = fa.SDFMap.inflatePlan((800, 800, 200), 2, (0, 0, 0), (799, 799, 199))
    assert p == {"kernel": FACTORED, "margin_words": 5011, "W": 2000000, "out": (0, 1999999), "t": (-5002, 2005001),
                 "s": (-5011, 2005010), "whole": True, "lds": 22000,
                 "grids": {"fused": 0, "box_and": 0, "yz": 7852, "x": 7816}}
    # the local box of a streaming frame on the large map: the fused kernel, masked
    p = fa.SDFMap.inflatePlan((800, 800, 200), 2, (300, 300, 0), (399, 399, 199))
    assert p["kernel"] == FUSED and not p["whole"] and p["grids"]["fused"] == -(-(p["out"][1] - p["out"][0] + 1) // 256)


def test_fused_lds_is_bounded_by_the_largest_nz(fa):
    """the `lds_f <= 64 KiB` term of the kernel choice cannot be false: the map refuses nz > 255"""
    p = fa.SDFMap.inflatePlan((3, 2, 255), 2, (0, 0, 0), (2, 1, 254))
    ry = (2 * 256 + 63) // 64 + 1
    assert p["lds"] == 5 * (2 * (256 + 2 * ry + 2) + 2) * 8 == 22160 and p["kernel"] == FUSED
    with pytest.raises(fa.FuelmiError, match="error -5"):
        fa.SDFMap.inflatePlan((3, 2, 256), 2, (0, 0, 0), (2, 1, 255))


def test_plan_refuses_what_the_map_refuses(fa):
    d = (5, 3, 7)
    with pytest.raises(fa.FuelmiError, match="error -5"):  # FUELMI_ELIMIT: the documented limit of 31
        fa.SDFMap.inflatePlan(d, ic.STEP_REFUSED, *ic.full_box(d))
    assert fa.SDFMap.inflatePlan(d, 31, *ic.full_box(d))["kernel"] == FACTORED
    for step in (0, 1, 3, 31):
        with pytest.raises(fa.FuelmiError, match="error -1"):  # FUELMI_EINVAL: the fused kernel is step 2's
            fa.SDFMap.inflatePlan(d, step, *ic.full_box(d), FUSED)
    with pytest.raises(fa.FuelmiError, match="error -1"):
        fa.SDFMap.inflatePlan(d, 2, (0, 0, 0), (5, 2, 6))
    assert fa.SDFMap.inflatePlan(d, 2, *ic.full_box(d), FUSED)["kernel"] == FUSED
    assert fa.SDFMap.inflatePlan(d, 2, *ic.full_box(d), FACTORED)["kernel"] == FACTORED
