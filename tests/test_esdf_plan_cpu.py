"""The ESDF update's launch plan (fuelmi_map_esdf_plan, host only) at the edges of its table: which z/y and x kernels a
box gets for each family, with which grid, block, dynamic LDS and z-chunks, and which family the update then reports.
fuelmi_map_update_esdf launches exactly this plan; the GPU parity tests assert it for the boxes they run."""
import pytest

PLAIN, FAR, PLAIN32 = 0, 1, 2


@pytest.fixture(scope="module")
def fa():
    import __graft_entry__ as ge
    ge.build()
    import fuel_amd
    return fuel_amd


def plan(fa, dims, ext=None, family=PLAIN, optimistic=False, signed_dist=False, lo=(0, 0, 0)):
    """the plan of the box of extents `ext` (default: the whole grid) from `lo`"""
    ext = ext or dims
    hi = tuple(l + e - 1 for l, e in zip(lo, ext))
    return fa.SDFMap.esdfPlan(dims, lo, hi, family, optimistic, signed_dist)


def kernels(p):
    return [launch["kernel"] for launch in p["launches"]]


def test_g400_full_box_launches(fa):
    """the flagship box, every launch field (the packed pair; the vector pair in FAR)"""
    p = plan(fa, (400, 400, 100))
    assert p["family"] == PLAIN
    assert p["launches"] == [
        {"kernel": "k_esdf_zy_pk2<0, 4, 2>", "grid": 1400, "block": 256, "lds": 25600, "ZC": 0, "nzc": 7, "z0a": 0},
        {"kernel": "k_esdf_x_pk2<0>", "grid": 1250, "block": 256, "lds": 25600, "ZC": 0, "nzc": 4, "z0a": 0}]
    p = plan(fa, (400, 400, 100), family=FAR, optimistic=True)
    assert p["family"] == FAR
    assert p["launches"] == [
        {"kernel": "k_esdf_zy4<1, true>", "grid": 2000, "block": 512, "lds": 36080, "ZC": 20, "nzc": 5, "z0a": 0},
        {"kernel": "k_esdf_x4<0, 8, true>", "grid": 1250, "block": 1024, "lds": 57728, "ZC": 0, "nzc": 0, "z0a": 0}]


@pytest.mark.parametrize("fam", [PLAIN, FAR, PLAIN32])
def test_nz_not_a_multiple_of_4_takes_the_scalar_kernels(fa, fam):
    """nz 40 / 42: the 4-z vector and packed kernels need nz % 4 == 0; the scalar pair reports FAR or PLAIN32"""
    p40, p42 = plan(fa, (40, 40, 40), family=fam), plan(fa, (40, 40, 42), family=fam)
    assert kernels(p40) == {PLAIN: ["k_esdf_zy_pk2<0, 4, 2>", "k_esdf_x_pk2<0>"],
                            FAR: ["k_esdf_zy4<0, true>", "k_esdf_x4<0, 8, true>"],
                            PLAIN32: ["k_esdf_zy4<0, false>", "k_esdf_x4<0, 8, false>"]}[fam]
    assert kernels(p42) == ["k_esdf_zy<0>", "k_esdf_x<32, 0>"]
    assert p40["family"] == fam
    assert p42["family"] == (FAR if fam == FAR else PLAIN32)
    assert p42["launches"][0]["ZC"] == 42 and p42["launches"][0]["nzc"] == 1


def test_z_extent_255_is_the_last_packed_one(fa):
    p, q = plan(fa, (8, 8, 260), (8, 8, 255)), plan(fa, (8, 8, 260), (8, 8, 256))
    assert kernels(p) == ["k_esdf_zy_pk2<0, 4, 4>", "k_esdf_x_pk2<0>"] and p["family"] == PLAIN
    assert kernels(q) == ["k_esdf_zy4<0, false>", "k_esdf_x4<0, 8, false>"] and q["family"] == PLAIN32


def test_y_extent_832_is_the_last_4_segment_chunk(fa):
    """G = 4 while the two tiles of a slab pair stay within 52 KiB, else 2"""
    p, q = plan(fa, (8, 1000, 8), (8, 832, 8)), plan(fa, (8, 1000, 8), (8, 833, 8))
    assert kernels(p) == ["k_esdf_zy_pk2<0, 4, 2>", "k_esdf_x_pk2<0>"] and p["launches"][0]["lds"] == 416 * 4 * 32
    assert kernels(q) == ["k_esdf_zy_pk2<0, 2, 2>", "k_esdf_x_pk2<0>"] and q["launches"][0]["lds"] == 417 * 2 * 32
    assert p["family"] == q["family"] == PLAIN


def test_aligned_z_range_above_128_takes_four_plane_words(fa):
    """NW = 4 when the 4-aligned z range is > 128 voxels; a ragged box counts its aligned range"""
    assert kernels(plan(fa, (8, 8, 160), (8, 8, 128)))[0] == "k_esdf_zy_pk2<0, 4, 2>"
    assert kernels(plan(fa, (8, 8, 160), (8, 8, 132)))[0] == "k_esdf_zy_pk2<0, 4, 4>"
    assert kernels(plan(fa, (8, 8, 160), (8, 8, 126), lo=(0, 0, 3)))[0] == "k_esdf_zy_pk2<0, 4, 4>"  # z 3..128: 0..131


@pytest.mark.parametrize("x, want", [(512, "k_esdf_x<32, 0>"), (513, "k_esdf_x<16, 0>"), (2048, "k_esdf_x<16, 0>"),
                                     (2049, "k_esdf_x<8, 0>"), (4096, "k_esdf_x<8, 0>")])
def test_scalar_x_tile_edges(fa, x, want):
    for fam in (PLAIN, FAR, PLAIN32):
        p = plan(fa, (4200, 3, 3), (x, 3, 3), family=fam)
        assert kernels(p) == ["k_esdf_zy<0>", want]
        assert p["family"] == (FAR if fam == FAR else PLAIN32)


def test_x_extent_above_4096_is_refused(fa):
    from fuel_amd._lib import FuelmiError
    with pytest.raises(FuelmiError, match="ESDF x-line of 4097 voxels does not fit the LDS tile"):
        plan(fa, (4200, 3, 3), (4097, 3, 3))


@pytest.mark.parametrize("x, plain32, far", [
    (1136, "k_esdf_x4<0, 8, false>", "k_esdf_x4<0, 8, true>"),
    (1137, "k_esdf_x4<0, 8, false>", "k_esdf_x4<0, 8, false>"),   # FAR minima no longer fit beside the 32-column tile
    (1200, "k_esdf_x4<0, 8, false>", "k_esdf_x4<0, 8, false>"),
    (1201, "k_esdf_x4<0, 4, false>", "k_esdf_x4<0, 4, true>"),     # the 16-column tile
    (2274, "k_esdf_x4<0, 4, false>", "k_esdf_x4<0, 4, true>"),
    (2275, "k_esdf_x4<0, 4, false>", "k_esdf_x4<0, 4, false>"),    # ... nor beside the 16-column one
    (2400, "k_esdf_x4<0, 4, false>", "k_esdf_x4<0, 4, false>"),
    (2401, "k_esdf_x<8, 0>", "k_esdf_x<8, 0>"),                    # past the vector tile: scalar
])
def test_long_x_line_edges(fa, x, plain32, far):
    pp, pf = plan(fa, (4200, 8, 8), (x, 8, 8), family=PLAIN32), plan(fa, (4200, 8, 8), (x, 8, 8), family=FAR)
    assert kernels(pp)[1] == plain32 and kernels(pf)[1] == far
    assert kernels(pf)[0] == ("k_esdf_zy4<0, true>" if x <= 2400 else "k_esdf_zy<0>")
    assert pp["family"] == PLAIN32 and pf["family"] == FAR  # (the FAR fallbacks still report FAR)
    # PLAIN: packed while the x pass's 16-bit tile of (x + 1) / 2 x-pairs x 128 B stays within 150 KiB (x <= 2400)
    assert kernels(plan(fa, (4200, 8, 8), (x, 8, 8)))[1] == ("k_esdf_x_pk2<0>" if x <= 2400 else "k_esdf_x<8, 0>")


def test_far_zy_falls_back_to_plain_for_long_y_lines(fa):
    """k_esdf_zy4's block and line minima beside a 4-z tile: y lines up to 9101 voxels; plain ones up to 10240"""
    from fuel_amd._lib import FuelmiError
    assert kernels(plan(fa, (8, 11000, 8), (8, 9101, 8), family=FAR))[0] == "k_esdf_zy4<0, true>"
    p = plan(fa, (8, 11000, 8), (8, 9102, 8), family=FAR)
    assert kernels(p) == ["k_esdf_zy4<0, false>", "k_esdf_x4<0, 8, true>"] and p["family"] == FAR
    assert kernels(plan(fa, (8, 11000, 8), (8, 10240, 8)))[0] == "k_esdf_zy4<0, false>"
    with pytest.raises(FuelmiError, match="ESDF y-line of 10241 voxels does not fit the LDS tile"):
        plan(fa, (8, 11000, 8), (8, 10241, 8))


@pytest.mark.parametrize("optimistic", [False, True])
def test_signed_far_runs_the_negative_pass_packed(fa, optimistic):
    mode = int(optimistic)
    p = plan(fa, (400, 400, 100), family=FAR, optimistic=optimistic, signed_dist=True)
    assert kernels(p) == ["k_esdf_zy4<%d, true>" % mode, "k_esdf_x4<0, 8, true>", "k_esdf_zy_pk2<2, 4, 2>",
                          "k_esdf_x_pk2<1>"]
    assert p["family"] == FAR
    p = plan(fa, (400, 400, 100), family=PLAIN32, optimistic=optimistic, signed_dist=True)
    assert kernels(p) == ["k_esdf_zy4<%d, false>" % mode, "k_esdf_x4<0, 8, false>", "k_esdf_zy4<2, false>",
                          "k_esdf_x4<1, 8, false>"]
    assert p["family"] == PLAIN32


def test_signed_negative_pass_follows_the_positive_box_kind(fa):
    """x- is packed exactly when z/y- is; a box the packed family does not take runs both passes in 32 bits"""
    p = plan(fa, (8, 8, 260), (8, 8, 256), signed_dist=True)
    assert kernels(p) == ["k_esdf_zy4<0, false>", "k_esdf_x4<0, 8, false>", "k_esdf_zy4<2, false>",
                          "k_esdf_x4<1, 8, false>"]
    p = plan(fa, (40, 40, 42), family=FAR, signed_dist=True)
    assert kernels(p) == ["k_esdf_zy<0>", "k_esdf_x<32, 0>", "k_esdf_zy<2>", "k_esdf_x<32, 1>"] and p["family"] == FAR


def test_auto_is_refused(fa):
    from fuel_amd._lib import FuelmiError
    with pytest.raises(FuelmiError):
        plan(fa, (40, 40, 40), family=-1)
