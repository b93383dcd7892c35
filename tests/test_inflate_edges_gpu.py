"""clearAndInflateLocalMap on the device at its step, word and kernel edges: every scene of tests/inflate_cases.py under
every kernel pin it allows (fuelmi_map_set_inflate_kernel: AUTO, the fused kernel at step 2, the factored pair at any
step), the kernel that ran asserted after every call, the inflated plane after every call bit-equal to the oracle's.
test_inflate_edges_cpu.py checks that the scenes hit their edges; tests/golden/check_inflate_host_build.py runs the same
scenes on planes of exactly the allocated size under sanitizers.  The largest map has 135 168 voxels."""
import numpy as np
import pytest

import inflate_cases as ic

pytestmark = pytest.mark.gpu

AUTO, FUSED, FACTORED = ic.AUTO, ic.FUSED, ic.FACTORED


@pytest.fixture(scope="module")
def fa():
    import fuel_amd
    assert fuel_amd.lib().fuelmi_device_count() > 0, "no GPU visible: the HIP path cannot run"
    return fuel_amd


def device_map(fa, sc, consts):
    gm = fa.SDFMap(sc.map_size, **sc.map_kw)
    assert gm.nvox == sc.nvox and gm.info.inflate_step == sc.step
    # the scene's log-odds are built from the oracle's constants: the device map's must be the same doubles
    assert (gm.info.clamp_min_log, gm.info.clamp_max_log, gm.info.min_occupancy_log) == consts
    return gm


def run(fa, sc, pin):
    """the scene under one pin -> the inflated plane after every call; kernel and plane asserted on the way"""
    occ, planes, consts = ic.expected(sc)
    gm = device_map(fa, sc, consts)
    try:
        gm.uploadOccupancy(occ)
        if sc.pre:
            gm.setOccupied([sc.centre(a) for a in sc.pre])
        assert gm.lastInflateKernel() == -1
        gm.setInflateKernel(pin)
        got = []
        for i, call in enumerate(sc.calls):
            if call[2] is not None:
                gm.setInflateKernel(call[2])
            gm.setLocalBound(call[0], call[1])
            gm.clearAndInflateLocalMap()
            assert gm.lastInflateKernel() == sc.kernel_of(pin, call), (sc, pin, i)
            plane = gm.syncHost(inflate=True)["inflate"]
            assert np.array_equal(plane, planes[i]), \
                "%s pin %d call %d: %d voxels differ from the oracle" % (sc, pin, i, np.count_nonzero(plane != planes[i]))
            got.append(plane)
            if call[2] is not None:
                gm.setInflateKernel(pin)
        return got, gm
    except BaseException:
        gm.close()
        raise


@pytest.mark.parametrize("sc", ic.SCENES, ids=repr)
def test_scene_is_bit_equal_to_the_oracle_under_every_pin(fa, sc):
    by_pin = {}
    for pin in sc.pins:
        by_pin[pin], gm = run(fa, sc, pin)
        gm.close()
    # two pins on the same scene: byte-equal planes
    first = by_pin[sc.pins[0]]
    for pin in sc.pins[1:]:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, by_pin[pin])), (sc, pin)


QUERIED = [sc for sc in ic.SCENES if sc.drawn.get("wrap")][::3] + [sc for sc in ic.SCENES if sc.drawn.get("thresholds")]


@pytest.mark.parametrize("sc", QUERIED, ids=repr)
def test_query_state_at_the_stamps_corners(fa, sc):
    """the result read through fuelmi_map_query_state: the eight corner voxels of every seed's stamp (-1 where a corner
    leaves the map: the query, unlike the stamp, tests every index), the seeds and the voxels on the two thresholds"""
    occ, planes, (l_min, l_max, l_occ) = ic.expected(sc)
    got, gm = run(fa, sc, sc.pins[-1])
    try:
        s = sc.step
        ids = [ic.idx(sc.dims, a) for a in sc.occupied + sc.at_occ_threshold + sc.at_unknown_threshold + sc.unknown[:4]]
        for a in sc.occupied:
            x, y, z = ic.idx(sc.dims, a)
            ids += [(x + dx, y + dy, z + dz) for dx in (-s, s) for dy in (-s, s) for dz in (-s, s)]
        state, infl = gm.getOccupancy(ids)
        for id3, st, bit in zip(ids, state, infl):
            if not all(0 <= id3[k] < sc.dims[k] for k in range(3)):
                assert (st, bit) == (-1, -1), id3
                continue
            a = ic.adr(sc.dims, *id3)
            want = fa.SDFMap.UNKNOWN if occ[a] < l_min - 1e-3 else fa.SDFMap.OCCUPIED if occ[a] > l_occ else fa.SDFMap.FREE
            assert (st, bit) == (want, planes[-1][a]), id3
        # exactly on a threshold: neither occupied nor unknown
        for a in sc.at_occ_threshold + sc.at_unknown_threshold:
            assert state[ids.index(ic.idx(sc.dims, a))] == fa.SDFMap.FREE
    finally:
        gm.close()


def test_queried_scenes_cover_wrap_and_thresholds():
    assert 4 <= len(QUERIED) <= 10
    assert any(sc.drawn.get("thresholds") for sc in QUERIED) and any(sc.drawn.get("wrap") for sc in QUERIED)


def test_step_32_is_refused_at_creation(fa):
    """the documented limit of the inflation stamp is 31 voxels"""
    d = (5, 3, 7)
    size = tuple(v * ic.RES for v in d)
    with pytest.raises(fa.FuelmiError, match="error -5"):  # FUELMI_ELIMIT
        fa.SDFMap(size, resolution=ic.RES, obstacles_inflation=(ic.STEP_REFUSED - 0.5) * ic.RES, ground_height=0.0)
    gm = fa.SDFMap(size, resolution=ic.RES, obstacles_inflation=(31 - 0.5) * ic.RES, ground_height=0.0)
    assert gm.info.inflate_step == 31
    gm.close()


@pytest.mark.parametrize("step", ic.STEPS)
def test_pin_is_refused_where_the_kernel_does_not_exist(fa, step):
    """FUSED on a map whose step is not 2: FUELMI_EINVAL, and the pin in force stays; FACTORED and AUTO always pass"""
    sc = next(s for s in ic.SCENES if s.step == step and not s.pre)
    occ, planes, consts = ic.expected(sc)
    gm = device_map(fa, sc, consts)
    try:
        gm.uploadOccupancy(occ)
        gm.setInflateKernel(FACTORED)
        if step == 2:
            gm.setInflateKernel(FUSED)
        else:
            with pytest.raises(fa.FuelmiError, match="error -1"):
                gm.setInflateKernel(FUSED)
        for bad in (-2, 2):
            with pytest.raises(fa.FuelmiError, match="error -1"):
                gm.setInflateKernel(bad)
        gm.setLocalBound(*sc.calls[0][:2])
        gm.clearAndInflateLocalMap()
        assert gm.lastInflateKernel() == (FUSED if step == 2 else FACTORED)
        assert np.array_equal(gm.syncHost(inflate=True)["inflate"], planes[0])
        gm.setInflateKernel(AUTO)
        gm.clearAndInflateLocalMap()
        assert gm.lastInflateKernel() == (FUSED if step == 2 else FACTORED)
    finally:
        gm.close()
