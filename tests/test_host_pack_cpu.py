"""CPU checks of fuel_amd._pack on its own: the ragged packer, the per-problem broadcaster, the output table, the limit
helper, the plan query and the typed pointers every batched wrapper of fuel_amd.host goes through.  No library is loaded."""
import ctypes as C

import numpy as np
import pytest

from fuel_amd import _lib, _pack, host

I, D = np.int32, np.float64


def test_pack_empty_batch():
    cnt, arr, w = _pack.pack([], None, 3, floor=4)
    assert cnt.dtype == I and cnt.shape == (0,) and arr.shape == (0, 4, 3) and arr.dtype == D and w == 4
    cnt, arr, w = _pack.pack(None, None, 0)
    assert cnt.shape == (0,) and arr.shape == (0, 0) and w == 0


def test_pack_counts_the_true_length_and_cuts_the_content():
    a, b = np.arange(6.0).reshape(2, 3), np.arange(15.0).reshape(5, 3) + 10
    cnt, arr, w = _pack.pack([a, b], 3, 3)
    assert cnt.tolist() == [2, 5] and w == 3 and arr.shape == (2, 3, 3) and arr.flags.c_contiguous
    assert np.array_equal(arr[0, :2], a) and not arr[0, 2:].any() and np.array_equal(arr[1], b[:3])


@pytest.mark.parametrize("width", [0, -1])
def test_pack_width_goes_back_as_given_with_no_rows_allocated(width):
    cnt, arr, w = _pack.pack([np.ones((2, 3)), np.ones((4, 3))], width, 3, floor=4)
    assert w == width and arr.shape == (2, 0, 3) and cnt.tolist() == [2, 4]


def test_pack_none_row_flat_rows_int_rows_and_trailing_shapes():
    cnt, arr, w = _pack.pack([[1.0, 2.0, 3.0], None, 4.0], None, 0)
    assert cnt.tolist() == [3, 0, 1] and w == 3 and arr.tolist() == [[1, 2, 3], [0, 0, 0], [4, 0, 0]]
    cnt, arr, w = _pack.pack([[2], [1, 3]], 2, 0, np.int32)
    assert arr.dtype == I and arr.tolist() == [[2, 0], [1, 3]] and cnt.tolist() == [1, 2]
    cnt, arr, w = _pack.pack([np.ones((2, 3, 6)), np.ones((1, 3, 6))], None, (3, 6))
    assert arr.shape == (2, 2, 3, 6) and cnt.tolist() == [2, 1] and arr[1, 0].all() and not arr[1, 1].any()
    cnt, arr, w = _pack.pack([np.arange(4.0)], None, 1)  # (one column is not "1-D rows")
    assert arr.shape == (1, 4, 1)


def test_pack_default_width_floor():
    rows = [np.ones((2, 3)), np.ones((5, 3))]
    assert _pack.pack(rows, None, 3, floor=4)[2] == 5 and _pack.pack(rows, None, 3, floor=7)[2] == 7
    assert _pack.pack(rows, None, 3)[2] == 5 and _pack.pack([], None, 3)[2] == 0
    assert _pack.pack(rows, None, 3, floor=7)[1].shape == (2, 7, 3)


def test_pack_fills_a_batch_and_refuses_a_row_too_many():
    cnt, arr, w = _pack.pack([[1.0]], 2, 0, n=3)
    assert cnt.tolist() == [1, 0, 0] and arr.shape == (3, 2)
    assert _pack.pack(None, 2, 3, n=2)[1].shape == (2, 2, 3)
    with pytest.raises(IndexError):
        _pack.pack([[1.0]] * 3, 2, 0, n=2)


def test_per_problem():
    a = _pack.per_problem(0.5, 3)
    assert a.dtype == D and a.tolist() == [0.5] * 3 and a.flags.c_contiguous and a.flags.writeable
    b = _pack.per_problem([1, 2, 3], 3, np.int32)
    assert b.dtype == I and b.tolist() == [1, 2, 3]
    assert _pack.per_problem(1.0, 0).shape == (0,)
    with pytest.raises(ValueError):
        _pack.per_problem([1.0, 2.0], 3)
    assert _pack.per_problem(None, 3, optional=True) is None
    assert np.isnan(_pack.per_problem(None, 2)).all()  # (None is a value unless the call says the argument may be absent)


def test_outputs_table():
    o, ptrs = _pack.outputs(2, [("status n", I, ()), ("pos", D, (4, 3)), ("dot", D, (5,), False), ("best", I, (2,), 8)])
    assert list(o) == ["status", "n", "pos", "dot", "best"]
    assert o["dot"] is None and ptrs[3] is None
    assert [(o[k].dtype, o[k].shape) for k in ("status", "n", "pos", "best")] == [(I, (2,)), (I, (2,)), (D, (2, 4, 3)), (I, (2, 2))]
    assert not any(o[k].any() for k in ("status", "n", "pos", "best"))
    assert [type(p) for p in ptrs if p is not None] == [_lib._ip, _lib._ip, _lib._dp, _lib._ip]
    assert all(C.addressof(p.contents) == o[k].ctypes.data for p, k in zip(ptrs, o) if p is not None)
    assert o["status"] is not o["n"]


def test_limited(monkeypatch):
    monkeypatch.setattr(_lib, "_LIB", type("L", (), {"fuelmi_last_error": staticmethod(lambda: b"stand-in")})())
    assert _pack.limited(0, False) is False and _pack.limited(0, True) is False
    assert _pack.limited(_lib.ELIMIT, True) is True
    with pytest.raises(_lib.FuelmiError):
        _pack.limited(_lib.ELIMIT, False)
    for rc in (_lib.EINVAL, -2, 7):
        for allow in (False, True):
            with pytest.raises(_lib.FuelmiError):
                _pack.limited(rc, allow)


def test_plan_query(monkeypatch):
    monkeypatch.setattr(_lib, "_LIB", type("L", (), {"fuelmi_last_error": staticmethod(lambda: b"stand-in")})())
    seen = []

    def fn(*args):
        seen.append(args)
        for k in range(len(args[-1])):
            args[-1][k] = 10 + k
        return 0
    cfg = _lib.QuadCfg(1, 3, 4, 3, 0, 0)
    assert _pack.plan_query(fn, 3, cfg) == (10, 11, 12)
    assert seen[0][0]._obj is cfg and isinstance(seen[0][1], C.c_int * 3)
    assert _pack.plan_query(fn, 2, 7, ctype=C.c_longlong, names=("a", "b")) == {"a": 10, "b": 11}
    assert seen[1][0] == 7 and isinstance(seen[1][1], C.c_longlong * 2)
    with pytest.raises(_lib.FuelmiError):
        _pack.plan_query(lambda *a: _lib.EINVAL, 3, cfg)


def test_weights():
    w = _lib.BsplineCfg(ld_smooth=1.0)
    assert _pack.weights(w, host.DEFAULT_BSPLINE) is w
    d = _pack.weights(None, host.DEFAULT_BSPLINE)
    assert (d.ld_smooth, d.ld_guide, d.bspline_degree) == (20.0, 1.5, 3)
    d = _pack.weights({"ld_guide": 4.0}, host.DEFAULT_BSPLINE)
    assert (d.ld_smooth, d.ld_guide) == (20.0, 4.0)


def test_ptr_follows_the_dtype_and_refuses_the_rest():
    assert _pack.ptr(None) is None and host._dp(None) is None and host._ip(None) is None
    d, i = np.zeros((2, 3)), np.zeros(4, dtype=np.int32)
    assert isinstance(_pack.ptr(d), _lib._dp) and isinstance(_pack.ptr(i), _lib._ip)
    assert isinstance(host._dp(d), _lib._dp) and isinstance(host._ip(i), _lib._ip)
    assert isinstance(_pack.ptr(np.zeros((0, 3))), _lib._dp)
    for bad in (np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.float32), np.zeros((3, 2)).T, np.zeros(6)[::2],
                np.zeros(3, dtype=np.int8), [0.0, 1.0]):
        for f in (_pack.ptr, host._dp, host._ip):
            with pytest.raises(TypeError):
                f(bad)
    with pytest.raises(TypeError):
        host._dp(i)
    with pytest.raises(TypeError):
        host._ip(d)


def test_scripts_names_stay_importable():
    from fuel_amd.host import _dp, _ip, _ptr  # noqa: F401
    assert host.SDFMap.sample_trajs is host.SDFMap.sampleTrajs
