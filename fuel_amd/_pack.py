"""What every batched call of fuel_amd.host does on the way into and out of libfuelmi: pack ragged per-problem rows,
broadcast a value to one per problem, type a pointer by its array, declare result arrays once, read the limit code, ask a
plan query.  numpy and ctypes only: nothing here loads the library."""
import ctypes as C

import numpy as np

from . import _lib

_POINTER = {np.dtype(np.float64): _lib._dp, np.dtype(np.int32): _lib._ip}


def ptr(a, dtype=None):
    """The typed pointer to a's data: double* for float64, int* for int32 (`dtype` fixes which), None for None.  Any
    other dtype or a view that is not C-contiguous would reach a kernel as garbage behind a well-typed pointer:
    TypeError."""
    if a is None:
        return None
    if not isinstance(a, np.ndarray) or a.dtype not in _POINTER or not a.flags.c_contiguous or \
            (dtype is not None and a.dtype != dtype):
        raise TypeError("a C-contiguous %s array is needed, got %s" % (
            np.dtype(dtype).name if dtype is not None else "float64 or int32",
            "%s %s%s" % (a.dtype, a.shape, "" if a.flags.c_contiguous else " (not contiguous)")
            if isinstance(a, np.ndarray) else type(a).__name__))
    return a.ctypes.data_as(_POINTER[a.dtype])


def dp(a):
    return ptr(a, np.float64)


def ip(a):
    return ptr(a, np.int32)


def pack(rows, width, cols, dtype=np.float64, floor=0, n=None):
    """A list of per-problem [k, cols] arrays (cols 0: 1-D rows; a tuple: that trailing shape; a None row: an empty one)
    as (counts int32 [n], padded [n, max(width, 0), cols], width).  width None: the longest row, at least `floor`; a
    given width comes back as given, for the cfg.  A count is its row's true length while the row is copied only up to
    the width: the C side refuses a problem longer than its stride by its count.  n: the batch size when `rows` (or
    None) may fall short of it; the missing rows are empty, one too many is an IndexError."""
    tail = tuple(cols) if isinstance(cols, tuple) else (cols,) if cols else ()
    rs = [np.zeros((0,) + tail, dtype=dtype) if r is None else np.ascontiguousarray(r, dtype=dtype).reshape((-1,) + tail)
          for r in (rows if rows is not None else [])]
    if n is not None:
        if len(rs) > n:
            raise IndexError("%d rows for a batch of %d" % (len(rs), n))
        rs += [np.zeros((0,) + tail, dtype=dtype)] * (n - len(rs))
    w = int(width) if width is not None else max([len(r) for r in rs] + [floor])
    arr = np.zeros((len(rs), max(w, 0)) + tail, dtype=dtype)
    for b, r in enumerate(rs):
        k = min(len(r), arr.shape[1])
        arr[b, :k] = r[:k]
    return np.array([len(r) for r in rs], dtype=np.int32), arr, w


def per_problem(v, n, dtype=np.float64, optional=False):
    """a value or an array of n values as a contiguous [n] array (optional: None stays None); ValueError for another
    length"""
    if v is None and optional:
        return None
    return np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dtype), (n,)))


def outputs(n, table):
    """The result arrays of a call, declared once and in the C argument order: rows of (names, dtype, trailing shape
    [, present]), `names` one key or several separated by blanks.  Returns ({name: zeros [n, ...] or None}, the pointers
    as the call takes them); an absent result is None in the dict and NULL in the call."""
    o = {}
    for names, dtype, tail, *present in table:
        for name in names.split():
            o[name] = np.zeros((n,) + tuple(tail), dtype=dtype) if not present or present[0] else None
    return o, tuple(ptr(a) for a in o.values())


def limited(rc, allow_limit):
    """the `limit` flag of a call's return code: True for FUELMI_ELIMIT where the caller allows it, False for success;
    everything else raises FuelmiError"""
    if allow_limit and rc == _lib.ELIMIT:
        return True
    _lib.check(rc)
    return False


def plan_query(fn, length, *args, ctype=C.c_int, names=None):
    """A host-only plan query fn(*args, out[length]): the numbers as a tuple, or as a dict under `names`.  A cfg
    structure among args goes by reference."""
    out = (ctype * length)()
    _lib.check(fn(*[C.byref(a) if isinstance(a, C.Structure) else a for a in args], out))
    vals = tuple(int(v) for v in out)
    return dict(zip(names, vals)) if names else vals


def weights(w, defaults):
    """a BsplineCfg as given, or one made of `defaults` overlaid with a dict of its fields (None: the defaults)"""
    return w if isinstance(w, _lib.BsplineCfg) else _lib.BsplineCfg(**dict(defaults, **(w or {})))
