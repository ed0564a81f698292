"""ctypes loader of vpin_amd/lib/libvpin_hosttest.so (tests/hostarith/hostarith.cpp): one function per host function, flat
arrays of 64-bit words in and out.  The library is built when it is missing or older than its sources; a library that cannot
be built or loaded is an error, never a skip.  VPIN_HOSTTEST_LIB names another build of the harness (one compiled against a
mutated copy of the headers, to see that the tests notice)."""
import ctypes as C
import os

import numpy as np

_lib = None
_table = None


class _Entry(C.Structure):
    _fields_ = [("name", C.c_char_p), ("iw", C.c_int), ("ow", C.c_int), ("fn", C.c_void_p)]


def lib():
    global _lib
    if _lib is None:
        from vpin_amd import build as vbuild
        path = os.environ.get("VPIN_HOSTTEST_LIB") or vbuild.build_hosttest()
        _lib = C.CDLL(path)
    return _lib


def table():
    """{function: (words in, words out)} as the library itself declares them"""
    global _table
    if _table is None:
        p = C.POINTER(_Entry)()
        fn = lib().hv_table
        fn.restype = C.c_int
        fn.argtypes = [C.POINTER(C.POINTER(_Entry))]
        n = fn(C.byref(p))
        _table = {p[i].name.decode(): (p[i].iw, p[i].ow) for i in range(n)}
    return _table


def run(name, rows):
    """rows: n cases of equal length (lists of ints below 2^64); returns n rows of Python ints"""
    iw, ow = table()[name]
    a = np.ascontiguousarray(np.array([[int(w) for w in r] for r in rows], dtype=np.uint64))
    assert a.ndim == 2 and a.shape[1] == iw, (name, a.shape, iw)
    out = np.full((a.shape[0], ow), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    fn = getattr(lib(), "hv_" + name)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    rc = fn(a.ctypes.data, out.ctypes.data, a.shape[0])
    assert rc == 0, f"hv_{name}: {rc}"
    return [[int(w) for w in row] for row in out]
