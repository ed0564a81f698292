"""ctypes loader of vpin_amd/lib/libvpin_devtest.so (tests/devarith/devarith.hip): one launcher per device function, flat
arrays of 32-bit words in and out.  The library is built when it is missing or older than its sources; a library that cannot
be built or loaded is an error, never a skip.  VPIN_DEVTEST_LIB names another build of the harness (one compiled against a
mutated copy of the headers, to see that the tests notice); it has to sit beside libvpin_hip.so, which it refers to."""
import ctypes as C
import os

import numpy as np

_lib = None
_failed = None  # the first launcher that returned a HIP error: nothing more is launched after it


def lib():
    global _lib
    if _lib is None:
        from vpin_amd import build as vbuild
        path = os.environ.get("VPIN_DEVTEST_LIB") or vbuild.build_devtest()
        _lib = C.CDLL(path)
    return _lib


def _call(name, fn, *args):
    global _failed
    assert _failed is None, f"not launched: {_failed} returned a HIP error earlier in this process"
    rc = fn(*args)
    if rc != 0:
        _failed = f"dv_{name}"
    assert rc == 0, f"dv_{name}: HIP error {rc}"


def run(name, rows, out_words):
    """rows: n cases of equal length (lists of ints below 2^32, or a 2-D array); returns an (n, out_words) uint32 array"""
    a = np.ascontiguousarray(np.array(rows, dtype=np.uint64).astype(np.uint32))
    assert a.ndim == 2, a.shape
    out = np.zeros((a.shape[0], out_words), dtype=np.uint32)
    fn = getattr(lib(), "dv_" + name)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    _call(name, fn, a.ctypes.data, out.ctypes.data, a.shape[0])
    return out


def run_mul_const_host(r_words, rows):
    a = np.ascontiguousarray(np.array(rows, dtype=np.uint64).astype(np.uint32))
    out = np.zeros_like(a)
    r = np.array(r_words, dtype=np.uint64).astype(np.uint32)
    fn = lib().dv_fq_mul_const_host
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    _call("fq_mul_const_host", fn, r.ctypes.data, a.ctypes.data, out.ctypes.data, a.shape[0])
    return out


def ints(arr, n=8):
    """rows of n little-endian 32-bit words -> Python ints"""
    return [sum(int(w) << (32 * i) for i, w in enumerate(row[:n])) for row in arr]
