"""CPU tests of the search C-ABI (drhip_find_if, drhip_is_sorted_until,
drhip_mismatch, drhip_min_element, drhip_max_element, drhip_minmax_element):
declared, exported, in drhip.EXPORTS, and every refusal of the header returns
its code, leaves *index untouched and names the function.  The arguments are
checked before the segment, so the refusals need no device; the pointers given
here are never dereferenced.  No compute calls."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "drhip.h")
SYMBOLS = ["drhip_find_if", "drhip_is_sorted_until", "drhip_mismatch", "drhip_min_element", "drhip_max_element",
           "drhip_minmax_element"]
OK, NOT_INIT, BAD_ARG = 0, 2, 4
A, B = 0x10000000, 0x20000000  # two far-apart fake device addresses
SENTINEL = 0xDEADBEEF12345678


def test_header_declares_search_symbols():
    src = open(HEADER).read()
    declared = set(re.findall(r"^\s*int\s*(drhip_\w+)\s*\(", src, re.M))
    assert not [s for s in SYMBOLS if s not in declared]


def test_library_exports_search_symbols():
    import drhip
    drhip.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", drhip.LIB_PATH], text=True)
    exported = set(re.findall(r" T (drhip_\w+)$", out, re.M))
    assert not [s for s in SYMBOLS if s not in exported]
    assert not [s for s in SYMBOLS if s not in drhip.EXPORTS]
    for f in ("find_if", "is_sorted_until", "mismatch", "min_element", "max_element", "minmax_element"):
        assert callable(getattr(drhip, f)), f
        assert callable(getattr(drhip, f + "_async")), f


def _lib():
    import drhip
    return drhip, drhip.load()


def _refused(L, rc, index, fn):
    assert rc == BAD_ARG, (fn, rc)
    assert index.value == SENTINEL, fn
    assert fn.encode() in L.drhip_last_error(), L.drhip_last_error()


def test_find_if_refusals():
    drhip, L = _lib()
    idx = C.c_uint64(SENTINEL)
    sc = np.array([5], np.int32).ctypes.data_as(C.c_void_p)
    p = C.byref(idx)
    fn = "drhip_find_if"
    _refused(L, L.drhip_find_if(0, 6, drhip.LT, A, 100, sc, p), idx, fn)       # unknown dtype
    _refused(L, L.drhip_find_if(0, -1, drhip.LT, A, 100, sc, p), idx, fn)
    _refused(L, L.drhip_find_if(0, drhip.I32, 6, A, 100, sc, p), idx, fn)      # unknown cmp
    _refused(L, L.drhip_find_if(0, drhip.I32, -1, A, 100, sc, p), idx, fn)
    _refused(L, L.drhip_find_if(0, drhip.I32, drhip.LT, None, 100, sc, p), idx, fn)  # null x, n > 0
    _refused(L, L.drhip_find_if(0, drhip.I32, drhip.LT, A, 100, None, p), idx, fn)   # null scalar
    _refused(L, L.drhip_find_if(0, drhip.I32, drhip.LT, A, 1 << 32, sc, p), idx, fn)  # n >= 2^32
    _refused(L, L.drhip_find_if(0, drhip.I32, drhip.LT, A, (1 << 32) + 5, sc, p), idx, fn)
    assert L.drhip_find_if(0, drhip.I32, drhip.LT, A, 100, sc, None) == BAD_ARG  # null index
    assert b"drhip_find_if" in L.drhip_last_error()


@pytest.mark.parametrize("name", ["drhip_is_sorted_until", "drhip_min_element", "drhip_max_element",
                                  "drhip_minmax_element"])
def test_one_input_refusals(name):
    drhip, L = _lib()
    f = getattr(L, name)
    idx = (C.c_uint64 * 2)(SENTINEL, SENTINEL)
    first = C.c_uint64.from_buffer(idx)
    _refused(L, f(0, 6, A, 100, idx), first, name)
    _refused(L, f(0, -1, A, 100, idx), first, name)
    _refused(L, f(0, drhip.F64, None, 100, idx), first, name)
    _refused(L, f(0, drhip.F64, A, 1 << 32, idx), first, name)
    assert idx[1] == SENTINEL
    assert f(0, drhip.F64, A, 100, None) == BAD_ARG
    assert name.encode() in L.drhip_last_error()


def test_mismatch_refusals():
    drhip, L = _lib()
    idx = C.c_uint64(SENTINEL)
    p = C.byref(idx)
    fn = "drhip_mismatch"
    _refused(L, L.drhip_mismatch(0, 9, A, B, 100, p), idx, fn)
    _refused(L, L.drhip_mismatch(0, drhip.U64, None, B, 100, p), idx, fn)
    _refused(L, L.drhip_mismatch(0, drhip.U64, A, None, 100, p), idx, fn)
    _refused(L, L.drhip_mismatch(0, drhip.U64, A, B, 1 << 32, p), idx, fn)
    assert L.drhip_mismatch(0, drhip.U64, A, B, 100, None) == BAD_ARG
    assert b"drhip_mismatch" in L.drhip_last_error()


def test_search_calls_before_init_fail_cleanly():
    drhip, L = _lib()
    if drhip.device_count() > 0:
        pytest.skip("a device is visible; covered by the gpu tests")
    idx = C.c_uint64(SENTINEL)
    sc = np.array([5], np.uint32).ctypes.data_as(C.c_void_p)
    p = C.byref(idx)
    assert L.drhip_find_if(0, drhip.U32, drhip.EQ, A, 100, sc, p) == NOT_INIT
    assert b"drhip_init" in L.drhip_last_error()
    assert L.drhip_is_sorted_until(0, drhip.U32, A, 100, p) == NOT_INIT
    assert L.drhip_mismatch(0, drhip.U32, A, B, 100, p) == NOT_INIT
    assert L.drhip_min_element(0, drhip.U32, A, 100, p) == NOT_INIT
    assert L.drhip_max_element(0, drhip.U32, A, 100, p) == NOT_INIT
    assert L.drhip_minmax_element(0, drhip.U32, A, 100, p) == NOT_INIT
    assert b"drhip_init" in L.drhip_last_error()
    assert L.drhip_find_if(0, drhip.U32, drhip.EQ, None, 0, sc, p) == NOT_INIT  # n == 0 too
    assert idx.value == SENTINEL
