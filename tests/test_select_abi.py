"""CPU tests of the selection C-ABI (drhip_count_if, drhip_copy_if,
drhip_copy_flagged): declared, exported, in drhip.EXPORTS, and every refusal
of the header returns its code and leaves *count untouched.  The arguments
are checked before the segment, so the refusals need no device; the pointers
given here are never dereferenced.  No compute calls."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "drhip.h")
SYMBOLS = ["drhip_count_if", "drhip_copy_if", "drhip_copy_flagged"]
OK, NOT_INIT, BAD_ARG = 0, 2, 4
A, B, F = 0x10000000, 0x20000000, 0x30000000  # three far-apart fake device addresses
SENTINEL = 0xDEADBEEF12345678


def test_header_declares_select_symbols():
    src = open(HEADER).read()
    declared = set(re.findall(r"^\s*int\s*(drhip_\w+)\s*\(", src, re.M))
    assert not [s for s in SYMBOLS if s not in declared]
    for name in ("DRHIP_LT = 0", "DRHIP_LE = 1", "DRHIP_GT = 2", "DRHIP_GE = 3", "DRHIP_EQ = 4", "DRHIP_NE = 5"):
        assert name in src, name


def test_library_exports_select_symbols():
    import drhip
    drhip.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", drhip.LIB_PATH], text=True)
    exported = set(re.findall(r" T (drhip_\w+)$", out, re.M))
    assert not [s for s in SYMBOLS if s not in exported]
    assert not [s for s in SYMBOLS if s not in drhip.EXPORTS]
    assert (drhip.LT, drhip.LE, drhip.GT, drhip.GE, drhip.EQ, drhip.NE) == (0, 1, 2, 3, 4, 5)
    for f in ("count_if_async", "copy_if_async", "copy_flagged_async", "count_if", "copy_if", "copy_flagged"):
        assert callable(getattr(drhip, f)), f


def _lib():
    import drhip
    return drhip, drhip.load()


def _refused(L, rc, count, fn):
    assert rc == BAD_ARG, (fn, rc)
    assert count.value == SENTINEL, fn
    assert fn.encode() in L.drhip_last_error(), L.drhip_last_error()


def test_count_if_refusals():
    drhip, L = _lib()
    cnt = C.c_uint64(SENTINEL)
    sc = np.array([5], np.int32).ctypes.data_as(C.c_void_p)
    c = C.byref(cnt)
    fn = "drhip_count_if"
    _refused(L, L.drhip_count_if(0, 6, drhip.LT, A, 100, sc, c), cnt, fn)      # unknown dtype
    _refused(L, L.drhip_count_if(0, -1, drhip.LT, A, 100, sc, c), cnt, fn)
    _refused(L, L.drhip_count_if(0, drhip.I32, 6, A, 100, sc, c), cnt, fn)     # unknown cmp
    _refused(L, L.drhip_count_if(0, drhip.I32, -1, A, 100, sc, c), cnt, fn)
    _refused(L, L.drhip_count_if(0, drhip.I32, drhip.LT, None, 100, sc, c), cnt, fn)  # null x, n > 0
    _refused(L, L.drhip_count_if(0, drhip.I32, drhip.LT, A, 1 << 32, sc, c), cnt, fn)  # n >= 2^32
    assert L.drhip_count_if(0, drhip.I32, drhip.LT, A, 100, sc, None) == BAD_ARG  # null count
    assert b"drhip_count_if" in L.drhip_last_error()


def test_copy_if_refusals():
    drhip, L = _lib()
    cnt = C.c_uint64(SENTINEL)
    sc = np.array([5.0], np.float32).ctypes.data_as(C.c_void_p)
    c = C.byref(cnt)
    fn = "drhip_copy_if"
    _refused(L, L.drhip_copy_if(0, 17, drhip.GT, A, B, 100, sc, c), cnt, fn)
    _refused(L, L.drhip_copy_if(0, drhip.F32, 9, A, B, 100, sc, c), cnt, fn)
    _refused(L, L.drhip_copy_if(0, drhip.F32, drhip.GT, None, B, 100, sc, c), cnt, fn)
    _refused(L, L.drhip_copy_if(0, drhip.F32, drhip.GT, A, None, 100, sc, c), cnt, fn)
    _refused(L, L.drhip_copy_if(0, drhip.F32, drhip.GT, A, B, 1 << 32, sc, c), cnt, fn)
    _refused(L, L.drhip_copy_if(0, drhip.F32, drhip.GT, A, B, (1 << 32) + 5, sc, c), cnt, fn)
    # out overlaps in: the same range, out inside in, out ending inside in
    _refused(L, L.drhip_copy_if(0, drhip.F32, drhip.GT, A, A, 100, sc, c), cnt, fn)
    _refused(L, L.drhip_copy_if(0, drhip.F32, drhip.GT, A, A + 396, 100, sc, c), cnt, fn)
    _refused(L, L.drhip_copy_if(0, drhip.F32, drhip.GT, A + 396, A, 100, sc, c), cnt, fn)
    assert L.drhip_copy_if(0, drhip.F32, drhip.GT, A, B, 100, sc, None) == BAD_ARG
    assert b"drhip_copy_if" in L.drhip_last_error()


def test_copy_flagged_refusals():
    drhip, L = _lib()
    cnt = C.c_uint64(SENTINEL)
    c = C.byref(cnt)
    fn = "drhip_copy_flagged"
    for eb in (0, 1, 2, 3, 5, 12, 16):
        _refused(L, L.drhip_copy_flagged(0, eb, A, F, B, 100, c), cnt, fn)
    _refused(L, L.drhip_copy_flagged(0, 4, None, F, B, 100, c), cnt, fn)
    _refused(L, L.drhip_copy_flagged(0, 4, A, None, B, 100, c), cnt, fn)
    _refused(L, L.drhip_copy_flagged(0, 8, A, F, None, 100, c), cnt, fn)
    _refused(L, L.drhip_copy_flagged(0, 8, A, F, B, 1 << 32, c), cnt, fn)
    _refused(L, L.drhip_copy_flagged(0, 4, A, F, A + 4, 100, c), cnt, fn)   # out overlaps in
    _refused(L, L.drhip_copy_flagged(0, 8, A, B + 799, B, 100, c), cnt, fn)  # out overlaps flags
    assert L.drhip_copy_flagged(0, 4, A, F, B, 100, None) == BAD_ARG
    assert b"drhip_copy_flagged" in L.drhip_last_error()


def test_select_calls_before_init_fail_cleanly():
    drhip, L = _lib()
    if drhip.device_count() > 0:
        pytest.skip("a device is visible; covered by the gpu tests")
    cnt = C.c_uint64(SENTINEL)
    sc = np.array([5], np.uint32).ctypes.data_as(C.c_void_p)
    assert L.drhip_count_if(0, drhip.U32, drhip.EQ, A, 100, sc, C.byref(cnt)) == NOT_INIT
    assert b"drhip_init" in L.drhip_last_error()
    assert L.drhip_copy_if(0, drhip.U32, drhip.EQ, A, B, 100, sc, C.byref(cnt)) == NOT_INIT
    assert b"drhip_init" in L.drhip_last_error()
    assert L.drhip_copy_flagged(0, 4, A, F, B, 100, C.byref(cnt)) == NOT_INIT
    assert b"drhip_init" in L.drhip_last_error()
    assert L.drhip_count_if(0, drhip.U32, drhip.EQ, None, 0, sc, C.byref(cnt)) == NOT_INIT  # n == 0 too
    assert cnt.value == SENTINEL
