"""CPU tests of the by-key reduction C-ABI (drhip_reduce_by_key,
drhip_run_length_encode, drhip_unique_copy): declared, exported, in
drhip.EXPORTS, and every refusal of the header returns DRHIP_ERR_BAD_ARG,
names the function and leaves *num_runs untouched.  The arguments are checked
before the segment, so the refusals need no device; the pointers given here
are never dereferenced.  No compute calls."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "drhip.h")
SYMBOLS = ["drhip_reduce_by_key", "drhip_run_length_encode", "drhip_unique_copy"]
OK, NOT_INIT, BAD_ARG = 0, 2, 4
KI, VI, KO, VO = 0x10000000, 0x20000000, 0x30000000, 0x40000000  # four far-apart fake device addresses
SENTINEL = 0xDEADBEEF12345678


def test_header_declares_segreduce_symbols():
    src = open(HEADER).read()
    declared = set(re.findall(r"^\s*int\s*(drhip_\w+)\s*\(", src, re.M))
    assert not [s for s in SYMBOLS if s not in declared]


def test_library_exports_segreduce_symbols():
    import drhip
    drhip.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", drhip.LIB_PATH], text=True)
    exported = set(re.findall(r" T (drhip_\w+)$", out, re.M))
    assert not [s for s in SYMBOLS if s not in exported]
    assert not [s for s in SYMBOLS if s not in drhip.EXPORTS]
    for f in ("reduce_by_key_async", "run_length_encode_async", "unique_copy_async", "reduce_by_key",
              "run_length_encode", "unique_copy"):
        assert callable(getattr(drhip, f)), f


def _lib():
    import drhip
    return drhip, drhip.load()


def _refused(L, rc, runs, fn):
    assert rc == BAD_ARG, (fn, rc)
    assert runs.value == SENTINEL, fn
    assert fn.encode() in L.drhip_last_error(), L.drhip_last_error()


def test_reduce_by_key_refusals():
    drhip, L = _lib()
    runs = C.c_uint64(SENTINEL)
    r = C.byref(runs)
    fn = "drhip_reduce_by_key"
    U32, F64, PLUS = drhip.U32, drhip.F64, drhip.PLUS
    f = L.drhip_reduce_by_key
    _refused(L, f(0, 6, U32, PLUS, KI, VI, 100, KO, VO, r), runs, fn)     # unknown key dtype
    _refused(L, f(0, -1, U32, PLUS, KI, VI, 100, KO, VO, r), runs, fn)
    _refused(L, f(0, U32, 6, PLUS, KI, VI, 100, KO, VO, r), runs, fn)     # unknown value dtype
    _refused(L, f(0, U32, -1, PLUS, KI, VI, 100, KO, VO, r), runs, fn)
    _refused(L, f(0, U32, U32, 4, KI, VI, 100, KO, VO, r), runs, fn)      # unknown op
    _refused(L, f(0, U32, U32, -1, KI, VI, 100, KO, VO, r), runs, fn)
    for args in ((None, VI, KO, VO), (KI, None, KO, VO), (KI, VI, None, VO), (KI, VI, KO, None)):  # null, n > 0
        _refused(L, f(0, U32, U32, PLUS, args[0], args[1], 100, args[2], args[3], r), runs, fn)
    _refused(L, f(0, U32, U32, PLUS, KI, VI, 1 << 32, KO, VO, r), runs, fn)  # n >= 2^32
    _refused(L, f(0, U32, U32, PLUS, KI, VI, (1 << 32) + 5, KO, VO, r), runs, fn)
    # any output overlapping any input: the same range, an output inside an input, one ending inside an input
    _refused(L, f(0, U32, U32, PLUS, KI, VI, 100, KI, VO, r), runs, fn)          # keys_out on keys_in
    _refused(L, f(0, U32, U32, PLUS, KI, VI, 100, VI + 396, VO, r), runs, fn)    # keys_out on vals_in
    _refused(L, f(0, U32, U32, PLUS, KI, VI, 100, KO, KI - 396, r), runs, fn)    # vals_out on keys_in
    _refused(L, f(0, U32, F64, PLUS, KI, VI, 100, KO, VI + 799, r), runs, fn)    # vals_out on vals_in (8-byte values)
    assert f(0, U32, U32, PLUS, KI, VI, 100, KO, VO, None) == BAD_ARG            # null num_runs
    assert fn.encode() in L.drhip_last_error()


def test_run_length_encode_refusals():
    drhip, L = _lib()
    runs = C.c_uint64(SENTINEL)
    r = C.byref(runs)
    fn = "drhip_run_length_encode"
    f = L.drhip_run_length_encode
    _refused(L, f(0, 6, KI, 100, KO, VO, r), runs, fn)
    _refused(L, f(0, -1, KI, 100, KO, VO, r), runs, fn)
    _refused(L, f(0, drhip.I64, None, 100, KO, VO, r), runs, fn)
    _refused(L, f(0, drhip.I64, KI, 100, None, VO, r), runs, fn)
    _refused(L, f(0, drhip.I64, KI, 100, KO, None, r), runs, fn)
    _refused(L, f(0, drhip.I64, KI, 1 << 32, KO, VO, r), runs, fn)
    _refused(L, f(0, drhip.I64, KI, 100, KI + 8, VO, r), runs, fn)     # keys_out overlaps keys_in
    _refused(L, f(0, drhip.F32, KI, 100, KO, KI + 399, r), runs, fn)   # counts_out (uint64) overlaps keys_in
    assert f(0, drhip.I64, KI, 100, KO, VO, None) == BAD_ARG
    assert fn.encode() in L.drhip_last_error()


def test_unique_copy_refusals():
    drhip, L = _lib()
    runs = C.c_uint64(SENTINEL)
    r = C.byref(runs)
    fn = "drhip_unique_copy"
    f = L.drhip_unique_copy
    _refused(L, f(0, 6, KI, 100, KO, r), runs, fn)
    _refused(L, f(0, -1, KI, 100, KO, r), runs, fn)
    _refused(L, f(0, drhip.F64, None, 100, KO, r), runs, fn)
    _refused(L, f(0, drhip.F64, KI, 100, None, r), runs, fn)
    _refused(L, f(0, drhip.F64, KI, 1 << 32, KO, r), runs, fn)
    _refused(L, f(0, drhip.F64, KI, 100, KI, r), runs, fn)
    _refused(L, f(0, drhip.F64, KI, 100, KI + 792, r), runs, fn)
    _refused(L, f(0, drhip.F64, KI + 792, 100, KI, r), runs, fn)
    assert f(0, drhip.F64, KI, 100, KO, None) == BAD_ARG
    assert fn.encode() in L.drhip_last_error()


def test_segreduce_calls_before_init_fail_cleanly():
    drhip, L = _lib()
    if drhip.device_count() > 0:
        pytest.skip("a device is visible; covered by the gpu tests")
    runs = C.c_uint64(SENTINEL)
    r = C.byref(runs)
    assert L.drhip_reduce_by_key(0, drhip.U32, drhip.U32, drhip.PLUS, KI, VI, 100, KO, VO, r) == NOT_INIT
    assert b"drhip_init" in L.drhip_last_error()
    assert L.drhip_run_length_encode(0, drhip.U32, KI, 100, KO, VO, r) == NOT_INIT
    assert b"drhip_init" in L.drhip_last_error()
    assert L.drhip_unique_copy(0, drhip.U32, KI, 100, KO, r) == NOT_INIT
    assert b"drhip_init" in L.drhip_last_error()
    assert L.drhip_unique_copy(0, drhip.U32, None, 0, None, r) == NOT_INIT  # n == 0 too
    assert runs.value == SENTINEL
