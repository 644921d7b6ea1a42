"""CPU tests of the by-key scan C-ABI (drhip_inclusive_scan_by_key,
drhip_exclusive_scan_by_key): declared, exported, in drhip.EXPORTS, the Python
callables exist, and every refusal of the header returns DRHIP_ERR_BAD_ARG and
names the function.  The arguments are checked before the segment, so the
refusals need no device; the pointers given here are never dereferenced.
vals_out == vals_in is the in-place form and is not refused.  No compute calls."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "drhip.h")
SYMBOLS = ["drhip_inclusive_scan_by_key", "drhip_exclusive_scan_by_key"]
OK, NOT_INIT, BAD_ARG = 0, 2, 4
KI, VI, VO = 0x10000000, 0x20000000, 0x40000000  # far-apart fake device addresses


def test_header_declares_segscan_symbols():
    src = open(HEADER).read()
    declared = set(re.findall(r"^\s*int\s*(drhip_\w+)\s*\(", src, re.M))
    assert not [s for s in SYMBOLS if s not in declared]


def test_library_exports_segscan_symbols():
    import drhip
    drhip.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", drhip.LIB_PATH], text=True)
    exported = set(re.findall(r" T (drhip_\w+)$", out, re.M))
    assert not [s for s in SYMBOLS if s not in exported]
    assert not [s for s in SYMBOLS if s not in drhip.EXPORTS]
    for f in ("inclusive_scan_by_key_async", "exclusive_scan_by_key_async", "inclusive_scan_by_key",
              "exclusive_scan_by_key"):
        assert callable(getattr(drhip, f)), f


def _calls():
    """(name, f(seg, kdtype, vdtype, op, keys, vals, n, out)) for both entries; the exclusive one with and without init."""
    import drhip
    L = drhip.load()
    init = np.array([5], np.uint64)  # 8 readable bytes: enough for every value dtype
    ip = init.ctypes.data_as(C.c_void_p)
    return drhip, L, [
        ("drhip_inclusive_scan_by_key", lambda s, kd, vd, op, k, v, n, o: L.drhip_inclusive_scan_by_key(s, kd, vd, op, k, v, n, o)),
        ("drhip_exclusive_scan_by_key", lambda s, kd, vd, op, k, v, n, o: L.drhip_exclusive_scan_by_key(s, kd, vd, op, k, v, n, ip, o)),
        ("drhip_exclusive_scan_by_key", lambda s, kd, vd, op, k, v, n, o: L.drhip_exclusive_scan_by_key(s, kd, vd, op, k, v, n, None, o)),
    ]


def _refused(L, rc, fn):
    assert rc == BAD_ARG, (fn, rc)
    assert fn.encode() in L.drhip_last_error(), L.drhip_last_error()


def test_scan_by_key_refusals():
    drhip, L, calls = _calls()
    U32, F64, PLUS = drhip.U32, drhip.F64, drhip.PLUS
    for fn, f in calls:
        _refused(L, f(0, 6, U32, PLUS, KI, VI, 100, VO), fn)      # unknown key dtype
        _refused(L, f(0, -1, U32, PLUS, KI, VI, 100, VO), fn)
        _refused(L, f(0, U32, 6, PLUS, KI, VI, 100, VO), fn)      # unknown value dtype
        _refused(L, f(0, U32, -1, PLUS, KI, VI, 100, VO), fn)
        _refused(L, f(0, U32, U32, 4, KI, VI, 100, VO), fn)       # unknown op
        _refused(L, f(0, U32, U32, -1, KI, VI, 100, VO), fn)
        _refused(L, f(0, U32, U32, PLUS, None, VI, 100, VO), fn)  # null with n > 0
        _refused(L, f(0, U32, U32, PLUS, KI, None, 100, VO), fn)
        _refused(L, f(0, U32, U32, PLUS, KI, VI, 100, None), fn)
        _refused(L, f(0, U32, U32, PLUS, KI, VI, 1 << 32, VO), fn)  # n >= 2^32
        _refused(L, f(0, U32, U32, PLUS, KI, VI, (1 << 32) + 5, VO), fn)
        # vals_out on keys_in: the same range, ending inside it, starting inside it
        _refused(L, f(0, U32, U32, PLUS, KI, VI, 100, KI), fn)
        _refused(L, f(0, U32, U32, PLUS, KI, VI, 100, KI - 396), fn)
        _refused(L, f(0, U32, F64, PLUS, KI, VI, 100, KI + 399), fn)
        # vals_out on vals_in other than vals_out == vals_in
        _refused(L, f(0, U32, U32, PLUS, KI, VI, 100, VI + 4), fn)
        _refused(L, f(0, U32, U32, PLUS, KI, VI, 100, VI - 396), fn)
        _refused(L, f(0, U32, F64, PLUS, KI, VI, 100, VI + 799), fn)
        _refused(L, f(0, U32, F64, PLUS, KI, VI, 100, VI - 8), fn)


def test_segscan_calls_before_init_fail_cleanly():
    drhip, L, calls = _calls()
    if drhip.device_count() > 0:
        pytest.skip("a device is visible; covered by the gpu tests")
    for fn, f in calls:
        assert f(0, drhip.U32, drhip.U32, drhip.PLUS, KI, VI, 100, VO) == NOT_INIT
        assert b"drhip_init" in L.drhip_last_error()
        assert f(0, drhip.U32, drhip.U32, drhip.PLUS, KI, VI, 100, VI) == NOT_INIT  # in place: not refused
        assert b"drhip_init" in L.drhip_last_error()
        assert f(0, drhip.U32, drhip.F64, drhip.MAX, KI, VI, 100, VO) == NOT_INIT
        assert f(0, drhip.U32, drhip.U32, drhip.PLUS, None, None, 0, None) == NOT_INIT  # n == 0 too
