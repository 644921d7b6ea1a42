"""CPU tests of the sorted-search C-ABI (drhip_lower_bound, drhip_upper_bound,
drhip_binary_search): declared, exported, in drhip.EXPORTS, wrapped, and every
refusal of the header returns DRHIP_ERR_BAD_ARG and names the function.  The
arguments are checked before the segment, so the refusals need no device; the
device pointers given here are fake and never dereferenced, and where the
output is a real host word the refusal leaves it untouched.  No compute calls."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "drhip.h")
KERNEL = os.path.join(ROOT, "distributed-ranges_amd", "include", "dr", "details", "bsearch_kernel.hpp")
SYMBOLS = ["drhip_lower_bound", "drhip_upper_bound", "drhip_binary_search"]
OK, NOT_INIT, BAD_ARG = 0, 2, 4
A, B, OUT = 0x10000000, 0x20000000, 0x30000000  # far-apart fake device addresses
SENTINEL = 0xDEADBEEF12345678


def test_header_declares_sorted_search_symbols():
    src = open(HEADER).read()
    declared = set(re.findall(r"^\s*int\s*(drhip_\w+)\s*\(", src, re.M))
    assert not [s for s in SYMBOLS if s not in declared]


def test_library_exports_sorted_search_symbols():
    import drhip
    drhip.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", drhip.LIB_PATH], text=True)
    exported = set(re.findall(r" T (drhip_\w+)$", out, re.M))
    assert not [s for s in SYMBOLS if s not in exported]
    assert not [s for s in SYMBOLS if s not in drhip.EXPORTS]
    for f in ("lower_bound", "upper_bound", "binary_search"):
        assert callable(getattr(drhip, f)), f
        assert callable(getattr(drhip, f + "_async")), f


def test_stage_constant_matches_the_kernel():
    """drhip.SORTED_SEARCH_STAGE, DRHIP_SORTED_SEARCH_STAGE and the kernel's constants are one number per width."""
    import drhip
    k = open(KERNEL).read()
    s4 = int(re.search(r"kBsStage4\s*=\s*(\d+)", k).group(1))
    s8 = int(re.search(r"kBsStage8\s*=\s*(\d+)", k).group(1))
    assert drhip.SORTED_SEARCH_STAGE == {4: s4, 8: s8}
    m = re.search(r"#define DRHIP_SORTED_SEARCH_STAGE\(elem_bytes\) \(\(elem_bytes\) <= 4 \? (\d+) : (\d+)\)",
                  open(HEADER).read())
    assert (int(m.group(1)), int(m.group(2))) == (s4, s8)
    for s in (s4, s8):
        assert 1024 <= s <= 8192 and s & (s - 1) == 0


def _lib():
    import drhip
    return drhip, drhip.load()


def _refused(L, rc, word, fn):
    assert rc == BAD_ARG, (fn, rc)
    assert word.value == SENTINEL, fn
    assert fn.encode() in L.drhip_last_error(), L.drhip_last_error()


@pytest.mark.parametrize("name", SYMBOLS)
def test_refusals(name):
    drhip, L = _lib()
    f = getattr(L, name)
    word = C.c_uint64(SENTINEL)  # a real output: 1 position, or 8 flags
    p = C.cast(C.byref(word), C.c_void_p)
    es_out = 1 if name == "drhip_binary_search" else 8
    _refused(L, f(0, 6, A, 100, B, 1, p), word, name)                      # unknown dtype
    _refused(L, f(0, -1, A, 100, B, 1, p), word, name)
    _refused(L, f(0, drhip.I32, None, 100, B, 1, p), word, name)           # null hay, n > 0
    _refused(L, f(0, drhip.I32, A, 100, None, 1, p), word, name)           # null needles, m > 0
    _refused(L, f(0, drhip.I32, A, 100, B, 1, None), word, name)           # null output, m > 0
    _refused(L, f(0, drhip.I32, A, 1 << 32, B, 1, p), word, name)          # n >= 2^32
    _refused(L, f(0, drhip.I32, A, (1 << 32) + 5, B, 1, p), word, name)
    _refused(L, f(0, drhip.F64, A, 100, B, 1 << 32, OUT), word, name)      # m >= 2^32
    # the output inside hay, at its last element, and hay inside the output; likewise the needles
    _refused(L, f(0, drhip.U64, A, 100, B, 10, A + 8 * 99), word, name)
    _refused(L, f(0, drhip.U64, A + es_out * 5, 1, B, 10, A), word, name)
    _refused(L, f(0, drhip.U64, A, 100, B, 10, B + 8 * 9), word, name)
    _refused(L, f(0, drhip.U64, A, 100, B + es_out * 9, 10, B), word, name)
    _refused(L, f(0, drhip.U32, A, 100, B, 10, B), word, name)
    # the real word as an output that overlaps real needles
    nd = (C.c_uint64 * 2)(1, 2)
    _refused(L, f(0, drhip.U64, A, 100, nd, 2, C.cast(C.byref(nd, 8), C.c_void_p)), word, name)
    assert (nd[0], nd[1]) == (1, 2)


@pytest.mark.parametrize("name", SYMBOLS)
def test_adjacent_buffers_are_not_an_overlap(name):
    """The output right behind hay and right before the needles passes the argument checks: without a device
    the call then stops at the segment, with the output still untouched."""
    drhip, L = _lib()
    if drhip.device_count() > 0:
        pytest.skip("a device is visible; covered by the gpu tests")
    f = getattr(L, name)
    es_out = 1 if name == "drhip_binary_search" else 8
    assert f(0, drhip.U32, A, 100, A + 400 + es_out * 10, 10, A + 400) == NOT_INIT
    assert b"drhip_init" in L.drhip_last_error()


@pytest.mark.parametrize("name", SYMBOLS)
def test_no_needles_is_ok_and_touches_nothing(name):
    drhip, L = _lib()
    f = getattr(L, name)
    word = C.c_uint64(SENTINEL)
    assert f(0, drhip.I64, A, 100, None, 0, C.cast(C.byref(word), C.c_void_p)) == OK
    assert f(0, drhip.I64, None, 0, None, 0, None) == OK
    assert word.value == SENTINEL
