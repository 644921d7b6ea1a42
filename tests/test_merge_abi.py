"""CPU tests of the merge C-ABI (drhip_merge, drhip_merge_pairs): declared,
exported, in drhip.EXPORTS, wrapped, the tile constant stated once per width,
and every refusal of the header returns DRHIP_ERR_BAD_ARG and names the
function.  The arguments are checked before the segment, so the refusals need
no device; the device pointers given here are fake and never dereferenced, and
where the output is a real host word the refusal leaves it untouched.  No
compute calls."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "drhip.h")
KERNEL = os.path.join(ROOT, "distributed-ranges_amd", "include", "dr", "details", "merge_kernel.hpp")
SYMBOLS = ["drhip_merge", "drhip_merge_pairs"]
OK, NOT_INIT, BAD_ARG = 0, 2, 4
# far-apart fake device addresses
A, B, OUT, AV, BV, VOUT = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000
SENTINEL = 0xDEADBEEF12345678


def test_header_declares_merge_symbols():
    src = open(HEADER).read()
    declared = set(re.findall(r"^\s*int\s*(drhip_\w+)\s*\(", src, re.M))
    assert not [s for s in SYMBOLS if s not in declared]


def test_library_exports_merge_symbols():
    import drhip
    drhip.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", drhip.LIB_PATH], text=True)
    exported = set(re.findall(r" T (drhip_\w+)$", out, re.M))
    assert not [s for s in SYMBOLS if s not in exported]
    assert not [s for s in SYMBOLS if s not in drhip.EXPORTS]
    for f in ("merge", "merge_pairs"):
        assert callable(getattr(drhip, f)), f
        assert callable(getattr(drhip, f + "_async")), f


def test_tile_constant_matches_the_kernel():
    """drhip.MERGE_TILE, DRHIP_MERGE_TILE and the kernel's constants are one number per width."""
    import drhip
    k = open(KERNEL).read()
    t4 = int(re.search(r"kMgTile4\s*=\s*(\d+)", k).group(1))
    t8 = int(re.search(r"kMgTile8\s*=\s*(\d+)", k).group(1))
    threads = int(re.search(r"kMgThreads\s*=\s*(\d+)", k).group(1))
    assert drhip.MERGE_TILE == {4: t4, 8: t8}
    m = re.search(r"#define DRHIP_MERGE_TILE\(elem_bytes\) \(\(elem_bytes\) <= 4 \? (\d+) : (\d+)\)", open(HEADER).read())
    assert (int(m.group(1)), int(m.group(2))) == (t4, t8)
    for t in (t4, t8):
        assert t % threads == 0 and 1 <= t // threads <= 16


def _lib():
    import drhip
    return drhip, drhip.load()


def _refused(L, rc, words, fn):
    assert rc == BAD_ARG, (fn, rc)
    for w in words:
        assert w.value == SENTINEL, fn
    assert fn.encode() in L.drhip_last_error(), L.drhip_last_error()


def test_merge_refusals():
    drhip, L = _lib()
    f, name = L.drhip_merge, "drhip_merge"
    word = C.c_uint64(SENTINEL)  # a real output: 1 or 2 elements
    p = C.cast(C.byref(word), C.c_void_p)
    no = lambda rc: _refused(L, rc, [word], name)  # noqa: E731
    no(f(0, 6, A, 1, B, 1, p))                                  # unknown dtype
    no(f(0, -1, A, 1, B, 1, p))
    no(f(0, drhip.I32, None, 1, B, 1, p))                       # null a, na > 0
    no(f(0, drhip.I32, A, 1, None, 1, p))                       # null b, nb > 0
    no(f(0, drhip.I32, A, 1, B, 1, None))                       # null output
    no(f(0, drhip.I32, None, 0, B, 1, None))                    # null output of a copy
    no(f(0, drhip.I32, A, 1 << 32, B, 0, OUT))                  # na + nb >= 2^32
    no(f(0, drhip.I32, A, 1 << 31, B, 1 << 31, OUT))
    no(f(0, drhip.F64, A, 5, B, (1 << 32) - 5, OUT))
    no(f(0, drhip.U32, A, (1 << 64) - 1, B, 2, OUT))            # the sum wraps
    # the output on a's last element, a inside the output; likewise b; the output's tail on b
    no(f(0, drhip.U64, A, 100, B, 10, A + 8 * 99))
    no(f(0, drhip.U64, A + 8 * 5, 1, B, 10, A))
    no(f(0, drhip.U64, A, 100, B, 10, B + 8 * 9))
    no(f(0, drhip.U64, A, 100, B + 8 * 109, 10, B))
    no(f(0, drhip.U32, A, 100, B, 10, B))
    no(f(0, drhip.U32, A, 100, A + 400 + 440 - 4, 10, A + 400))
    # the real word as an output that overlaps a real input, also where that input is the one only copied
    nd = (C.c_uint64 * 2)(1, 2)
    no(f(0, drhip.U64, nd, 2, B, 1, C.cast(C.byref(nd, 8), C.c_void_p)))
    no(f(0, drhip.U64, nd, 2, None, 0, C.cast(C.byref(nd, 8), C.c_void_p)))
    assert (nd[0], nd[1]) == (1, 2)


def test_merge_pairs_refusals():
    drhip, L = _lib()
    f, name = L.drhip_merge_pairs, "drhip_merge_pairs"
    kw, vw = C.c_uint64(SENTINEL), C.c_uint64(SENTINEL)  # real outputs
    pk, pv = C.cast(C.byref(kw), C.c_void_p), C.cast(C.byref(vw), C.c_void_p)
    no = lambda rc: _refused(L, rc, [kw, vw], name)  # noqa: E731
    no(f(0, 6, A, AV, 1, B, BV, 1, 4, pk, pv))                  # unknown dtype
    for vb in (0, 1, 2, 3, 5, 12, 16):                          # val_bytes outside {4, 8}
        no(f(0, drhip.I32, A, AV, 1, B, BV, 1, vb, pk, pv))
    no(f(0, drhip.I32, A, AV, 0, B, BV, 0, 3, pk, pv))          # ... also with nothing to merge
    no(f(0, drhip.I32, None, AV, 1, B, BV, 1, 4, pk, pv))       # null pointers with a non-zero length
    no(f(0, drhip.I32, A, None, 1, B, BV, 1, 4, pk, pv))
    no(f(0, drhip.I32, A, AV, 1, None, BV, 1, 4, pk, pv))
    no(f(0, drhip.I32, A, AV, 1, B, None, 1, 4, pk, pv))
    no(f(0, drhip.I32, A, AV, 1, B, BV, 1, 4, None, pv))
    no(f(0, drhip.I32, A, AV, 1, B, BV, 1, 4, pk, None))
    no(f(0, drhip.I32, A, AV, 1 << 31, B, BV, 1 << 31, 8, OUT, VOUT))  # na + nb >= 2^32
    # either output on any input, over the full extents; the outputs on each other
    no(f(0, drhip.U32, A, AV, 100, B, BV, 10, 8, A + 4 * 99, VOUT))
    no(f(0, drhip.U32, A, AV, 100, B, BV, 10, 8, AV + 8 * 99, VOUT))
    no(f(0, drhip.U32, A, AV, 100, B, BV, 10, 8, OUT, B + 4 * 9))
    no(f(0, drhip.U32, A, AV, 100, B, BV, 10, 8, OUT, BV + 8 * 9))
    no(f(0, drhip.U32, A, AV, 100, B, BV + 8 * 109, 10, 8, OUT, BV))
    no(f(0, drhip.U32, A, AV, 100, B, BV, 10, 4, OUT, OUT + 4 * 109))
    nd = (C.c_uint64 * 2)(1, 2)
    no(f(0, drhip.U64, A, nd, 2, B, BV, 1, 8, OUT, C.cast(C.byref(nd, 8), C.c_void_p)))
    assert (nd[0], nd[1]) == (1, 2)


def test_adjacent_buffers_are_not_an_overlap():
    """a, b and the output back to back pass the argument checks: without a device the call then stops at the
    segment."""
    drhip, L = _lib()
    if drhip.device_count() > 0:
        pytest.skip("a device is visible; covered by the gpu tests")
    # a[100] | out[110] | b[10], 4-byte elements
    assert L.drhip_merge(0, drhip.U32, A, 100, A + 400 + 440, 10, A + 400) == NOT_INIT
    assert b"drhip_init" in L.drhip_last_error()
    # keys: a | out | b; values (8 bytes): a | b | out
    assert L.drhip_merge_pairs(0, drhip.U32, A, AV, 100, A + 400 + 440, AV + 800, 10, 8, A + 400, AV + 880) == NOT_INIT
    assert b"drhip_init" in L.drhip_last_error()


def test_nothing_to_merge_is_ok_and_touches_nothing():
    drhip, L = _lib()
    word = C.c_uint64(SENTINEL)
    p = C.cast(C.byref(word), C.c_void_p)
    assert L.drhip_merge(0, drhip.I64, A, 0, B, 0, p) == OK
    assert L.drhip_merge(0, drhip.I64, None, 0, None, 0, None) == OK
    assert L.drhip_merge_pairs(0, drhip.I64, A, AV, 0, B, BV, 0, 4, p, p) == OK
    assert L.drhip_merge_pairs(0, drhip.F32, None, None, 0, None, None, 0, 8, None, None) == OK
    assert word.value == SENTINEL
