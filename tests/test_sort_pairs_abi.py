"""CPU tests of the by-key sort's C-ABI (drhip_sort_pairs, drhip_merge_pairs_
runs_to and their workspace queries): declared, exported, the workspace
arithmetic, and clean refusals without a device.  No compute calls."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "drhip.h")
SYMBOLS = ["drhip_sort_pairs_workspace", "drhip_sort_pairs", "drhip_merge_pairs_workspace",
           "drhip_merge_pairs_runs_to"]
OK, NOT_INIT, BAD_ARG = 0, 2, 4


def test_header_declares_pairs_symbols():
    src = open(HEADER).read()
    declared = set(re.findall(r"^\s*int\s*(drhip_\w+)\s*\(", src, re.M))
    assert not [s for s in SYMBOLS if s not in declared]


def test_library_exports_pairs_symbols():
    import drhip
    drhip.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", drhip.LIB_PATH], text=True)
    exported = set(re.findall(r" T (drhip_\w+)$", out, re.M))
    assert not [s for s in SYMBOLS if s not in exported]
    assert not [s for s in SYMBOLS if s not in drhip.EXPORTS]


@pytest.mark.parametrize("kdtype", [np.uint32, np.float32, np.uint64, np.float64])
@pytest.mark.parametrize("val_bytes", [4, 8])
def test_sort_pairs_workspace_size(kdtype, val_bytes):
    """Never below the keys-only workspace plus the alternate values, and monotone in n."""
    import drhip
    last = 0
    for n in [0, 1, 2, 100, 4096, 4097, 16384, 16385, 65537, (1 << 20) + 13, 1 << 24, (1 << 26) - 1, 1 << 26,
              (1 << 26) + 1, 1 << 28, (1 << 30) + 5, (1 << 32) - 1]:
        ws = drhip.sort_pairs_workspace(0, kdtype, val_bytes, n)
        assert ws >= drhip.sort_workspace(0, kdtype, n) + n * val_bytes, n
        assert ws >= last, n
        last = ws


def test_sort_pairs_workspace_refusals():
    import drhip
    L = drhip.load()
    out = C.c_size_t(77)
    for vb in (0, 2, 3, 16):
        assert L.drhip_sort_pairs_workspace(0, drhip.U32, vb, 1000, C.byref(out)) == BAD_ARG, vb
        assert L.drhip_merge_pairs_workspace(0, drhip.U32, vb, 1000, 4, C.byref(out)) == BAD_ARG, vb
    assert out.value == 77
    assert L.drhip_sort_pairs_workspace(0, drhip.U32, 4, 1000, None) == BAD_ARG
    assert L.drhip_merge_pairs_workspace(0, drhip.U32, 4, 1000, 4, None) == BAD_ARG
    assert b"sort_pairs" in L.drhip_last_error() or b"merge_pairs" in L.drhip_last_error()


@pytest.mark.parametrize("kdtype", [np.uint32, np.int64])
@pytest.mark.parametrize("val_bytes", [4, 8])
def test_merge_pairs_workspace_size(kdtype, val_bytes):
    import drhip
    for n, nruns in [(0, 1), (5, 2), (100003, 8), ((1 << 20) + 13, 17)]:
        ws = drhip.merge_pairs_workspace(0, kdtype, val_bytes, n, nruns)
        assert ws >= drhip.merge_workspace(0, kdtype, n, nruns) + n * val_bytes


def test_pairs_calls_before_init_fail_cleanly():
    import drhip
    L = drhip.load()
    if drhip.device_count() > 0:
        pytest.skip("a device is visible; covered by the gpu tests")
    assert L.drhip_sort_pairs(0, drhip.U32, None, None, 4, 100, None, 0) == NOT_INIT
    assert b"drhip_init" in L.drhip_last_error()
    offs = (C.c_size_t * 2)(0, 100)
    assert L.drhip_merge_pairs_runs_to(0, drhip.U32, 4, None, None, None, None, 100, offs, 1, None, 0) == NOT_INIT
    assert b"drhip_init" in L.drhip_last_error()
