"""The general-comparator tier of shp::sort / shp::stable_sort
(distributed-ranges_amd/include/dr/shp/merge_sort.hpp, detail::sort_general in
dr/shp/sort.hpp): the C++ suite tests/cpp/merge_sort_tests.cpp compares every
result byte for byte with std::stable_sort on a host copy -- segment lengths
on, one past and one short of every tile multiple, thirteen element sizes from
1 to 256 bytes, key patterns that leave runs empty or one element long,
comparators with state, sub-ranges and uneven distributed_spans -- on the
default device list and with 1, 2, 3, 5, 7 and 8 segments duplicated on one
GPU (5, 6 and 7 runs take three merge rounds with an odd run left over).
merge_sort_tests_st512 is the same file built with 512-thread block sorts
(first runs twice the merge tile); merge_path_test checks msort::merge_path
against its definition on the host."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINDIR = os.path.join(ROOT, "tests", "cpp", "bin")
BIN = os.path.join(BINDIR, "merge_sort_tests")
BIN_ST512 = os.path.join(BINDIR, "merge_sort_tests_st512")
MERGE_PATH = os.path.join(BINDIR, "merge_path_test")

# set by the first child that ends in anything but 0 (passed) or 1 (a test
# failed): a signal, an abort or a timeout is a fault of the GPU program, and
# nothing more is started on the GPU by this file after one
_fault = []


def test_merge_sort_tests_built():
    """build() compiles the three programs with hipcc for gfx950 (make -C distributed-ranges_amd)."""
    for exe in (BIN, BIN_ST512, MERGE_PATH):
        assert os.path.exists(exe), f"{exe}: run __graft_entry__.build() (make -C distributed-ranges_amd)"


def test_merge_path_on_the_host():
    """msort::merge_path against std::merge's prefix counts, exhaustively on short inputs (no GPU, no HIP call)."""
    r = subprocess.run([MERGE_PATH], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    print(r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "PASSED" in r.stdout and " 0 wrong" in r.stdout


def _run(exe, args):
    if _fault:
        pytest.fail(f"not started: {_fault[0]}")
    try:
        r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        _fault.append(f"{os.path.basename(exe)} {' '.join(args)} did not end within its time limit")
        raise
    print(r.stdout[-6000:])
    print(r.stderr[-2000:])
    if r.returncode not in (0, 1):
        _fault.append(f"{os.path.basename(exe)} {' '.join(args)} ended with status {r.returncode}")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " 0 failed" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("devices", [0, 1, 2, 3, 5, 7, 8])
def test_cpp_merge_sort_suite(devices):
    _run(BIN, ["--devicesCount", str(devices)] if devices else [])


@pytest.mark.gpu
@pytest.mark.parametrize("devices", [1, 3])
def test_cpp_merge_sort_suite_512_thread_block_sort(devices):
    """DR_SHP_MSORT_SORT_THREADS=512: the first sorted runs are twice the merge tile for elements up to 128 bytes
    (a wrong ratio merges the wrong elements), and the 256-byte element falls back to 256 threads."""
    _run(BIN_ST512, ["--devicesCount", str(devices)])


def _visible_gpus():
    import drhip
    drhip.load()
    return drhip.device_count()


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["distinct", "alternating"])
def test_cpp_merge_sort_distinct_devices(pattern):
    """Segments on DIFFERENT GPUs: the pieces move by peer copies and every device reads the indirect
    comparator's pinned table.  Needs >= 2 visible GPUs (skipped on a one-GPU box)."""
    n = _visible_gpus()
    if n < 2:
        pytest.skip(f"{n} GPU visible: distinct-device segments need >= 2")
    ids = list(range(n)) if pattern == "distinct" else [0, 1, 0, 1]
    _run(BIN, ["--devices", ",".join(map(str, ids))])
