"""Bit-exact GPU parity of drhip_stencil1d / drhip_stencil2d (csrc/stencil.hip)
on the paths the oracle-based tests of test_gpu_elementwise.py do not reach:
the 8-byte types (Vec16<T>::N == 2, so radius 2 is the full vector width and
radius 3+ changes kernel), radius >= 5, sub-ranges with radius > 1 and bounds
off the vector width, misaligned sub-ranges, int32 and misaligned 2-D, small
2-D widths, and the per-call kernel knobs DRHIP_ST1D_BLK / DRHIP_ST_NT.

The references are ref1d / ref2d of test_reference_helpers.py (checked there
against the oracle).  Every output buffer starts as a sentinel; everything
outside the cells the call owns -- halo cells, the rest of a sub-range's
buffer, columns 0 and nx - 1, 16 guard cells on both sides -- must keep it."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_reference_helpers import ref1d, ref2d

pytestmark = pytest.mark.gpu

G = 16  # guard elements around every buffer (keeps the 16-byte alignment)


def bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def sentinel(dtype):
    return np.dtype(dtype).type(-12345)


def make(dtype, n, seed, exact=True):
    """Integers over the full range; floats integer-valued (window sums exact
    in any order, so the summation order cannot hide an indexing error) or,
    exact=False, random (bit-exact only in the reference's order)."""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    if dt.kind == "i":
        return rng.integers(np.iinfo(dt).min, np.iinfo(dt).max, n, endpoint=True, dtype=dt)
    if exact:
        return rng.integers(-1000, 1000, n, endpoint=True).astype(dt)
    return (rng.random(n) * 100).astype(dt)


def run1d(dr, x, r, off, lo=None, hi=None):
    """drhip_stencil1d on the buffer x = [r halo | owned | r halo] placed
    `off` elements past a 16-byte boundary; returns the whole output buffer
    (guards included) and the expected one."""
    dt, n = x.dtype, x.size
    n_owned = n - 2 * r
    lo, hi = (0, n_owned) if lo is None else (lo, hi)
    hin = np.concatenate([np.full(G + off, 7, dt), x, np.full(G, 7, dt)])
    hout = np.full(G + off + n + G, sentinel(dt), dt)
    src = dr.DeviceArray(0, hin.size, dt, host=hin)
    dst = dr.DeviceArray(0, hout.size, dt, host=hout)
    dr.stencil1d(0, dt, src.at(G + off), dst.at(G + off), n_owned, r, lo, hi)
    got = dst.numpy()
    src.free()
    dst.free()
    hout[G + off + r + lo:G + off + r + hi] = ref1d(x, r)[lo:hi]
    return got, hout


@pytest.mark.parametrize("dtype", [np.float32, np.int32, np.float64, np.int64])
@pytest.mark.parametrize("r", [1, 2, 3, 4, 5, 9])
def test_stencil1d_types_radii(dr, dtype, r):
    """8-byte types: radius 1-2 the vector kernels, 3+ stencil1d_generic;
    4-byte types: radius 1-4 vector, 5+ generic; misaligned buffers: radius 1
    the LDS kernel, else generic."""
    for n in [2 * r + 1, 2 * r + 2, 1000, 1001, 4099, (1 << 20) + 3]:
        x = make(dtype, n, seed=n + r)
        for off in (0, 1):
            got, want = run1d(dr, x, r, off)
            assert np.array_equal(bits(got), bits(want)), (np.dtype(dtype).name, r, n, off)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("r", [1, 2, 3, 4, 5, 9])
def test_stencil1d_random_floats_in_reference_order(dr, dtype, r):
    x = make(dtype, 4099, seed=r, exact=False)
    for off in (0, 1):
        got, want = run1d(dr, x, r, off)
        assert np.array_equal(bits(got), bits(want)), (np.dtype(dtype).name, r, off)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("r", [1, 2, 3, 4, 5])
def test_stencil1d_subrange_radius_alignment(dr, dtype, r):
    """Owned cells [lo, hi) only, bounds on and off the vector width V, one
    range spanning more than a block of 256 vectors on both sides."""
    v = 16 // np.dtype(dtype).itemsize
    n_owned = 2 * 257 * v + 5
    x = make(dtype, n_owned + 2 * r, seed=r)
    for lo, hi in [(0, 0), (0, 1), (1, 2), (3, 700), (v - 1, v + 1), (n_owned - 1, n_owned),
                   (257 * v - 1, 2 * 257 * v + 1)]:
        for off in (0, 1):
            got, want = run1d(dr, x, r, off, lo, hi)
            assert np.array_equal(bits(got), bits(want)), (np.dtype(dtype).name, r, lo, hi, off)


KNOBS = [{"DRHIP_ST1D_BLK": "0"}, {"DRHIP_ST_NT": "1"}, {"DRHIP_ST_NT": "2"}, {"DRHIP_ST_NT": "3"},
         {"DRHIP_ST1D_BLK": "0", "DRHIP_ST_NT": "1"}, {"DRHIP_ST1D_BLK": "0", "DRHIP_ST_NT": "2"},
         {"DRHIP_ST1D_BLK": "0", "DRHIP_ST_NT": "3"}]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [4099, (1 << 20) + 3])
def test_stencil1d_knob_kernels_match_default(dr, monkeypatch, dtype, n):
    """DRHIP_ST1D_BLK=0 (the wave-level stencil1d_vec, radius 1-4) and
    DRHIP_ST_NT=1..3 (the nontemporal forms of either kernel, radius 1) are
    read on every call and select kernels of the shipped library: identical
    results to the default, sub-range included."""
    for k in ("DRHIP_ST1D_BLK", "DRHIP_ST_NT"):
        monkeypatch.delenv(k, raising=False)
    x = make(dtype, n, seed=n, exact=False)
    cases = [(r, 0, n - 2 * r) for r in (1, 2, 3, 4)] + [(1, 5, n - 9), (2, 1, 1030)]
    base = []
    for r, lo, hi in cases:
        got, want = run1d(dr, x, r, 0, lo, hi)
        assert np.array_equal(bits(got), bits(want)), ("default", r, lo, hi)
        base.append(got)
    for env in KNOBS:
        for k, val in env.items():
            monkeypatch.setenv(k, val)
        for (r, lo, hi), ref in zip(cases, base):
            if "DRHIP_ST1D_BLK" not in env and r != 1:
                continue  # the cache policy alone changes radius 1 only
            got, _ = run1d(dr, x, r, 0, lo, hi)
            assert np.array_equal(bits(got), bits(ref)), (env, r, lo, hi)
        for k in env:
            monkeypatch.delenv(k)


def run2d(dr, x, nx, ny, off, rlo, rhi):
    dt = x.dtype
    hin = np.concatenate([np.full(G + off, 7, dt), x, np.full(G, 7, dt)])
    hout = np.full(G + off + nx * ny + G, sentinel(dt), dt)
    src = dr.DeviceArray(0, hin.size, dt, host=hin)
    dst = dr.DeviceArray(0, hout.size, dt, host=hout)
    dr.stencil2d(0, dt, src.at(G + off), dst.at(G + off), nx, ny - 2, rlo, rhi)
    got = dst.numpy()
    src.free()
    dst.free()
    grid = hout[G + off:G + off + nx * ny].reshape(ny, nx)  # a view: fills hout
    grid[1 + rlo:1 + rhi, 1:-1] = ref2d(x, nx, ny)[rlo:rhi]
    return got, hout


# (1024, 77) int32: 5 strips of 16 rows, 4 column blocks of 64 vectors in one workgroup (wave edges through
# LDS); (260, 70): 5 strips, 2 column blocks (wave edges from global memory); (513, 300) and every misaligned
# pointer: the scalar kernel; nx < 2 V: the scalar kernel
SHAPES_2D = [(3, 3), (4, 3), (5, 4), (7, 9), (8, 5), (12, 3), (256, 70), (260, 70), (513, 300), (1024, 77)]


@pytest.mark.parametrize("dtype", [np.float32, np.int32])
@pytest.mark.parametrize("nx,ny", SHAPES_2D)
def test_stencil2d_types_shapes_rows(dr, dtype, nx, ny):
    rows = ny - 2
    x = make(dtype, nx * ny, seed=nx + ny, exact=False)
    ranges = {(0, rows), (0, 1), (rows - 1, rows)}
    # starts and ends inside one strip of rows and one step of it
    if rows > 69:
        ranges.add((66, 69))
    elif rows > 6:
        ranges.add((3, 6))
    for rlo, rhi in sorted(ranges):
        for off in (0, 1):
            got, want = run2d(dr, x, nx, ny, off, rlo, rhi)
            assert np.array_equal(bits(got), bits(want)), (np.dtype(dtype).name, nx, ny, off, rlo, rhi)


_ROWVEC_CHILD = """
import sys
import numpy as np
sys.path[:0] = sys.argv[1:3]
import drhip as dr
from test_gpu_stencil_types import make, run2d, bits
dr.load(); dr.init([0])
for dtype in (np.float32, np.int32):
    for nx, ny, rlo, rhi in [(256, 70, 0, 68), (1024, 77, 3, 70), (8, 5, 1, 2)]:
        got, want = run2d(dr, make(dtype, nx * ny, 1, exact=False), nx, ny, 0, rlo, rhi)
        assert np.array_equal(bits(got), bits(want)), (dtype, nx, ny)
dr.finalize()
print("rowvec ok")
"""


def test_stencil2d_rowvec_knob_in_child_process():
    """DRHIP_ST2D_ROWVEC is read once per process: a fresh child runs the
    row-vector kernel (stencil2d_vec) it selects against the same reference."""
    here = os.path.dirname(os.path.abspath(__file__))
    pkg = os.path.join(os.path.dirname(here), "distributed-ranges_amd")
    env = dict(os.environ, DRHIP_ST2D_ROWVEC="1")
    p = subprocess.run([sys.executable, "-c", _ROWVEC_CHILD, pkg, here], env=env, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0 and "rowvec ok" in p.stdout, p.stdout + p.stderr
