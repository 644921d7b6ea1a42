"""Exact GPU parity of drhip_inclusive_scan (csrc/scan.hip, scan_kernel.hpp)
where test_gpu_scan.py cannot look: float64 in the parity and misaligned
sweeps, the float carry / total plumbing on inputs whose every prefix is exact
in any association order (the output IS the fp64 prefix -- a tile that drops
or repeats one element past index ~10^5 fails here and passes rtol 1e-5 on
U[0,1) sums), and scan_dispatch's switch to the 128 KiB tile.  Every output
range sits between guard cells that must keep their sentinel.

Inputs and their exactness bounds: test_reference_helpers.py."""
import numpy as np
import pytest

from test_gpu_scan import SIZES, make_input
from test_reference_helpers import SCAN_SIZES, big_tile_sizes, bounded_prefix_floats, exact_floats, exact_scan

pytestmark = pytest.mark.gpu

assert SIZES == SCAN_SIZES  # the sizes whose exact-float bounds test_reference_helpers.py asserts
OPS = ["plus", "mul", "min", "max"]
G = 16  # guard elements before and after every output range


def scan_guarded(dr, x, op, in_off=0, out_off=0, **kw):
    """Scans x (placed in_off elements past a 16-byte boundary) into a buffer
    of sentinels with G guard cells on each side; returns the scanned range
    after asserting that nothing outside it was written."""
    dt, n = x.dtype, x.size
    sent = dt.type(-77) if dt.kind != "u" else dt.type(0xA5A5A5A5)
    src = dr.DeviceArray(0, in_off + n, dt, host=np.concatenate([np.zeros(in_off, dt), x]))
    dst = dr.DeviceArray(0, G + out_off + n + G, dt, host=np.full(G + out_off + n + G, sent, dt))
    dr.scan_async(0, dt, op, src.at(in_off), dst.at(G + out_off), n, **kw)
    got = dst.numpy()
    src.free()
    dst.free()
    assert np.all(got[:G + out_off] == sent) and np.all(got[G + out_off + n:] == sent), "guard cells"
    return got[G + out_off:G + out_off + n]


def assert_exact(got, ref):
    assert np.array_equal(got.astype(np.float64), ref), np.nonzero(got != ref)[0][:10]


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("n", SIZES)
def test_scan_parity_float64(dr, op, n):
    """test_scan_parity's sweep for the dtype it leaves out; the reference is
    np.cumsum / cumprod / minimum.accumulate / maximum.accumulate in fp64."""
    x = exact_floats(np.float64, op, n, seed=n + len(op))
    assert_exact(scan_guarded(dr, x, op), exact_scan(x, op))


@pytest.mark.parametrize("n,in_off,out_off", [(1000, 1, 0), (9001, 0, 3), (50000, 2, 1), (4096, 1, 1)])
def test_scan_misaligned_float64(dr, n, in_off, out_off):
    """test_scan_misaligned's layouts (the scalar path) for float64."""
    x = exact_floats(np.float64, "plus", n, seed=n)
    assert_exact(scan_guarded(dr, x, "plus", in_off, out_off), exact_scan(x, "plus"))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("n", SIZES)
def test_scan_exact_floats(dr, dtype, op, n):
    x = exact_floats(dtype, op, n, seed=n + 2 * len(op))
    assert_exact(scan_guarded(dr, x, op), exact_scan(x, op))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [4097, 123457])
def test_scan_exact_floats_init_carry_total(dr, dtype, n):
    """init, host carry, carry_dev and total_dev, exactly: out[i] = carry +
    (init + x[0] + ... + x[i]), *total = out[n - 1]."""
    x = exact_floats(dtype, "plus", n, seed=n)
    pre = exact_scan(x, "plus")
    cdev = dr.DeviceArray(0, 1, np.float64, host=np.array([1000.0]))
    tot = dr.DeviceArray(0, 1, np.float64, host=np.array([-1.0]))
    try:
        assert_exact(scan_guarded(dr, x, "plus", init=dtype(3)), pre + 3)
        assert_exact(scan_guarded(dr, x, "plus", carry=np.float64(-7)), pre - 7)
        assert_exact(scan_guarded(dr, x, "plus", carry_dev=cdev.ptr), pre + 1000)
        got = scan_guarded(dr, x, "plus", init=dtype(3), carry=np.float64(-7), carry_dev=cdev.ptr, total_dev=tot.ptr)
        assert_exact(got, pre + 996)
        assert tot.numpy()[0] == pre[-1] + 996
    finally:
        cdev.free()
        tot.free()


BIG_TILE_OPS = [(np.int32, "plus"), (np.uint32, "plus"), (np.int64, "plus"), (np.float32, "plus"),
                (np.float64, "plus"), (np.int64, "max"), (np.uint32, "mul")]


def big_tile_case(dtype, op, n, seed):
    """Input and exact reference of one big-tile scan: integers bit-exact
    against the NumPy prefix in the dtype (wrapping; `mul` on odd values),
    floats on bounded_prefix_floats (every prefix and every tile sum exact)."""
    dt = np.dtype(dtype)
    if dt.kind == "f":
        x = bounded_prefix_floats(dt, n, seed)
        return x, np.cumsum(x.astype(np.float64)).astype(dt)
    x = make_input(dt, op, n, seed)
    if op == "plus":
        return x, np.cumsum(x, dtype=dt)
    if op == "mul":
        return x, np.cumprod(x, dtype=dt)
    return x, np.maximum.accumulate(x)


@pytest.mark.parametrize("dtype,op", BIG_TILE_OPS)
@pytest.mark.parametrize("which", [0, 1, 2])
def test_scan_big_tile_switch(dr, dtype, op, which):
    """scan_dispatch takes the 128 KiB tile (kScanUBig) from n * sizeof(T) >=
    kScanBigBytes = 2^27: one element below the switch (the 64 KiB tile's
    largest input), at it, and one big tile plus one element above it."""
    n = big_tile_sizes(np.dtype(dtype).itemsize)[which]
    x, ref = big_tile_case(dtype, op, n, seed=which)
    got = scan_guarded(dr, x, op)
    assert np.array_equal(got, ref), np.nonzero(got != ref)[0][:10]


@pytest.mark.parametrize("dtype", [np.float32, np.int64])
def test_scan_big_tile_misaligned(dr, dtype):
    """The big tile's scalar path: input and output off the 16-byte boundary."""
    n = big_tile_sizes(np.dtype(dtype).itemsize)[1]
    x, ref = big_tile_case(dtype, "plus", n, seed=5)
    got = scan_guarded(dr, x, "plus", in_off=1, out_off=1)
    assert np.array_equal(got, ref), np.nonzero(got != ref)[0][:10]
