"""The NumPy references and exact-float input generators the bit-exact GPU
tests share, with the CPU checks that they may be trusted:

* ref1d / ref2d (the stencil references of tests/test_gpu_stencil_types.py,
  which also cover the 8-byte types the oracle does not have) equal
  oracle.stencil1d / oracle.stencil2d where the oracle has the type;
* exact_floats / bounded_prefix_floats produce integer-valued floats whose sum
  of absolute values stays below 2^24 (f32) or 2^53 (f64) at every size the
  GPU tests use, so every partial sum in any association order is exactly
  representable and a float kernel must return the integer sum exactly;
* an f32 product formed in fp64 and rounded once is the float32 product (the
  reference of the elementwise `mul` sweep).

No test here needs a GPU."""
import math

import numpy as np
import pytest

# the sizes of the reduce / scan / dot sweeps that use exact floats
REDUCE_CASES = [(0, 0), (1, 0), (7, 1), (1000, 3), (4097, 0), (70001, 1), ((1 << 20) + 3, 2)]
# reduce.hip: the grid is min(chunks, kReduceBlocksPerCU x CUs = 2 x 256 = 512, kReduceMaxBlocks = 4096) with
# chunks = ceil(nv / (256 threads x kReduceU = 8)) vectors, so the cap binds from nv > 512 x 2048 = 2^20 vectors:
# 2^22 4-byte / 2^21 8-byte elements.  At 2^23 + 5 (either offset) nv = 2^21 + 1 (4-byte) or 2^22 + 2 (8-byte),
# per = ceil(nv / 512) = 4097 / 8193: not a multiple of the unrolled step (2048), and 512 blocks = 16 full groups
# of kReduceGroup = 32.  A retune of any of those constants moves this size.
CAPPED_N = (1 << 23) + 5
SCAN_SIZES = [1, 5, 4095, 4096, 4097, 2048 * 3 + 1, 100000, (1 << 21) + 5]
DOT_SIZES = [0, 5, 7, 4099, 300001, 1 << 20, (1 << 22) + 3, (1 << 22) + (1 << 12) + 3]
LIMIT = {np.dtype(np.float32): 2.0 ** 24, np.dtype(np.float64): 2.0 ** 53}


def exact_floats(dtype, op, n, seed):
    """Integer-valued floats whose fold by `op` is exact in any order.
    plus: nonzero integers in [-4, 4] ([-1, 1] for f32 from 2^22 elements up;
    no zeros, so that dropping any one element changes the sum);
    mul: +-1 with min(100, n // 2) entries of 2 and as many of 0.5 at random
    positions (every sub-product within 2^+-100); min / max: integers in
    [-10^6, 10^6]."""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    if op == "plus":
        a = 1 if dt == np.float32 and n >= 1 << 22 else 4
        return (rng.integers(1, a, n, endpoint=True) * (rng.integers(0, 2, n) * 2 - 1)).astype(dt)
    if op == "mul":
        x = (rng.integers(0, 2, n) * 2 - 1).astype(dt)
        k = min(100, n // 2)
        pos = rng.permutation(n)[:2 * k]
        x[pos[:k]] *= 2
        x[pos[k:]] *= 0.5
        return x
    return rng.integers(-10 ** 6, 10 ** 6, n, endpoint=True).astype(dt)


def exact_fold(x, op):
    """The exact fold of exact_floats(.., op, ..) in fp64 (None when empty)."""
    if x.size == 0:
        return None
    x = x.astype(np.float64)
    return {"plus": lambda: float(np.sum(x.astype(np.int64))), "mul": lambda: float(np.prod(x)),
            "min": lambda: float(x.min()), "max": lambda: float(x.max())}[op]()


def exact_scan(x, op):
    """The inclusive scan of exact inputs, in fp64 (every value exact)."""
    x = x.astype(np.float64)
    return {"plus": np.cumsum, "mul": np.cumprod, "min": np.minimum.accumulate, "max": np.maximum.accumulate}[op](x)


def exact_dot_inputs(dtype, n, seed):
    """Two vectors of nonzero integers in [-2, 2] (every product counts):
    sum |x y| <= 4 n < 2^53, and the kernel's per-iteration fp32 partial (4
    vectors of products) stays below 2^24, so the fp64-accumulated dot is the
    integer dot exactly."""
    rng = np.random.default_rng(seed)
    draw = lambda: (rng.integers(1, 2, n, endpoint=True) * (rng.integers(0, 2, n) * 2 - 1)).astype(dtype)
    return draw(), draw()


def bounded_prefix_floats(dtype, n, seed):
    """+-1 for scans too long for sum |x| < 2^24: the sign alternates between
    blocks of random lengths 1..64, so a prefix is a random walk of block
    length differences (tens of thousands at 2^25 elements, far below 2^24;
    test_bounded_prefix_floats_bounds asserts it for every input used) and any
    sub-sum inside a scan tile (<= 2^15 elements) is at most the tile size.
    No zeros: every element moves every later prefix."""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(1, 65, n // 16 + 1)  # mean 32.5: far more than n elements in all
    signs = np.where(np.arange(lengths.size) % 2 == 0, 1, -1).astype(np.int8)
    x = np.repeat(signs, lengths)[:n]
    assert x.size == n
    return x.astype(dtype)


# (size index into big_tile_sizes, seed) of every bounded_prefix_floats input the GPU tests draw
BIG_TILE_INPUTS = [(0, 0), (1, 1), (2, 2), (1, 5)]


def _unsigned(x):
    return x.view(np.dtype("u%d" % x.dtype.itemsize)) if x.dtype.kind == "i" else x


def ref1d(x, r):
    """Outputs r .. n - r - 1 of the radius-r window sum, left to right from
    the first term in the element dtype (integers wrap)."""
    m = x.size - 2 * r
    u = _unsigned(x)
    s = u[0:m].copy()
    for d in range(1, 2 * r + 1):
        s = s + u[d:d + m]
    return s.view(x.dtype)


def ref2d(x, nx, ny):
    """The interior (ny - 2, nx - 2) of the 5-point sum c + w + e + n + s, in
    that order, in the element dtype (integers wrap)."""
    g = _unsigned(x).reshape(ny, nx)
    s = g[1:-1, 1:-1] + g[1:-1, :-2]
    s = s + g[1:-1, 2:]
    s = s + g[:-2, 1:-1]
    s = s + g[2:, 1:-1]
    return s.view(x.dtype)


# ------------------------------------------------------------------ checks


@pytest.mark.parametrize("dtype", [np.float32, np.int32])
@pytest.mark.parametrize("r", [1, 2, 3, 4, 5, 9])
@pytest.mark.parametrize("n", [19, 20, 1001, 4099])
def test_ref1d_equals_oracle(oracle, dtype, r, n):
    rng = np.random.default_rng(n + r)
    x = (rng.random(n) * 100).astype(dtype) if dtype == np.float32 else rng.integers(
        np.iinfo(np.int32).min, np.iinfo(np.int32).max, n, endpoint=True).astype(dtype)
    out = oracle.stencil1d(x, r, out=np.zeros(n, dtype))
    assert np.array_equal(out[r:n - r].view(np.uint32), ref1d(x, r).view(np.uint32))


@pytest.mark.parametrize("nx,ny", [(3, 3), (7, 9), (8, 5), (260, 70)])
def test_ref2d_equals_oracle(oracle, nx, ny):
    """The oracle's 2-D stencil is f32 only: random f32 bit for bit, and the
    int32 reference on small integers against the oracle on their f32 copies
    (exact in both)."""
    x = np.random.default_rng(nx).random(nx * ny, dtype=np.float32)
    full = oracle.stencil2d(x, nx, ny, out=x.copy()).reshape(ny, nx)
    assert np.array_equal(full[1:-1, 1:-1].view(np.uint32), ref2d(x, nx, ny).view(np.uint32))
    xi = np.random.default_rng(ny).integers(-1000, 1000, nx * ny).astype(np.int32)
    fi = oracle.stencil2d(xi.astype(np.float32), nx, ny, out=np.zeros(nx * ny, np.float32)).reshape(ny, nx)
    assert np.array_equal(fi[1:-1, 1:-1], ref2d(xi, nx, ny).astype(np.float32))


def test_ref_stencils_wrap():
    x = np.full(5, np.iinfo(np.int64).max, np.int64)
    assert ref1d(x, 1).tolist() == [np.iinfo(np.int64).max - 2] * 3
    g = np.full(9, np.iinfo(np.int32).min, np.int32)
    assert ref2d(g, 3, 3).tolist() == [[np.iinfo(np.int32).min]]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_exact_floats_bounds(dtype):
    """sum |x| below 2^24 / 2^53 and fsum == the integer sum at every size
    used; every prefix product of the `mul` inputs within 2^+-100."""
    dt = np.dtype(dtype)
    ns = sorted({n + off for n, off in REDUCE_CASES} | {CAPPED_N + 3} | set(SCAN_SIZES) | {1001, 9001, 50002, 123457})
    for n in ns:
        x = exact_floats(dt, "plus", n, seed=n)
        assert x.dtype == dt and np.array_equal(x, np.rint(x))
        assert float(np.sum(np.abs(x.astype(np.float64)))) < LIMIT[dt], n
        assert math.fsum(x.tolist()) == int(np.sum(x.astype(np.int64)))
        assert (exact_fold(x, "plus") or 0.0) == int(np.sum(x.astype(np.int64)))
        m = exact_floats(dt, "mul", n, seed=n)
        k = min(100, n // 2)
        assert np.count_nonzero(np.abs(m) == 2) == k and np.count_nonzero(np.abs(m) == 0.5) == k
        assert np.count_nonzero(np.abs(m) == 1) == n - 2 * k
        if n:
            assert np.max(np.abs(np.cumsum(np.log2(np.abs(m.astype(np.float64)))))) <= 100
            assert abs(exact_fold(m, "mul")) == 1.0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_exact_dot_bounds(dtype):
    for n in DOT_SIZES:
        x, y = exact_dot_inputs(dtype, n + 3, seed=n)
        assert np.max(np.abs(x), initial=0) <= 2 and np.max(np.abs(y), initial=0) <= 2
        assert float(np.sum(np.abs(x.astype(np.float64) * y))) <= 4 * (n + 3) < 2.0 ** 53
        assert 16 * 4 < 2.0 ** 24  # one unrolled iteration's fp32 partial: 4 vectors x 4 products of <= 4


def big_tile_sizes(itemsize):
    """Around scan_dispatch's switch to the 128 KiB tile (kScanUBig) at
    n * sizeof(T) >= kScanBigBytes = 2^27: one element below, at it, and one
    big tile (256 threads x 32 vectors) plus one element above."""
    n0, v = (1 << 27) // itemsize, 16 // itemsize
    return [n0 - 1, n0, n0 + 256 * 32 * v + 1]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bounded_prefix_floats_bounds(dtype):
    """f32 at 2^25 elements has sum |x| = 2^25: the alternating blocks keep
    every prefix, and every window of one big tile, below 2^24 (f64: 2^53),
    for each input test_gpu_scan.py's big-tile tests use."""
    dt = np.dtype(dtype)
    tile = 256 * 32 * (16 // dt.itemsize)
    assert tile < LIMIT[dt]  # sum |x| of any subset of one tile
    for which, seed in BIG_TILE_INPUTS:
        n = big_tile_sizes(dt.itemsize)[which]
        x = bounded_prefix_floats(dt, n, seed)
        assert x.dtype == dt and x.size == n and np.all(np.abs(x) == 1)
        pre = np.cumsum(x.astype(np.int64))
        assert np.max(np.abs(pre)) < LIMIT[dt], (n, seed)
        assert np.array_equal(np.cumsum(x.astype(np.float64)), pre.astype(np.float64))


def test_f32_product_in_double_rounds_once():
    """The kernels form f32 products in fp64 and round once (compute_of<MUL,
    float>): the exact product of two f32 values fits a double, so this is
    the float32 product, the reference of the elementwise `mul` sweep."""
    from test_gpu_elementwise_ops import base_input, bits
    x, y = base_input(np.float32, 1), base_input(np.float32, 2)
    with np.errstate(all="ignore"):
        a = (x.astype(np.float64) * y.astype(np.float64)).astype(np.float32)
        b = x * y
    nan = np.isnan(b)
    assert np.array_equal(np.isnan(a), nan) and np.array_equal(bits(a)[~nan], bits(b)[~nan])
