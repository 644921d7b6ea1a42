"""GPU tests of the sorted-search C-ABI (drhip_lower_bound, drhip_upper_bound,
drhip_binary_search) on one segment, through drhip.py, against
numpy.searchsorted(side='left' / 'right') and left < right on the host copy.
Every position and flag must be exact.

Shapes of the kernel (include/dr/details/bsearch_kernel.hpp): a workgroup
stages S = drhip.SORTED_SEARCH_STAGE[itemsize] evenly spaced haystack elements
in LDS when the call has at least S needles, and searches global memory
directly below that; with a haystack of fewer than S elements the whole of it
is staged.  A tile is 256 threads x 4 consecutive needles; 16-byte needle
loads and output stores need 16-byte aligned pointers, anything else takes the
element path, as does the ragged last group of 4."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DTYPES = [np.int32, np.uint32, np.int64, np.uint64, np.float32, np.float64]
M_LIST = [0, 1, 3, 255, 256, 257, 4099, (1 << 17) + 5]


def stage(dr, dtype):
    return dr.SORTED_SEARCH_STAGE[np.dtype(dtype).itemsize]


def n_list(dr, dtype):
    s = stage(dr, dtype)
    return [0, 1, 2, 3, s - 1, s, s + 1, 2 * s + 1, 100003, (1 << 20) + 7]


def haystack(n, dtype, seed):
    """n sorted integer-valued elements with duplicates and gaps (even values only, so +-1 is absent); floats
    also hold -inf, -0.0, +0.0 and +inf, signed types negative values."""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    span = max(4, n // 2)
    lo = 10 if dt.kind == "u" else -span
    x = (lo + 2 * rng.integers(0, span, n)).astype(dt)
    if dt.kind == "f" and n >= 4:
        x[:4] = [-np.inf, -0.0, 0.0, np.inf]
    elif dt.kind == "f" and n >= 2:
        x[:2] = [-0.0, 0.0]
    return np.sort(x)


def needle_pool(h, dtype, seed):
    """Below the minimum and above the maximum, every haystack element, every element +-1, random values
    (and both zeros and both infinities for floats), shuffled."""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    finite = h[np.isfinite(h)] if dt.kind == "f" else h
    lo = finite.min() if finite.size else dt.type(10)
    hi = finite.max() if finite.size else dt.type(10)
    parts = [np.array([lo - 3, lo - 1, hi + 1, hi + 3], dt), h, finite - dt.type(1), finite + dt.type(1),
             (int(lo) - 5 + rng.integers(0, int(hi) - int(lo) + 11, 1000)).astype(dt)]
    if dt.kind == "f":
        parts.append(np.array([-np.inf, np.inf, -0.0, 0.0], dt))
    pool = np.concatenate(parts)
    rng.shuffle(pool)
    return pool


class Hay:
    """A haystack on the device, `offset` elements into its buffer (offset = 1: not 16-byte aligned)."""

    def __init__(self, dr, h, offset=0):
        self.dr, self.h, self.n, self.dtype = dr, h, h.size, h.dtype
        whole = np.concatenate([np.zeros(offset, h.dtype), h])
        self.buf = dr.DeviceArray(0, whole.size, h.dtype, host=whole if whole.size else None)
        self.ptr = self.buf.ptr + offset * h.dtype.itemsize

    def free(self):
        self.buf.free()

    def check(self, needles, offset=0, pad=3):
        """All three searches of `needles` (uploaded `offset` elements into their buffer; the outputs `offset`
        elements into theirs, with `pad` sentinel elements behind) against numpy."""
        dr, m, dt = self.dr, needles.size, self.dtype
        whole = np.concatenate([np.zeros(offset, dt), needles])
        nd = dr.DeviceArray(0, whole.size, dt, host=whole if whole.size else None)
        pos = dr.DeviceArray(0, offset + m + pad, np.uint64, host=np.full(offset + m + pad, 0xDEADBEEF12345678, np.uint64))
        fl = dr.DeviceArray(0, offset + m + pad, np.uint8, host=np.full(offset + m + pad, 0xEE, np.uint8))
        try:
            np_ptr = nd.ptr + offset * dt.itemsize
            left = np.searchsorted(self.h, needles, side="left").astype(np.uint64)
            right = np.searchsorted(self.h, needles, side="right").astype(np.uint64)
            for fn, want in ((dr.lower_bound_async, left), (dr.upper_bound_async, right)):
                fn(0, dt, self.ptr, self.n, np_ptr, m, pos.ptr + 8 * offset)
                got = pos.numpy()
                assert np.array_equal(got[offset:offset + m], want), fn.__name__
                assert (got[:offset] == 0xDEADBEEF12345678).all() and (got[offset + m:] == 0xDEADBEEF12345678).all()
            dr.binary_search_async(0, dt, self.ptr, self.n, np_ptr, m, fl.ptr + offset)
            got = fl.numpy()
            assert np.array_equal(got[offset:offset + m], (left < right).astype(np.uint8))
            assert (got[:offset] == 0xEE).all() and (got[offset + m:] == 0xEE).all()
        finally:
            nd.free()
            pos.free()
            fl.free()


@pytest.mark.parametrize("ni", range(10))
@pytest.mark.parametrize("dtype", DTYPES)
def test_sizes(dr, dtype, ni):
    """Every haystack size around the staging threshold and the sample stride (n_list), with every needle count
    around a tile, a ragged group of 4 and the staging threshold; and the whole pool of needles at once."""
    n = n_list(dr, dtype)[ni]
    h = haystack(n, dtype, 100 + n)
    pool = needle_pool(h, dtype, 200 + n)
    d = Hay(dr, h)
    try:
        for m in M_LIST:
            d.check(np.resize(pool, m) if m else pool[:0])
        d.check(pool)
    finally:
        d.free()


@pytest.mark.parametrize("dtype", [np.uint32, np.float64])
def test_haystacks_of_duplicates(dr, dtype):
    s = stage(dr, dtype)
    for n in (s + 1, 100003):
        for values in ([7], [4, 6, 8]):
            h = np.sort(np.resize(np.array(values, dtype), n))
            d = Hay(dr, h)
            try:
                needles = np.array([3, 4, 5, 6, 7, 8, 9], dtype)
                d.check(needles)
                d.check(np.resize(needles, 2 * s + 3))
            finally:
                d.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_unaligned_pointers(dr, dtype):
    """Haystack, needles and outputs one element into their buffers: element loads and element stores."""
    s = stage(dr, dtype)
    h = haystack(3 * s + 5, dtype, 31)
    pool = needle_pool(h, dtype, 32)
    for hay_off, io_off in ((1, 0), (0, 1), (1, 1)):
        d = Hay(dr, h, hay_off)
        try:
            for m in (3, 257, s + 7):
                d.check(np.resize(pool, m), io_off)
        finally:
            d.free()


def test_graph_replay_without_warm_up(dr):
    """A call captured with no eager call before it, replayed after the needles were overwritten, returns the
    new needles' positions: the kernel keeps no state outside its arguments."""
    dtype = np.dtype(np.int64)
    s = stage(dr, dtype)
    n, m = 100003, 2 * s + 9
    h = haystack(n, dtype, 41)
    pool = needle_pool(h, dtype, 42)
    d = Hay(dr, h)
    nd = dr.DeviceArray(0, m, dtype)
    few = dr.DeviceArray(0, 5, dtype)
    pos = dr.DeviceArray(0, m, np.uint64)
    fl = dr.DeviceArray(0, 5, np.uint8)
    g = None
    try:
        dr.sync(0)
        dr.graph_begin(0)
        dr.upper_bound_async(0, dtype, d.ptr, n, nd.ptr, m, pos.ptr)   # staged
        dr.binary_search_async(0, dtype, d.ptr, n, few.ptr, 5, fl.ptr)  # direct
        g = dr.graph_end(0)
        for round_ in range(3):
            needles = np.resize(np.roll(pool, 1000 * round_ + 1), m)
            dr.h2d(0, nd.ptr, needles)
            dr.h2d(0, few.ptr, needles[:5])
            dr.h2d(0, pos.ptr, np.full(m, 0xDEAD, np.uint64))
            dr.graph_launch(0, g)
            dr.sync(0)
            assert np.array_equal(pos.numpy(), np.searchsorted(h, needles, side="right").astype(np.uint64))
            want = np.searchsorted(h, needles[:5], side="left") < np.searchsorted(h, needles[:5], side="right")
            assert np.array_equal(fl.numpy(), want.astype(np.uint8))
    finally:
        if g:
            dr.graph_destroy(g)
        for b in (nd, few, pos, fl):
            b.free()
        d.free()


def test_blocking_helpers_and_empty_inputs(dr):
    h = np.array([1, 3, 3, 3, 8, 9], np.int32)
    v = np.array([0, 3, 4, 9, 10], np.int32)
    d = Hay(dr, h)
    nd = dr.DeviceArray(0, v.size, np.int32, host=v)
    try:
        lo = dr.lower_bound(0, d.ptr, h.size, nd.ptr, v.size, np.int32)
        up = dr.upper_bound(0, d.ptr, h.size, nd.ptr, v.size, np.int32)
        fd = dr.binary_search(0, d.ptr, h.size, nd.ptr, v.size, np.int32)
        assert lo.dtype == np.uint64 and lo.tolist() == [0, 1, 4, 5, 6]
        assert up.dtype == np.uint64 and up.tolist() == [0, 4, 4, 6, 6]
        assert fd.dtype == np.uint8 and fd.tolist() == [0, 1, 0, 1, 0]
        # an empty haystack: m zeros; no needles: an empty array
        assert dr.lower_bound(0, d.ptr, 0, nd.ptr, v.size, np.int32).tolist() == [0] * v.size
        assert dr.upper_bound(0, 0, 0, nd.ptr, v.size, np.int32).tolist() == [0] * v.size
        assert dr.binary_search(0, 0, 0, nd.ptr, v.size, np.int32).tolist() == [0] * v.size
        assert dr.lower_bound(0, d.ptr, h.size, nd.ptr, 0, np.int32).size == 0
        # a refusal on real buffers leaves the output untouched
        with pytest.raises(dr.DrhipError, match="drhip_lower_bound"):
            dr.lower_bound_async(0, np.int32, d.ptr, h.size, nd.ptr, v.size, nd.ptr)
        assert np.array_equal(nd.numpy(), v)
    finally:
        nd.free()
        d.free()
