"""GPU tests of the selection C-ABI (drhip_copy_if, drhip_count_if,
drhip_copy_flagged) on one segment.  The expected values are numpy's x[mask]
and mask.sum(), compared bit for bit (through .view(np.uint8)); `out` always
has room for n and is pre-filled with a sentinel, and every element at or
past the returned count must still be the sentinel.

Tile sizes of the kernel (include/dr/details/select_kernel.hpp): T = 16384
elements for a 16-byte-aligned input of 4-byte elements, T8 = 8192 for aligned
8-byte elements, TU = 4096 for any input that is not 16-byte aligned (the
element-load form).  Survivors are staged in LDS 32 KiB at a time, so an
aligned tile with more than half its elements selected takes two passes (the
"all" masks).  The sizes below are derived from all three."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T = 16384   # 64 KiB / 4 B: aligned 4-byte elements
T8 = 8192   # aligned 8-byte elements
TU = 4096   # unaligned input of 4- and 8-byte elements
BIG = 130 * T + 13  # more than two 64-tile look-back steps for every tile size
SIZES = sorted({0, 1, 2, 63, 64, 65, BIG} | {t + d for t in (T, T8, TU) for d in (-1, 0, 1)} |
               {2 * t + 1 for t in (T, T8, TU)})
MASKS = ["none", "all", "alternating", "random50", "random1", "first", "last", "empty_tile", "empty_tile8"]
EMPTY_TILE = {"empty_tile": T, "empty_tile8": T8, "empty_tileu": TU}
DTYPES = [np.int32, np.uint32, np.int64, np.uint64, np.float32, np.float64]
CMPS = ["lt", "le", "gt", "ge", "eq", "ne"]
NP_CMP = {"lt": np.less, "le": np.less_equal, "gt": np.greater, "ge": np.greater_equal, "eq": np.equal,
          "ne": np.not_equal}
SENT_BYTE = 0xA5
COUNT_SENTINEL = 0xDEADBEEF12345678


def make_mask(kind, n, seed=0):
    rng = np.random.default_rng(1000 + seed + n)
    m = np.zeros(n, bool)
    if kind == "all":
        m[:] = True
    elif kind == "alternating":
        m[::2] = True
    elif kind == "random50":
        m = rng.random(n) < 0.5
    elif kind == "random1":
        m = rng.random(n) < 0.01
    elif kind == "first":
        m[:1] = True
    elif kind == "last":
        m[-1:] = True
    elif kind in EMPTY_TILE:  # one whole tile (of T / T8 / TU elements) empty between two full ones
        t = EMPTY_TILE[kind]
        m[:] = True
        m[t:2 * t] = False
    return m


class Bufs:
    """in / out / count buffers of one call; out holds n elements of sentinel bytes."""

    def __init__(self, dr, x, offset=0, flags=None):
        self.dr, self.n, self.dtype = dr, x.size, x.dtype
        isz = x.dtype.itemsize
        self.src = dr.DeviceArray(0, x.size + offset + 1, x.dtype, host=np.concatenate(
            [np.zeros(offset, x.dtype), x, np.zeros(1, x.dtype)]))
        self.src_ptr = self.src.ptr + offset * isz
        self.dst = dr.DeviceArray(0, (x.size + 1) * isz, np.uint8, host=np.full((x.size + 1) * isz, SENT_BYTE, np.uint8))
        self.cnt = dr.DeviceArray(0, 1, np.uint64, host=np.array([COUNT_SENTINEL], np.uint64))
        self.flg = None
        if flags is not None:
            self.flg = dr.DeviceArray(0, x.size + 1, np.uint8, host=np.concatenate([flags, np.zeros(1, np.uint8)]))

    def result(self):
        """(out as the element type, n + 1 elements; count)"""
        self.dr.sync(0)
        return self.dst.numpy().view(self.dtype), int(self.cnt.numpy()[0])

    def free(self):
        for b in (self.src, self.dst, self.cnt, self.flg):
            if b is not None:
                b.free()


def check_selected(out, count, x, mask):
    want = x[mask]
    assert count == int(mask.sum())
    assert np.array_equal(out[:count].view(np.uint8), want.view(np.uint8))
    tail = out[count:].view(np.uint8)  # includes the one element past n
    assert tail.size and np.all(tail == SENT_BYTE), "an element at or past count was written"


def copy_if_case(dr, x, cmp, scalar, mask, offset=0):
    b = Bufs(dr, x, offset)
    try:
        dr.copy_if_async(0, x.dtype, cmp, b.src_ptr, b.dst.ptr, x.size, scalar, b.cnt.ptr)
        out, count = b.result()
        check_selected(out, count, x, mask)
        b.cnt.free()
        b.cnt = dr.DeviceArray(0, 1, np.uint64, host=np.array([COUNT_SENTINEL], np.uint64))
        dr.count_if_async(0, x.dtype, cmp, b.src_ptr, x.size, scalar, b.cnt.ptr)
        dr.sync(0)
        assert int(b.cnt.numpy()[0]) == int(mask.sum())
        assert dr.count_if(0, b.src_ptr, x.size, x.dtype, cmp, scalar) == int(mask.sum())
    finally:
        b.free()


def flagged_case(dr, x, mask, offset=0):
    b = Bufs(dr, x, offset, flags=mask.astype(np.uint8) * 3)  # any non-zero byte selects
    try:
        dr.copy_flagged_async(0, x.dtype.itemsize, b.src_ptr, b.flg.ptr, b.dst.ptr, x.size, b.cnt.ptr)
        out, count = b.result()
        check_selected(out, count, x, mask)
    finally:
        b.free()


def values_for(mask, dtype, seed=0):
    """x with x > 0 exactly where mask is set (signed / float dtypes) -- distinct values, so order shows."""
    n = mask.size
    rng = np.random.default_rng(7 + seed + n)
    mag = rng.integers(1, 1 << 30, n).astype(np.int64)
    return np.where(mask, mag, -mag).astype(dtype)


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("n", SIZES)
def test_masks_at_every_size(dr, n, kind):
    mask = make_mask(kind, n)
    copy_if_case(dr, values_for(mask, np.int32), "gt", 0, mask)
    rng = np.random.default_rng(n)
    flagged_case(dr, rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32), mask)
    flagged_case(dr, rng.integers(0, 1 << 63, n, dtype=np.uint64), mask)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [T + 1, T8 + 1, BIG])
def test_all_dtypes(dr, dtype, n):
    rng = np.random.default_rng(n)
    if np.issubdtype(dtype, np.floating):
        x = rng.normal(0, 100, n).astype(dtype)
        thr = 10.5
    else:
        x = rng.integers(0, 1000, n).astype(dtype)
        thr = 500
    copy_if_case(dr, x, "lt", thr, x < np.array(thr, dtype))
    copy_if_case(dr, x, "ge", thr, x >= np.array(thr, dtype))


@pytest.mark.parametrize("cmp", CMPS)
@pytest.mark.parametrize("dtype", [np.int32, np.float32])
def test_all_comparisons(dr, dtype, cmp):
    n = 2 * T + 1
    x = np.random.default_rng(5).integers(-3, 4, n).astype(dtype)  # many ties with the scalar
    copy_if_case(dr, x, cmp, 1, NP_CMP[cmp](x, np.array(1, dtype)))


@pytest.mark.parametrize("cmp", CMPS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_float_specials(dr, dtype, cmp):
    """IEEE comparisons: NaN passes only NE, -0.0 == +0.0."""
    pat = np.array([np.nan, -0.0, 0.0, 1.0, -1.0, np.inf, -np.inf, -np.nan, 5e-324, -1e-45], dtype)
    x = np.resize(pat, T + 1)
    with np.errstate(invalid="ignore"):
        mask = NP_CMP[cmp](x, np.array(0.0, dtype))
    nan = np.isnan(x)
    assert np.all(mask[nan] == (cmp == "ne"))
    copy_if_case(dr, x, cmp, 0.0, mask)


@pytest.mark.parametrize("dtype", [np.uint32, np.float64])
@pytest.mark.parametrize("n", [65, TU - 1, TU, TU + 1, 2 * TU + 1, 2 * T + 1, BIG])
def test_unaligned_input(dr, dtype, n):
    """`in` one element past a 16-byte boundary: the element-load form."""
    rng = np.random.default_rng(n + 1)
    x = rng.integers(0, 1000, n).astype(dtype)
    copy_if_case(dr, x, "lt", 500, x < 500, offset=1)
    for kind in ("random50", "all", "empty_tileu"):
        flagged_case(dr, x, make_mask(kind, n, seed=3), offset=1)


def test_empty_input_writes_zero(dr):
    """n == 0: *count receives 0 in stream order, nothing else is touched (null in / out allowed)."""
    cnt = dr.DeviceArray(0, 1, np.uint64, host=np.array([COUNT_SENTINEL], np.uint64))
    try:
        for call in (lambda: dr.copy_if_async(0, np.int32, "lt", None, None, 0, 0, cnt.ptr),
                     lambda: dr.count_if_async(0, np.int32, "lt", None, 0, 0, cnt.ptr),
                     lambda: dr.copy_flagged_async(0, 4, None, None, None, 0, cnt.ptr)):
            dr.h2d(0, cnt.ptr, np.array([COUNT_SENTINEL], np.uint64))
            call()
            dr.sync(0)
            assert int(cnt.numpy()[0]) == 0
    finally:
        cnt.free()


def test_graph_replay(dr):
    n = 5 * T + 77
    rng = np.random.default_rng(11)
    x1 = rng.integers(-1000, 1000, n).astype(np.int32)
    x2 = rng.integers(-1000, 1000, n).astype(np.int32)
    x2[: 2 * T] = -5  # a different count, and two empty tiles
    b = Bufs(dr, x1)
    g = None
    try:
        dr.copy_if_async(0, np.int32, "gt", b.src_ptr, b.dst.ptr, n, 0, b.cnt.ptr)  # warm: the workspace grows here
        dr.sync(0)
        dr.graph_begin(0)
        dr.copy_if_async(0, np.int32, "gt", b.src_ptr, b.dst.ptr, n, 0, b.cnt.ptr)
        g = dr.graph_end(0)
        for x in (x1, x2, x1):
            dr.h2d(0, b.src_ptr, x)
            dr.h2d(0, b.dst.ptr, np.full((n + 1) * 4, SENT_BYTE, np.uint8))
            dr.h2d(0, b.cnt.ptr, np.array([COUNT_SENTINEL], np.uint64))
            dr.graph_launch(0, g)
            out, count = b.result()
            check_selected(out, count, x, x > 0)
    finally:
        if g:
            dr.graph_destroy(g)
        b.free()


def test_status_storage_reused(dr):
    """Two calls back to back on the segment, different n, no sync between them."""
    rng = np.random.default_rng(12)
    xa = rng.integers(0, 100, BIG).astype(np.uint32)
    xb = rng.integers(0, 100, 3 * T + 5).astype(np.uint32)
    a, b, c = Bufs(dr, xa), Bufs(dr, xb), Bufs(dr, xa)
    try:
        dr.copy_if_async(0, np.uint32, "lt", a.src_ptr, a.dst.ptr, xa.size, 50, a.cnt.ptr)
        dr.copy_if_async(0, np.uint32, "ge", b.src_ptr, b.dst.ptr, xb.size, 50, b.cnt.ptr)
        dr.copy_if_async(0, np.uint32, "eq", c.src_ptr, c.dst.ptr, xa.size, 7, c.cnt.ptr)
        check_selected(*a.result(), xa, xa < 50)
        check_selected(*b.result(), xb, xb >= 50)
        check_selected(*c.result(), xa, xa == 7)
    finally:
        for t in (a, b, c):
            t.free()


def test_blocking_conveniences(dr):
    n = T + 100
    x = np.arange(n, dtype=np.int64)
    src = dr.DeviceArray(0, n, np.int64, host=x)
    dst = dr.DeviceArray(0, n, np.int64, host=np.full(n, -1, np.int64))
    flg = dr.DeviceArray(0, n, np.uint8, host=(x % 3 == 0).astype(np.uint8))
    try:
        assert dr.count_if(0, src.ptr, n, np.int64, dr.GE, 100) == n - 100
        c = dr.copy_if(0, src.ptr, dst.ptr, n, np.int64, "<", 10)
        assert c == 10 and np.array_equal(dst.numpy()[:11], np.array(list(range(10)) + [-1]))
        c = dr.copy_flagged(0, src.ptr, flg.ptr, dst.ptr, n, 8)
        assert c == int((x % 3 == 0).sum()) and np.array_equal(dst.numpy()[:c], x[x % 3 == 0])
    finally:
        for b in (src, dst, flg):
            b.free()
