"""GPU tests of the search C-ABI (drhip_find_if, drhip_is_sorted_until,
drhip_mismatch, drhip_min_element, drhip_max_element, drhip_minmax_element) on
one segment, against numpy on the host copy: np.flatnonzero(...)[0] for a
first match, np.argmin / np.argmax for the first extremum and
n - 1 - np.argmax(x[::-1]) for the last maximum.  Every index must be exact.

Tile sizes of the kernel (include/dr/details/search_kernel.hpp): a 16-byte
aligned input is read in tiles of T = 64 KiB / itemsize elements (16384 4-byte,
8192 8-byte; drhip_mismatch splits the 64 KiB between its two inputs), an input
that is not 16-byte aligned in tiles of 4096.  The grid is 2 workgroups per CU,
512 on a 256-CU device, and workgroup b takes the tiles b, b + 512, ...; BIG is
above 512 tiles, so workgroups take more than one tile each.  Inside a tile
every wave owns a contiguous quarter and a lane 16 bytes (or one element) per
slot; the last, partial tile of an input is read element by element.  An array is
uploaded once per size and a case changes single elements of it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GRID = 512
DTYPES = [np.int32, np.uint32, np.int64, np.uint64, np.float32, np.float64]
LARGE_DTYPES = [np.uint32, np.float32, np.int64, np.float64]
SMALL = [0, 1, 2, 63, 64, 65, 255, 256, 257]
CMPS = ["lt", "le", "gt", "ge", "eq", "ne"]
NP_CMP = {"lt": np.less, "le": np.less_equal, "gt": np.greater, "ge": np.greater_equal, "eq": np.equal,
          "ne": np.not_equal}
SENTINEL = 0xDEADBEEF12345678


def tile(dtype):
    return 65536 // np.dtype(dtype).itemsize


def large(dtype):
    t = tile(dtype)
    return [t - 1, t, t + 1, 3 * t + 5, (1 << 20) + 37]


def big(dtype):
    return (GRID + 60) * tile(dtype) + 13


def positions(n, dtype):
    t = tile(dtype)
    return sorted({p for p in (0, 1, n - 1, t - 1, t, t + 1, n // 2) if 0 <= p < n})


class Dev:
    """x on the device (offset elements into its buffer, so offset = 1 is not 16-byte aligned) and an index pair."""

    def __init__(self, dr, x, offset=0):
        self.dr, self.n, self.dtype, self.isz = dr, x.size, x.dtype, x.dtype.itemsize
        self.buf = dr.DeviceArray(0, x.size + offset + 1, x.dtype,
                                  host=np.concatenate([np.zeros(offset, x.dtype), x, np.zeros(1, x.dtype)]))
        self.ptr = self.buf.ptr + offset * self.isz
        self.idx = dr.DeviceArray(0, 2, np.uint64)

    def poke(self, p, value):
        self.dr.h2d(0, self.ptr + p * self.isz, np.array([value], self.dtype))

    def call(self, fn, *args):
        """fn(seg, ..., index) with a sentinel in both index words; returns them."""
        self.dr.h2d(0, self.idx.ptr, np.array([SENTINEL, SENTINEL], np.uint64))
        fn(*args, self.idx.ptr)
        r = self.idx.numpy()
        return int(r[0]), int(r[1])

    def find(self, cmp, scalar):
        r = self.call(self.dr.find_if_async, 0, self.dtype, cmp, self.ptr, self.n, scalar)
        assert r[1] == SENTINEL
        return r[0]

    def sorted_until(self):
        r = self.call(self.dr.is_sorted_until_async, 0, self.dtype, self.ptr, self.n)
        assert r[1] == SENTINEL
        return r[0]

    def mismatch(self, other):
        r = self.call(self.dr.mismatch_async, 0, self.dtype, self.ptr, other.ptr, self.n)
        assert r[1] == SENTINEL
        return r[0]

    def extrema(self):
        """(min_element, max_element, minmax_element)"""
        lo = self.call(self.dr.min_element_async, 0, self.dtype, self.ptr, self.n)
        hi = self.call(self.dr.max_element_async, 0, self.dtype, self.ptr, self.n)
        assert lo[1] == SENTINEL and hi[1] == SENTINEL
        return lo[0], hi[0], self.call(self.dr.minmax_element_async, 0, self.dtype, self.ptr, self.n)

    def free(self):
        self.buf.free()
        self.idx.free()


def first_true(mask):
    hits = np.flatnonzero(mask)
    return int(hits[0]) if hits.size else mask.size


def ref_extrema(x):
    """(first least, first greatest, (first least, last greatest)); 0 for an empty array."""
    if not x.size:
        return 0, 0, (0, 0)
    lo, hi = int(np.argmin(x)), int(np.argmax(x))
    return lo, hi, (lo, x.size - 1 - int(np.argmax(x[::-1])))


def iota(n, dtype):
    return (np.arange(n, dtype=np.int64) + 10).astype(dtype)  # exact in f32 up to 2^24


# ------------------------------------------------------------ first match

def check_find(dr, dtype, n, offset=0):
    x = iota(n, dtype)
    d = Dev(dr, x, offset)
    try:
        assert d.find("eq", 5) == n  # no hit
        for p in positions(n, dtype):
            # the only hit; then every element from p on is a hit: the first wins over later ones found sooner
            assert d.find("eq", x[p]) == p
            assert d.find("ge", x[p]) == p
        if n:
            s = x[n // 2]
            for c in CMPS:
                assert d.find(c, s) == first_true(NP_CMP[c](x, s)), c
            # a hit that is not an element of the progression
            p = n // 2
            d.poke(p, 5)
            assert d.find("lt", 10) == p
            assert d.find("eq", 5) == p
            assert d.find("ne", x[0]) == (p if p == 0 else 1 if n > 1 else n)
    finally:
        d.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_find_if_small(dr, dtype):
    for n in SMALL:
        check_find(dr, dtype, n)
    check_find(dr, dtype, 257, offset=1)


@pytest.mark.parametrize("dtype", LARGE_DTYPES)
def test_find_if_large(dr, dtype):
    for n in large(dtype):
        check_find(dr, dtype, n)
    check_find(dr, dtype, 3 * tile(dtype) + 5, offset=1)  # the accessor form


@pytest.mark.parametrize("dtype", LARGE_DTYPES)
def test_find_if_many_tiles_per_workgroup(dr, dtype):
    check_find(dr, dtype, big(dtype))


def test_find_if_descending_all_cmps(dr):
    n = 3 * tile(np.int32) + 5
    x = (np.arange(n, dtype=np.int64)[::-1] - n // 3).astype(np.int32)  # crosses 0
    d = Dev(dr, x)
    try:
        for s in (x[0], x[n // 2], x[-1], 0, x[0] + 1, x[-1] - 1):
            for c in CMPS:
                assert d.find(c, s) == first_true(NP_CMP[c](x, np.int32(s))), (c, s)
    finally:
        d.free()


def test_find_if_float_zeros_and_nan(dr):
    n = 2 * tile(np.float32) + 7
    x = np.zeros(n, np.float32)
    x[::2] = -0.0
    p = tile(np.float32) + 3
    x[p] = np.nan
    d = Dev(dr, x)
    try:
        assert d.find("ne", 0.0) == p   # a NaN passes only NE
        assert d.find("eq", 0.0) == 0   # -0.0 == +0.0
        assert d.find("eq", -0.0) == 0
        for c in ("lt", "le", "gt", "ge"):
            assert d.find(c, np.nan) == n
        assert d.find("le", 0.0) == 0
        assert d.find("lt", 0.0) == n
    finally:
        d.free()


@pytest.mark.parametrize("dtype", [np.int64, np.uint64])
def test_find_if_high_words(dr, dtype):
    """Values that differ only above bit 32, or only in the sign bit."""
    n = tile(dtype) + 9
    base = 5 | (1 << 32)
    x = np.full(n, base, dtype)
    d = Dev(dr, x)
    try:
        for p in positions(n, dtype):
            other = 5 | (2 << 32)
            d.poke(p, other)
            assert d.find("eq", other) == p
            assert d.find("gt", base) == p
            assert d.find("eq", 5) == n
            if dtype == np.int64:
                d.poke(p, base - (1 << 63))  # only the sign bit differs
                assert d.find("lt", 0) == p
            else:
                d.poke(p, base | (1 << 63))
                assert d.find("gt", 1 << 62) == p
            assert d.find("ne", base) == p
            d.poke(p, base)
        assert d.find("ne", base) == n
    finally:
        d.free()


# -------------------------------------------------------- is_sorted_until

def check_sorted(dr, dtype, n, offset=0):
    x = iota(n, dtype)
    d = Dev(dr, x, offset)
    try:
        assert d.sorted_until() == n
        t = tile(dtype)
        # one inversion: the pair (p - 1, p), among them (T - 1, T) across two tiles, the last pair, and the pairs
        # across two lanes' slots (64 V elements) and two waves' runs of a tile (1024 to 4096 elements)
        for p in sorted({p for p in positions(n, dtype) + [n - 1, t, 64, 128, 256, 1024, 2048, 4096] if 1 <= p < n}):
            d.poke(p, x[p - 1] - 1)
            assert d.sorted_until() == p, p
            d.poke(p, x[p])
        assert d.sorted_until() == n
    finally:
        d.free()
    for y, want in ((np.full(n, 7, dtype), n), (iota(n, dtype)[::-1].copy(), 1 if n >= 2 else n)):
        d = Dev(dr, y, offset)
        try:
            assert d.sorted_until() == want
        finally:
            d.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_is_sorted_until_small(dr, dtype):
    for n in SMALL:
        check_sorted(dr, dtype, n)
    check_sorted(dr, dtype, 257, offset=1)


@pytest.mark.parametrize("dtype", LARGE_DTYPES)
def test_is_sorted_until_large(dr, dtype):
    for n in large(dtype):
        check_sorted(dr, dtype, n)
    check_sorted(dr, dtype, 3 * tile(dtype) + 5, offset=1)
    check_sorted(dr, dtype, 2 * 4096 + 1, offset=1)


@pytest.mark.parametrize("dtype", [np.uint32, np.float64])
def test_is_sorted_until_many_tiles_per_workgroup(dr, dtype):
    check_sorted(dr, dtype, big(dtype))


# --------------------------------------------------------------- mismatch

def check_mismatch(dr, dtype, n, off_a=0, off_b=0):
    x = iota(n, dtype)
    a, b = Dev(dr, x, off_a), Dev(dr, x, off_b)
    try:
        assert a.mismatch(b) == n
        for p in sorted(set(positions(n, dtype)) | {q for q in (tile(dtype) // 2 - 1, tile(dtype) // 2) if q < n}):
            b.poke(p, x[p] + 1)
            assert a.mismatch(b) == p
            assert b.mismatch(a) == p
            if p + 1 < n:  # a later difference does not win
                b.poke(n - 1, 0)
                assert a.mismatch(b) == p
                b.poke(n - 1, x[n - 1])
            b.poke(p, x[p])
        assert a.mismatch(b) == n
    finally:
        a.free()
        b.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_mismatch_small(dr, dtype):
    for n in SMALL:
        check_mismatch(dr, dtype, n)
    check_mismatch(dr, dtype, 257, off_b=1)


@pytest.mark.parametrize("dtype", LARGE_DTYPES)
def test_mismatch_large(dr, dtype):
    for n in large(dtype):
        check_mismatch(dr, dtype, n)
    check_mismatch(dr, dtype, 3 * tile(dtype) + 5, off_a=1)  # a and b aligned differently
    check_mismatch(dr, dtype, 3 * tile(dtype) + 5, off_b=1)


def test_mismatch_many_tiles_per_workgroup(dr):
    check_mismatch(dr, np.uint32, big(np.uint32))  # two inputs share the 64 KiB tile: 8192-element tiles


# ---------------------------------------------------------------- extrema

def check_against_numpy(d, x):
    lo, hi, mm = d.extrema()
    want = ref_extrema(x)
    assert (lo, hi, mm) == want, ((lo, hi, mm), want)
    assert mm[0] == lo  # minmax agrees with min_element


def check_extrema(dr, dtype, n, offset=0):
    rng = np.random.default_rng(7 + n)
    x = rng.integers(100, 1000, n).astype(dtype)
    d = Dev(dr, x, offset)
    try:
        check_against_numpy(d, x)
        t = tile(dtype)
        # the extreme values twice: in one wave, in two tiles of different workgroups, in two tiles of one
        # workgroup, at 0 and n - 1
        for a, b in ((3, 40), (10, t + 10), (10, GRID * t + 10), (t - 1, 2 * t), (0, n - 1)):
            if not (0 <= a < b and b + 1 < n + (b == n - 1)) or n < 4:
                continue
            y = x.copy()
            lo_at = (a, b)
            hi_at = (a + 1, b - 1) if b == n - 1 else (a + 1, b + 1)
            for p in lo_at:
                y[p] = 5
            for p in hi_at:
                y[p] = 5000
            for p in lo_at + hi_at:
                d.poke(p, y[p])
            check_against_numpy(d, y)
            for p in lo_at + hi_at:
                d.poke(p, x[p])
    finally:
        d.free()
    if n > (1 << 20):
        return
    for y in (np.full(n, 7, dtype), iota(n, dtype), iota(n, dtype)[::-1].copy()):
        d = Dev(dr, y, offset)
        try:
            check_against_numpy(d, y)
            if n and y[0] == y[-1]:
                assert d.extrema() == (0, 0, (0, n - 1))
        finally:
            d.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_extrema_small(dr, dtype):
    for n in SMALL:
        check_extrema(dr, dtype, n)
    check_extrema(dr, dtype, 257, offset=1)


@pytest.mark.parametrize("dtype", LARGE_DTYPES)
def test_extrema_large(dr, dtype):
    for n in large(dtype):
        check_extrema(dr, dtype, n)
    check_extrema(dr, dtype, 3 * tile(dtype) + 5, offset=1)


@pytest.mark.parametrize("dtype", LARGE_DTYPES)
def test_extrema_many_tiles_per_workgroup(dr, dtype):
    check_extrema(dr, dtype, big(dtype))


@pytest.mark.parametrize("dtype,values", [
    (np.int32, [0, np.iinfo(np.int32).min, np.iinfo(np.int32).max, -1, 1]),
    (np.uint32, [5, 0, np.iinfo(np.uint32).max, 1 << 31, (1 << 31) - 1]),
    (np.int64, [1, -(1 << 31) - 1, -(1 << 40), 1 << 40, np.iinfo(np.int64).min, np.iinfo(np.int64).max, (1 << 32) + 1]),
    (np.uint64, [5, (1 << 63) + 1, 1 << 63, np.iinfo(np.uint64).max, 0, (1 << 32) + 5]),
])
def test_extrema_integer_limits(dr, dtype, values):
    n = 2 * tile(dtype) + 11
    rng = np.random.default_rng(3)
    x = np.array(values, dtype)[rng.integers(0, len(values), n)]
    d = Dev(dr, x)
    try:
        check_against_numpy(d, x)
    finally:
        d.free()
    # two values that differ only above bit 32 / only in the top bit
    for pair in ([values[0], values[-1]], values[1:3]):
        y = np.array(pair, dtype)[rng.integers(0, 2, n)]
        d = Dev(dr, y)
        try:
            check_against_numpy(d, y)
        finally:
            d.free()


def test_extrema_float_signed_zeros(dr):
    """-0.0 == +0.0: whichever comes first wins a first extremum, whichever comes last the last maximum."""
    n = tile(np.float32) + 5
    for first, second in ((-0.0, 0.0), (0.0, -0.0)):
        for fill, a, b in ((1.0, 70, tile(np.float32) + 1), (-1.0, 3, 200)):
            x = np.full(n, fill, np.float32)
            x[a], x[b] = first, second
            d = Dev(dr, x)
            try:
                lo, hi, mm = d.extrema()
                if fill > 0:  # the zeros are the least
                    assert lo == a and mm[0] == a
                    assert hi == 0 and mm[1] == n - 1
                else:         # the zeros are the greatest
                    assert hi == a and mm[1] == b
                    assert lo == 0 and mm[0] == 0
            finally:
                d.free()


# ---------------------------------------------------------------- capture

def test_graph_replay(dr):
    """A captured find_if + min_element, replayed after the input has changed: the state clear is part of the graph."""
    n = 5 * tile(np.int32) + 77
    rng = np.random.default_rng(11)
    xs = []
    for hit, lo in ((4 * tile(np.int32) + 5, 17), (3, 2 * tile(np.int32)), (n - 1, 0)):
        x = rng.integers(100, 1000, n).astype(np.int32)
        x[hit] = 7
        x[lo] = -3
        xs.append((x, hit, lo))
    d = Dev(dr, xs[0][0])
    out = dr.DeviceArray(0, 2, np.uint64)
    g = None
    try:
        dr.find_if_async(0, np.int32, "eq", d.ptr, n, 7, out.ptr)  # warm: the workspace grows here
        dr.min_element_async(0, np.int32, d.ptr, n, out.ptr + 8)
        dr.sync(0)
        dr.graph_begin(0)
        dr.find_if_async(0, np.int32, "eq", d.ptr, n, 7, out.ptr)
        dr.min_element_async(0, np.int32, d.ptr, n, out.ptr + 8)
        g = dr.graph_end(0)
        for x, hit, lo in xs + xs[:1]:
            dr.h2d(0, d.ptr, x)
            dr.h2d(0, out.ptr, np.array([SENTINEL, SENTINEL], np.uint64))
            dr.graph_launch(0, g)
            dr.sync(0)
            r = out.numpy()
            assert (int(r[0]), int(r[1])) == (hit, lo)
    finally:
        if g:
            dr.graph_destroy(g)
        d.free()
        out.free()


def test_blocking_helpers(dr):
    x = np.array([5, 3, 9, 3, 9, 1, 1, 2], np.int32)
    d = Dev(dr, x)
    try:
        assert dr.find_if(0, d.ptr, x.size, np.int32, "eq", 9) == 2
        assert dr.is_sorted_until(0, d.ptr, x.size, np.int32) == 1
        assert dr.min_element(0, d.ptr, x.size, np.int32) == 5
        assert dr.max_element(0, d.ptr, x.size, np.int32) == 2
        assert dr.minmax_element(0, d.ptr, x.size, np.int32) == (5, 4)
        assert dr.mismatch(0, d.ptr, d.ptr, x.size, np.int32) == x.size
        assert dr.min_element(0, d.ptr, 0, np.int32) == 0
        assert dr.minmax_element(0, d.ptr, 0, np.int32) == (0, 0)
        assert dr.find_if(0, d.ptr, 0, np.int32, "eq", 9) == 0
    finally:
        d.free()
