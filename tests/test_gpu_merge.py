"""GPU tests of the merge C-ABI (drhip_merge, drhip_merge_pairs) on one segment,
through drhip.py.  Every output must be exact, byte for byte: the reference is
the concatenation a ++ b sorted STABLY (numpy.argsort(kind="stable")), which on
sorted inputs is std::merge -- a's element first on ties, each input in its
own order.

Shapes of the kernel (include/dr/details/merge_kernel.hpp): the output is cut
into tiles of T = drhip.MERGE_TILE[itemsize] elements, a workgroup takes a
contiguous run of tiles and finds each tile's split on the merge path itself;
whole tiles leave as 16-byte stores when the output is 16-byte aligned, the
ragged last tile and unaligned outputs as element stores."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DTYPES = [np.int32, np.uint32, np.int64, np.uint64, np.float32, np.float64]
SENT = 0x5A


def tile(dr, dtype):
    return dr.MERGE_TILE[np.dtype(dtype).itemsize]


def small_lengths(dr, dtype):
    t = tile(dr, dtype)
    edge = [0, 1, 3, t - 1, t, t + 1]
    return [(na, nb) for na in edge for nb in edge] + [(2 * t + 1, 5), (5, 2 * t + 1), (3 * t + 5, 3 * t - 7)]


LARGE = ((1 << 19) + 3, (1 << 19) + 11)


def dense(n, dtype, seed, span=None):
    """n sorted integer-valued elements drawn from about n / 4 values: dense duplicates.  Signed types and floats
    hold negative values too."""
    dt = np.dtype(dtype)
    span = span or max(1, n // 4)
    lo = 10 if dt.kind == "u" else -(span // 2)
    return np.sort((lo + np.random.default_rng(seed).integers(0, span, n)).astype(dt))


def reference(a, b, va=None, vb=None):
    keys = np.concatenate([a, b])
    order = np.argsort(keys, kind="stable")
    if va is None:
        return keys[order], None
    return keys[order], np.concatenate([va, vb])[order]


def same_bits(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def sentinels(n, dt):
    return np.frombuffer(bytes([SENT]) * (n * dt.itemsize), dt)


class Buf:
    """`host` on the device, `offset` elements into its buffer (offset = 1: not 16-byte aligned), with `pad`
    sentinel elements behind."""

    def __init__(self, dr, host, offset=0, pad=0):
        dt = host.dtype
        self.n, self.offset, self.pad, self.dtype = host.size, offset, pad, dt
        whole = np.concatenate([sentinels(offset, dt), host, sentinels(pad, dt)])
        self.buf = dr.DeviceArray(0, whole.size, dt, host=whole if whole.size else None)
        self.ptr = self.buf.ptr + offset * dt.itemsize

    def result(self):
        """The n elements, after checking that the sentinels around them are intact."""
        got = self.buf.numpy()
        raw = got.view(np.uint8)
        es = self.dtype.itemsize
        assert (raw[:self.offset * es] == SENT).all(), "an element before the output was written"
        assert (raw[(self.offset + self.n) * es:] == SENT).all(), "an element behind the output was written"
        return got[self.offset:self.offset + self.n]

    def free(self):
        self.buf.free()


def check_merge(dr, a, b, offset=0, vdtype=None):
    """drhip_merge (vdtype None) or drhip_merge_pairs of a and b against the reference; the values are the source
    tags arange(na) and 2^31 + arange(nb).  Inputs and outputs start `offset` elements into their buffers; one
    sentinel element before (offset = 1) and three behind every output must stay intact."""
    dt = a.dtype
    n = a.size + b.size
    bufs = [Buf(dr, a, offset), Buf(dr, b, offset), Buf(dr, sentinels(n, dt), offset, 3)]
    try:
        if vdtype is None:
            want, _ = reference(a, b)
            dr.merge_async(0, dt, bufs[0].ptr, a.size, bufs[1].ptr, b.size, bufs[2].ptr)
            assert same_bits(bufs[2].result(), want), (dt, a.size, b.size, offset)
            return
        vdt = np.dtype(vdtype)
        va = np.arange(a.size, dtype=vdt)
        vb = (1 << 31) + np.arange(b.size, dtype=np.uint64).astype(vdt) if vdt.itemsize == 8 else \
            (np.uint32(1 << 31) + np.arange(b.size, dtype=np.uint32)).astype(vdt)
        want_k, want_v = reference(a, b, va, vb)
        bufs += [Buf(dr, va, offset), Buf(dr, vb, offset),
                 Buf(dr, sentinels(n, vdt), offset, 3)]
        dr.merge_pairs_async(0, dt, bufs[0].ptr, bufs[3].ptr, a.size, bufs[1].ptr, bufs[4].ptr, b.size, vdt.itemsize,
                             bufs[2].ptr, bufs[5].ptr)
        assert same_bits(bufs[2].result(), want_k), (dt, vdt, a.size, b.size, offset)
        assert same_bits(bufs[5].result(), want_v), (dt, vdt, a.size, b.size, offset)
    finally:
        for x in bufs:
            x.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_lengths(dr, dtype):
    """Every pair of lengths around a tile, an empty and a one-element input included, on dense duplicates."""
    for na, nb in small_lengths(dr, dtype):
        span = max(1, (na + nb) // 4)
        check_merge(dr, dense(na, dtype, 1 + na, span), dense(nb, dtype, 2 + nb, span))


@pytest.mark.parametrize("dtype", [np.uint32, np.float64])
def test_large(dr, dtype):
    """Many tiles per workgroup's run: 2^19 + 3 and 2^19 + 11 elements."""
    na, nb = LARGE
    check_merge(dr, dense(na, dtype, 11, (na + nb) // 4), dense(nb, dtype, 12, (na + nb) // 4))
    check_merge(dr, dense(na, dtype, 13, (na + nb) // 4), dense(nb, dtype, 14, (na + nb) // 4), vdtype=np.uint64)


@pytest.mark.parametrize("vdtype", [np.uint32, np.uint64])
@pytest.mark.parametrize("dtype", DTYPES)
def test_pairs_lengths(dr, dtype, vdtype):
    """merge_pairs at every length pair above: the values are source tags, so exact values pin the stability and
    the payload permutation at every tile edge."""
    for na, nb in small_lengths(dr, dtype):
        span = max(1, (na + nb) // 4)
        check_merge(dr, dense(na, dtype, 3 + na, span), dense(nb, dtype, 4 + nb, span), vdtype=vdtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_contents(dr, dtype):
    """a entirely below b, b entirely below a, all elements equal; floats with -inf, +inf and both zeros."""
    t = tile(dr, dtype)
    dt = np.dtype(dtype)
    na, nb = 3 * t + 5, 3 * t - 7
    low, high = dense(na, dtype, 21, 50), dense(nb, dtype, 22, 50) + dt.type(1000)
    for a, b in ((low, high), (high, low), (np.full(na, 7, dt), np.full(nb, 7, dt))):
        check_merge(dr, a, b)
        check_merge(dr, a, b, vdtype=np.uint32)
    if dt.kind == "f":
        special = np.array([-np.inf, -np.inf, -0.0, 0.0, 0.0, -0.0, np.inf, np.inf], dt)
        a = np.sort(np.concatenate([dense(na, dtype, 23, 20), special]), kind="stable")
        b = np.sort(np.concatenate([dense(nb, dtype, 24, 20), special[::-1]]), kind="stable")
        check_merge(dr, a, b)
        check_merge(dr, a, b, vdtype=np.uint64)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_zeros_tie_and_a_comes_first(dr, dtype):
    """-0.0 and +0.0 are a tie under <: the output is a's zeros and then b's, whatever their signs -- visible in
    the key bits."""
    t = tile(dr, dtype)
    dt = np.dtype(dtype)
    neg, pos = np.full(t + 1, -0.0, dt), np.full(2 * t + 1, 0.0, dt)
    bits = np.dtype("u%d" % dt.itemsize)
    for a, b in ((neg, pos), (pos, neg)):
        out = Buf(dr, np.ones(a.size + b.size, dt))
        ba, bb = Buf(dr, a), Buf(dr, b)
        try:
            dr.merge_async(0, dt, ba.ptr, a.size, bb.ptr, b.size, out.ptr)
            got = out.result().view(bits)
            assert np.array_equal(got, np.concatenate([a, b]).view(bits))
        finally:
            for x in (out, ba, bb):
                x.free()
        check_merge(dr, a, b, vdtype=np.uint32)


@pytest.mark.parametrize("dtype", DTYPES)
def test_unaligned_pointers(dr, dtype):
    """Inputs and outputs one element into their buffers: every 16-byte path falls back to element stores; the
    element before each output and the three behind it stay intact."""
    t = tile(dr, dtype)
    for na, nb in ((3, 5), (t, t + 1), (3 * t + 5, 3 * t - 7)):
        span = max(1, (na + nb) // 4)
        a, b = dense(na, dtype, 31 + na, span), dense(nb, dtype, 32 + nb, span)
        check_merge(dr, a, b, offset=1)
        check_merge(dr, a, b, offset=1, vdtype=np.uint32)
        check_merge(dr, a, b, offset=1, vdtype=np.uint64)


def test_graph_replay_without_warm_up(dr):
    """Calls captured with no eager call before them, replayed after the inputs were overwritten, merge the new
    inputs: the kernel keeps no state outside its arguments."""
    dtype = np.dtype(np.int64)
    t = tile(dr, dtype)
    na, nb = 5 * t + 3, 2 * t + 9
    a_d, b_d = dr.DeviceArray(0, na, dtype), dr.DeviceArray(0, nb, dtype)
    va_d, vb_d = dr.DeviceArray(0, na, np.uint32), dr.DeviceArray(0, nb, np.uint32)
    out = dr.DeviceArray(0, na + nb, dtype)
    ko, vo = dr.DeviceArray(0, na + nb, dtype), dr.DeviceArray(0, na + nb, np.uint32)
    va = np.arange(na, dtype=np.uint32)
    vb = np.uint32(1 << 31) + np.arange(nb, dtype=np.uint32)
    g = None
    try:
        dr.sync(0)
        dr.graph_begin(0)
        dr.merge_async(0, dtype, a_d.ptr, na, b_d.ptr, nb, out.ptr)
        dr.merge_pairs_async(0, dtype, a_d.ptr, va_d.ptr, na, b_d.ptr, vb_d.ptr, nb, 4, ko.ptr, vo.ptr)
        g = dr.graph_end(0)
        dr.h2d(0, va_d.ptr, va)
        dr.h2d(0, vb_d.ptr, vb)
        for round_ in range(3):
            a, b = dense(na, dtype, 41 + round_, 300 * (round_ + 1)), dense(nb, dtype, 51 + round_, 300 * (round_ + 1))
            dr.h2d(0, a_d.ptr, a)
            dr.h2d(0, b_d.ptr, b)
            dr.h2d(0, out.ptr, np.full(na + nb, 0xDEAD, dtype))
            dr.h2d(0, ko.ptr, np.full(na + nb, 0xDEAD, dtype))
            dr.graph_launch(0, g)
            dr.sync(0)
            want_k, want_v = reference(a, b, va, vb)
            assert same_bits(out.numpy(), want_k)
            assert same_bits(ko.numpy(), want_k)
            assert same_bits(vo.numpy(), want_v)
    finally:
        if g:
            dr.graph_destroy(g)
        for x in (a_d, b_d, va_d, vb_d, out, ko, vo):
            x.free()


def test_blocking_helpers_and_refusal_on_real_buffers(dr):
    a = np.array([1, 3, 3, 8], np.int32)
    b = np.array([0, 3, 9, 9, 10], np.int32)
    a_d, b_d = dr.DeviceArray(0, a.size, np.int32, host=a), dr.DeviceArray(0, b.size, np.int32, host=b)
    va_d = dr.DeviceArray(0, a.size, np.uint64, host=np.arange(4, dtype=np.uint64))
    vb_d = dr.DeviceArray(0, b.size, np.uint64, host=10 + np.arange(5, dtype=np.uint64))
    try:
        got = dr.merge(0, a_d.ptr, a.size, b_d.ptr, b.size, np.int32)
        assert got.dtype == np.int32 and got.tolist() == [0, 1, 3, 3, 3, 8, 9, 9, 10]
        k, v = dr.merge_pairs(0, a_d.ptr, va_d.ptr, a.size, b_d.ptr, vb_d.ptr, b.size, np.int32, np.uint64)
        assert k.tolist() == [0, 1, 3, 3, 3, 8, 9, 9, 10] and v.tolist() == [10, 0, 1, 2, 11, 3, 12, 13, 14]
        # one empty input: a copy of the other; both empty: an empty array
        assert dr.merge(0, a_d.ptr, 0, b_d.ptr, b.size, np.int32).tolist() == b.tolist()
        assert dr.merge(0, a_d.ptr, a.size, 0, 0, np.int32).tolist() == a.tolist()
        assert dr.merge(0, 0, 0, 0, 0, np.int32).size == 0
        # a refusal on real buffers leaves them untouched
        with pytest.raises(dr.DrhipError, match="drhip_merge"):
            dr.merge_async(0, np.int32, a_d.ptr, a.size, b_d.ptr, b.size, b_d.ptr)
        assert np.array_equal(b_d.numpy(), b) and np.array_equal(a_d.numpy(), a)
    finally:
        for x in (a_d, b_d, va_d, vb_d):
            x.free()
