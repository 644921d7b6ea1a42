"""Bit-exact GPU parity of the elementwise family (csrc/elementwise.hip):
drhip_transform_scalar / drhip_transform_binary over every dtype and op,
drhip_negate, drhip_iota and drhip_fill, on aligned and misaligned operands
(vector and scalar kernels), out of place and in place, with guard cells on
both sides of every written range.

References are plain NumPy in the element dtype.  min / max follow the
kernel's stated definition (b < a ? b : a and a < b ? b : a), written with
np.where: np.minimum / np.maximum differ for a NaN operand and for signed
zeros.  Floats are compared by bit pattern; where an operation *creates* a
NaN (inf - inf, 0 * inf) only its position is compared, because the bits of a
generated NaN are the platform's choice.

Not covered: the grid-stride second iteration (more than kEwMaxBlocks * 256 =
2^30 vectors, over 16 GiB per operand)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DTYPES = [np.int32, np.uint32, np.int64, np.uint64, np.float32, np.float64]
OPS = ["plus", "mul", "min", "max"]
G = 16  # guard elements on each side of the written range
NMAX = (1 << 20) + 7


def sizes(itemsize):
    v = 16 // itemsize
    return [0, 1, 3, 256 * v - 1, 256 * v, 256 * v + 1, 100003, NMAX]


def bits(a):
    return np.ascontiguousarray(a).view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@functools.lru_cache(maxsize=None)
def base_input(dtype, seed):
    """NMAX + 1 elements: integers over the full range; floats of mixed
    magnitude and sign with +-0, +-inf, NaN, denormals and the extremes
    scattered through (and at the first and last positions)."""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    n = NMAX + 1
    if dt.kind != "f":
        info = np.iinfo(dt)
        x = rng.integers(info.min, info.max, size=n, endpoint=True, dtype=dt)
        x[:4] = [info.min, info.max, 0, 1]
    else:
        fi = np.finfo(dt)
        x = ((rng.random(n) - 0.5) * np.exp2(rng.integers(-20, 20, n))).astype(dt)
        spec = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, fi.smallest_subnormal, -fi.smallest_subnormal,
                         fi.tiny / 2, fi.tiny, fi.max, -fi.max, 1.0, -1.0], dtype=dt)
        pos = rng.integers(0, n, n // 16)
        x[pos] = spec[rng.integers(0, spec.size, pos.size)]
        x[:spec.size] = spec
        x[-spec.size:] = spec[::-1]
    x.setflags(write=False)
    return x


def ref_op(op, a, b):
    """a op b in the element dtype; b an array or a 0-d array of a's dtype."""
    dt = a.dtype
    if op in ("plus", "mul"):
        if dt.kind == "i":  # two's-complement wrap, formed unsigned
            u = np.dtype("u%d" % dt.itemsize)
            a, b = a.view(u), np.asarray(b).view(u)
        with np.errstate(all="ignore"):
            r = a + b if op == "plus" else a * b
        return r.astype(r.dtype).view(dt) if dt.kind == "i" else r.astype(dt)
    if op == "min":
        return np.where(b < a, b, a).astype(dt)
    return np.where(a < b, b, a).astype(dt)


def assert_same(op, got, ref, what):
    if got.dtype.kind == "f" and op in ("plus", "mul"):
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(got), nan), what
        assert np.array_equal(bits(got)[~nan], bits(ref)[~nan]), what
    else:
        assert np.array_equal(bits(got), bits(ref)), what


def guard_values(dtype, op):
    """(sentinel, input guard): no op of the sweep turns guard inputs into
    the sentinel, so a store one slot outside the range shows."""
    return np.dtype(dtype).type(77), np.dtype(dtype).type(100 if op == "max" else 3)


def padded(dtype, off, n, fill, body=None):
    h = np.full(G + off + n + G, fill, dtype)
    if body is not None:
        h[G + off:G + off + n] = body
    return h


def scalars_for(dtype, op):
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return {"plus": [1.5, -np.inf], "mul": [-3.0, 0.0], "min": [0.25, np.nan, -0.0, 0.0],
                "max": [0.25, np.nan, -0.0, 0.0]}[op]
    info = np.iinfo(dt)
    # plus / mul wrap for most inputs; min / max split the inputs
    return {"plus": [info.max - 5], "mul": [info.max // 3 * 2 + 1], "min": [5 if dt.kind == "u" else -5],
            "max": [1000]}[op]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", OPS)
def test_transform_scalar_sweep(dr, dtype, op):
    dt = np.dtype(dtype)
    sent, gin = guard_values(dtype, op)
    x_all = base_input(dtype, 1)
    small = 256 * (16 // dt.itemsize) + 1
    for k, sc in enumerate(scalars_for(dtype, op)):
        s = np.array(sc, dtype=dt)
        for n in sizes(dt.itemsize):
            if k and n > small and n != 100003:
                continue
            x = x_all[1:1 + n]
            ref = ref_op(op, x, s)
            for io, oo in [(0, 0), (0, 1), (1, 0), (1, 1)]:  # out of place
                hin, hout = padded(dt, io, n, gin, x), padded(dt, oo, n, sent)
                src, dst = dr.DeviceArray(0, hin.size, dt, host=hin), dr.DeviceArray(0, hout.size, dt, host=hout)
                dr.transform_scalar(0, dt, op, src.at(G + io), dst.at(G + oo), n, s[()])
                got, kept = dst.numpy(), src.numpy()
                src.free()
                dst.free()
                what = (dt.name, op, sc, n, io, oo)
                assert_same(op, got[G + oo:G + oo + n], ref, what)
                hout[G + oo:G + oo + n] = got[G + oo:G + oo + n]
                assert np.array_equal(bits(got), bits(hout)), ("guard cells", what)
                assert np.array_equal(bits(kept), bits(hin)), ("input changed", what)
            for off in (0, 1):  # in place
                h = padded(dt, off, n, sent, x)
                buf = dr.DeviceArray(0, h.size, dt, host=h)
                dr.transform_scalar(0, dt, op, buf.at(G + off), buf.at(G + off), n, s[()])
                got = buf.numpy()
                buf.free()
                what = (dt.name, op, sc, n, off, "in place")
                assert_same(op, got[G + off:G + off + n], ref, what)
                h[G + off:G + off + n] = got[G + off:G + off + n]
                assert np.array_equal(bits(got), bits(h)), ("guard cells", what)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", OPS)
def test_transform_binary_sweep(dr, dtype, op):
    """One misaligned operand of three sends the call to the scalar kernel:
    every combination of operand offsets from {0, 1}."""
    dt = np.dtype(dtype)
    sent, gin = guard_values(dtype, op)
    a_all, b_all = base_input(dtype, 1), base_input(dtype, 2)
    for n in sizes(dt.itemsize):
        a, b = a_all[1:1 + n], b_all[:n]
        ref = ref_op(op, a, b)
        for ao, bo, oo in [(i, j, k) for i in (0, 1) for j in (0, 1) for k in (0, 1)]:  # out of place
            ha, hb, ho = padded(dt, ao, n, gin, a), padded(dt, bo, n, gin, b), padded(dt, oo, n, sent)
            da, db, do = (dr.DeviceArray(0, h.size, dt, host=h) for h in (ha, hb, ho))
            dr.transform_binary(0, dt, op, da.at(G + ao), db.at(G + bo), do.at(G + oo), n)
            got, ka, kb = do.numpy(), da.numpy(), db.numpy()
            for d in (da, db, do):
                d.free()
            what = (dt.name, op, n, ao, bo, oo)
            assert_same(op, got[G + oo:G + oo + n], ref, what)
            ho[G + oo:G + oo + n] = got[G + oo:G + oo + n]
            assert np.array_equal(bits(got), bits(ho)), ("guard cells", what)
            assert np.array_equal(bits(ka), bits(ha)) and np.array_equal(bits(kb), bits(hb)), ("input changed", what)
        for ao, bo in [(0, 0), (0, 1), (1, 0), (1, 1)]:  # in place: out == a
            ha, hb = padded(dt, ao, n, sent, a), padded(dt, bo, n, gin, b)
            da, db = (dr.DeviceArray(0, h.size, dt, host=h) for h in (ha, hb))
            dr.transform_binary(0, dt, op, da.at(G + ao), db.at(G + bo), da.at(G + ao), n)
            got = da.numpy()
            da.free()
            db.free()
            what = (dt.name, op, n, ao, bo, "in place")
            assert_same(op, got[G + ao:G + ao + n], ref, what)
            ha[G + ao:G + ao + n] = got[G + ao:G + ao + n]
            assert np.array_equal(bits(got), bits(ha)), ("guard cells", what)


@pytest.mark.parametrize("dtype", DTYPES)
def test_negate_sweep(dr, dtype):
    """0 - x with unsigned wrap for integers (iinfo.min stays, unsigned values
    wrap); a sign-bit flip for floats (-0.0, NaN payloads kept)."""
    dt = np.dtype(dtype)
    x_all = base_input(dtype, 3)
    u = np.dtype("u%d" % dt.itemsize)
    for n in sizes(dt.itemsize):
        x = x_all[:n]
        if dt.kind == "f":
            ref = bits(x) ^ u.type(1 << (8 * dt.itemsize - 1))
        else:
            ref = (u.type(0) - x.view(u)).astype(u)
        for off in (0, 1):
            h = padded(dt, off, n, 77, x)
            buf = dr.DeviceArray(0, h.size, dt, host=h)
            dr.negate(0, dt, buf.at(G + off), n)
            got = buf.numpy()
            buf.free()
            assert np.array_equal(bits(got[G + off:G + off + n]), ref), (dt.name, n, off)
            h[G + off:G + off + n] = got[G + off:G + off + n]
            assert np.array_equal(bits(got), bits(h)), ("guard cells", dt.name, n, off)


@pytest.mark.parametrize("dtype", DTYPES)
def test_iota_sweep(dr, dtype):
    """start + i in the element's compute type: integer starts within 5 of
    iinfo.max wrap, negative starts; float start + index rounds once (the
    index itself is exact: n <= 2^24)."""
    dt = np.dtype(dtype)
    if dt.kind == "f":
        starts = [0.5, -1000.25, 3e7 if dt == np.float32 else 3e15]
    else:
        starts = [np.iinfo(dt).max - 3, 20] + ([-7, np.iinfo(dt).min] if dt.kind == "i" else [])
    for start in starts:
        s = np.array(start, dtype=dt)
        for n in sizes(dt.itemsize):
            if dt.kind == "f":
                ref = (s + np.arange(n).astype(dt)).astype(dt)
            else:
                u = np.dtype("u%d" % dt.itemsize)
                ref = (s.view(u) + np.arange(n, dtype=u)).astype(u).view(dt)
            for off in (0, 1):
                h = padded(dt, off, n, 77)
                h[G + off:G + off + n] = 78  # never read: iota writes every element
                buf = dr.DeviceArray(0, h.size, dt, host=h)
                dr.iota(0, buf.at(G + off), n, s[()], dt)
                got = buf.numpy()
                buf.free()
                assert np.array_equal(bits(got[G + off:G + off + n]), bits(ref)), (dt.name, start, n, off)
                h[G + off:G + off + n] = got[G + off:G + off + n]
                assert np.array_equal(bits(got), bits(h)), ("guard cells", dt.name, start, n, off)


FILL_VALUES = {
    1: [0xA7, 0x00],
    2: [0x0102, 0xFF00],
    # bytes all different; a NaN payload; -0.0
    4: [0x01020304, 0x7FC12345, 0x80000000],
    8: [0x0102030405060708, 0x7FF8000012345678, 0x8000000000000000],
}


@pytest.mark.parametrize("elem", [1, 2, 4, 8])
def test_fill_sweep(dr, elem):
    """Element sizes 1 (memset), 2, 4 and 8 -- distributed_vector<char / short>
    construction reaches the first two -- at even and odd element offsets."""
    dt = np.dtype("u%d" % elem)
    for value in FILL_VALUES[elem]:
        for n in sizes(elem):
            for off in (0, 1, 3):
                h = padded(dt, off, n, 0x5A)
                buf = dr.DeviceArray(0, h.size, dt, host=h)
                dr.fill(0, buf.at(G + off), n, value, dt)
                got = buf.numpy()
                buf.free()
                h[G + off:G + off + n] = value
                assert np.array_equal(got, h), (elem, hex(value), n, off)
