"""GPU tests of the by-key reduction C-ABI (drhip_reduce_by_key,
drhip_run_length_encode, drhip_unique_copy) on one segment.  The expected
values come from numpy: run starts from np.flatnonzero(k[1:] != k[:-1]), folds
from np.<ufunc>.reduceat, compared bit for bit (through .view(np.uint8)).
Every output has one element more than n and is pre-filled with a sentinel
byte; everything at or past the returned run count must still be the sentinel.

Tile sizes of the kernel (include/dr/details/segreduce_kernel.hpp, 256 threads
x 8 slots x E elements): T4 = 8192 elements when keys and values are 16-byte
aligned and both 4 bytes wide (and for unique_copy and run_length_encode of
4-byte keys: the counts are 4 bytes inside the tile), T8 = 4096 when either is
8 bytes wide, TU = 2048 for the element-load form any unaligned span takes.  Every size and
pattern below is derived from these three."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T4 = 8192   # aligned, 4-byte keys with 4-byte values
T8 = 4096   # aligned, a key or a value of 8 bytes
TU = 2048   # the element-load form
TILES = (T4, T8, TU)
BIG = 130 * max(TILES) + 13  # more than two 64-tile look-back steps for every tile size
SIZES = sorted({0, 1, 2, 63, 64, 65, BIG} | {t + d for t in TILES for d in (-1, 0, 1)} | {2 * t + 1 for t in TILES})
PATTERNS = ["distinct", "equal", "len2", "rand3", "rand1000", "tile_runs", "last_of_tile", "cover", "mid_last"]
DTYPES = [np.int32, np.uint32, np.int64, np.uint64, np.float32, np.float64]
OPS = ["plus", "mul", "min", "max"]
UFUNC = {"plus": np.add, "mul": np.multiply, "min": np.minimum, "max": np.maximum}
# (key dtype, value dtype, op) of the size x pattern grid
COMBOS = [(np.uint32, np.uint32, "plus"), (np.int64, np.float64, "plus"), (np.float32, np.int64, "max")]
SENT_BYTE = 0xA5
COUNT_SENTINEL = 0xDEADBEEF12345678


def tile_of(kdtype, vdtype, aligned=True):
    if not aligned:
        return TU
    return T4 if max(np.dtype(kdtype).itemsize, np.dtype(vdtype).itemsize) == 4 else T8


def run_ids(kind, n, t, seed=0):
    """The run index of every element (non-decreasing, +1 at every head); t = the tile size the pattern aims at."""
    rng = np.random.default_rng(2000 + seed + n)
    heads = np.zeros(n, bool)
    if kind == "distinct":
        heads[:] = True
    elif kind == "equal":       # one run across every tile: the fix-up chain over head-less tiles
        pass
    elif kind == "len2":
        heads[::2] = True
    elif kind == "rand3":
        heads = rng.random(n) < 1 / 3
    elif kind == "rand1000":
        heads = rng.random(n) < 1 / 1000
    elif kind == "tile_runs":   # runs of exactly t: heads fall on tile starts
        heads[::t] = True
    elif kind == "last_of_tile":  # a run that starts on the last element of a tile
        heads[t - 1::2 * t] = True
    elif kind == "cover":       # one run covers tiles 1-3 whole, short runs around it
        heads[::3] = True
        heads[t:4 * t] = False
        heads[t:t + 1] = True
    elif kind == "mid_last":    # a single head in the middle of the last tile
        if n > 1:
            first = (n - 1) // t * t
            heads[first + (n - first) // 2] = True
    if n:
        heads[0] = True
    return np.cumsum(heads) - 1


def keys_of(rid, dtype):
    """Neighbouring runs get different keys, far runs may share one (the value repeats every 1000 / 3 runs)."""
    k = (rid * 3) % 1000
    if np.dtype(dtype).kind != "u":
        k = k - 500
    return k.astype(dtype)


def values_of(n, dtype, op, seed=0):
    """Values whose every partial fold is exact: integers wrap, float sums stay below 2^24, float products are
    powers of two, min / max take anything finite."""
    rng = np.random.default_rng(3000 + seed + n)
    dt = np.dtype(dtype)
    if dt.kind in "iu":
        return rng.integers(0, 1 << (8 * dt.itemsize), n, dtype=np.uint64).astype(dtype)
    if op == "plus":
        return rng.integers(0, 8, n).astype(dtype)
    if op == "mul":  # from {1, -1, 2, 0.5}; 2 and 0.5 alternate, so a product is at most 2^(run length)
        v = np.where(np.arange(n) % 2 == 0, 2.0, 0.5) * rng.choice([1.0, -1.0], n)
        v[rng.random(n) < 0.3] = 1.0
        return v.astype(dtype)
    return (rng.normal(0, 1e3, n)).astype(dtype)


def starts_of(k):
    if k.size == 0:
        return np.zeros(0, np.int64)
    with np.errstate(invalid="ignore"):
        return np.concatenate([[0], np.flatnonzero(k[1:] != k[:-1]) + 1])


def reference(k, v, op):
    s = starts_of(k)
    if k.size == 0:
        return k[:0], v[:0]
    with np.errstate(over="ignore"):
        return k[s], UFUNC[op].reduceat(v, s, dtype=v.dtype)  # add / multiply would widen small integers


_REF = {}


def cached_case(kind, n, kd, vd, op, aligned=True):
    """(keys, values, expected keys, expected values), computed once per case and left unchanged."""
    key = (kind, n, np.dtype(kd).str, np.dtype(vd).str, op, aligned)
    if key not in _REF:
        k = keys_of(run_ids(kind, n, tile_of(kd, vd, aligned)), kd)
        v = values_of(n, vd, op)
        wk, wv = reference(k, v, op)
        for a in (k, v, wk, wv):
            a.setflags(write=False)
        _REF[key] = (k, v, wk, wv)
    return _REF[key]


class Bufs:
    """keys / values in (each `off` elements past a 16-byte boundary), sentinel-filled outputs of n + 1 elements."""

    def __init__(self, dr, k, v=None, koff=0, voff=0, out_vdtype=None):
        self.dr, self.n = dr, k.size
        self.kd = k.dtype
        self.vd = np.dtype(out_vdtype) if out_vdtype is not None else (v.dtype if v is not None else None)
        self.all = []
        self.kin = self._dev(np.concatenate([np.zeros(koff, k.dtype), k, np.zeros(1, k.dtype)]), k.dtype)
        self.kin_ptr = self.kin.ptr + koff * k.dtype.itemsize
        self.vin_ptr = None
        if v is not None:
            self.vin = self._dev(np.concatenate([np.zeros(voff, v.dtype), v, np.zeros(1, v.dtype)]), v.dtype)
            self.vin_ptr = self.vin.ptr + voff * v.dtype.itemsize
        self.kout = self._dev(np.full((self.n + 1) * k.dtype.itemsize, SENT_BYTE, np.uint8), np.uint8)
        self.vout = None
        if self.vd is not None:
            self.vout = self._dev(np.full((self.n + 1) * self.vd.itemsize, SENT_BYTE, np.uint8), np.uint8)
        self.cnt = self._dev(np.array([COUNT_SENTINEL], np.uint64), np.uint64)

    def _dev(self, host, dtype):
        a = self.dr.DeviceArray(0, host.size, dtype, host=host)
        self.all.append(a)
        return a

    def refill(self):
        dr = self.dr
        dr.h2d(0, self.kout.ptr, np.full(self.kout.count, SENT_BYTE, np.uint8))
        if self.vout is not None:
            dr.h2d(0, self.vout.ptr, np.full(self.vout.count, SENT_BYTE, np.uint8))
        dr.h2d(0, self.cnt.ptr, np.array([COUNT_SENTINEL], np.uint64))

    def result(self):
        self.dr.sync(0)
        ko = self.kout.numpy().view(self.kd)
        vo = self.vout.numpy().view(self.vd) if self.vout is not None else None
        return ko, vo, int(self.cnt.numpy()[0])

    def free(self):
        for b in self.all:
            b.free()


def check_out(out, runs, want, what):
    assert np.array_equal(out[:runs].view(np.uint8), want.view(np.uint8)), what
    tail = out[runs:].view(np.uint8)  # includes the one element past n
    assert tail.size and np.all(tail == SENT_BYTE), what + ": an element at or past the run count was written"


def check_result(res, wk, wv):
    ko, vo, runs = res
    assert runs == wk.size
    check_out(ko, runs, wk, "keys")
    if wv is not None:
        check_out(vo, runs, wv, "values")


def rbk_case(dr, k, v, op, wk, wv, koff=0, voff=0):
    b = Bufs(dr, k, v, koff, voff)
    try:
        dr.reduce_by_key_async(0, k.dtype, v.dtype, op, b.kin_ptr, b.vin_ptr, k.size, b.kout.ptr, b.vout.ptr, b.cnt.ptr)
        check_result(b.result(), wk, wv)
    finally:
        b.free()


def rle_unique_case(dr, k, koff=0):
    s = starts_of(k)
    wk = k[s]
    wc = np.diff(np.concatenate([s, [k.size]])).astype(np.uint64)
    b = Bufs(dr, k, None, koff, out_vdtype=np.uint64)
    try:
        dr.run_length_encode_async(0, k.dtype, b.kin_ptr, k.size, b.kout.ptr, b.vout.ptr, b.cnt.ptr)
        check_result(b.result(), wk, wc)
        b.refill()
        dr.unique_copy_async(0, k.dtype, b.kin_ptr, k.size, b.kout.ptr, b.cnt.ptr)
        ko, _, runs = b.result()
        check_result((ko, None, runs), wk, None)
    finally:
        b.free()


@pytest.mark.parametrize("kind", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_patterns_at_every_size(dr, n, kind):
    for kd, vd, op in COMBOS:
        k, v, wk, wv = cached_case(kind, n, kd, vd, op)
        rbk_case(dr, k, v, op, wk, wv)


@pytest.mark.parametrize("kd", DTYPES)
def test_type_sweep(dr, kd):
    """All six key dtypes x all six value dtypes x all four ops, mean-3 runs."""
    for vd in DTYPES:
        n = 2 * tile_of(kd, vd) + 1
        for op in OPS:
            k, v, wk, wv = cached_case("rand3", n, kd, vd, op)
            rbk_case(dr, k, v, op, wk, wv)


def test_f32_plus_tolerance(dr):
    """F32 PLUS of values that do not add exactly: every run within L * 2^-24 relative of the float64 fold (the
    values are positive, so this bounds every order of association)."""
    n = 16 * T4 + 1
    rng = np.random.default_rng(17)
    heads = rng.random(n) < 1 / 1000
    heads[::4096] = True  # no run longer than 4096
    k = keys_of(np.cumsum(heads) - 1, np.uint32)
    v = rng.random(n, dtype=np.float32)
    s = starts_of(k)
    want = np.add.reduceat(v.astype(np.float64), s)
    length = np.diff(np.concatenate([s, [n]]))
    assert length.max() <= 4096
    b = Bufs(dr, k, v)
    try:
        dr.reduce_by_key_async(0, k.dtype, v.dtype, "plus", b.kin_ptr, b.vin_ptr, n, b.kout.ptr, b.vout.ptr, b.cnt.ptr)
        ko, vo, runs = b.result()
        assert runs == s.size
        check_out(ko, runs, k[s], "keys")
        rel = np.abs(vo[:runs].astype(np.float64) - want) / want
        print("largest relative error / bound:", float(np.max(rel / (length * 2.0 ** -24))))
        assert np.all(rel <= length * 2.0 ** -24)
    finally:
        b.free()


@pytest.mark.parametrize("kd", [np.float32, np.float64])
def test_float_keys(dr, kd):
    """IEEE ==: every NaN is a run of its own, -0.0 and +0.0 share a run whose key is the first one's bits."""
    k = np.array([np.nan, np.nan, 1, 1, -0.0, 0.0, 2], kd)
    v = np.arange(1, 8, dtype=np.uint32)
    wk, wv = reference(k, v, "plus")
    assert wk.size == 5 and np.signbit(wk[3]) and wk[3] == 0 and list(wv) == [1, 2, 7, 11, 7]
    rbk_case(dr, k, v, "plus", wk, wv)
    rle_unique_case(dr, k)
    # the same pattern across tile boundaries
    kk = np.resize(k, 2 * T8 + 1)
    vv = values_of(kk.size, np.uint32, "plus")
    rbk_case(dr, kk, vv, "plus", *reference(kk, vv, "plus"))
    rle_unique_case(dr, kk)


@pytest.mark.parametrize("kd,vd", [(np.uint32, np.uint32), (np.uint32, np.float64), (np.int64, np.int32)])
@pytest.mark.parametrize("koff,voff", [(1, 0), (0, 1), (1, 1)])
def test_alignment(dr, kd, vd, koff, voff):
    """Keys and values one element past a 16-byte boundary, separately and together; key and value sizes differ."""
    for n in (TU + 1, 2 * tile_of(kd, vd) + 1):
        for kind in ("rand3", "rand1000", "equal"):
            k, v, wk, wv = cached_case(kind, n, kd, vd, "plus", aligned=False)
            rbk_case(dr, k, v, "plus", wk, wv, koff, voff)


def test_mixed_sizes_aligned(dr):
    """A 4-byte key with an 8-byte value and the reverse, aligned, at every size of the 8-byte tile."""
    for kd, vd in ((np.float32, np.uint64), (np.uint64, np.float32)):
        for n in (T8 - 1, T8, T8 + 1, 2 * T8 + 1):
            for kind in ("rand3", "tile_runs", "equal"):
                k, v, wk, wv = cached_case(kind, n, kd, vd, "plus")
                rbk_case(dr, k, v, "plus", wk, wv)


@pytest.mark.parametrize("kind", PATTERNS)
def test_run_length_encode_and_unique(dr, kind):
    for kd in (np.uint32, np.float64):
        rle_unique_case(dr, keys_of(run_ids(kind, 2 * T8 + 1, T8), kd))
    rle_unique_case(dr, keys_of(run_ids(kind, 2 * T4 + 1, T4), np.int32))  # the 4-byte keys' tile
    rle_unique_case(dr, keys_of(run_ids(kind, 2 * TU + 1, TU), np.uint32), koff=1)


def test_run_length_encode_one_long_run(dr):
    """All keys equal at the largest size: one run whose count is n."""
    k = np.full(BIG, 7, np.uint32)
    rle_unique_case(dr, k)
    rle_unique_case(dr, k.astype(np.int64), koff=1)


def test_empty_input_writes_zero(dr):
    """n == 0: *num_runs receives 0 in stream order, nothing else is touched (null pointers allowed)."""
    cnt = dr.DeviceArray(0, 1, np.uint64, host=np.array([COUNT_SENTINEL], np.uint64))
    try:
        for call in (lambda: dr.reduce_by_key_async(0, np.int32, np.float32, "plus", None, None, 0, None, None, cnt.ptr),
                     lambda: dr.run_length_encode_async(0, np.int32, None, 0, None, None, cnt.ptr),
                     lambda: dr.unique_copy_async(0, np.int32, None, 0, None, cnt.ptr)):
            dr.h2d(0, cnt.ptr, np.array([COUNT_SENTINEL], np.uint64))
            call()
            dr.sync(0)
            assert int(cnt.numpy()[0]) == 0
    finally:
        cnt.free()


def test_graph_replay(dr):
    n = 5 * T4 + 77
    k1, v1, wk1, wv1 = cached_case("rand3", n, np.uint32, np.uint32, "plus")
    k2 = keys_of(run_ids("cover", n, T4, seed=1), np.uint32)  # another run count, head-less tiles
    v2 = values_of(n, np.uint32, "plus", seed=1)
    wk2, wv2 = reference(k2, v2, "plus")
    b = Bufs(dr, k1, v1)
    g = None

    def call():
        dr.reduce_by_key_async(0, np.uint32, np.uint32, "plus", b.kin_ptr, b.vin_ptr, n, b.kout.ptr, b.vout.ptr, b.cnt.ptr)

    try:
        call()  # warm: the workspace grows here
        dr.sync(0)
        dr.graph_begin(0)
        call()
        g = dr.graph_end(0)
        for k, v, wk, wv in ((k1, v1, wk1, wv1), (k2, v2, wk2, wv2), (k1, v1, wk1, wv1)):
            dr.h2d(0, b.kin_ptr, k)
            dr.h2d(0, b.vin_ptr, v)
            b.refill()
            dr.graph_launch(0, g)
            check_result(b.result(), wk, wv)
    finally:
        if g:
            dr.graph_destroy(g)
        b.free()


def test_state_reused_back_to_back(dr):
    """Three calls on the segment, different n and entry points, no sync between them."""
    ka, va, wka, wva = cached_case("rand3", BIG, np.uint32, np.uint32, "plus")
    kb, vb, wkb, wvb = cached_case("rand1000", 3 * T8 + 5, np.int64, np.float64, "plus")
    a, b, c = Bufs(dr, ka, va), Bufs(dr, kb, vb), Bufs(dr, ka, None)
    try:
        dr.reduce_by_key_async(0, ka.dtype, va.dtype, "plus", a.kin_ptr, a.vin_ptr, BIG, a.kout.ptr, a.vout.ptr, a.cnt.ptr)
        dr.reduce_by_key_async(0, kb.dtype, vb.dtype, "plus", b.kin_ptr, b.vin_ptr, kb.size, b.kout.ptr, b.vout.ptr,
                               b.cnt.ptr)
        dr.unique_copy_async(0, ka.dtype, c.kin_ptr, BIG, c.kout.ptr, c.cnt.ptr)
        check_result(a.result(), wka, wva)
        check_result(b.result(), wkb, wvb)
        check_result(c.result(), wka, None)
    finally:
        for t in (a, b, c):
            t.free()


def test_blocking_conveniences(dr):
    n = T8 + 104  # a multiple of 10
    k = (np.arange(n) // 10).astype(np.int64)
    v = np.ones(n, np.float64)
    kin = dr.DeviceArray(0, n, np.int64, host=k)
    vin = dr.DeviceArray(0, n, np.float64, host=v)
    kout = dr.DeviceArray(0, n, np.int64, host=np.full(n, -1, np.int64))
    vout = dr.DeviceArray(0, n, np.float64, host=np.full(n, -1.0))
    cout = dr.DeviceArray(0, n, np.uint64, host=np.zeros(n, np.uint64))
    runs = n // 10
    try:
        assert dr.reduce_by_key(0, kin.ptr, vin.ptr, n, np.int64, np.float64, kout.ptr, vout.ptr) == runs
        assert np.array_equal(kout.numpy()[:runs + 1], np.concatenate([np.arange(runs), [-1]]))
        assert np.array_equal(vout.numpy()[:runs + 1], np.concatenate([np.full(runs, 10.0), [-1.0]]))
        assert dr.run_length_encode(0, kin.ptr, n, np.int64, kout.ptr, cout.ptr) == runs
        assert np.all(cout.numpy()[:runs] == 10) and cout.numpy()[runs] == 0
        assert dr.unique_copy(0, kin.ptr, n, np.int64, kout.ptr) == runs
    finally:
        for b in (kin, vin, kout, vout, cout):
            b.free()
