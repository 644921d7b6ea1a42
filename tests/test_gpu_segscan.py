"""GPU tests of the by-key scan C-ABI (drhip_inclusive_scan_by_key,
drhip_exclusive_scan_by_key) on one segment.  The expected values come from
numpy: run starts from np.flatnonzero(k[1:] != k[:-1]) as in
test_gpu_segreduce.py, the scan from a vectorised segmented scan (log-step
doubling under head flags, checked once against a plain Python loop), compared
bit for bit (through .view(np.uint8)): the values are built so that every
partial fold is exact.  Every output has one element more than n and is
pre-filled with a sentinel byte; the element past n must still be the sentinel.

Tile sizes of the kernel (include/dr/details/segscan_kernel.hpp, 256 threads
x 8 slots x E elements): T4 = 8192 elements when keys and values are 16-byte
aligned and both 4 bytes wide, T8 = 4096 when either is 8 bytes wide, TU =
2048 for the element-load form any unaligned input takes.  Every size and
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
# the exclusive form's init: never the identity; float folds stay exact (plus: sums stay below 2^24; mul: a power of 2)
INIT = {"plus": 5, "mul": 2, "min": 3, "max": 3}
SENT_BYTE = 0xA5


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
    elif kind == "equal":       # one run across every tile: the look-back chain over head-less tiles
        pass
    elif kind == "len2":
        heads[::2] = True
    elif kind == "rand3":
        heads = rng.random(n) < 1 / 3
    elif kind == "rand1000":
        heads = rng.random(n) < 1 / 1000
    elif kind == "tile_runs":   # runs of exactly t: a head on every tile start, no carry may leak
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
    powers of two (short runs only), min / max take anything finite."""
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


def heads_of(k):
    h = np.ones(k.size, bool)
    if k.size > 1:
        with np.errstate(invalid="ignore"):
            h[1:] = k[1:] != k[:-1]
    return h


def seg_scan(v, heads, op):
    """Inclusive segmented scan: after the step of width d, out[i] folds the last min(2d, i - s + 1) elements up to i
    of the run that starts at s; `open` marks the elements that have not reached their head yet."""
    f = UFUNC[op]
    out = v.copy()
    closed = heads.copy()  # the fold of out[i] already starts at i's head
    d = 1
    with np.errstate(over="ignore"):
        while d < v.size and not closed[d:].all():
            take = ~closed[d:]
            out[d:] = np.where(take, f(out[:-d], out[d:], dtype=v.dtype), out[d:])
            closed[d:] = closed[d:] | closed[:-d]
            d *= 2
    return out


def excl_of(incl, heads, op, init):
    """The exclusive scan from the inclusive one: init at a head, init op (the fold up to the predecessor) elsewhere."""
    out = np.full(incl.size, init, incl.dtype)
    if incl.size > 1:
        with np.errstate(over="ignore"):
            rest = UFUNC[op](out[1:], incl[:-1], dtype=incl.dtype)
        out[1:] = np.where(heads[1:], out[1:], rest)
    return out


def loop_scan(v, heads, op, init=None):
    out = np.empty_like(v)
    f = UFUNC[op]
    acc = None
    with np.errstate(over="ignore"):
        for i in range(v.size):
            if init is None:
                acc = v[i] if heads[i] else f(acc, v[i], dtype=v.dtype)
                out[i] = acc
            else:
                out[i] = v.dtype.type(init) if heads[i] else f(v.dtype.type(init), acc, dtype=v.dtype)
                acc = v[i] if heads[i] else f(acc, v[i], dtype=v.dtype)
    return out


_REF = {}


def cached_case(kind, n, kd, vd, op, aligned=True):
    """(keys, values, expected inclusive, expected exclusive with INIT[op]), computed once per case, left unchanged."""
    key = (kind, n, np.dtype(kd).str, np.dtype(vd).str, op, aligned)
    if key not in _REF:
        k = keys_of(run_ids(kind, n, tile_of(kd, vd, aligned)), kd)
        v = values_of(n, vd, op)
        h = heads_of(k)
        wi = seg_scan(v, h, op)
        we = excl_of(wi, h, op, INIT[op])
        for a in (k, v, wi, we):
            a.setflags(write=False)
        _REF[key] = (k, v, wi, we)
    return _REF[key]


def test_reference_against_a_python_loop():
    """The vectorised reference itself, once, at n = 200, for every op on an integer and a float type."""
    n = 200
    k = keys_of(run_ids("rand3", n, TU), np.int32)
    k[100:140] = k[100]  # and one run of 40
    h = heads_of(k)
    for vd in (np.int32, np.float64):
        for op in OPS:
            v = values_of(n, vd, op)
            wi = seg_scan(v, h, op)
            assert np.array_equal(wi.view(np.uint8), loop_scan(v, h, op).view(np.uint8)), (vd, op)
            we = excl_of(wi, h, op, INIT[op])
            assert np.array_equal(we.view(np.uint8), loop_scan(v, h, op, INIT[op]).view(np.uint8)), (vd, op)


class Bufs:
    """keys / values in (each `off` elements past a 16-byte boundary), a sentinel-filled output of n + 1 elements."""

    def __init__(self, dr, k, v, koff=0, voff=0, ooff=0):
        self.dr, self.n, self.vd, self.ooff = dr, k.size, v.dtype, ooff
        self.all = []
        self.kin = self._dev(np.concatenate([np.zeros(koff, k.dtype), k, np.zeros(1, k.dtype)]), k.dtype)
        self.kin_ptr = self.kin.ptr + koff * k.dtype.itemsize
        self.vin = self._dev(np.concatenate([np.zeros(voff, v.dtype), v, np.zeros(1, v.dtype)]), v.dtype)
        self.vin_ptr = self.vin.ptr + voff * v.dtype.itemsize
        self.out = self._dev(np.full((ooff + self.n + 1) * v.dtype.itemsize, SENT_BYTE, np.uint8), np.uint8)
        self.out_ptr = self.out.ptr + ooff * v.dtype.itemsize

    def _dev(self, host, dtype):
        a = self.dr.DeviceArray(0, host.size, dtype, host=host)
        self.all.append(a)
        return a

    def refill(self):
        self.dr.h2d(0, self.out.ptr, np.full(self.out.count, SENT_BYTE, np.uint8))

    def result(self):
        self.dr.sync(0)
        return self.out.numpy().view(self.vd)

    def free(self):
        for b in self.all:
            b.free()


def check_out(b, want, what):
    o = b.result()
    sent = np.full(o.dtype.itemsize, SENT_BYTE, np.uint8)
    assert np.array_equal(o[b.ooff:b.ooff + b.n].view(np.uint8), want.view(np.uint8)), what
    assert np.array_equal(o[b.ooff + b.n:].view(np.uint8), sent), what + ": the element past n was written"
    assert np.all(o[:b.ooff].view(np.uint8) == SENT_BYTE), what + ": an element before the output was written"


def scan_case(dr, k, v, op, wi, we, koff=0, voff=0, ooff=0, init="default"):
    """Both entries on one set of buffers: inclusive against wi, exclusive (INIT[op] unless given) against we."""
    b = Bufs(dr, k, v, koff, voff, ooff)
    try:
        dr.inclusive_scan_by_key_async(0, k.dtype, v.dtype, op, b.kin_ptr, b.vin_ptr, k.size, b.out_ptr)
        check_out(b, wi, "inclusive")
        b.refill()
        dr.exclusive_scan_by_key_async(0, k.dtype, v.dtype, op, b.kin_ptr, b.vin_ptr, k.size, b.out_ptr,
                                       INIT[op] if init == "default" else init)
        check_out(b, we, "exclusive")
    finally:
        b.free()


@pytest.mark.parametrize("kind", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_patterns_at_every_size(dr, n, kind):
    for kd, vd, op in COMBOS:
        k, v, wi, we = cached_case(kind, n, kd, vd, op)
        scan_case(dr, k, v, op, wi, we)


@pytest.mark.parametrize("kd", DTYPES)
def test_type_sweep(dr, kd):
    """All six key dtypes x all six value dtypes x all four ops, mean-3 runs, at 2T + 1."""
    for vd in DTYPES:
        n = 2 * tile_of(kd, vd) + 1
        for op in OPS:
            k, v, wi, we = cached_case("rand3", n, kd, vd, op)
            scan_case(dr, k, v, op, wi, we)


@pytest.mark.parametrize("kd", [np.float32, np.float64])
def test_float_keys(dr, kd):
    """IEEE ==: every NaN is a run of its own, -0.0 and +0.0 share a run."""
    k = np.array([np.nan, np.nan, 1, 1, -0.0, 0.0, 2], kd)
    v = np.arange(1, 8, dtype=np.uint32)
    h = heads_of(k)
    wi = seg_scan(v, h, "plus")
    assert list(wi) == [1, 2, 3, 7, 5, 11, 7]
    we = excl_of(wi, h, "plus", 5)
    assert list(we) == [5, 5, 5, 8, 5, 10, 5]
    scan_case(dr, k, v, "plus", wi, we)
    # the same pattern across tile boundaries
    kk = np.resize(k, 2 * T8 + 1)
    vv = values_of(kk.size, np.uint32, "plus")
    hh = heads_of(kk)
    wwi = seg_scan(vv, hh, "plus")
    scan_case(dr, kk, vv, "plus", wwi, excl_of(wwi, hh, "plus", 5))


@pytest.mark.parametrize("kd,vd", [(np.uint32, np.uint32), (np.uint32, np.float64), (np.int64, np.int32)])
@pytest.mark.parametrize("koff,voff,ooff", [(1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, 1), (1, 1, 1)])
def test_alignment(dr, kd, vd, koff, voff, ooff):
    """Keys, values and the output one element past a 16-byte boundary, separately and together."""
    aligned = koff == 0 and voff == 0
    for n in (TU + 1, 2 * tile_of(kd, vd) + 1):
        for kind in ("rand3", "rand1000", "equal"):
            k, v, wi, we = cached_case(kind, n, kd, vd, "plus", aligned=aligned)
            scan_case(dr, k, v, "plus", wi, we, koff, voff, ooff)


def test_mixed_sizes_aligned(dr):
    """A 4-byte key with an 8-byte value and the reverse, aligned, at every size of the 8-byte tile."""
    for kd, vd in ((np.float32, np.uint64), (np.uint64, np.float32)):
        for n in (T8 - 1, T8, T8 + 1, 2 * T8 + 1):
            for kind in ("rand3", "tile_runs", "equal"):
                k, v, wi, we = cached_case(kind, n, kd, vd, "plus")
                scan_case(dr, k, v, "plus", wi, we)


@pytest.mark.parametrize("voff", [0, 1])
def test_in_place(dr, voff):
    """vals_out == vals_in, the 16-byte form and the element-load form, head-less tiles included."""
    for kind in ("rand1000", "equal", "cover"):
        n = 5 * T4 + 77
        k, v, wi, we = cached_case(kind, n, np.uint32, np.uint32, "plus", aligned=voff == 0)
        b = Bufs(dr, k, v, 0, voff)
        try:
            dr.inclusive_scan_by_key_async(0, k.dtype, v.dtype, "plus", b.kin_ptr, b.vin_ptr, n, b.vin_ptr)
            dr.sync(0)
            got = b.vin.numpy()
            assert np.array_equal(got[voff:voff + n], wi), kind
            assert got[voff + n] == 0 and np.all(got[:voff] == 0)
            dr.h2d(0, b.vin_ptr, v)
            dr.exclusive_scan_by_key_async(0, k.dtype, v.dtype, "plus", b.kin_ptr, b.vin_ptr, n, b.vin_ptr, INIT["plus"])
            dr.sync(0)
            got = b.vin.numpy()
            assert np.array_equal(got[voff:voff + n], we), kind
            assert got[voff + n] == 0 and np.all(got[:voff] == 0)
        finally:
            b.free()


@pytest.mark.parametrize("vd", [np.int32, np.uint64, np.float32, np.float64])
def test_init_none_is_the_identity(dr, vd):
    ident = {"plus": 0, "mul": 1}
    if np.dtype(vd).kind == "f":
        ident.update(min=np.inf, max=-np.inf)
    else:
        ident.update(min=np.iinfo(vd).max, max=np.iinfo(vd).min)
    n = 2 * T8 + 1
    for op in OPS:
        k, v, wi, _ = cached_case("rand3", n, np.uint32, vd, op)
        we = excl_of(wi, heads_of(k), op, ident[op])
        scan_case(dr, k, v, op, wi, we, init=None)


def test_f32_plus_tolerance(dr):
    """F32 PLUS of values that do not add exactly: every element within m * 2^-24 relative of the float64 segmented
    cumsum, m = the number of elements folded (the values are positive, so this bounds every order of association)."""
    n = 16 * T4 + 1
    rng = np.random.default_rng(17)
    heads = rng.random(n) < 1 / 1000
    heads[::4096] = True  # no run longer than 4096
    k = keys_of(np.cumsum(heads) - 1, np.uint32)
    v = rng.random(n, dtype=np.float32) + np.float32(2.0 ** -20)
    h = heads_of(k)
    s = np.flatnonzero(h)
    m = np.arange(n) - np.repeat(s, np.diff(np.concatenate([s, [n]]))) + 1
    assert m.max() <= 4096
    want = seg_scan(v.astype(np.float64), h, "plus")
    b = Bufs(dr, k, v)
    try:
        dr.inclusive_scan_by_key_async(0, k.dtype, v.dtype, "plus", b.kin_ptr, b.vin_ptr, n, b.out_ptr)
        got = b.result()[:n].astype(np.float64)
        rel = np.abs(got - want) / want
        print("inclusive: largest relative error / bound:", float(np.max(rel / (m * 2.0 ** -24))))
        assert np.all(rel <= m * 2.0 ** -24)
        b.refill()
        dr.exclusive_scan_by_key_async(0, k.dtype, v.dtype, "plus", b.kin_ptr, b.vin_ptr, n, b.out_ptr, 1.0)
        got = b.result()[:n].astype(np.float64)
        wante = np.where(h, 1.0, 1.0 + np.concatenate([[0.0], want[:-1]]))
        rel = np.abs(got - wante) / wante
        print("exclusive: largest relative error / bound:", float(np.max(rel / (m * 2.0 ** -24))))
        assert np.all(rel <= m * 2.0 ** -24)
    finally:
        b.free()


def test_graph_replay(dr):
    n = 5 * T4 + 77
    cases = [cached_case("rand3", n, np.uint32, np.uint32, "plus"),
             cached_case("cover", n, np.uint32, np.uint32, "plus"),   # head-less tiles
             cached_case("equal", n, np.uint32, np.uint32, "plus")]   # every tile but the first looks back
    b = Bufs(dr, cases[0][0], cases[0][1])
    e = Bufs(dr, cases[0][0], cases[0][1])
    g = None

    def call():
        dr.inclusive_scan_by_key_async(0, np.uint32, np.uint32, "plus", b.kin_ptr, b.vin_ptr, n, b.out_ptr)
        dr.exclusive_scan_by_key_async(0, np.uint32, np.uint32, "plus", b.kin_ptr, b.vin_ptr, n, e.out_ptr, INIT["plus"])

    try:
        call()  # warm: the workspace grows here
        dr.sync(0)
        dr.graph_begin(0)
        call()
        g = dr.graph_end(0)
        for k, v, wi, we in cases:
            dr.h2d(0, b.kin_ptr, k)
            dr.h2d(0, b.vin_ptr, v)
            b.refill()
            e.refill()
            dr.graph_launch(0, g)
            check_out(b, wi, "inclusive replay")
            check_out(e, we, "exclusive replay")
    finally:
        if g:
            dr.graph_destroy(g)
        b.free()
        e.free()


def test_state_shared_back_to_back(dr):
    """Calls of three algorithms that share the segment's workspace, different n, no sync between them."""
    ka, va, wia, wea = cached_case("rand3", BIG, np.uint32, np.uint32, "plus")
    kb, vb, wib, web = cached_case("equal", 3 * T8 + 5, np.int64, np.float64, "plus")
    a, b, c = Bufs(dr, ka, va), Bufs(dr, kb, vb), Bufs(dr, ka, va)
    n = ka.size
    s = np.flatnonzero(heads_of(ka))
    rk = dr.DeviceArray(0, n, np.uint32, host=np.zeros(n, np.uint32))
    rv = dr.DeviceArray(0, n, np.uint32, host=np.zeros(n, np.uint32))
    sel = dr.DeviceArray(0, n, np.uint32, host=np.zeros(n, np.uint32))
    cnt = dr.DeviceArray(0, 2, np.uint64, host=np.zeros(2, np.uint64))
    try:
        dr.inclusive_scan_by_key_async(0, ka.dtype, va.dtype, "plus", a.kin_ptr, a.vin_ptr, n, a.out_ptr)
        dr.reduce_by_key_async(0, ka.dtype, va.dtype, "plus", a.kin_ptr, a.vin_ptr, n, rk.ptr, rv.ptr, cnt.ptr)
        dr.exclusive_scan_by_key_async(0, kb.dtype, vb.dtype, "plus", b.kin_ptr, b.vin_ptr, kb.size, b.out_ptr, INIT["plus"])
        dr.copy_if_async(0, np.uint32, "lt", a.vin_ptr, sel.ptr, n, 1 << 31, cnt.ptr + 8)
        dr.exclusive_scan_by_key_async(0, ka.dtype, va.dtype, "plus", c.kin_ptr, c.vin_ptr, n, c.out_ptr, INIT["plus"])
        check_out(a, wia, "inclusive")
        check_out(b, web, "exclusive after reduce_by_key")
        check_out(c, wea, "exclusive after copy_if")
        runs, kept = (int(x) for x in cnt.numpy())
        assert runs == s.size
        with np.errstate(over="ignore"):
            assert np.array_equal(rv.numpy()[:runs], np.add.reduceat(va, s, dtype=va.dtype))
        assert np.array_equal(sel.numpy()[:kept], va[va < (1 << 31)])
    finally:
        for t in (a, b, c, rk, rv, sel, cnt):
            t.free()


def test_blocking_conveniences(dr):
    n = T8 + 104  # a multiple of 10
    k = (np.arange(n) // 10).astype(np.int64)
    v = np.ones(n, np.float64)
    kin = dr.DeviceArray(0, n, np.int64, host=k)
    vin = dr.DeviceArray(0, n, np.float64, host=v)
    out = dr.DeviceArray(0, n + 1, np.float64, host=np.full(n + 1, -1.0))
    try:
        dr.inclusive_scan_by_key(0, kin.ptr, vin.ptr, n, np.int64, np.float64, out.ptr)
        assert np.array_equal(out.numpy(), np.concatenate([np.arange(n) % 10 + 1.0, [-1.0]]))
        dr.exclusive_scan_by_key(0, kin.ptr, vin.ptr, n, np.int64, np.float64, out.ptr)  # the rank inside the group
        assert np.array_equal(out.numpy(), np.concatenate([np.arange(n) % 10 + 0.0, [-1.0]]))
        dr.exclusive_scan_by_key(0, kin.ptr, vin.ptr, n, np.int64, np.float64, out.ptr, op="max", init=7.0)
        assert np.array_equal(out.numpy(), np.concatenate([np.full(n, 7.0), [-1.0]]))
    finally:
        for b in (kin, vin, out):
            b.free()
