"""Exact GPU parity of drhip_reduce / drhip_dot (csrc/reduce.hip) where
test_gpu_reduce.py cannot look: the float-only code on inputs whose fold is
exact in any order (the result IS the integer fold, so one skipped, repeated
or misplaced element fails -- rtol 1e-5 on U[0,1) sums cannot see it), the
capped grid, the dot's int64 / uint32 / uint64 instantiations with wrapping
products, and a per-position check that the dot reads every element once.

Inputs and their exactness bounds: test_reference_helpers.py."""
import numpy as np
import pytest

from test_gpu_reduce import DTYPES, OPS, check_value, make_input
from test_reference_helpers import CAPPED_N, REDUCE_CASES, exact_dot_inputs, exact_floats, exact_fold

pytestmark = pytest.mark.gpu

IDENT = {"plus": 0.0, "mul": 1.0, "min": np.inf, "max": -np.inf}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("n,offset", REDUCE_CASES)  # the sizes and offsets of test_reduce_parity
def test_reduce_exact_floats(dr, dtype, op, n, offset):
    """The fp32 compute / fp64 accumulator split and the fp32 products in
    fp64, which the bit-exact integer instantiations do not share."""
    x = exact_floats(dtype, op, n + offset, seed=n * 7 + offset)
    buf = dr.DeviceArray(0, n + offset, dtype, host=x)
    got = dr.reduce(0, buf.at(offset), n, dtype, op)
    buf.free()
    want = exact_fold(x[offset:], op) if n else IDENT[op]
    assert got == want, (got, want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", OPS)
def test_reduce_capped_grid(dr, oracle, dtype, op):
    """CAPPED_N = 2^23 + 5 elements at element offsets 0 and 3 (derived next to
    its definition): the grid is capped at 2 x CUs blocks, every block runs
    the remainder loop after its unrolled iterations, and the last-block
    count has 16 full groups.  Integers bit-exact against the oracle, floats
    on exact inputs."""
    n = CAPPED_N
    dt = np.dtype(dtype)
    if dt.kind == "f":
        x = exact_floats(dtype, op, n + 3, seed=len(op))
    else:
        x = make_input(dtype, op, n + 3, seed=len(op))
        if op == "mul":
            x |= 1  # odd factors: the wrapped product never collapses to 0, so every factor counts
    buf = dr.DeviceArray(0, n + 3, dtype, host=x)
    got = [dr.reduce(0, buf.at(off), n, dtype, op) for off in (0, 3)]
    planted = []
    if op in ("min", "max"):
        # a min / max sees one element only when it is the extremum: plant it at the first and last
        # element, in the single remainder-loop vector of a middle block (block 200 of 512 folds vectors
        # [200 per, 201 per), per = ceil(nv / 512)) and in the last vector
        v = 16 // dt.itemsize
        nv = n // v
        per = -(-nv // 512)
        assert per % (256 * 8) == 1  # one vector left for the remainder loop (CAPPED_N's derivation)
        if dt.kind == "f":
            ext = dt.type(-2e6 if op == "min" else 2e6)
        else:
            ext = dt.type(np.iinfo(dt).min if op == "min" else np.iinfo(dt).max)
        for p in (0, n - 1, (200 * per + per - 1) * v + 1, (nv - 1) * v):
            dr.h2d(0, buf.at(p), np.array([ext], dt))
            planted.append((p, dr.reduce(0, buf.ptr, n, dtype, op)))
            dr.h2d(0, buf.at(p), x[p:p + 1])
    buf.free()
    for p, g in planted:
        assert g == ext, (p, g)
    for off, g in zip((0, 3), got):
        xs = x[off:off + n]
        if dt.kind == "f":
            assert g == exact_fold(xs, op), (off, g)
        else:
            ident = {"plus": 0, "mul": 1, "min": np.iinfo(dtype).max, "max": np.iinfo(dtype).min}[op]
            check_value(g, oracle.shp_reduce(xs, [n], ident, op), dtype)


def wrapping_dot(x, y):
    """sum x[i] * y[i] modulo 2^bits, in NumPy (the oracle's dot is int32 / float only)."""
    u = np.dtype("u%d" % x.dtype.itemsize)
    s = np.sum(x.view(u).astype(np.uint64) * y.view(u).astype(np.uint64), dtype=np.uint64)
    return np.array([s]).astype(u).view(x.dtype)[0]


def run_dot(dr, x, y, xo, yo, n):
    dt = x.dtype
    bx = dr.DeviceArray(0, x.size, dt, host=x)
    by = dr.DeviceArray(0, y.size, dt, host=y)
    out = dr.DeviceArray(0, 1, np.float64 if dt.kind == "f" else dt)
    dr.dot_async(0, dt, bx.at(xo), by.at(yo), n, out.ptr)
    got = out.numpy()[0]
    for b in (bx, by, out):
        b.free()
    return got


@pytest.mark.parametrize("dtype", [np.int64, np.uint32, np.uint64])
# the layouts of test_dot_parity (y shares x's alignment), then those of test_dot_shifted_operands
@pytest.mark.parametrize("n,xo,yo", [(0, 0, 0), (5, 1, 1), (4099, 0, 0), (1 << 20, 0, 0), (300001, 2, 2),
                                     (7, 1, 0), (4099, 0, 1), (300001, 1, 2), ((1 << 22) + 3, 1, 0)])
def test_dot_wrapping_integers(dr, dtype, n, xo, yo):
    """The three dot instantiations the oracle-based tests leave out, on
    full-range values: the products and their sum wrap."""
    x, y = make_input(dtype, "plus", n + 3, n + 17), make_input(dtype, "plus", n + 3, n + 18)
    got = run_dot(dr, x, y, xo, yo, n)
    assert int(got) == int(wrapping_dot(x[xo:xo + n], y[yo:yo + n]))


DOT_LAYOUTS = [(0, 0, 0), (5, 1, 1), (4099, 0, 0), (1 << 20, 0, 0), (300001, 2, 2),  # y shares x's alignment
               (7, 1, 0), (4099, 0, 1), (300001, 1, 2), ((1 << 22) + 3, 1, 0),       # y shifted: element loads
               # just past the grid cap (513 chunks of 2048 vectors for f32, 512 blocks)
               ((1 << 22) + (1 << 12) + 3, 0, 0), ((1 << 22) + (1 << 12) + 3, 1, 0)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,xo,yo", DOT_LAYOUTS)
def test_dot_exact_floats(dr, dtype, n, xo, yo):
    """Values in {-2..2}: the fp64-accumulated dot equals the integer dot."""
    x, y = exact_dot_inputs(dtype, n + 3, seed=n + xo)
    got = run_dot(dr, x, y, xo, yo, n)
    want = int(np.sum(x[xo:xo + n].astype(np.int64) * y[yo:yo + n].astype(np.int64)))
    assert got == want, (got, want)


@pytest.mark.parametrize("dtype", [np.float32, np.int64])
@pytest.mark.parametrize("xo,yo", [(0, 0), (1, 0)])  # dot_stage1<T, true> / <T, false>
def test_dot_reads_every_position_once(dr, dtype, xo, yo):
    """x[p] += 1 moves the dot by exactly y[p], at the first and last element,
    the last vector slot, the first scalar-tail slot and one mid-block."""
    n = (1 << 22) + (1 << 12) + 3 - xo  # past the grid cap; leaves a scalar tail after x's vector slots
    v = 16 // np.dtype(dtype).itemsize
    x, y = exact_dot_inputs(dtype, n + 3, seed=3)
    head = min((-xo) % v, n)
    nv = (n - head) // v
    assert head + nv * v < n  # there is a scalar tail
    pos = [0, n - 1, head + nv * v - 1, head + nv * v, n // 2 + 1]
    y[[yo + p for p in pos]] = [2, -2, 1, 2, -1]
    acc = np.float64 if np.dtype(dtype).kind == "f" else dtype
    bx = dr.DeviceArray(0, n + 3, dtype, host=x)
    by = dr.DeviceArray(0, n + 3, dtype, host=y)
    out = dr.DeviceArray(0, 1, acc)

    def dot():
        dr.dot_async(0, dtype, bx.at(xo), by.at(yo), n, out.ptr)
        return int(out.numpy()[0])

    base = dot()
    moved = []
    for p in pos:
        dr.h2d(0, bx.at(xo + p), x[xo + p:xo + p + 1] + 1)
        moved.append(dot() - base)
        dr.h2d(0, bx.at(xo + p), x[xo + p:xo + p + 1])
    again = dot()
    for b in (bx, by, out):
        b.free()
    assert base == int(np.sum(x[xo:xo + n].astype(np.int64) * y[yo:yo + n].astype(np.int64)))
    assert moved == [int(y[yo + p]) for p in pos] and again == base
