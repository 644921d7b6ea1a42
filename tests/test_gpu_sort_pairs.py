"""GPU tests of the by-key sort (drhip_sort_pairs, drhip_merge_pairs_runs_to)
on one segment.  The oracle has no by-key sort: the expected result is
numpy's stable argsort.  Values are arange(n) as u32 / u64, so the returned
values must BE the stable argsort, bit for bit, and the keys keys[argsort].
Inputs avoid NaN and -0.0 (as tests/test_gpu_sort.py)."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_sort import DTYPES, make_keys  # the keys-only tests' key patterns ("few": 5 distinct keys)

pytestmark = pytest.mark.gpu

VTYPES = {4: np.uint32, 8: np.uint64}
ENV_KEYS = ["DRHIP_SORT_ALGO", "DRHIP_SORT_RANK", "DRHIP_SORT_OS_SHAPE", "DRHIP_SORT_STATUS", "DRHIP_SORT_OS_PT"]


@pytest.fixture(params=["atomic-or-probed", "ballot"])
def rank(request, monkeypatch):
    """Both ranking paths: the device's own choice and the forced ballot ranking."""
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    if request.param == "ballot":
        monkeypatch.setenv("DRHIP_SORT_RANK", "ballot")
    return request.param


def run_pairs(dr, keys, val_bytes):
    n = keys.size
    vals = np.arange(n, dtype=VTYPES[val_bytes])
    kb = dr.DeviceArray(0, max(n, 1), keys.dtype, host=keys if n else np.zeros(1, keys.dtype))
    vb = dr.DeviceArray(0, max(n, 1), vals.dtype, host=vals if n else np.zeros(1, vals.dtype))
    ws = dr.sort_pairs_workspace(0, keys.dtype, val_bytes, n)
    tmp = dr.DeviceArray(0, max(ws, 16), np.uint8)
    try:
        dr.sort_pairs_async(0, keys.dtype, kb.ptr, vb.ptr, val_bytes, n, tmp.ptr, ws)
        return kb.numpy()[:n], vb.numpy()[:n]
    finally:
        for b in (kb, vb, tmp):
            b.free()


def check_pairs(dr, keys, val_bytes):
    gk, gv = run_pairs(dr, keys, val_bytes)
    order = np.argsort(keys, kind="stable")
    assert np.array_equal(gv, order.astype(VTYPES[val_bytes]))
    assert np.array_equal(gk.view(np.uint8), keys[order].view(np.uint8))
    return gv


@pytest.mark.parametrize("val_bytes", [4, 8])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [65537, (1 << 20) + 13])
def test_sort_pairs_many_blocks(dr, rank, dtype, val_bytes, n):
    check_pairs(dr, make_keys(dtype, n, "random", seed=n + val_bytes), val_bytes)


# sub-tile and chunk edges of the small block shape: 4096 / 16384 keys at
# 4-byte keys, 2048 / 8192 at 8-byte keys
EDGES4 = [0, 1, 2, 63, 100, 4095, 4096, 4097, 16383, 16384, 16385]
EDGES8 = [0, 1, 2, 63, 100, 2047, 2048, 2049, 8191, 8192, 8193]


@pytest.mark.parametrize("val_bytes", [4, 8])
@pytest.mark.parametrize("dtype,n", [(d, n) for d in (np.uint32, np.float32) for n in EDGES4] +
                         [(np.int64, n) for n in EDGES8])
def test_sort_pairs_edge_sizes(dr, rank, dtype, val_bytes, n):
    check_pairs(dr, make_keys(dtype, n, "random", seed=3 * n + 1), val_bytes)
    if n > 2:  # the same edge with ties in every wave
        check_pairs(dr, make_keys(dtype, n, "few", seed=n), val_bytes)


@pytest.mark.parametrize("val_bytes", [4, 8])
@pytest.mark.parametrize("dtype", [np.uint32, np.float32, np.int64])
@pytest.mark.parametrize("kind", ["few", "const", "small16", "sorted", "reversed"])
def test_sort_pairs_patterns(dr, rank, dtype, val_bytes, kind):
    n = 300001
    gv = check_pairs(dr, make_keys(dtype, n, kind, seed=7), val_bytes)
    if kind == "const":
        assert np.array_equal(gv, np.arange(n, dtype=VTYPES[val_bytes]))


@pytest.mark.parametrize("dtype", [np.uint32, np.int64])
def test_sort_pairs_ignores_sort_algo(dr, monkeypatch, dtype):
    """DRHIP_SORT_ALGO picks the keys-only path; pairs take the classic pass whatever it says."""
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    keys = make_keys(dtype, (1 << 18) + 5, "few", seed=5)
    base = run_pairs(dr, keys, 8)
    monkeypatch.setenv("DRHIP_SORT_ALGO", "onesweep")
    forced = run_pairs(dr, keys, 8)
    assert np.array_equal(base[0], forced[0]) and np.array_equal(base[1], forced[1])
    check_pairs(dr, keys, 8)


@pytest.mark.parametrize("val_bytes", [4, 8])
@pytest.mark.parametrize("dtype", [np.uint32, np.float32, np.int64])
@pytest.mark.parametrize("offset", [1, 2, 3])
@pytest.mark.parametrize("n", [5, 70001])
def test_sort_pairs_misaligned_subrange(dr, rank, dtype, val_bytes, offset, n):
    """Keys and values start `offset` elements into their buffers; everything outside stays untouched."""
    vt = VTYPES[val_bytes]
    keys = make_keys(dtype, n + 2 * offset, "few" if n > 5 else "random", seed=n + offset)
    vals = np.arange(1000, 1000 + n + 2 * offset, dtype=vt)
    kb = dr.DeviceArray(0, keys.size, keys.dtype, host=keys)
    vb = dr.DeviceArray(0, vals.size, vt, host=vals)
    ws = dr.sort_pairs_workspace(0, dtype, val_bytes, n)
    tmp = dr.DeviceArray(0, max(ws, 16), np.uint8)
    try:
        dr.sort_pairs_async(0, dtype, kb.at(offset), vb.at(offset), val_bytes, n, tmp.ptr, ws)
        gk, gv = kb.numpy(), vb.numpy()
    finally:
        for b in (kb, vb, tmp):
            b.free()
    order = np.argsort(keys[offset:offset + n], kind="stable")
    wk, wv = keys.copy(), vals.copy()
    wk[offset:offset + n] = keys[offset:offset + n][order]
    wv[offset:offset + n] = vals[offset:offset + n][order]
    assert np.array_equal(gv, wv)
    assert np.array_equal(gk.view(np.uint8), wk.view(np.uint8))


MERGE_SIZES = [[1000], [5, 7], [0, 3000, 0], [2048, 2048, 2047, 1], [100000] * 8,
               [1, 0, 2, 0, 3, 0, 4, 5000, 9, 77777, 3, 4096, 0, 1, 2, 3, 65536]]


@pytest.mark.parametrize("val_bytes", [4, 8])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["few", "random"])
@pytest.mark.parametrize("sizes", MERGE_SIZES)
@pytest.mark.parametrize("dst_shift", [0, 1])
def test_merge_pairs_runs_to(dr, dtype, val_bytes, kind, sizes, dst_shift):
    """Sorted runs with their values (the position in the concatenation) merged into a
    separate, possibly misaligned destination: the stable argsort, src unchanged,
    nothing written around dst."""
    vt = VTYPES[val_bytes]
    runs = [np.sort(make_keys(dtype, s, kind, seed=31 + i)) for i, s in enumerate(sizes)]
    x = np.concatenate(runs)
    n = x.size
    v = np.arange(n, dtype=vt)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    ksent = make_keys(dtype, n + 2, "random", seed=5)
    vsent = np.arange(7000, 7000 + n + 2, dtype=vt)
    bufs = [dr.DeviceArray(0, n, x.dtype, host=x), dr.DeviceArray(0, n, vt, host=v),
            dr.DeviceArray(0, n + 2, x.dtype, host=ksent), dr.DeviceArray(0, n + 2, vt, host=vsent)]
    ws = dr.merge_pairs_workspace(0, dtype, val_bytes, n, len(sizes))
    bufs.append(dr.DeviceArray(0, max(ws, 16), np.uint8))
    sk, sv, dk, dv, tmp = bufs
    try:
        dr.merge_pairs_runs_to(0, dtype, val_bytes, sk.ptr, sv.ptr, dk.at(dst_shift), dv.at(dst_shift), n, offs,
                               tmp.ptr, ws)
        gk, gv, hk, hv = dk.numpy(), dv.numpy(), sk.numpy(), sv.numpy()
    finally:
        for b in bufs:
            b.free()
    order = np.argsort(x, kind="stable")
    assert np.array_equal(gv[dst_shift:dst_shift + n], order.astype(vt))
    assert np.array_equal(gk[dst_shift:dst_shift + n].view(np.uint8), x[order].view(np.uint8))
    outside = np.r_[0:dst_shift, dst_shift + n:n + 2]
    assert np.array_equal(gk[outside].view(np.uint8), ksent[outside].view(np.uint8))
    assert np.array_equal(gv[outside], vsent[outside])
    assert np.array_equal(hk.view(np.uint8), x.view(np.uint8)) and np.array_equal(hv, v)


def test_sort_pairs_refusals(dr):
    """val_bytes = 2, a short workspace and null vals with n > 1: DRHIP_ERR_BAD_ARG, buffers unchanged."""
    L = dr.load()
    n = 5000
    keys = make_keys(np.uint32, n, "random", seed=1)
    vals = np.arange(n, dtype=np.uint32)
    kb = dr.DeviceArray(0, n, np.uint32, host=keys)
    vb = dr.DeviceArray(0, n, np.uint32, host=vals)
    ws = dr.sort_pairs_workspace(0, np.uint32, 4, n)
    tmp = dr.DeviceArray(0, ws, np.uint8)
    try:
        assert L.drhip_sort_pairs(0, dr.U32, kb.ptr, vb.ptr, 2, n, tmp.ptr, ws) == 4
        assert L.drhip_sort_pairs(0, dr.U32, kb.ptr, vb.ptr, 4, n, tmp.ptr, ws - 256) == 4
        assert L.drhip_sort_pairs(0, dr.U32, kb.ptr, None, 4, n, tmp.ptr, ws) == 4
        offs = (C.c_size_t * 2)(0, n)
        assert L.drhip_merge_pairs_runs_to(0, dr.U32, 2, kb.ptr, vb.ptr, tmp.ptr, tmp.ptr, n, offs, 1, tmp.ptr,
                                           ws) == 4
        dr.sync()
        assert np.array_equal(kb.numpy(), keys) and np.array_equal(vb.numpy(), vals)
        # n <= 1 needs no buffers at all
        assert L.drhip_sort_pairs(0, dr.U32, None, None, 4, 1, None, 0) == 0
        assert L.drhip_sort_pairs(0, dr.U32, None, None, 8, 0, None, 0) == 0
    finally:
        for b in (kb, vb, tmp):
            b.free()
