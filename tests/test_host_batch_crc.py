"""Host-memory batches with block checksums (hrs_decode_batch_host_crc /
hrs_encode_batch_host_crc): the bytes of hrs_decode_batch_host /
hrs_encode_batch_host, plus the CRC-32 of every repaired cell / of all k + p
cells of every stripe, computed on the GPU while the chunks pass through it
(Encoder.java:408-450; Decoder.java:222-229, :645-655).

Bit-exact throughout: repaired bytes against the oracle's decodeBulk on
NON-codeword rows, parity against the oracle's encodeBulk and against
encode_batch_host, CRCs against zlib.crc32(bytes, start). Every test runs in
every transfer mode, pinned and pageable."""
import random
import zlib

import numpy as np
import pytest

from lambdafs_amd import HipReedSolomonCode, HrsError, TooManyErasedLocations, _lib, device
from oracle import rs_oracle as C

pytestmark = pytest.mark.gpu

FILL = 0xEE


@pytest.fixture(autouse=True, params=["zero_copy", "copy_engine", "duplex"])
def transfer_mode(request, monkeypatch):
    """Zero copy (the default: pinned batches in place, pageable ones through
    pinned staging), the copy engine (HRS_ZEROCOPY=0), and the copy engine with
    the directions on the shared copy-in / copy-out streams
    (HRS_HBATCH_DUPLEX=1; the CRC buffer is still written by the slot streams
    only)."""
    monkeypatch.delenv("HRS_HBATCH_DUPLEX", raising=False)
    monkeypatch.delenv("HRS_HOST_NT", raising=False)
    if request.param == "zero_copy":
        monkeypatch.delenv("HRS_ZEROCOPY", raising=False)
    else:
        monkeypatch.setenv("HRS_ZEROCOPY", "0")
        monkeypatch.setenv("HRS_HOST_NT", "auto")
        if request.param == "duplex":
            monkeypatch.setenv("HRS_HBATCH_DUPLEX", "1")
            monkeypatch.setenv("HRS_HOST_NT", "0")
    return request.param


def _path(mode, pinned):
    if mode != "zero_copy":
        return "copy_engine"
    return "pinned" if pinned else "staged"


def _alloc(torch, shape, pinned):
    if pinned:
        return torch.empty(shape, dtype=torch.uint8, pin_memory=True).numpy()
    return np.empty(shape, dtype=np.uint8)


def _patterns(rnd, S, n, max_e, dist):
    er = np.full((S, max_e), -1, dtype=np.int32)
    for s in range(S):
        e = sorted(rnd.sample(range(n), dist(s)))
        er[s, :len(e)] = e
    return er


def _decoder_sets(k, p, erased):
    n = k + p
    tr = C.locations_to_read(k, p, erased)
    return sorted(tr), [x for x in range(n) if x not in tr or x in erased]


def _check_repair(k, p, st, er, out, crc, start, stripes=None):
    """Every repaired cell vs the oracle, rows past a stripe's losses untouched,
    every CRC vs zlib (the start value for the absent ones)."""
    n, L = k + p, st.shape[2]
    S, E = er.shape
    want = np.zeros((S, E), np.uint32) if start is None else start.copy()
    for s in range(S):
        lost = [int(x) for x in er[s] if x >= 0]
        if lost and (stripes is None or s in stripes):
            tr, ntr = _decoder_sets(k, p, lost)
            reads = [np.zeros(L, np.uint8) if x in ntr else st[s, x] for x in range(n)]
            ref = C.decode_bulk5(k, p, reads, lost, tr, ntr)
            for t in range(len(lost)):
                assert (out[s, t] == ref[t]).all(), (s, lost, t)
        assert (out[s, len(lost):] == FILL).all(), s
        for t in range(len(lost)):
            want[s, t] = zlib.crc32(out[s, t].tobytes(), int(want[s, t]))
    assert crc.dtype == np.uint32 and crc.shape == (S, E)
    bad = np.argwhere(crc != want)
    assert bad.size == 0, (bad[:4].tolist(), [hex(int(crc[tuple(b)])) for b in bad[:4]])


def _random_words(shape, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, shape, dtype=np.uint32)


@pytest.mark.parametrize("pinned", [True, False], ids=["pinned", "pageable"])
@pytest.mark.parametrize("L", [64 << 10, (96 << 10) + 40])
def test_decode_rs124_mixed_losses(cuda, transfer_mode, pinned, L):
    torch = cuda
    k, p, S = 12, 4, 24
    n = k + p
    code = HipReedSolomonCode(k, p, device=0)
    st = _alloc(torch, (S, n, L), pinned)
    st[:] = np.random.default_rng(L + pinned).integers(0, 256, (S, n, L), dtype=np.uint8)
    er = _patterns(random.Random(L), S, n, 4, lambda s: (2, 2, 2, 0, 1, 3, 4)[s % 7])
    out = _alloc(torch, (S, 4, L), pinned)
    out[:] = FILL
    start = _random_words((S, 4), seed=L)
    keep = start.copy()
    crc = device.decode_batch_host_crc(code, st, er, out, crc_in=start)
    assert code.lastHostPath() == _path(transfer_mode, pinned)
    assert np.array_equal(start, keep)  # crc_in is only read
    _check_repair(k, p, st, er, out, crc, start)
    # fresh CRCs, and crc_out given (and aliasing crc_in)
    out[:] = FILL
    _check_repair(k, p, st, er, out, device.decode_batch_host_crc(code, st, er, out), None, stripes=())
    both = start.copy()
    out[:] = FILL
    assert device.decode_batch_host_crc(code, st, er, out, crc_in=both, crc_out=both) is both
    assert np.array_equal(both, crc)


def _check_encode(k, p, st, data, crc, start):
    S, n = st.shape[0], k + p
    assert np.array_equal(st[:, p:], data)  # data rows unchanged
    want = np.zeros((S, n), np.uint32) if start is None else start.copy()
    for s in range(S):
        for r in range(n):  # CRC order: data rows 0..k-1 (locations p..n-1), then parity 0..p-1
            row = st[s, p + r] if r < k else st[s, r - k]
            want[s, r] = zlib.crc32(row.tobytes(), int(want[s, r]))
    assert crc.dtype == np.uint32 and np.array_equal(crc, want)


@pytest.mark.parametrize("pinned", [True, False], ids=["pinned", "pageable"])
@pytest.mark.parametrize("k,p,L", [(10, 4, 64 << 10), (10, 4, (32 << 10) + 24), (9, 3, 32 << 10)])
def test_encode_crc(cuda, transfer_mode, pinned, k, p, L):
    """RS(10,4) on whole 2 KiB windows takes the fused encode + CRC kernel,
    a ragged length and RS(9,3) (no static kernel) two passes."""
    torch = cuda
    S, n = 12, k + p
    code = HipReedSolomonCode(k, p, device=0)
    data = np.random.default_rng(L + k).integers(0, 256, (S, k, L), dtype=np.uint8)
    ref = _alloc(torch, (S, n, L), pinned)
    ref[:, :p] = 0x5A
    ref[:, p:] = data
    device.encode_batch_host(code, ref)
    for s in range(0, S, 5):
        par = C.encode_bulk(k, p, [data[s, c] for c in range(k)])
        assert all((ref[s, r] == par[r]).all() for r in range(p)), s
    st = _alloc(torch, (S, n, L), pinned)
    st[:, :p] = 0x5A
    st[:, p:] = data
    start = _random_words((S, n), seed=L)
    crc = device.encode_batch_host_crc(code, st, crc_in=start)
    assert code.lastHostPath() == _path(transfer_mode, pinned)
    if (k, p) == (10, 4) and L % 2048 == 0 and transfer_mode == "zero_copy":
        assert code.lastKernel().startswith("encode_crc_grouped_kernel"), code.lastKernel()
    if (k, p) == (9, 3) or L % 2048:
        assert not code.lastKernel().startswith("encode_crc"), code.lastKernel()
    assert np.array_equal(st, ref)  # parity equals encode_batch_host's, nothing else moved
    _check_encode(k, p, st, data, crc, start)
    _check_encode(k, p, st, data, device.encode_batch_host_crc(code, st), None)


def test_many_chunks_through_the_slot_ring(cuda, monkeypatch):
    """A small HRS_HBATCH_BYTES: >= 7 chunks over the 3 slots on pageable
    memory, so the raw scratch, the slots and the CRC buffer are reused while
    earlier chunks are still in flight; the last chunk is a short one."""
    k, p, S, L = 10, 4, 22, 16 << 10
    n = k + p
    dpitch = (L + 255) & ~255
    monkeypatch.setenv("HRS_HBATCH_BYTES", str(3 * n * dpitch))  # 3 stripes per chunk: 8 chunks
    code = HipReedSolomonCode(k, p, device=0)
    st = np.random.default_rng(5).integers(0, 256, (S, n, L), dtype=np.uint8)
    er = _patterns(random.Random(5), S, n, 4, lambda s: (1, 3, 0, 2, 2)[s % 5])
    out = np.full((S, 4, L), FILL, np.uint8)
    start = _random_words((S, 4), seed=6)
    crc = device.decode_batch_host_crc(code, st, er, out, crc_in=start)
    _check_repair(k, p, st, er, out, crc, start, stripes=set(range(0, S, 3)))
    ref = np.full((S, 4, L), FILL, np.uint8)
    device.decode_batch_host(code, st, er, ref)
    assert np.array_equal(out, ref)
    data = st[:, p:].copy()
    enc = st.copy()
    device.encode_batch_host(code, enc)
    start = _random_words((S, n), seed=7)
    crc = device.encode_batch_host_crc(code, st, crc_in=start)
    assert np.array_equal(st, enc)
    _check_encode(k, p, st, data, crc, start)


@pytest.mark.parametrize("blocks", ["1", "3"])
def test_many_tasks_per_wave(cuda, monkeypatch, blocks):
    """Pinned, HRS_ZC_BLOCKS 1 and 3: one block walks >= 16 windows per wave
    across stripes with different loss counts (200 windows over 12 or 36 waves)."""
    torch = cuda
    monkeypatch.setenv("HRS_ZC_BLOCKS", blocks)
    k, p, S, L = 10, 4, 40, 10 << 10
    n = k + p
    code = HipReedSolomonCode(k, p, device=0)
    st = _alloc(torch, (S, n, L), True)
    st[:] = np.random.default_rng(int(blocks)).integers(0, 256, (S, n, L), dtype=np.uint8)
    er = _patterns(random.Random(8), S, n, 3, lambda s: (2, 1, 0, 3, 1)[s % 5])
    out = _alloc(torch, (S, 3, L), True)
    out[:] = FILL
    start = _random_words((S, 3), seed=9)
    crc = device.decode_batch_host_crc(code, st, er, out, crc_in=start)
    _check_repair(k, p, st, er, out, crc, start)


def test_interior_pinned_views(cuda):
    """Views that start inside larger pinned allocations, the stripes with a
    non-contiguous stripe stride (every second stripe of the allocation)."""
    torch = cuda
    k, p, S, L = 10, 4, 10, 32 << 10
    n = k + p
    code = HipReedSolomonCode(k, p, device=0)
    big = torch.empty((2 * S + 5, n, L), dtype=torch.uint8, pin_memory=True).numpy()
    big[:] = 0x77
    st = big[5::2]
    assert st.shape[0] == S and st.strides[0] == 2 * n * L
    st[:] = np.random.default_rng(12).integers(0, 256, (S, n, L), dtype=np.uint8)
    outbig = torch.empty((S + 3, 2, L), dtype=torch.uint8, pin_memory=True).numpy()
    out = outbig[3:]
    out[:] = FILL
    er = _patterns(random.Random(12), S, n, 2, lambda s: s % 3)
    start = _random_words((S, 2), seed=13)
    crc = device.decode_batch_host_crc(code, st, er, out, crc_in=start)
    _check_repair(k, p, st, er, out, crc, start)
    data = st[:, p:].copy()
    crc = device.encode_batch_host_crc(code, st)
    for s in range(S):
        par = C.encode_bulk(k, p, [data[s, c] for c in range(k)])
        assert all((st[s, r] == par[r]).all() for r in range(p)), s
    _check_encode(k, p, st, data, crc, None)
    assert (big[6::2] == 0x77).all() and (big[:5] == 0x77).all()  # the stripes between and before: untouched


@pytest.mark.parametrize("pinned", [True, False], ids=["pinned", "pageable"])
def test_errors_leave_the_handle_usable(cuda, pinned):
    torch = cuda
    k, p, S, L, E = 10, 4, 4, 8192, 5
    n = k + p
    code = HipReedSolomonCode(k, p, device=0)
    lib, h = _lib.lib(), code._handle()
    st = _alloc(torch, (S, n, L), pinned)
    st[:] = np.random.default_rng(2).integers(0, 256, (S, n, L), dtype=np.uint8)
    out = _alloc(torch, (S, E, L), pinned)
    out[:] = FILL
    er = _patterns(random.Random(2), S, n, E, lambda s: (2, 0, 1, 4)[s])
    dec = (h, st.ctypes.data, L, n * L, er.ctypes.data, E, out.ctypes.data, L, E * L, L, S)
    words = np.zeros(S * n + 1, np.uint32)
    base = words.ctypes.data
    assert lib.hrs_decode_batch_host_crc(*dec, None, None) == _lib.HRS_EINVAL
    assert lib.hrs_encode_batch_host_crc(h, st.ctypes.data, L, n * L, L, S, None, None) == _lib.HRS_EINVAL
    assert lib.hrs_decode_batch_host_crc(*dec, base, base + 4) == _lib.HRS_EINVAL
    assert lib.hrs_encode_batch_host_crc(h, st.ctypes.data, L, n * L, L, S, base + 4, base) == _lib.HRS_EINVAL
    too_many = er.copy()
    too_many[1] = [0, 1, 2, 3, 4]
    with pytest.raises(TooManyErasedLocations):
        device.decode_batch_host_crc(code, st, too_many, out)
    with pytest.raises(HrsError):
        device.decode_batch_host_crc(code, st, np.full((S, E), 20, np.int32), out)
    assert not words.any() and (out == FILL).all()  # every refusal came before any work
    start = _random_words((S, E), seed=3)
    crc = device.decode_batch_host_crc(code, st, er, out, crc_in=start)
    _check_repair(k, p, st, er, out, crc, start)
