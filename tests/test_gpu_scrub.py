"""GPU tests of stripe scrubbing (hrs_scrub_dev / hrs_scrub_batch_host): the
report of every stripe must equal, word for word, the one built on the host by
running the oracle's computeErrorLocations on every byte column."""
import random

import numpy as np
import pytest

from lambdafs_amd import HipReedSolomonCode, device
from oracle import rs_oracle as C

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
SHAPES = [(10, 4), (12, 4), (6, 3), (3, 2), (4, 1), (20, 8)]
LENGTHS = [1, 16, 2047, 2048, 2049, 4129]  # tail only, one window, window + tail, two windows + tail
S = 3


def _u32(t):
    return (t.cpu().numpy().astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)


def _expected(k, p, host):
    """Reports of host[S, n, L] by the oracle, column by column."""
    n = k + p
    rep = np.zeros((host.shape[0], 4 + n), dtype=np.uint32)
    rep[:, 2] = NONE
    for s in range(host.shape[0]):
        cols = host[s].T.tolist()
        for c, data in enumerate(cols):
            ok, found, _ = C.compute_error_locations(k, p, data)
            if ok and not found:
                continue
            rep[s, 0] += 1
            rep[s, 2] = min(int(rep[s, 2]), c)
            if not ok:
                rep[s, 1] += 1
            else:
                for l in found:
                    rep[s, 4 + l] += 1
    return rep


_cache = {}


def _stripes(k, p, L):
    """(corrupted host stripes [S, n, L], expected reports), built once per shape."""
    key = (k, p, L)
    if key in _cache:
        return _cache[key]
    n = k + p
    rng = np.random.default_rng(7919 * k + 31 * p + L)
    rnd = random.Random(7919 * k + 31 * p + L)
    host = np.zeros((S, n, L), dtype=np.uint8)
    for s in range(S):
        data = [rng.integers(0, 256, L, dtype=np.uint8) for _ in range(k)]
        par = C.encode_bulk(k, p, data)
        for r in range(p):
            host[s, r] = par[r]
        for c in range(k):
            host[s, p + c] = data[c]
    # stripe 0 stays clean
    # stripe 1: single and double errors at the window and lane edges
    cols = sorted({c for c in (0, 15, 16, 1023, 1024, 2047, 2048, L - 1) if c < L})
    edge = [0, p - 1, p, n - 1]
    for i, c in enumerate(cols):
        kind = i % 4
        if kind == 0:    # a one-bit flip
            host[1, edge[(i // 4) % 4], c] ^= 1 << (i % 8)
        elif kind == 1:  # two errors, first and last location
            host[1, 0, c] ^= rnd.randrange(1, 256)
            host[1, n - 1, c] ^= rnd.randrange(1, 256)
        elif kind == 2:  # an equal-value pair (S_0 = 0) across the parity / data border
            v = rnd.randrange(1, 256)
            host[1, p - 1, c] ^= v
            host[1, p, c] ^= v
        else:
            host[1, edge[(i // 4 + 3) % 4], c] ^= rnd.randrange(1, 256)
    # stripe 2: one whole row replaced, plus one 3-error column (the replaced
    # row's byte and two more), picked so that the oracle calls it unresolved
    # wherever three errors are past the code (p <= 4; at p = 8 three errors
    # resolve, so there a second column with p / 2 + 1 errors is the unresolved one)
    row = p + (k // 2)
    fresh = rng.integers(0, 256, L, dtype=np.uint8)
    host[2, row] = fresh
    others = [l for l in range(n) if l != row]

    def plant(extra, want_unresolved, taken):
        for _ in range(400):
            c = rnd.randrange(L)
            if c in taken:
                continue
            trial = host[2, :, c].copy()
            trial[row] ^= rnd.randrange(1, 256)  # surely differs from the clean byte or from `fresh`
            for l in rnd.sample(others, extra):
                trial[l] ^= rnd.randrange(1, 256)
            ok, _, _ = C.compute_error_locations(k, p, trial.tolist())
            if not want_unresolved or not ok:
                host[2, :, c] = trial
                return c
        raise AssertionError("no such column found")

    c3 = plant(2, p <= 4, set())
    if p > 4 and L > 1:
        plant(p // 2, True, {c3})
    want = _expected(k, p, host)
    _cache[key] = (host, want)
    return host, want


def _device_view(torch, host, shift=0):
    """host[S, n, L] as a view of a larger device tensor: stripe stride
    (n + 1) * pitch, row stride pitch (a multiple of 16), rows offset by `shift`."""
    s, n, L = host.shape
    pitch = ((L + shift + 15) // 16) * 16 + 16
    big = torch.zeros((s, n + 1, pitch), dtype=torch.uint8, device="cuda:0")
    view = big[:, :n, shift:shift + L]
    view.copy_(torch.from_numpy(host).to("cuda:0"))
    assert view.stride(0) != n * L
    return view


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("k,p", SHAPES)
def test_scrub_matches_oracle(cuda, k, p, L, mode):
    host, want = _stripes(k, p, L)
    assert not want[0, [0, 1, 3]].any() and want[0, 2] == NONE and not want[0, 4:].any()
    assert want[1, 0] >= 1
    assert want[2, 0] >= max(1, L - 40)  # the replaced row, bar bytes that came out equal by chance
    if p <= 4 or L > 1:  # the unresolved branch runs for every shape (p = 8 needs a second column)
        assert want[2, 1] >= 1
    code = HipReedSolomonCode(k, p, device=0)
    code.setKernelMode(mode)
    view = _device_view(cuda, host)
    got = _u32(device.scrub_stripes(code, view))
    print(f"RS({k},{p}) L={L} mode={mode}: kernel {code.lastKernel()}, stripe 2 report head {got[2, :4].tolist()}")
    assert got.tolist() == want.tolist()
    vector = mode == 0 and L >= 2048
    assert code.lastKernel() == (f"scrub_kernel<{p}>" if vector else f"scrub_bytewise_kernel<{p}>")
    rows = device.scrub_rows(code, [view[:, l, :] for l in range(k + p)])
    assert _u32(rows).tolist() == want.tolist()


@pytest.mark.parametrize("k,p,L", [(10, 4, 4129), (6, 3, 2049)])
def test_scrub_unaligned_rows(cuda, k, p, L):
    """Every row pointer offset by one byte: the byte-granular kernel, same reports."""
    host, want = _stripes(k, p, L)
    code = HipReedSolomonCode(k, p, device=0)
    view = _device_view(cuda, host, shift=1)
    assert view.data_ptr() % 16 == 1
    got = _u32(device.scrub_stripes(code, view))
    assert got.tolist() == want.tolist()
    assert code.lastKernel() == f"scrub_bytewise_kernel<{p}>"


@pytest.mark.parametrize("mode", [0, 2])
def test_scrub_widest_code_n255(cuda, mode):
    """RS(247,8), n = 255: the last entry of the kernels' row table and of the
    per-wave histogram (location 254 is blamed in stripe 1), one window + tail."""
    k, p, L = 247, 8, 2049
    host, want = _stripes(k, p, L)
    assert want[1, 4 + 254] >= 1 and want[2, 1] >= 1
    code = HipReedSolomonCode(k, p, device=0)
    code.setKernelMode(mode)
    got = _u32(device.scrub_stripes(code, _device_view(cuda, host)))
    assert got.tolist() == want.tolist()
    assert code.lastKernel() == ("scrub_kernel<8>" if mode == 0 else "scrub_bytewise_kernel<8>")


def test_scrub_report_stride_and_padding_words(cuda):
    """A report_stride above 4 + n: the words past 4 + n are not written."""
    from lambdafs_amd import _lib
    torch = cuda
    k, p, L = 6, 3, 2049
    n = k + p
    host, want = _stripes(k, p, L)
    code = HipReedSolomonCode(k, p, device=0)
    view = _device_view(torch, host)
    rep = torch.full((S, 4 + n + 3), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    rows = _lib.ptr_array([view.data_ptr() + l * view.stride(1) for l in range(n)])
    code._check(_lib.lib().hrs_scrub_dev(code._handle(), rows, view.stride(0), L, S, rep.data_ptr(), 4 + n + 3,
                                         torch.cuda.current_stream().cuda_stream))
    got = _u32(rep)
    assert got[:, :4 + n].tolist() == want.tolist()
    assert (got[:, 4 + n:] == 0x5A5A5A5A).all()


def test_scrub_clean_at_size(cuda):
    """RS(10,4), 1 MiB cells, 8 stripes: clean stripes give empty reports; one
    flipped byte in the last column of the last stripe is the only thing
    reported, by both kernels."""
    torch = cuda
    k, p, L, ns = 10, 4, 1 << 20, 8
    n = k + p
    code = HipReedSolomonCode(k, p, device=0)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(5)
    st = torch.randint(0, 256, (ns, n, L), dtype=torch.uint8, device="cuda:0", generator=g)
    device.encode_stripes(code, st)
    empty = np.zeros((ns, 4 + n), dtype=np.uint32)
    empty[:, 2] = NONE
    reports = {}
    for mode in (0, 2):
        code.setKernelMode(mode)
        assert _u32(device.scrub_stripes(code, st)).tolist() == empty.tolist()
    st[ns - 1, p + 3, L - 1] ^= 0x10
    want = empty.copy()
    want[ns - 1, [0, 2, 4 + p + 3]] = [1, L - 1, 1]
    for mode in (0, 2):
        code.setKernelMode(mode)
        reports[mode] = _u32(device.scrub_stripes(code, st))
        assert reports[mode].tolist() == want.tolist()
    assert (reports[0] == reports[2]).all()


def test_scrub_round_trip_repairs(cuda):
    """Silent corruption of up to two whole cells per stripe: scrub_stripes ->
    scrub_to_erased -> decode_batch gives back the original cells."""
    torch = cuda
    k, p, L, ns = 10, 4, 4096 + 100, 4
    n = k + p
    code = HipReedSolomonCode(k, p, device=0)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(9)
    st = torch.randint(0, 256, (ns, n, L), dtype=torch.uint8, device="cuda:0", generator=g)
    device.encode_stripes(code, st)
    orig = st.clone()
    lost = [[], [5], [0, 13], [3, 4]]
    for s, locs in enumerate(lost):
        for l in locs:
            st[s, l] = torch.randint(0, 256, (L,), dtype=torch.uint8, device="cuda:0", generator=g)
    reports = device.scrub_stripes(code, st)
    erased = device.scrub_to_erased(reports, p)
    assert erased.tolist() == [l + [-1] * (p - len(l)) for l in lost]
    out = torch.zeros((ns, p, L), dtype=torch.uint8, device="cuda:0")
    device.decode_batch(code, st, erased, out)
    torch.cuda.synchronize()
    for s, locs in enumerate(lost):
        for t, l in enumerate(locs):
            assert torch.equal(out[s, t], orig[s, l]), (s, l)


def test_scrub_batch_host_pinned_and_pageable(cuda):
    """hrs_scrub_batch_host from a pinned tensor (read in place) and from a
    numpy array (staged) gives the reports scrub_stripes gives on the device:
    RS(12,4), 256 KiB cells, 16 stripes."""
    torch = cuda
    k, p, L, ns = 12, 4, 256 << 10, 16
    n = k + p
    code = HipReedSolomonCode(k, p, device=0)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(11)
    st = torch.randint(0, 256, (ns, n, L), dtype=torch.uint8, device="cuda:0", generator=g)
    device.encode_stripes(code, st)
    st[3, 7] = torch.randint(0, 256, (L,), dtype=torch.uint8, device="cuda:0", generator=g)  # a whole cell
    st[9, 0, 12345] ^= 1
    st[9, 15, 12345] ^= 0x80
    st[15, 2, L - 1] ^= 0xFF
    want = _u32(device.scrub_stripes(code, st))
    assert want[3, 0] >= L - 2000 and want[9, :3].tolist() == [1, 0, 12345] and want[15, 4 + 2] == 1
    assert not want[0, [0, 1]].any() and want[0, 2] == NONE
    pinned = st.cpu().pin_memory()
    got = device.scrub_batch_host(code, pinned)
    assert got.dtype == np.uint32 and got.tolist() == want.tolist()
    assert code.lastHostPath() == "pinned"
    assert code.lastKernel() == f"scrub_kernel<{p}>"
    pageable = st.cpu().numpy().copy()
    got = device.scrub_batch_host(code, pageable)
    assert got.tolist() == want.tolist()
    assert code.lastHostPath() == "staged"


@pytest.mark.parametrize("duplex", ["0", "1"])
def test_scrub_batch_host_copy_engine(cuda, monkeypatch, duplex):
    """Zero copy switched off: the host-batch pipeline's copy-engine branches
    (H2D -> kernel, no D2H: the job has no output rows), pinned stripes DMA'd
    directly and pageable ones through staging, with the copies on the slot
    streams and on the two duplex streams. Chunks of 2 stripes, so the 3
    slots are reused. Same reports as on the device."""
    torch = cuda
    k, p, L, ns = 12, 4, (256 << 10) + 100, 16
    n = k + p
    code = HipReedSolomonCode(k, p, device=0)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(13)
    st = torch.randint(0, 256, (ns, n, L), dtype=torch.uint8, device="cuda:0", generator=g)
    device.encode_stripes(code, st)
    st[0, 1, 0] ^= 1
    st[5, 9] = torch.randint(0, 256, (L,), dtype=torch.uint8, device="cuda:0", generator=g)
    st[15, 15, L - 1] ^= 0x42
    want = _u32(device.scrub_stripes(code, st))
    assert want[0, :3].tolist() == [1, 0, 0] and want[5, 0] >= L - 2000 and want[15, :3].tolist() == [1, 0, L - 1]
    monkeypatch.setenv("HRS_ZEROCOPY", "0")
    monkeypatch.setenv("HRS_HBATCH_DUPLEX", duplex)
    monkeypatch.setenv("HRS_HBATCH_BYTES", str(2 * n * (L + 256)))
    for batch in (st.cpu().pin_memory(), st.cpu().numpy().copy()):
        got = device.scrub_batch_host(code, batch)
        assert got.tolist() == want.tolist()
        assert code.lastHostPath() == "copy_engine"
        assert code.lastKernel() == f"scrub_kernel<{p}>"
