"""hrs_decode_batch_crc_dev (device.decode_batch_crc): a repair batch with one
erasure pattern per stripe, and the CRC-32 of every repaired cell from the
same pass (Decoder.java:222-229, :645-655 per lost block).

Everything is bit-exact: repaired bytes against the oracle's decodeBulk on
NON-codeword rows (survivors and not-to-read as Decoder.fixErasedBlockImpl
builds them) or against decode_batch, which other tests pin to the oracle;
CRCs against zlib.crc32(bytes, start). Entries past a stripe's losses continue
over no bytes: they keep crc_in (0 without one), and their output rows keep
their fill."""
import os
import random
import zlib

import numpy as np
import pytest

from lambdafs_amd import (HipNativeReedSolomonCode, HipReedSolomonCode, HipSimpleRegeneratingCode, HipXORCode,
                          HrsError, TooManyErasedLocations, _lib, device)
from oracle import rs_oracle as C

pytestmark = pytest.mark.gpu

FILL = 0xEE
FUSED = "batch_decode_crc_kernel<"


def _patterns(rnd, S, n, E, losses):
    er = np.full((S, E), -1, dtype=np.int32)
    for s in range(S):
        e = sorted(rnd.sample(range(n), losses(s)))
        er[s, :len(e)] = e
    return er


def _lost(er, s):
    return [int(x) for x in er[s] if x >= 0]


def _decoder_sets(k, p, erased):
    n = k + p
    tr = C.locations_to_read(k, p, erased)
    return sorted(tr), [x for x in range(n) if x not in tr or x in erased]


def _oracle_rows(k, p, host, er, s):
    """The repaired rows of stripe s as the Decoder computes them."""
    n, L = k + p, host.shape[2]
    lost = _lost(er, s)
    tr, ntr = _decoder_sets(k, p, lost)
    reads = [np.zeros(L, np.uint8) if x in ntr else host[s, x] for x in range(n)]
    return C.decode_bulk5(k, p, reads, lost, tr, ntr)


def _random_stripes(torch, S, n, L, seed):
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    return torch.randint(0, 256, (S, n, L), dtype=torch.uint8, device="cuda:0", generator=g)


def _random_crcs(torch, S, E, seed):
    words = np.random.default_rng(seed).integers(0, 1 << 32, (S, E), dtype=np.uint32)
    return words, torch.from_numpy(words.view(np.int32).copy()).to("cuda:0")


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _want_crcs(out_host, er, start):
    """zlib over the present outputs, the start value for the absent ones."""
    S, E = er.shape
    want = np.zeros((S, E), np.uint32) if start is None else start.copy()
    for s in range(S):
        for t in range(len(_lost(er, s))):
            want[s, t] = zlib.crc32(out_host[s, t].tobytes(), int(want[s, t]))
    return want


def _check_vs_oracle(k, p, host, er, out_host, stripes=None):
    for s in (range(host.shape[0]) if stripes is None else stripes):
        lost = _lost(er, s)
        if lost:
            want = _oracle_rows(k, p, host, er, s)
            for t in range(len(lost)):
                assert np.array_equal(out_host[s, t], want[t]), (s, lost, t)
        assert (out_host[s, len(lost):] == FILL).all(), s  # rows past a stripe's losses untouched


def _capped(k, p):
    """Losses per stripe cycling 2, 1, 0, 3, 1, 2, 4, capped at p and at 3
    where 4 losses would read more than 8 survivors (the fused shapes)."""
    def losses(s):
        ne = min((2, 1, 0, 3, 1, 2, 4)[s % 7], p)
        return 3 if ne == 4 and k > 8 else ne
    return losses


@pytest.mark.parametrize("with_in", [True, False], ids=["crc_in", "fresh"])
@pytest.mark.parametrize("k,p", [(10, 4), (6, 3), (12, 4), (3, 2)])
def test_mixed_losses_fused_shapes(cuda, k, p, with_in):
    torch = cuda
    n, S, L, E = k + p, 24, 10 << 10, p
    code = HipReedSolomonCode(k, p, device=0)
    st = _random_stripes(torch, S, n, L, seed=k)
    er = _patterns(random.Random(k * 16 + p), S, n, E, _capped(k, p))
    out = torch.full((S, E, L), FILL, dtype=torch.uint8, device="cuda:0")
    start, cin = _random_crcs(torch, S, E, seed=p) if with_in else (None, None)
    crc = device.decode_batch_crc(code, st, er, out, crc_in=cin)
    assert code.lastKernel().startswith(FUSED), code.lastKernel()
    torch.cuda.synchronize()
    out_host = out.cpu().numpy()
    _check_vs_oracle(k, p, st.cpu().numpy(), er, out_host)
    assert crc.shape == (S, E) and crc.dtype == torch.int32
    assert np.array_equal(_u32(crc), _want_crcs(out_host, er, start))
    if with_in:
        assert np.array_equal(_u32(cin), start)  # crc_in is only read


def test_crc_out_may_be_crc_in(cuda):
    torch = cuda
    k, p, S, L, E = 10, 4, 24, 10 << 10, 4
    n = k + p
    code = HipReedSolomonCode(k, p, device=0)
    st = _random_stripes(torch, S, n, L, seed=3)
    er = _patterns(random.Random(3), S, n, E, _capped(k, p))
    out = torch.full((S, E, L), FILL, dtype=torch.uint8, device="cuda:0")
    _, cin = _random_crcs(torch, S, E, seed=5)
    apart = device.decode_batch_crc(code, st, er, out, crc_in=cin)
    both = cin.clone()
    got = device.decode_batch_crc(code, st, er, out, crc_in=both, crc_out=both)
    assert got is both and code.lastKernel().startswith(FUSED)
    assert torch.equal(both, apart)


@pytest.mark.parametrize("order", ["0", "1", "2", "32"])
def test_more_tasks_than_resident_waves(cuda, monkeypatch, order):
    """Every wave walks several windows of stripes with different loss counts
    (and lossless ones), under each window -> wave order."""
    torch = cuda
    assert "HRS_BLOCKS_PER_CU" not in os.environ and "HRS_BCRC_THREADS" not in os.environ
    monkeypatch.setenv("HRS_TASK_ORDER", order)
    k, p, L, E = 6, 3, 20 << 10, 2
    n, nwin = k + p, (20 << 10) // 2048
    waves = torch.cuda.get_device_properties(0).multi_processor_count * (768 // 64)
    S = -(-5 * waves // (2 * nwin))  # S * nwin >= 2.5 x the resident waves
    assert S * nwin >= 2.5 * waves
    code = HipReedSolomonCode(k, p, device=0)
    st = _random_stripes(torch, S, n, L, seed=9)
    rnd = random.Random(9)
    er = _patterns(rnd, S, n, E, lambda s: 0 if s % 7 == 6 else rnd.choice((1, 2)))
    ref = torch.full((S, E, L), FILL, dtype=torch.uint8, device="cuda:0")
    device.decode_batch(code, st, er, ref)
    out = torch.full((S, E, L), FILL, dtype=torch.uint8, device="cuda:0")
    start, cin = _random_crcs(torch, S, E, seed=11)
    crc = device.decode_batch_crc(code, st, er, out, crc_in=cin)
    assert code.lastKernel() == "batch_decode_crc_kernel<2, 8, 768>"
    assert torch.equal(out, ref)
    out_host = out.cpu().numpy()
    sample = random.Random(1).sample(range(S), 16)
    host = np.zeros((S, n, L), np.uint8)
    host[sample] = st[sample].cpu().numpy()
    _check_vs_oracle(k, p, host, er, out_host, stripes=sample)
    assert np.array_equal(_u32(crc), _want_crcs(out_host, er, start))


def _fixed(lists, E):
    er = np.full((len(lists), E), -1, dtype=np.int32)
    for s, e in enumerate(lists):
        er[s, :len(e)] = e
    return er


# name -> (k, p, L, byte offset of the stripes tensor, kernel mode, per-stripe losses)
FALLBACKS = {
    "ragged_len": (10, 4, 100007, 0, 0, [(5,), (0, 13), (), (2, 7, 11)] * 2),
    "stripes_offset_3": (10, 4, 4096, 3, 0, [(5,), (0, 13), (), (2, 7, 11)] * 2),
    "kernel_mode_1": (10, 4, 4096, 0, 1, [(5,), (0, 13), (), (2, 7, 11)] * 2),
    "kernel_mode_2": (10, 4, 4096, 0, 2, [(5,), (0, 13), (), (2, 7, 11)] * 2),
    "four_losses_ten_survivors": (10, 4, 4096, 0, 0, [(5,), (1, 4, 8, 12), (), (0, 13)] * 2),
    "rs_20_8_six_losses": (20, 8, 4096, 0, 0, [(0, 3, 8, 12, 19, 22), (4,), (), (1, 27)] * 2),
    "per_stripe_over_32_survivors": (40, 6, 4096, 0, 0, [(7,), (0, 20, 45), (), (1, 2, 3, 10, 30, 44)] * 2),
}


@pytest.mark.parametrize("name", list(FALLBACKS))
def test_two_pass_fallbacks(cuda, name):
    """Shapes the fused kernel does not take: the batch repair, then the CRC
    window pass over `out` and the masked fold; same bytes, same CRCs."""
    torch = cuda
    k, p, L, offset, mode, lists = FALLBACKS[name]
    n, S = k + p, len(lists)
    E = max(len(e) for e in lists)
    er = _fixed(lists, E)
    code = HipReedSolomonCode(k, p, device=0)
    code.setKernelMode(mode)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(L + k)
    flat = torch.randint(0, 256, (S * n * L + 16,), dtype=torch.uint8, device="cuda:0", generator=g)
    st = torch.as_strided(flat, (S, n, L), (n * L, L, 1), offset)
    assert st.data_ptr() % 16 == offset
    out = torch.full((S, E, L), FILL, dtype=torch.uint8, device="cuda:0")
    start, cin = _random_crcs(torch, S, E, seed=L)
    crc = device.decode_batch_crc(code, st, er, out, crc_in=cin)
    assert not code.lastKernel().startswith("batch_decode_crc"), code.lastKernel()
    out_host = out.cpu().numpy()
    _check_vs_oracle(k, p, st.cpu().numpy(), er, out_host)
    assert np.array_equal(_u32(crc), _want_crcs(out_host, er, start))
    fresh = device.decode_batch_crc(code, st, er, out)
    assert np.array_equal(_u32(fresh), _want_crcs(out_host, er, None))


def test_chaining_across_four_calls(cuda):
    """crc_out fed back as crc_in over four successive cells of every block:
    zlib chained over the four; the absent slots stay at their start value."""
    torch = cuda
    k, p, S, L, E = 10, 4, 12, 6 << 10, 3
    n = k + p
    code = HipReedSolomonCode(k, p, device=0)
    er = _patterns(random.Random(4), S, n, E, lambda s: (2, 0, 1, 3)[s % 4])
    start, crc = _random_crcs(torch, S, E, seed=8)
    want = start.copy()
    for call in range(4):
        st = _random_stripes(torch, S, n, L, seed=100 + call)
        out = torch.full((S, E, L), FILL, dtype=torch.uint8, device="cuda:0")
        crc = device.decode_batch_crc(code, st, er, out, crc_in=crc)
        assert code.lastKernel().startswith(FUSED)
        out_host = out.cpu().numpy()
        _check_vs_oracle(k, p, st.cpu().numpy(), er, out_host, stripes=range(0, S, 5))
        want = _want_crcs(out_host, er, want)
    assert np.array_equal(_u32(crc), want)
    absent = er < 0
    assert absent.any() and np.array_equal(_u32(crc)[absent], start[absent])


FAMILIES = {
    "nrs_10_4": (lambda: HipNativeReedSolomonCode(10, 4, device=0), 14, 4, (2, 1, 0, 3, 4)),
    "xor_10_1": (lambda: HipXORCode(10, 1, device=0), 11, 1, (1, 0, 1)),
    "src_10_6_2": (lambda: HipSimpleRegeneratingCode(10, 6, 2, device=0), 16, 2, (1, 0, 2, 1)),
}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_other_code_families(cuda, family):
    torch = cuda
    make, n, E, cycle = FAMILIES[family]
    S, L = 15, 6 << 10
    code = make()
    st = _random_stripes(torch, S, n, L, seed=n)
    er = _patterns(random.Random(n), S, n, E, lambda s: cycle[s % len(cycle)])
    ref = torch.full((S, E, L), FILL, dtype=torch.uint8, device="cuda:0")
    device.decode_batch(code, st, er, ref)
    out = torch.full((S, E, L), FILL, dtype=torch.uint8, device="cuda:0")
    start, cin = _random_crcs(torch, S, E, seed=n)
    crc = device.decode_batch_crc(code, st, er, out, crc_in=cin)
    assert torch.equal(out, ref)
    assert np.array_equal(_u32(crc), _want_crcs(out.cpu().numpy(), er, start))


def test_errors(cuda):
    torch = cuda
    k, p, S, L, E = 10, 4, 3, 4096, 5
    n = k + p
    code = HipReedSolomonCode(k, p, device=0)
    st = _random_stripes(torch, S, n, L, seed=1)
    out = torch.zeros((S, E, L), dtype=torch.uint8, device="cuda:0")
    er = _fixed([(5,), (), (0, 13)], E)
    good = torch.zeros((S, E), dtype=torch.int32, device="cuda:0")
    for bad in (torch.zeros((S, E + 1), dtype=torch.int32, device="cuda:0"),
                torch.zeros((S, E), dtype=torch.int64, device="cuda:0"),
                torch.zeros((E, S), dtype=torch.int32, device="cuda:0").t()):
        with pytest.raises(ValueError):
            device.decode_batch_crc(code, st, er, out, crc_in=bad)
        with pytest.raises(ValueError):
            device.decode_batch_crc(code, st, er, out, crc_in=good, crc_out=bad)
    too_many = _fixed([(0, 1, 2, 3, 4), (), ()], E)
    with pytest.raises(TooManyErasedLocations):
        device.decode_batch(code, st, too_many, out)
    with pytest.raises(TooManyErasedLocations):
        device.decode_batch_crc(code, st, too_many, out)
    words = torch.zeros(S * E + 1, dtype=torch.int32, device="cuda:0")
    with pytest.raises(HrsError) as ei:  # overlapping, but not the same array
        device.decode_batch_crc(code, st, er, out, crc_in=words[:-1].view(S, E), crc_out=words[1:].view(S, E))
    assert ei.value.status == _lib.HRS_EINVAL
    torch.cuda.synchronize()
    assert not words.any() and not out.any()  # refused before anything ran
    crc = device.decode_batch_crc(code, st, er, out)  # the handle stays usable
    assert np.array_equal(_u32(crc), _want_crcs(out.cpu().numpy(), er, None))
