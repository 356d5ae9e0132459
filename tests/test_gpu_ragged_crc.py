"""hrs_encode_ragged_crc_dev on the GPU: parity against the oracle's encodeBulk
over zero-filled cells and all k + p CRCs of every stripe against zlib over
the zero-filled data cells and the oracle's parity rows, exact, for every code
kind (the six static shapes, then rs (5,3), xor (4,1) and an src layout), at
whole 2 KiB windows and windows plus an 80-byte tail, every valid class at
every row position and the file-tail stripes (ragged_inputs.class_batch),
through the C ABI and the Python mirror, chained from a seeded non-zero crc_in
in half of the cases. Routing by hrs_last_kernel: the fused kernel for the
static shapes at whole windows in modes 0 and 3, the ragged encode's kernels
otherwise (modes 1 and 2: two passes, equal bytes and CRCs); an all-full batch
names the plain hrs_encode_crc_dev kernel in mode 0 and the ragged one in mode
3; one entry one byte short takes the ragged route; crc_out may be crc_in."""
import numpy as np
import pytest

from lambdafs_amd import device
from ragged_crc_inputs import (abi_call_dev, crc_mismatch, dev_words, expected_crcs, fused_kernel, route_kernel,
                               seeded_crc_in)
from ragged_inputs import (BYTEWISE, RUNTIME, STATIC, class_batch, code_id, expected, full_batch, make_code, mismatch,
                           vector_kernel)

pytestmark = pytest.mark.gpu

LENGTHS = [4096, 4096 + 80]
_crcs = {}


def _want_crcs(key, p, stripes, valid, want, crc_in):
    """Reference CRCs, computed once per (batch, chaining) and shared."""
    key = (key, crc_in is not None)
    if key not in _crcs:
        _crcs[key] = expected_crcs(p, stripes, valid, want, crc_in)
    return _crcs[key]


def _run(torch, code, stripes, valid, via, crc_in, alias=False):
    """(bytes, crcs [S, n] uint32, kernel) of one call on a fresh device copy."""
    t = torch.from_numpy(np.array(stripes)).to("cuda:0")
    S, n, _ = t.shape
    cin = None if crc_in is None else dev_words(torch, crc_in)
    if via == "abi":
        out = cin if alias else torch.full((S, n), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
        abi_call_dev(torch, code, t, np.array(valid), cin, out)
    else:
        out = device.encode_stripes_ragged_crc(code, t, valid, crc_in=cin)
    kernel = code.lastKernel()
    torch.cuda.synchronize()
    if cin is not None and not alias:
        assert (cin.cpu().numpy().view(np.uint32) == crc_in).all(), "crc_in was written"
    return t.cpu().numpy(), out.cpu().numpy().view(np.uint32), kernel


@pytest.mark.parametrize("via", ["abi", "mirror"])
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("cfg", STATIC + RUNTIME, ids=code_id)
def test_ragged_encode_crc_matches_the_oracle_and_zlib(cuda, cfg, L, via):
    stripes, valid, want = class_batch(cfg, L)
    k, p = cfg[1], cfg[2]
    chained = (LENGTHS.index(L) + (via == "abi")) % 2 == 0
    crc_in = seeded_crc_in(len(valid), k + p, 1) if chained else None
    got, crcs, kernel = _run(cuda, make_code(cfg), stripes, valid, via, crc_in)
    assert kernel == route_kernel(cfg, L)
    d = mismatch(got, want, p)
    assert d is None, d
    d = crc_mismatch(crcs, _want_crcs(("class", cfg, L), p, stripes, valid, want, crc_in), k)
    assert d is None, d


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("cfg", STATIC + RUNTIME, ids=code_id)
def test_kernel_modes_give_equal_bytes_and_crcs(cuda, cfg, L):
    """Mode 3 fuses like mode 0; modes 1 and 2 never fuse: the ragged encode
    (vector, byte-granular), then the ragged window pass and the fold."""
    stripes, valid, want = class_batch(cfg, L)
    k, p = cfg[1], cfg[2]
    for mode, name in ((3, route_kernel(cfg, L, 3)), (1, vector_kernel(cfg)), (2, BYTEWISE)):
        crc_in = seeded_crc_in(len(valid), k + p, 1) if mode != 1 else None
        got, crcs, kernel = _run(cuda, make_code(cfg, mode), stripes, valid, "mirror", crc_in)
        assert kernel == name, mode
        d = mismatch(got, want, p)
        assert d is None, (mode, d)
        d = crc_mismatch(crcs, _want_crcs(("class", cfg, L), p, stripes, valid, want, crc_in), k)
        assert d is None, (mode, d)


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("cfg", STATIC + RUNTIME[:1], ids=code_id)
def test_all_full_batch_routes_to_the_plain_encode_crc(cuda, cfg, L):
    torch = cuda
    stripes, valid, want = full_batch(cfg, L)
    k, p = cfg[1], cfg[2]
    twin = make_code(cfg)
    t = torch.from_numpy(np.array(stripes)).to("cuda:0")
    plain_crcs = device.encode_stripes_crc(twin, t)
    plain_kernel = twin.lastKernel()
    torch.cuda.synchronize()
    want_crcs = _want_crcs(("full", cfg, L), p, stripes, valid, want, None)
    assert crc_mismatch(plain_crcs.cpu().numpy(), want_crcs, k) is None  # the two oracles of the test agree
    for mode, name in ((0, plain_kernel), (3, route_kernel(cfg, L, 3)), (2, BYTEWISE)):
        got, crcs, kernel = _run(torch, make_code(cfg, mode), stripes, valid, "abi", None)
        assert kernel == name, mode
        d = mismatch(got, want, p)
        assert d is None, (mode, d)
        d = crc_mismatch(crcs, want_crcs, k)
        assert d is None, (mode, d)
    assert plain_kernel and "ragged" not in plain_kernel


def test_one_entry_short_of_full_takes_the_ragged_route(cuda):
    """The all-full route needs EVERY entry at len."""
    cfg, L = STATIC[2], LENGTHS[0]
    stripes, valid, _ = full_batch(cfg, L)
    valid = np.array(valid)
    valid[-1, -1] = L - 1
    want = expected(cfg, stripes, valid)
    got, crcs, kernel = _run(cuda, make_code(cfg), stripes, valid, "mirror", None)
    assert kernel == fused_kernel(cfg)
    d = mismatch(got, want, cfg[2])
    assert d is None, d
    d = crc_mismatch(crcs, expected_crcs(cfg[2], stripes, valid, want), cfg[1])
    assert d is None, d


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("cfg", [STATIC[2], RUNTIME[2]], ids=code_id)
def test_crc_out_may_be_crc_in(cuda, cfg, mode):
    L = LENGTHS[0]
    stripes, valid, want = class_batch(cfg, L)
    k, p = cfg[1], cfg[2]
    crc_in = seeded_crc_in(len(valid), k + p, 1)
    got, crcs, kernel = _run(cuda, make_code(cfg, mode), stripes, valid, "abi", crc_in, alias=True)
    assert kernel == route_kernel(cfg, L, mode)
    d = mismatch(got, want, p)
    assert d is None, d
    d = crc_mismatch(crcs, _want_crcs(("class", cfg, L), p, stripes, valid, want, crc_in), k)
    assert d is None, d
