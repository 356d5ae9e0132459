"""hrs_decode_batch_ragged_dev on the GPU against the oracle's decodeBulk over
zero-filled survivors, bit-exact, for every code kind: rs (10,4), (6,3), (3,2),
(12,4), (5,3), nrs (10,4), xor (4,1) and an src layout; cell lengths of whole
2 KiB windows and of windows plus an 80-byte tail; every length class at every
input and every output position under erasure lists of 0 to p losses, and the
file-tail stripes (ragged_repair_inputs.class_batch_inputs). Every cell holds
non-zero bytes behind its length and `out` starts as a sentinel, every byte of
which is compared: a tail byte that is used shows, and so does a byte written
at or beyond an output's length. Both the C ABI and the Python mirror are
called. Routing: the kernel name per shape (src with more than 4 losses takes
the byte-granular kernel), kernel modes 1 / 2 / 3, the all-full batch and the
batch one entry short of full; table-slot reuse over back-to-back calls."""
import numpy as np
import pytest

from lambdafs_amd import _lib, device
from ragged_repair_inputs import (BYTEWISE, CODES, SENTINEL, class_batch, code_id, expected, expected_kernel,
                                  full_batch, make_code, mismatch)

pytestmark = pytest.mark.gpu

LENGTHS = [4096, 4096 + 80]
SRC = CODES[-1]
# (code, the most losses per stripe): src twice, within the vector kernel's 4 outputs and beyond
CASES = [(cfg, 4 if cfg == SRC else cfg[2]) for cfg in CODES] + [(SRC, SRC[2])]


def case_id(case):
    return "%s_upto%d" % (code_id(case[0]), case[1])


def _abi_call(torch, code, t, erased, out, valid):
    """hrs_decode_batch_ragged_dev over the device batch t[S, n, L] with host erased and valid arrays."""
    S, n, L = t.shape
    e = np.ascontiguousarray(erased, dtype=np.int32)
    v = np.ascontiguousarray(valid, dtype=np.uint32)
    st = _lib.lib().hrs_decode_batch_ragged_dev(code._handle(), t.data_ptr(), L, n * L, e.ctypes.data, e.shape[1],
                                                out.data_ptr(), L, e.shape[1] * L, L, S, v.ctypes.data,
                                                torch.cuda.current_stream().cuda_stream)
    v[...] = 0xFFFFFFFF  # the caller's array is free as soon as the call returns
    code._check(st)


def _run(torch, code, stripes, erased, valid, via):
    t = torch.from_numpy(np.array(stripes)).to("cuda:0")
    out = torch.full((t.shape[0], erased.shape[1], t.shape[2]), SENTINEL, dtype=torch.uint8, device="cuda:0")
    if via == "abi":
        _abi_call(torch, code, t, erased, out, np.array(valid))
    else:
        device.decode_batch_ragged(code, t, np.array(erased), out, valid)
    kernel = code.lastKernel()
    torch.cuda.synchronize()
    assert (t.cpu().numpy() == stripes).all()  # survivors are never written
    return out.cpu().numpy(), kernel


@pytest.mark.parametrize("via", ["abi", "mirror"])
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_ragged_repair_matches_the_oracle(cuda, case, L, via):
    cfg, max_loss = case
    stripes, erased, valid, want = class_batch(cfg, L, max_loss)
    got, kernel = _run(cuda, make_code(cfg), stripes, erased, valid, via)
    name = expected_kernel(cfg, erased)
    assert kernel == name
    assert (name == BYTEWISE) == (max_loss > 4)
    d = mismatch(got, want, erased, valid)
    assert d is None, d


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_kernel_modes_give_equal_bytes(cuda, case, L):
    """Mode 1 behaves like mode 0, mode 3 keeps the shape's ragged kernel and
    mode 2 takes the byte-granular one; every mode gives the oracle's bytes."""
    cfg, max_loss = case
    stripes, erased, valid, want = class_batch(cfg, L, max_loss)
    name = expected_kernel(cfg, erased)
    for mode, wanted in ((1, name), (3, name), (2, BYTEWISE)):
        got, kernel = _run(cuda, make_code(cfg, mode), stripes, erased, valid, "mirror")
        assert kernel == wanted, mode
        d = mismatch(got, want, erased, valid)
        assert d is None, (mode, d)


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("cfg", CODES, ids=code_id)
def test_all_full_batch_routes_to_the_plain_batch(cuda, cfg, L):
    torch = cuda
    stripes, erased, valid, want = full_batch(cfg, L)
    plain = make_code(cfg)
    t = torch.from_numpy(np.array(stripes)).to("cuda:0")
    out = torch.full((t.shape[0], erased.shape[1], L), SENTINEL, dtype=torch.uint8, device="cuda:0")
    device.decode_batch(plain, t, np.array(erased), out)
    plain_kernel = plain.lastKernel()
    torch.cuda.synchronize()
    assert mismatch(out.cpu().numpy(), want, erased, valid) is None  # the two oracles of the test agree
    for mode, name in ((0, plain_kernel), (1, plain_kernel), (3, expected_kernel(cfg, erased)), (2, BYTEWISE)):
        got, kernel = _run(torch, make_code(cfg, mode), stripes, erased, valid, "abi")
        assert kernel == name, mode
        d = mismatch(got, want, erased, valid)
        assert d is None, (mode, d)
    assert plain_kernel and "ragged" not in plain_kernel


def test_one_entry_short_of_full_takes_the_ragged_kernel(cuda):
    """The all-full route needs EVERY entry at len, the ignored ones too:
    location 0 of the last stripe is neither read nor lost there."""
    cfg, L = CODES[0], LENGTHS[1]
    stripes, erased, valid, _ = full_batch(cfg, L)
    valid = np.array(valid)
    valid[-1, 0] = L - 1
    got, kernel = _run(cuda, make_code(cfg), stripes, erased, valid, "mirror")
    assert kernel == expected_kernel(cfg, erased)
    d = mismatch(got, expected(cfg, stripes, erased, valid), erased, valid)
    assert d is None, d


def test_sixteen_row_instantiation(cuda):
    """RS(14,2): 14 survivors per pattern, the only shape here that takes the
    NINB = 16 kernels."""
    cfg, L = ("rs", 14, 2, 0), LENGTHS[1]
    stripes, erased, valid, want = class_batch(cfg, L)
    got, kernel = _run(cuda, make_code(cfg), stripes, erased, valid, "abi")
    assert kernel == "batch_ragged_kernel<2, 16>" == expected_kernel(cfg, erased)
    d = mismatch(got, want, erased, valid)
    assert d is None, d


def test_repeated_calls_reuse_the_table_slots(cuda):
    """Five calls back to back on one handle and stream, each with its own
    valid array overwritten right after the call: the two per-call table slots
    are refilled only when their upload's launch has finished."""
    torch = cuda
    cfg, L = CODES[0], LENGTHS[1]
    stripes, erased, valid, want = class_batch(cfg, L)
    code = make_code(cfg)
    runs = []
    for i in range(5):
        t = torch.from_numpy(np.roll(np.array(stripes), i, axis=0)).to("cuda:0")
        out = torch.full(want.shape, SENTINEL, dtype=torch.uint8, device="cuda:0")
        _abi_call(torch, code, t, np.roll(np.array(erased), i, axis=0), out, np.roll(np.array(valid), i, axis=0))
        runs.append((t, out))
    torch.cuda.synchronize()
    for i, (_, out) in enumerate(runs):
        d = mismatch(out.cpu().numpy(), np.roll(want, i, axis=0), np.roll(erased, i, axis=0),
                     np.roll(valid, i, axis=0))
        assert d is None, (i, d)
