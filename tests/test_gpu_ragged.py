"""hrs_encode_ragged_dev on the GPU against the oracle's encodeBulk over
zero-filled cells, bit-exact, for every code kind: the six shapes with a
compile-time network (encode_ragged_kernel<K, P>) and rs (5,3), xor (4,1) and
an src layout (encode_ragged_bytewise_kernel); cell lengths of whole 2 KiB
windows and of windows plus an 80-byte tail; every valid class at every row
position, the file-tail stripes, all-zero and all-full stripes
(ragged_inputs.class_valid). The tails behind `valid` hold non-zero bytes, so
a byte that is used shows. Both the C ABI and the Python mirror are called.
Routing: an all-full batch names the plain encode's kernel, kernel mode 3
keeps the ragged kernel, mode 2 takes the byte-granular one, equal bytes."""
import numpy as np
import pytest

from lambdafs_amd import _lib, device
from ragged_inputs import (BYTEWISE, RUNTIME, STATIC, class_batch, code_id, full_batch, make_code, mismatch,
                           vector_kernel)

pytestmark = pytest.mark.gpu

LENGTHS = [4096, 4096 + 80]


def _abi_call(torch, code, t, valid):
    """hrs_encode_ragged_dev over the device batch t[S, n, L] with a host valid array."""
    k, p = code.stripeSize(), code.paritySize()
    S, n, L = t.shape
    ins = _lib.ptr_array([t[:, p + j].data_ptr() for j in range(k)])
    outs = _lib.ptr_array([t[:, r].data_ptr() for r in range(p)])
    v = np.ascontiguousarray(valid, dtype=np.uint32)
    st = _lib.lib().hrs_encode_ragged_dev(code._handle(), ins, n * L, outs, n * L, L, S, v.ctypes.data,
                                          torch.cuda.current_stream().cuda_stream)
    v[...] = 0xFFFFFFFF  # the caller's array is free as soon as the call returns
    code._check(st)


def _run(torch, code, stripes, valid, via):
    t = torch.from_numpy(np.array(stripes)).to("cuda:0")
    if via == "abi":
        _abi_call(torch, code, t, np.array(valid))
    else:
        device.encode_stripes_ragged(code, t, valid)
    kernel = code.lastKernel()
    torch.cuda.synchronize()
    return t.cpu().numpy(), kernel


@pytest.mark.parametrize("via", ["abi", "mirror"])
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("cfg", STATIC + RUNTIME, ids=code_id)
def test_ragged_encode_matches_the_oracle(cuda, cfg, L, via):
    stripes, valid, want = class_batch(cfg, L)
    got, kernel = _run(cuda, make_code(cfg), stripes, valid, via)
    assert kernel == vector_kernel(cfg)
    d = mismatch(got, want, cfg[2])
    assert d is None, d


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("cfg", STATIC + RUNTIME, ids=code_id)
def test_kernel_modes_give_equal_bytes(cuda, cfg, L):
    """Mode 1 behaves like mode 0, mode 3 keeps the shape's ragged kernel and
    mode 2 takes the byte-granular one; every mode gives the oracle's bytes."""
    stripes, valid, want = class_batch(cfg, L)
    for mode, name in ((1, vector_kernel(cfg)), (3, vector_kernel(cfg)), (2, BYTEWISE)):
        got, kernel = _run(cuda, make_code(cfg, mode), stripes, valid, "mirror")
        assert kernel == name, mode
        d = mismatch(got, want, cfg[2])
        assert d is None, (mode, d)


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("cfg", STATIC + RUNTIME, ids=code_id)
def test_all_full_batch_routes_to_the_plain_encode(cuda, cfg, L):
    torch = cuda
    stripes, valid, want = full_batch(cfg, L)
    plain = make_code(cfg)
    t = torch.from_numpy(np.array(stripes)).to("cuda:0")
    device.encode_stripes(plain, t)
    plain_kernel = plain.lastKernel()
    torch.cuda.synchronize()
    assert mismatch(t.cpu().numpy(), want, cfg[2]) is None  # the two oracles of the test agree
    for mode, name in ((0, plain_kernel), (3, vector_kernel(cfg)), (2, BYTEWISE)):
        got, kernel = _run(torch, make_code(cfg, mode), stripes, valid, "abi")
        assert kernel == name, mode
        d = mismatch(got, want, cfg[2])
        assert d is None, (mode, d)
    assert plain_kernel and "ragged" not in plain_kernel


def test_one_entry_short_of_full_takes_the_ragged_kernel(cuda):
    """The all-full route needs EVERY entry at len."""
    cfg, L = STATIC[2], LENGTHS[1]
    stripes, valid, _ = full_batch(cfg, L)
    valid = np.array(valid)
    valid[-1, -1] = L - 1
    from ragged_inputs import expected
    got, kernel = _run(cuda, make_code(cfg), stripes, valid, "mirror")
    assert kernel == vector_kernel(cfg)
    d = mismatch(got, expected(cfg, stripes, valid), cfg[2])
    assert d is None, d


def test_wide_code_runs_in_input_and_output_chunks(cuda):
    """RS(40,10): more inputs than one byte-granular launch reads (32) and more
    outputs than it writes (8), so later input chunks accumulate and the valid
    table is read at the chunk's first row."""
    cfg = ("rs", 40, 10, 0)
    stripes, valid, want = class_batch(cfg, 1024 + 80)
    got, kernel = _run(cuda, make_code(cfg), stripes, valid, "mirror")
    assert kernel == BYTEWISE
    d = mismatch(got, want, cfg[2])
    assert d is None, d


def test_repeated_calls_reuse_the_table_slots(cuda):
    """Five calls back to back on one handle and stream, each with its own
    valid array overwritten right after the call: the two per-call table slots
    are refilled only when their upload's launch has finished."""
    torch = cuda
    cfg, L = STATIC[2], LENGTHS[1]
    stripes, valid, want = class_batch(cfg, L)
    code = make_code(cfg)
    S = len(valid)
    outs = []
    for i in range(5):
        t = torch.from_numpy(np.roll(np.array(stripes), i, axis=0)).to("cuda:0")
        _abi_call(torch, code, t, np.roll(np.array(valid), i, axis=0))
        outs.append(t)
    torch.cuda.synchronize()
    for i, t in enumerate(outs):
        d = mismatch(t.cpu().numpy(), np.roll(want, i, axis=0), cfg[2])
        assert d is None, (i, d)
    assert S > 2
