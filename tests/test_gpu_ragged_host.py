"""hrs_encode_ragged_batch_host through every way a host batch moves:
pageable numpy memory (staged, the zero-copy kernel on the slot's staging),
torch-pinned memory (one zero-copy launch in place), HRS_ZEROCOPY=0 (the copy
engines, pinned and pageable), HRS_HBATCH_DUPLEX=1, and HRS_HBATCH_BYTES small
enough for four chunks with a short last one. RS(10,4) with 40 KiB cells and
RS(12,4) with 12 KiB + 80 bytes (a byte-granular tail), 20 stripes. The parity
equals the oracle's encodeBulk over zero-filled cells; every data cell of the
caller's batch is byte for byte what it was, the non-zero bytes behind `valid`
included; hrs_last_host_path names the path. The slot images keep stale bytes
behind `valid` from one call to the next on a handle, which the second round
of each case runs into."""
import numpy as np
import pytest

from lambdafs_amd import device
from ragged_inputs import (WINDOW, code_id, expected, fresh_stripes, full_batch, make_code, mismatch, valid_classes,
                           vector_kernel)

pytestmark = pytest.mark.gpu

S = 20
SHAPES = {("rs", 10, 4, 0): 20 * WINDOW, ("rs", 12, 4, 0): 6 * WINDOW + 80}


def _valid(k, L, turn):
    """Valid classes and window multiples in rotation, then file-tail stripes."""
    V = valid_classes(L) + [w * WINDOW + d for w in range(2, L // WINDOW) for d in (0, 700)]
    v = np.array([[V[(turn + 7 * s + 3 * j) % len(V)] for j in range(k)] for s in range(S)], np.uint32)
    for i, m in enumerate((0, 1, k // 2, k - 1, k)):
        v[S - 1 - i] = [L] * m + [0] * (k - m)
    return v


_cache = {}


def _batch(cfg, turn):
    key = (cfg, turn)
    if key not in _cache:
        L = SHAPES[cfg]
        valid = _valid(cfg[1], L, turn)
        st = fresh_stripes(cfg, S, L, seed=10 + turn)
        _cache[key] = (st, valid, expected(cfg, st, valid))
    return _cache[key]


def _chunk_bytes(cfg):
    """HRS_HBATCH_BYTES for chunks of 6 stripes: 6, 6, 6 and 2 of the 20."""
    L = SHAPES[cfg]
    pitch = (L + 255) // 256 * 256  # the device image's row pitch
    return 6 * pitch * (cfg[1] + cfg[2]) + 1


# case -> (memory, environment, hrs_last_host_path)
CASES = {
    "pageable": ("numpy", {}, "staged"),
    "pinned": ("pinned", {}, "pinned"),
    "copy_engine_pageable": ("numpy", {"HRS_ZEROCOPY": "0"}, "copy_engine"),
    "copy_engine_pinned": ("pinned", {"HRS_ZEROCOPY": "0"}, "copy_engine"),
    "duplex_pageable": ("numpy", {"HRS_ZEROCOPY": "0", "HRS_HBATCH_DUPLEX": "1"}, "copy_engine"),
    "duplex_pinned": ("pinned", {"HRS_ZEROCOPY": "0", "HRS_HBATCH_DUPLEX": "1"}, "copy_engine"),
    "chunks_pageable": ("numpy", {"HRS_HBATCH_BYTES": None}, "staged"),
    "chunks_copy_engine": ("numpy", {"HRS_HBATCH_BYTES": None, "HRS_ZEROCOPY": "0"}, "copy_engine"),
    "chunks_duplex_pinned": ("pinned", {"HRS_HBATCH_BYTES": None, "HRS_ZEROCOPY": "0", "HRS_HBATCH_DUPLEX": "1"},
                             "copy_engine"),
}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("cfg", list(SHAPES), ids=code_id)
def test_ragged_host_batch(cuda, monkeypatch, cfg, case):
    torch = cuda
    memory, env, path = CASES[case]
    for name in ("HRS_ZEROCOPY", "HRS_HBATCH_DUPLEX", "HRS_HBATCH_BYTES", "HRS_ZC_BLOCKS", "HRS_TASK_ORDER"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, str(_chunk_bytes(cfg)) if value is None else value)
    code = make_code(cfg)
    for turn in (0, 1):  # the second batch meets the first one's bytes in the slot images
        stripes, valid, want = _batch(cfg, turn)
        if memory == "pinned":
            t = torch.from_numpy(stripes.copy()).pin_memory()
            device.encode_batch_host_ragged(code, t, valid)
            got = t.numpy()
        else:
            got = stripes.copy()
            device.encode_batch_host_ragged(code, got, valid)
        assert code.lastHostPath() == path
        assert code.lastKernel() == vector_kernel(cfg)
        d = mismatch(got, want, cfg[2])
        assert d is None, (turn, d)


@pytest.mark.parametrize("memory", ["numpy", "pinned"])
def test_all_full_host_batch_is_the_plain_call(cuda, monkeypatch, memory):
    torch = cuda
    for name in ("HRS_ZEROCOPY", "HRS_HBATCH_DUPLEX", "HRS_HBATCH_BYTES"):
        monkeypatch.delenv(name, raising=False)
    cfg = ("rs", 10, 4, 0)
    stripes, valid, want = full_batch(cfg, 4096 + 80)
    plain, code = make_code(cfg), make_code(cfg)
    a = torch.from_numpy(stripes.copy())
    b = torch.from_numpy(stripes.copy())
    if memory == "pinned":
        a, b = a.pin_memory(), b.pin_memory()
    device.encode_batch_host(plain, a)
    device.encode_batch_host_ragged(code, b, valid)
    assert code.lastKernel() == plain.lastKernel() == "encode_static_kernel<10, 4>"
    assert code.lastHostPath() == plain.lastHostPath() == ("pinned" if memory == "pinned" else "staged")
    assert mismatch(b.numpy(), want, 4) is None and mismatch(a.numpy(), want, 4) is None
    code.setKernelMode(3)
    c = torch.from_numpy(stripes.copy())
    c = c.pin_memory() if memory == "pinned" else c
    device.encode_batch_host_ragged(code, c, valid)
    assert code.lastKernel() == vector_kernel(cfg)
    assert mismatch(c.numpy(), want, 4) is None
