"""hrs_decode_batch_ragged_host through every way a host batch moves: pageable
numpy memory (staged, the zero-copy kernel on the slot's staging), torch-pinned
memory (one zero-copy launch in place), HRS_ZEROCOPY=0 (the copy engines,
pinned and pageable), HRS_HBATCH_DUPLEX=1, and HRS_HBATCH_BYTES small enough
for four chunks with a short last one. RS(10,4) with 40 KiB cells and RS(12,4)
with 12 KiB + 80 bytes (a byte-granular tail), 20 stripes with 0 to 4 losses.
The outputs equal the oracle's decodeBulk over zero-filled survivors up to
each output's length; the caller's `out` starts as a sentinel and is compared
whole, so a byte copied back at or beyond a length shows; the caller's stripes
are byte for byte what they were; hrs_last_host_path names the path. The slot
images keep stale bytes behind each length (survivors and outputs) from one
call to the next on a handle, which the second round of each case runs into."""
import numpy as np
import pytest

from lambdafs_amd import device
from ragged_repair_inputs import (SENTINEL, WINDOW, code_id, expected, expected_kernel, fresh_stripes, full_batch,
                                  length_classes, make_code, mismatch, patterns)

pytestmark = pytest.mark.gpu

S = 20
SHAPES = {("rs", 10, 4, 0): 20 * WINDOW, ("rs", 12, 4, 0): 6 * WINDOW + 80}


def _inputs(cfg, L, turn):
    """Length classes and window multiples in rotation over every location,
    erasure lists of 0 to 4 losses in rotation, then file-tail stripes."""
    k, p = cfg[1], cfg[2]
    n = k + p
    V = length_classes(L) + [w * WINDOW + d for w in range(2, L // WINDOW) for d in (0, 700)]
    valid = np.array([[V[(turn + 7 * s + 3 * l) % len(V)] for l in range(n)] for s in range(S)], np.uint32)
    pats = patterns(cfg, p, seed=20 + turn)
    erased = np.full((S, p), -1, np.int32)
    for s in range(S):
        lost = pats[(s + turn) % len(pats)]
        erased[s, :len(lost)] = lost
    for i, m in enumerate((0, 1, k // 2, k - 1, k)):  # the first m data cells full, the rest empty; lost data cell 0
        valid[S - 1 - i] = [L] * p + [L] * m + [0] * (k - m)
        erased[S - 1 - i] = [p] + [-1] * (p - 1)
    return erased, valid


_cache = {}


def _batch(cfg, turn):
    key = (cfg, turn)
    if key not in _cache:
        L = SHAPES[cfg]
        erased, valid = _inputs(cfg, L, turn)
        st = fresh_stripes(cfg, S, L, seed=10 + turn)
        _cache[key] = (st, erased, valid, expected(cfg, st, erased, valid))
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


def _call(torch, code, memory, stripes, erased, valid, shape):
    """One ragged host repair on fresh buffers of the given memory: (out, the stripes after the call)."""
    t = torch.from_numpy(stripes.copy())
    out = torch.full(shape, SENTINEL, dtype=torch.uint8)
    if memory == "pinned":
        t, out = t.pin_memory(), out.pin_memory()
    device.decode_batch_host_ragged(code, t.numpy() if memory == "numpy" else t, erased,
                                    out.numpy() if memory == "numpy" else out, valid)
    return out.numpy(), t.numpy()


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("cfg", list(SHAPES), ids=code_id)
def test_ragged_repair_host_batch(cuda, monkeypatch, cfg, case):
    memory, env, path = CASES[case]
    for name in ("HRS_ZEROCOPY", "HRS_HBATCH_DUPLEX", "HRS_HBATCH_BYTES", "HRS_ZC_BLOCKS", "HRS_TASK_ORDER"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, str(_chunk_bytes(cfg)) if value is None else value)
    code = make_code(cfg)
    for turn in (0, 1):  # the second batch meets the first one's bytes in the slot images
        stripes, erased, valid, want = _batch(cfg, turn)
        got, after = _call(cuda, code, memory, stripes, erased, valid, want.shape)
        assert code.lastHostPath() == path
        assert code.lastKernel() == expected_kernel(cfg, erased)
        d = mismatch(got, want, erased, valid)
        assert d is None, (turn, d)
        assert (after == stripes).all()


@pytest.mark.parametrize("memory", ["numpy", "pinned"])
def test_all_full_host_batch_is_the_plain_call(cuda, monkeypatch, memory):
    torch = cuda
    for name in ("HRS_ZEROCOPY", "HRS_HBATCH_DUPLEX", "HRS_HBATCH_BYTES"):
        monkeypatch.delenv(name, raising=False)
    cfg = ("rs", 10, 4, 0)
    stripes, erased, valid, want = full_batch(cfg, 4096 + 80)
    plain, code = make_code(cfg), make_code(cfg)
    a = torch.from_numpy(stripes.copy())
    oa = torch.full(want.shape, SENTINEL, dtype=torch.uint8)
    if memory == "pinned":
        a, oa = a.pin_memory(), oa.pin_memory()
    device.decode_batch_host(plain, a, np.array(erased), oa)
    got, _ = _call(torch, code, memory, stripes, erased, valid, want.shape)
    assert code.lastKernel() == plain.lastKernel() and "ragged" not in plain.lastKernel()
    assert code.lastHostPath() == plain.lastHostPath() == ("pinned" if memory == "pinned" else "staged")
    assert mismatch(got, want, erased, valid) is None and mismatch(oa.numpy(), want, erased, valid) is None
    code.setKernelMode(3)
    got, _ = _call(torch, code, memory, stripes, erased, valid, want.shape)
    assert code.lastKernel() == expected_kernel(cfg, erased)
    assert mismatch(got, want, erased, valid) is None


def test_stripes_that_lost_nothing_write_nothing(cuda):
    """A batch with no loss anywhere answers without a launch, whatever its lengths."""
    cfg = ("rs", 6, 3, 0)
    stripes = fresh_stripes(cfg, 3, 4096, seed=5)
    erased = np.full((3, 2), -1, np.int32)
    valid = np.full((3, 9), 100, np.uint32)
    got, after = _call(cuda, make_code(cfg), "numpy", stripes, erased, valid, (3, 2, 4096))
    assert (got == SENTINEL).all() and (after == stripes).all()
