"""hrs_encode_ragged_batch_host_crc through every way a host batch moves:
pageable numpy memory (staged, the kernels on the slot's staging), torch-pinned
memory (one zero-copy launch in place), HRS_ZEROCOPY=0 (the copy engines), and
HRS_HBATCH_BYTES small enough for four chunks with a short last one, so every
chunk takes its own slice of valid and of the CRC arrays. RS(10,4) with 20 KiB
cells (the fused kernel) and RS(12,4) with 12 KiB + 80 bytes (two passes: the
ragged encode with a byte-granular tail, then the ragged window pass), 20
stripes. Two batches per handle with different valid arrays: the second meets
the first one's stale bytes behind `valid` in the slot images, and they must
reach neither parity nor CRC. Host crc_in and crc_out are distinct arrays in
the first round and one array in the second."""
import numpy as np
import pytest

from lambdafs_amd import device
from ragged_crc_inputs import crc_mismatch, expected_crcs, route_kernel, seeded_crc_in
from ragged_inputs import WINDOW, code_id, expected, fresh_stripes, full_batch, make_code, mismatch, valid_classes

pytestmark = pytest.mark.gpu

S = 20
SHAPES = {("rs", 10, 4, 0): 10 * WINDOW, ("rs", 12, 4, 0): 6 * WINDOW + 80}


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
        k, p = cfg[1], cfg[2]
        valid = _valid(k, L, turn)
        st = fresh_stripes(cfg, S, L, seed=20 + turn)
        want = expected(cfg, st, valid)
        crc_in = seeded_crc_in(S, k + p, 3 + turn)
        _cache[key] = (st, valid, want, crc_in, expected_crcs(p, st, valid, want, crc_in))
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
    "chunks_pageable": ("numpy", {"HRS_HBATCH_BYTES": None}, "staged"),
    "chunks_copy_engine": ("numpy", {"HRS_HBATCH_BYTES": None, "HRS_ZEROCOPY": "0"}, "copy_engine"),
}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("cfg", list(SHAPES), ids=code_id)
def test_ragged_host_batch_crc(cuda, monkeypatch, cfg, case):
    torch = cuda
    memory, env, path = CASES[case]
    for name in ("HRS_ZEROCOPY", "HRS_HBATCH_DUPLEX", "HRS_HBATCH_BYTES", "HRS_ZC_BLOCKS", "HRS_TASK_ORDER",
                 "HRS_RAGGED_CRC_SUBS"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, str(_chunk_bytes(cfg)) if value is None else value)
    code = make_code(cfg)
    for turn in (0, 1):  # the second batch meets the first one's bytes in the slot images
        stripes, valid, want, crc_in, want_crcs = _batch(cfg, turn)
        got = torch.from_numpy(stripes.copy()).pin_memory() if memory == "pinned" else stripes.copy()
        cin = crc_in.copy()
        out = cin if turn == 1 else np.full_like(cin, 0x5A5A5A5A)
        crcs = device.encode_batch_host_ragged_crc(code, got, valid, crc_in=cin, crc_out=out)
        assert crcs is out
        if turn == 0:
            assert (cin == crc_in).all(), "crc_in was written"
        assert code.lastHostPath() == path
        assert code.lastKernel() == route_kernel(cfg, SHAPES[cfg])
        d = mismatch(got.numpy() if memory == "pinned" else got, want, cfg[2])
        assert d is None, (turn, d)
        d = crc_mismatch(crcs, want_crcs, cfg[1])
        assert d is None, (turn, d)


@pytest.mark.parametrize("memory", ["numpy", "pinned"])
def test_all_full_host_batch_is_the_plain_crc_call(cuda, monkeypatch, memory):
    torch = cuda
    for name in ("HRS_ZEROCOPY", "HRS_HBATCH_DUPLEX", "HRS_HBATCH_BYTES"):
        monkeypatch.delenv(name, raising=False)
    cfg = ("rs", 10, 4, 0)
    stripes, valid, want = full_batch(cfg, 4096)
    want_crcs = expected_crcs(4, stripes, valid, want)
    plain, code = make_code(cfg), make_code(cfg)

    def fresh():
        t = torch.from_numpy(stripes.copy())
        return t.pin_memory() if memory == "pinned" else t

    a, b = fresh(), fresh()
    ca = device.encode_batch_host_crc(plain, a)
    cb = device.encode_batch_host_ragged_crc(code, b, valid)
    assert code.lastKernel() == plain.lastKernel() and "ragged" not in code.lastKernel()
    assert code.lastHostPath() == plain.lastHostPath() == ("pinned" if memory == "pinned" else "staged")
    assert mismatch(b.numpy(), want, 4) is None and mismatch(a.numpy(), want, 4) is None
    assert crc_mismatch(ca, want_crcs, 10) is None and crc_mismatch(cb, want_crcs, 10) is None
    code.setKernelMode(3)
    c = fresh()
    cc = device.encode_batch_host_ragged_crc(code, c, valid)
    assert code.lastKernel() == route_kernel(cfg, 4096, 3)
    assert mismatch(c.numpy(), want, 4) is None and crc_mismatch(cc, want_crcs, 10) is None
