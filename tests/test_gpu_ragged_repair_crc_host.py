"""hrs_decode_batch_ragged_host_crc through every way a host batch moves: the
cases of test_gpu_ragged_repair_host.py (pageable and torch-pinned memory,
HRS_ZEROCOPY=0, HRS_HBATCH_DUPLEX=1, HRS_HBATCH_BYTES small enough for four
chunks with a short last one), its shapes (RS(10,4) with 40 KiB cells, RS(12,4)
with 12 KiB + 80 bytes: two passes) plus RS(6,3) with 20 KiB cells (the fused
kernel), and its batches. Bytes against the same expectation,
`out` a sentinel compared whole; CRCs against zlib over exactly each rebuilt
cell's length, continued from a seeded crc_in, in HOST arrays whose chunk
offsets follow the chunk's first stripe; hrs_last_host_path. Each handle first
repairs a FULL batch, so the slot images hold stale non-zero bytes behind every
length of the ragged batches that follow: a CRC that read the image instead of
the registers, or beyond a cell's length, shows."""
import numpy as np
import pytest

from lambdafs_amd import device
from ragged_repair_inputs import SENTINEL, WINDOW, code_id, expected, expected_kernel, fresh_stripes, make_code, mismatch
from test_gpu_ragged_repair_crc import crc_mismatch, expected_crcs, fused_kernel, seeded
from test_gpu_ragged_repair_host import CASES, S, _inputs

pytestmark = pytest.mark.gpu

# the sibling's shapes (4 losses at 10 and 12 survivors: two passes) and RS(6,3), whose 3 losses fuse
SHAPES = {("rs", 10, 4, 0): 20 * WINDOW, ("rs", 12, 4, 0): 6 * WINDOW + 80, ("rs", 6, 3, 0): 10 * WINDOW}

_cache = {}
_full = {}


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
    pitch = (SHAPES[cfg] + 255) // 256 * 256  # the device image's row pitch
    return 6 * pitch * (cfg[1] + cfg[2]) + 1


def _full_batch(cfg):
    """The turn-0 batch's erasure lists over all-full cells of other bytes."""
    if cfg not in _full:
        L = SHAPES[cfg]
        _, erased, _, _ = _batch(cfg, 0)
        st = fresh_stripes(cfg, S, L, seed=30)
        valid = np.full((S, cfg[1] + cfg[2]), L, np.uint32)
        want = expected(cfg, st, erased, valid)
        _full[cfg] = (st, erased, valid, want, expected_crcs(want, erased, valid))
    return _full[cfg]


def _call(torch, code, memory, stripes, erased, valid, shape, crc_in):
    t = torch.from_numpy(stripes.copy())
    out = torch.full(shape, SENTINEL, dtype=torch.uint8)
    if memory == "pinned":
        t, out = t.pin_memory(), out.pin_memory()
    crc = device.decode_batch_host_ragged_crc(code, t.numpy() if memory == "numpy" else t, erased,
                                              out.numpy() if memory == "numpy" else out, valid, crc_in=crc_in)
    return out.numpy(), t.numpy(), crc


def _kernel(cfg, erased, L):
    return (fused_kernel(cfg, erased) if L % WINDOW == 0 else None) or expected_kernel(cfg, erased)


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("cfg", list(SHAPES), ids=code_id)
def test_ragged_repair_crc_host_batch(cuda, monkeypatch, cfg, case):
    memory, env, path = CASES[case]
    for name in ("HRS_ZEROCOPY", "HRS_HBATCH_DUPLEX", "HRS_HBATCH_BYTES", "HRS_ZC_BLOCKS", "HRS_TASK_ORDER"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, str(_chunk_bytes(cfg)) if value is None else value)
    code = make_code(cfg, 3)  # mode 3: the full batch stays on the ragged route, the same slot images
    stripes, erased, valid, want, crcs = _full_batch(cfg)
    got, _, crc = _call(cuda, code, memory, stripes, erased, valid, want.shape, None)
    assert mismatch(got, want, erased, valid) is None and crc_mismatch(crc, crcs) is None
    code.setKernelMode(0)
    for turn in (0, 1):  # each batch meets the one before in the slot images
        stripes, erased, valid, want = _batch(cfg, turn)
        cin = seeded(erased.shape, seed=40 + turn)
        got, after, crc = _call(cuda, code, memory, stripes, erased, valid, want.shape, cin)
        assert code.lastHostPath() == path
        assert code.lastKernel() == _kernel(cfg, erased, SHAPES[cfg])
        d = mismatch(got, want, erased, valid)
        assert d is None, (turn, d)
        d = crc_mismatch(crc, expected_crcs(want, erased, valid, cin))
        assert d is None, (turn, d)
        assert (after == stripes).all()


@pytest.mark.parametrize("memory", ["numpy", "pinned"])
def test_all_full_host_batch_is_the_plain_crc_call(cuda, monkeypatch, memory):
    torch = cuda
    for name in ("HRS_ZEROCOPY", "HRS_HBATCH_DUPLEX", "HRS_HBATCH_BYTES"):
        monkeypatch.delenv(name, raising=False)
    cfg = ("rs", 10, 4, 0)
    stripes, erased, valid, want, crcs = _full_batch(cfg)
    plain, code = make_code(cfg), make_code(cfg)
    a = torch.from_numpy(stripes.copy())
    oa = torch.full(want.shape, SENTINEL, dtype=torch.uint8)
    if memory == "pinned":
        a, oa = a.pin_memory(), oa.pin_memory()
    plain_crc = device.decode_batch_host_crc(plain, a, np.array(erased), oa)
    got, _, crc = _call(torch, code, memory, stripes, erased, valid, want.shape, None)
    assert code.lastKernel() == plain.lastKernel() and "ragged" not in plain.lastKernel()
    assert code.lastHostPath() == plain.lastHostPath() == ("pinned" if memory == "pinned" else "staged")
    assert mismatch(got, want, erased, valid) is None and mismatch(oa.numpy(), want, erased, valid) is None
    assert crc_mismatch(crc, crcs) is None and crc_mismatch(plain_crc, crcs) is None


def test_stripes_that_lost_nothing_keep_their_crcs(cuda):
    cfg = ("rs", 6, 3, 0)
    stripes = fresh_stripes(cfg, 3, 4096, seed=5)
    erased = np.full((3, 2), -1, np.int32)
    valid = np.full((3, 9), 100, np.uint32)
    cin = seeded((3, 2))
    got, after, crc = _call(cuda, make_code(cfg), "numpy", stripes, erased, valid, (3, 2, 4096), cin)
    assert (got == SENTINEL).all() and (after == stripes).all() and (crc == cin).all()
