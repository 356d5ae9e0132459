"""encode_ragged_crc_kernel along its sub-window walk, under every window size
and window order and on a capped grid. RS(10,4) and RS(12,4) (five and six row
groups), 32 KiB cells (16 sub-windows), 24 stripes. A row's sub-windows are
full up to its boundary and dead behind it, and the boundaries are spread as
in test_gpu_ragged_waves.BOUNDS scaled to 16 sub-windows: one inside every
sub-window, at its first, second, a middle and its last byte in turn, none,
whole sub-windows only, a full cell. Every row position meets every entry, so
along a window's walk each goes full -> boundary -> dead (a chain that must
keep advancing over the zeros), and some rows are dead from sub-window 0 (a
chain that stays 0). HRS_RAGGED_CRC_SUBS cuts the cell into windows of 1, 2, 4,
8 and 16 sub-windows: a window then starts full, on the boundary or dead.
HRS_TASK_ORDER 0, 1 and 32 change which windows a wave runs one after the
other; the pinned host batch on a grid of 1 and 2 blocks (HRS_ZC_BLOCKS) makes
one wave run many windows, so a case carried over in registers from the
window before shows in a parity byte or a CRC."""
import numpy as np
import pytest

from lambdafs_amd import device
from ragged_crc_inputs import crc_mismatch, expected_crcs, fused_kernel, seeded_crc_in
from ragged_inputs import WINDOW, code_id, expected, fresh_stripes, make_code, mismatch

pytestmark = pytest.mark.gpu

CODES = [("rs", 10, 4, 0), ("rs", 12, 4, 0)]
NSUB, S = 16, 24
L = NSUB * WINDOW
BOUNDS = [w * WINDOW + d for w, d in zip(range(NSUB), 2 * (1, 2, 1000, 2047, 16, 17, 1, 1025))] + \
    [0, 2 * WINDOW, 6 * WINDOW, 11 * WINDOW, L]


def _valid(k):
    return np.array([[BOUNDS[(5 * s + 7 * j) % len(BOUNDS)] for j in range(k)] for s in range(S)], np.uint32)


_cache = {}


def _batch(cfg):
    """(stripes, valid, want, crc_in, want_crcs), built once per code."""
    if cfg not in _cache:
        k, p = cfg[1], cfg[2]
        valid = _valid(k)
        st = fresh_stripes(cfg, S, L, seed=4)
        want = expected(cfg, st, valid)
        crc_in = seeded_crc_in(S, k + p, 2)
        _cache[cfg] = (st, valid, want, crc_in, expected_crcs(p, st, valid, want, crc_in))
    return _cache[cfg]


@pytest.mark.parametrize("cfg", CODES, ids=code_id)
def test_every_row_position_walks_through_the_three_cases(cfg):
    """What the batch must contain for the GPU cases below to mean anything."""
    valid = _valid(cfg[1])
    for j in range(cfg[1]):
        col = [int(v) for v in valid[:, j]]
        assert any(WINDOW < v < L - WINDOW and v % WINDOW for v in col)  # full -> boundary -> dead in one window
        assert any(v and v % WINDOW == 0 and v < L for v in col)         # full -> dead, no boundary sub-window
        assert 0 in col and L in col                                     # dead from sub-window 0; never dead
        for subs in (2, 4, 8):  # a window that starts on the boundary, and one that starts dead after live ones
            assert any(v % (subs * WINDOW) and v % (subs * WINDOW) < WINDOW for v in col)
            assert any(0 < v <= L - subs * WINDOW for v in col)


@pytest.mark.parametrize("order", [0, 1, 32])
@pytest.mark.parametrize("subs", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("cfg", CODES, ids=code_id)
def test_sub_window_walks_device(cuda, monkeypatch, cfg, subs, order):
    torch = cuda
    stripes, valid, want, crc_in, want_crcs = _batch(cfg)
    monkeypatch.setenv("HRS_RAGGED_CRC_SUBS", str(subs))
    monkeypatch.setenv("HRS_TASK_ORDER", str(order))
    code = make_code(cfg)
    t = torch.from_numpy(stripes.copy()).to("cuda:0")
    cin = torch.from_numpy(crc_in.view(np.int32).copy()).to("cuda:0")
    crcs = device.encode_stripes_ragged_crc(code, t, valid, crc_in=cin)
    assert code.lastKernel() == fused_kernel(cfg)
    torch.cuda.synchronize()
    d = mismatch(t.cpu().numpy(), want, cfg[2])
    assert d is None, d
    d = crc_mismatch(crcs.cpu().numpy(), want_crcs, cfg[1])
    assert d is None, d


@pytest.mark.parametrize("cap", [1, 2])
@pytest.mark.parametrize("subs", [1, 4, 16])
@pytest.mark.parametrize("cfg", CODES, ids=code_id)
def test_capped_grid_pinned_host_batch(cuda, monkeypatch, cfg, subs, cap):
    """One or two 1,024-thread blocks: at 1 sub-window per window a wave runs
    24 or 12 windows one after the other, at 16 it runs 1 or 2 whole cells."""
    torch = cuda
    stripes, valid, want, crc_in, want_crcs = _batch(cfg)
    monkeypatch.setenv("HRS_ZC_BLOCKS", str(cap))
    monkeypatch.setenv("HRS_RAGGED_CRC_SUBS", str(subs))
    monkeypatch.delenv("HRS_TASK_ORDER", raising=False)
    monkeypatch.delenv("HRS_ZEROCOPY", raising=False)
    code = make_code(cfg)
    t = torch.from_numpy(stripes.copy()).pin_memory()
    crcs = device.encode_batch_host_ragged_crc(code, t, valid, crc_in=crc_in.copy())
    assert code.lastHostPath() == "pinned" and code.lastKernel() == fused_kernel(cfg)
    d = mismatch(t.numpy(), want, cfg[2])
    assert d is None, d
    d = crc_mismatch(crcs, want_crcs, cfg[1])
    assert d is None, d
