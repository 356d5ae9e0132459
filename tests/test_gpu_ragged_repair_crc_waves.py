"""batch_ragged_crc_kernel with many windows per wave, under every window order
and on a capped grid: the batch of test_gpu_ragged_repair_waves.py (RS(10,4),
16 KiB cells of 8 windows, 24 stripes that lost one or two cells in turn, 192
window tasks, boundaries at a window's first, second, a middle and its last
byte, empty, whole-window and full cells) through
batch_ragged_crc_kernel<2, 12, 768>. Along a wave's walk some output position
passes between each pair of {full, boundary, dead}, and a task whose outputs
are all dead (skipped before any load, no raw word) is followed by a live one:
a CRC state or a mask carried over from the window before shows in a CRC word,
a raw word left out or written for a dead window in the fold.

The window -> wave assignment of wave_tasks (hrs_device.hpp) is restated for
this kernel's launch: 768-thread blocks of 12 waves, at most one block per CU.
The device call's grid is 16 blocks, so under HRS_TASK_ORDER 1 and 0 every wave
runs one window; under order 32 one block runs all 192, 16 per wave. The pinned
host batch runs on a grid capped at 1 and 2 blocks (HRS_ZC_BLOCKS): 16 and 8
windows per wave. Wherever a wave runs three or more windows, the transitions
are required."""
import numpy as np
import pytest

import test_gpu_ragged_repair_waves as sib
from lambdafs_amd import device
from ragged_repair_inputs import SENTINEL, make_code, mismatch
from test_gpu_ragged_repair_crc import as_i32, crc_mismatch, expected_crcs, seeded

pytestmark = pytest.mark.gpu

CFG, S, NWIN = sib.CFG, sib.S, sib.NWIN
WPB = 12  # waves per 768-thread block
KERNEL = "batch_ragged_crc_kernel<2, 12, 768>"


def _walks(ntasks, order, grid):
    """The tasks of every wave of the launch, in the order it runs them."""
    out = []
    for b in range(grid):
        for w in range(WPB):
            if order >= 1:
                t0, jump, end = b * order * WPB + w, grid * order * WPB, ntasks
                at = lambda j: t0 + (j // order) * jump + (j % order) * WPB
            else:
                per = -(-ntasks // grid)
                t0, end = per * b + w, min(per * b + per, ntasks)
                at = lambda j: t0 + j * WPB
            tasks, j = [], 0
            while at(j) < end:
                tasks.append(at(j))
                j += 1
            out.append(tasks)
    return out


def _check_schedule(erased, valid, order, grid):
    walks = _walks(S * NWIN, order, grid)
    assert sorted(t for w in walks for t in w) == list(range(S * NWIN))  # every window once
    longest = max(len(w) for w in walks)
    if longest < 3:
        return longest
    assert sib._all_six(walks, lambda task, t: sib._out_case(erased, valid, task, t), range(2)), \
        "no output position sees all six case transitions along the waves' walks"
    assert sib._all_six(walks, lambda task, r: sib._in_case(erased, valid, task, r), range(sib.K)), \
        "no input position sees all six case transitions along the waves' walks"
    assert any(sib._skipped(erased, valid, a) and not sib._skipped(erased, valid, b)
               for w in walks for a, b in zip(w, w[1:])), "no skipped task is followed by a live one"
    return longest


_cache = {}


def _batch():
    if not _cache:
        st, erased, valid, want = sib._batch()
        _cache["b"] = (st, erased, valid, want, expected_crcs(want, erased, valid, seeded(erased.shape)))
    return _cache["b"]


@pytest.mark.parametrize("order,longest", [(1, 1), (32, 16), (0, 1)])
def test_window_orders_device(cuda, monkeypatch, order, longest):
    torch = cuda
    stripes, erased, valid, want, crcs = _batch()
    grid = min(S * NWIN // WPB, sib._cus(torch))  # one block per CU
    got = _check_schedule(erased, valid, order, grid)
    assert grid != 16 or got == longest  # 16 blocks: any device with 16 CUs or more
    monkeypatch.setenv("HRS_TASK_ORDER", str(order))
    code = make_code(CFG)
    t = torch.from_numpy(stripes.copy()).to("cuda:0")
    out = torch.full(want.shape, SENTINEL, dtype=torch.uint8, device="cuda:0")
    crc = device.decode_batch_ragged_crc(code, t, erased, out, valid, crc_in=as_i32(torch, seeded(erased.shape)))
    assert code.lastKernel() == KERNEL
    torch.cuda.synchronize()
    d = mismatch(out.cpu().numpy(), want, erased, valid)
    assert d is None, d
    d = crc_mismatch(crc.cpu().numpy().view(np.uint32), crcs)
    assert d is None, d


@pytest.mark.parametrize("cap", [1, 2])
def test_capped_grid_pinned_host_batch(cuda, monkeypatch, cap):
    torch = cuda
    sib._cus(torch)
    stripes, erased, valid, want, crcs = _batch()
    assert _check_schedule(erased, valid, 1, cap) == S * NWIN // (cap * WPB)
    monkeypatch.setenv("HRS_ZC_BLOCKS", str(cap))
    monkeypatch.delenv("HRS_TASK_ORDER", raising=False)
    monkeypatch.delenv("HRS_ZEROCOPY", raising=False)
    code = make_code(CFG)
    t = torch.from_numpy(stripes.copy()).pin_memory()
    out = torch.full(want.shape, SENTINEL, dtype=torch.uint8).pin_memory()
    crc = device.decode_batch_host_ragged_crc(code, t, erased, out, valid, crc_in=seeded(erased.shape))
    assert code.lastHostPath() == "pinned" and code.lastKernel() == KERNEL
    d = mismatch(out.numpy(), want, erased, valid)
    assert d is None, d
    d = crc_mismatch(crc, crcs)
    assert d is None, d
    assert (t.numpy() == stripes).all()
