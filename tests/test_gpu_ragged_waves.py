"""encode_ragged_kernel with many windows per wave, under every window order
and on a capped grid. RS(10,4), 16 KiB cells (8 windows), 24 stripes: 192
window tasks. A row's windows are full up to its boundary and dead behind it,
and the boundaries are spread so that along a wave's walk the same row
position goes from any of the three cases (full, boundary, dead) to any other:
a case carried over from the window before (planes, masks or a skipped load
left in a register) shows in the parity.

The window -> wave assignment of wave_tasks (hrs_device.hpp) is restated here
and checked for what each launch can show. The device call's grid is 48
blocks, so under HRS_TASK_ORDER 1 and 0 every wave runs one window (those two
launches check the orders' coverage); under order 32 two blocks run all 192,
32 and 16 per wave. The pinned host batch runs on a grid capped at 1 and 2
blocks (HRS_ZC_BLOCKS): 48 and 24 windows per wave. Wherever a wave runs three
or more windows, all six transitions are required of some row position."""
import os

import numpy as np
import pytest

from lambdafs_amd import device
from ragged_inputs import WINDOW, expected, fresh_stripes, make_code, mismatch, vector_kernel

pytestmark = pytest.mark.gpu

CFG = ("rs", 10, 4, 0)
K, P = 10, 4
L, S = 8 * WINDOW, 24
NWIN = L // WINDOW
WPB = 4  # waves per 256-thread block (kWavesPerBlock)

# a boundary inside every window, at its first, second, a middle and its last
# byte in turn; no bytes; whole windows only (no boundary window); a full cell
BOUNDS = [w * WINDOW + d for w, d in zip(range(NWIN), (1, 2, 1000, 2047, 16, 17, 1, 1025))] + [0, 2 * WINDOW, 6 * WINDOW, L]


def _valid():
    return np.array([[BOUNDS[(5 * s + 7 * j) % len(BOUNDS)] for j in range(K)] for s in range(S)], np.uint32)


_cache = {}


def _batch():
    if not _cache:
        valid = _valid()
        st = fresh_stripes(CFG, S, L, seed=3)
        _cache["b"] = (st, valid, expected(CFG, st, valid))
    return _cache["b"]


def _walks(ntasks, order, grid):
    """The tasks of every wave of the launch, in the order it runs them."""
    out = []
    for b in range(grid):
        for w in range(WPB):
            if order >= 1:
                t0, jump = b * order * WPB + w, grid * order * WPB
                at = lambda j: t0 + (j // order) * jump + (j % order) * WPB
                end = ntasks
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


def _case(valid, task, row):
    s, lo = divmod(task, NWIN)
    v, lo = int(valid[s, row]), lo * WINDOW
    return "dead" if v <= lo else "full" if v >= lo + WINDOW else "boundary"


def _check_schedule(valid, order, grid):
    walks = _walks(S * NWIN, order, grid)
    assert sorted(t for w in walks for t in w) == list(range(S * NWIN))  # every window once
    longest = max(len(w) for w in walks)
    if longest < 3:
        return longest
    for row in range(K):
        seen = {(_case(valid, a, row), _case(valid, b, row)) for w in walks for a, b in zip(w, w[1:])}
        if len({t for t in seen if t[0] != t[1]}) == 6:
            return longest
    pytest.fail("no row position sees all six case transitions along the waves' walks")


def _cus(torch):
    assert "HRS_BLOCKS_PER_CU" not in os.environ, \
        "HRS_BLOCKS_PER_CU changes the grid these cases' wave schedules are checked for: unset it"
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("order,longest", [(1, 1), (32, 32), (0, 1)])
def test_window_orders_device(cuda, monkeypatch, order, longest):
    torch = cuda
    stripes, valid, want = _batch()
    grid = min(S * NWIN // WPB, 2 * _cus(torch))
    got = _check_schedule(valid, order, grid)
    assert grid != 48 or got == longest  # 48 blocks: any device with 24 CUs or more
    monkeypatch.setenv("HRS_TASK_ORDER", str(order))
    code = make_code(CFG)
    t = torch.from_numpy(stripes.copy()).to("cuda:0")
    device.encode_stripes_ragged(code, t, valid)
    assert code.lastKernel() == vector_kernel(CFG)
    torch.cuda.synchronize()
    d = mismatch(t.cpu().numpy(), want, P)
    assert d is None, d


@pytest.mark.parametrize("cap", [1, 2])
def test_capped_grid_pinned_host_batch(cuda, monkeypatch, cap):
    torch = cuda
    _cus(torch)
    stripes, valid, want = _batch()
    assert _check_schedule(valid, 1, cap) == S * NWIN // (cap * WPB)
    monkeypatch.setenv("HRS_ZC_BLOCKS", str(cap))
    monkeypatch.delenv("HRS_TASK_ORDER", raising=False)
    monkeypatch.delenv("HRS_ZEROCOPY", raising=False)
    code = make_code(CFG)
    t = torch.from_numpy(stripes.copy()).pin_memory()
    device.encode_batch_host_ragged(code, t, valid)
    assert code.lastHostPath() == "pinned" and code.lastKernel() == vector_kernel(CFG)
    d = mismatch(t.numpy(), want, P)
    assert d is None, d
