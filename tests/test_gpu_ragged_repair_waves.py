"""batch_ragged_kernel with many windows per wave, under every window order and
on a capped grid. RS(10,4), 16 KiB cells (8 windows), 24 stripes that lost one
or two cells in turn: 192 window tasks of batch_ragged_kernel<2, 12>. A cell's
windows are full up to its boundary and dead behind it, and the boundaries are
spread so that along a wave's walk some input position AND some output
position goes from any of the three cases (full, boundary, dead) to any other,
and a task whose outputs are all dead (skipped before any load) is followed by
a live one: a case carried over from the window before (planes, masks, a
skipped load or a skipped task's state left in a register) shows in an output.

The window -> wave assignment of wave_tasks (hrs_device.hpp) is restated here
and checked for what each launch can show. The device call's grid is 48
blocks, so under HRS_TASK_ORDER 1 and 0 every wave runs one window (those two
launches check the orders' coverage); under order 32 two blocks run all 192,
32 and 16 per wave. The pinned host batch runs on a grid capped at 1 and 2
blocks (HRS_ZC_BLOCKS): 48 and 24 windows per wave. Wherever a wave runs three
or more windows, the transitions are required."""
import os

import numpy as np
import pytest

from lambdafs_amd import device
from ragged_repair_inputs import (SENTINEL, WINDOW, expected, expected_kernel, fresh_stripes, live_inputs, lost_of,
                                  make_code, mismatch)

pytestmark = pytest.mark.gpu

CFG = ("rs", 10, 4, 0)
K, P = 10, 4
N = K + P
L, S = 8 * WINDOW, 24
NWIN = L // WINDOW
WPB = 4  # waves per 256-thread block (kWavesPerBlock)
KERNEL = "batch_ragged_kernel<2, 12>"

# a boundary inside every window, at its first, second, a middle and its last
# byte in turn; no bytes; whole windows only (no boundary window); a full cell
BOUNDS = [w * WINDOW + d for w, d in zip(range(NWIN), (1, 2, 1000, 2047, 16, 17, 1, 1025))] + [0, 2 * WINDOW, 6 * WINDOW, L]


def _inputs():
    erased = np.full((S, 2), -1, np.int32)
    for s in range(S):
        lost = sorted({(3 * s) % N} | ({(3 * s + 5) % N} if s % 2 else set()))
        erased[s, :len(lost)] = lost
    valid = np.array([[BOUNDS[(5 * s + 7 * l) % len(BOUNDS)] for l in range(N)] for s in range(S)], np.uint32)
    return erased, valid


_cache = {}


def _batch():
    if not _cache:
        erased, valid = _inputs()
        st = fresh_stripes(CFG, S, L, seed=3)
        _cache["b"] = (st, erased, valid, expected(CFG, st, erased, valid))
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


def _case(v, task):
    lo = (task % NWIN) * WINDOW
    return "dead" if v <= lo else "full" if v >= lo + WINDOW else "boundary"


def _in_case(erased, valid, task, r):
    """Input position r of the task's plan (a position the plan does not use is dead: the table says 0)."""
    s = task // NWIN
    live = live_inputs(CFG, tuple(lost_of(erased[s])))
    return _case(int(valid[s, live[r]]) if r < len(live) else 0, task)


def _out_case(erased, valid, task, t):
    s = task // NWIN
    lost = lost_of(erased[s])
    return _case(int(valid[s, lost[t]]) if t < len(lost) else 0, task)


def _skipped(erased, valid, task):
    return all(_out_case(erased, valid, task, t) == "dead" for t in range(2))


def _all_six(walks, case, positions):
    for pos in positions:
        seen = {(case(a, pos), case(b, pos)) for w in walks for a, b in zip(w, w[1:])}
        if len({t for t in seen if t[0] != t[1]}) == 6:
            return True
    return False


def _check_schedule(erased, valid, order, grid):
    walks = _walks(S * NWIN, order, grid)
    assert sorted(t for w in walks for t in w) == list(range(S * NWIN))  # every window once
    longest = max(len(w) for w in walks)
    if longest < 3:
        return longest
    assert _all_six(walks, lambda task, r: _in_case(erased, valid, task, r), range(K)), \
        "no input position sees all six case transitions along the waves' walks"
    assert _all_six(walks, lambda task, t: _out_case(erased, valid, task, t), range(2)), \
        "no output position sees all six case transitions along the waves' walks"
    assert any(_skipped(erased, valid, a) and not _skipped(erased, valid, b) for w in walks for a, b in zip(w, w[1:])), \
        "no skipped task is followed by a live one"
    return longest


def _cus(torch):
    assert "HRS_BLOCKS_PER_CU" not in os.environ, \
        "HRS_BLOCKS_PER_CU changes the grid these cases' wave schedules are checked for: unset it"
    return torch.cuda.get_device_properties(0).multi_processor_count


def test_the_batch_is_what_the_docstring_says():
    erased, _ = _inputs()
    assert expected_kernel(CFG, erased) == KERNEL
    assert {len(lost_of(r)) for r in erased} == {1, 2}
    assert all(len(live_inputs(CFG, tuple(lost_of(r)))) == K for r in erased)


@pytest.mark.parametrize("order,longest", [(1, 1), (32, 32), (0, 1)])
def test_window_orders_device(cuda, monkeypatch, order, longest):
    torch = cuda
    stripes, erased, valid, want = _batch()
    grid = min(S * NWIN // WPB, 2 * _cus(torch))  # 2 blocks per CU: <2, 12> keeps the unrolled bit loop
    got = _check_schedule(erased, valid, order, grid)
    assert grid != 48 or got == longest  # 48 blocks: any device with 24 CUs or more
    monkeypatch.setenv("HRS_TASK_ORDER", str(order))
    code = make_code(CFG)
    t = torch.from_numpy(stripes.copy()).to("cuda:0")
    out = torch.full(want.shape, SENTINEL, dtype=torch.uint8, device="cuda:0")
    device.decode_batch_ragged(code, t, erased, out, valid)
    assert code.lastKernel() == KERNEL
    torch.cuda.synchronize()
    d = mismatch(out.cpu().numpy(), want, erased, valid)
    assert d is None, d


@pytest.mark.parametrize("cap", [1, 2])
def test_capped_grid_pinned_host_batch(cuda, monkeypatch, cap):
    torch = cuda
    _cus(torch)
    stripes, erased, valid, want = _batch()
    assert _check_schedule(erased, valid, 1, cap) == S * NWIN // (cap * WPB)
    monkeypatch.setenv("HRS_ZC_BLOCKS", str(cap))
    monkeypatch.delenv("HRS_TASK_ORDER", raising=False)
    monkeypatch.delenv("HRS_ZEROCOPY", raising=False)
    code = make_code(CFG)
    t = torch.from_numpy(stripes.copy()).pin_memory()
    out = torch.full(want.shape, SENTINEL, dtype=torch.uint8).pin_memory()
    device.decode_batch_host_ragged(code, t, erased, out, valid)
    assert code.lastHostPath() == "pinned" and code.lastKernel() == KERNEL
    d = mismatch(out.numpy(), want, erased, valid)
    assert d is None, d
    assert (t.numpy() == stripes).all()
