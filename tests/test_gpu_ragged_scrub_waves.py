"""The ragged scrub and heal kernels with several windows per wave, under
HRS_TASK_ORDER 1, 0, 2 and 32, by the method of tests/test_gpu_scrub_waves.py:
the window -> wave assignment of wave_tasks (hrs_device.hpp) is restated here
and a CPU test asserts that, under order 32 (one block, 20 windows per wave),
some wave meets each hand-over the per-task state of scrub_ragged_kernel has to
survive:
  gap       dirty -> clean -> dirty (the histogram re-armed by the flush);
  dead      live -> wholly-dead window -> live (the early continue);
  handover  two consecutive dirty windows of different stripes;
  rearm     a window whose top rows are dead (the Horner step skipped), then one
            whose top row is live, and the other way round (the skip flag is
            per task).
Expectations are the oracle's (tests/ragged_scrub_inputs.py)."""
import os

import pytest

import ragged_scrub_inputs as R
from test_gpu_ragged_scrub import run_case
from test_gpu_scrub_waves import _grid, _wave_tasks

K, P, L = 10, 4, R.L_BIG
N = K + P
ORDERS = [1, 0, 2, 32]


def _facts(order, cus=256):
    stored, valid, _, _, _, classes, _ = R.batch(K, P, L)
    S, nwin = stored.shape[0], L // R.WINDOW
    ntasks = S * nwin
    waves = _wave_tasks(ntasks, order, _grid(ntasks, cus))
    assert sorted(t for w in waves for t in w) == list(range(ntasks))  # every window once

    def facts(t):
        s, lo = t // nwin, t % nwin * R.WINDOW
        dirty = any(lo <= c < lo + R.WINDOW for c in classes["bad"][s])
        live = int(valid[s].max()) > lo
        top_dead = live and int(valid[s, N - 1]) <= lo
        return s, dirty, live, top_dead

    shown = set()
    for tasks in waves:
        seq = [facts(t) for t in tasks]
        for a, b in zip(seq, seq[1:]):
            if a[1] and b[1] and a[0] != b[0]:
                shown.add("handover")
            if a[2] and b[2] and a[3] and not b[3]:
                shown.add("rearm_live")
            if a[2] and b[2] and not a[3] and b[3]:
                shown.add("rearm_dead")
        for a, b, c in zip(seq, seq[1:], seq[2:]):
            if a[1] and b[2] and not b[1] and c[1]:
                shown.add("gap")
            if a[2] and not b[2] and c[2]:
                shown.add("dead")
    return max(len(w) for w in waves), shown


@pytest.mark.parametrize("order", ORDERS)
def test_schedules_meet_every_handover(order):
    longest, shown = _facts(order)
    print(f"order {order}: longest run {longest} windows, shows {sorted(shown)}")
    assert longest == {1: 1, 0: 1, 2: 2, 32: 20}[order]
    if order == 32:
        assert shown == {"gap", "dead", "handover", "rearm_live", "rearm_dead"}
    elif order == 2:
        assert "handover" in shown


@pytest.mark.gpu
@pytest.mark.parametrize("order", ORDERS)
def test_window_orders(cuda, monkeypatch, order):
    assert "HRS_BLOCKS_PER_CU" not in os.environ
    cus = cuda.cuda.get_device_properties(0).multi_processor_count
    if order == 32:
        assert _facts(order, cus)[1] >= {"gap", "dead", "handover", "rearm_live", "rearm_dead"}
    monkeypatch.setenv("HRS_TASK_ORDER", str(order))
    run_case(cuda, K, P, L, 0)
