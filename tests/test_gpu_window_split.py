"""The window map (hrs_window_map.hpp; HRS_WINDOW_SPLIT = the half distance H
between a wave task's two 1 KiB pieces) on the kernels that take it: the RS
and nrs (10,4) static encodes, the 1- to 4-loss runtime-matrix repairs, the
streaming kernel (a 20-input, 2-output apply) and the chunked accumulate
launches (the same apply under HRS_STREAM=0, in a child process: the library
reads that variable once). H in {2048, 65536} crossed with the window orders
HRS_TASK_ORDER in {1, 0, 2}, at shapes that put a row through every part of
the map: one group, group + contiguous window + tail, several groups, a short
last block, and a row shorter than a group (all contiguous).

Bar: bit-exact, the whole output tensor against the byte-granular kernel
(kernel mode 2), which the oracle checks on stripes 0, S/2 and S - 1
(tests/window_split_cases.py). A wrong map writes H bytes away, not next door,
so the encode and the 1-loss repair also run in a guarded arena
(tests/gpu_arena.py) with at least H guard bytes on both sides of every row.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import window_split_cases as W
from gpu_arena import Arena
from lambdafs_amd import HipReedSolomonCode, device
from oracle import rs_oracle as C

pytestmark = pytest.mark.gpu

GRID = [(h, s, l) for h in W.SHAPES for (s, l) in W.SHAPES[h]]
GRID_IDS = [f"H{h}-{s}x{l}" for h, s, l in GRID]


@pytest.fixture(params=W.ORDERS, ids=["grid_stride", "block_range", "cyclic2"])
def order(request, monkeypatch):
    monkeypatch.setenv("HRS_TASK_ORDER", str(request.param))
    return request.param


@pytest.fixture
def split(monkeypatch):
    def set_split(h):
        monkeypatch.setenv("HRS_WINDOW_SPLIT", str(h))
    return set_split


@pytest.mark.parametrize("H,S,L", GRID, ids=GRID_IDS)
@pytest.mark.parametrize("kind", ["rs", "nrs"])
def test_encode(cuda, order, split, kind, H, S, L):
    split(H)
    W.check_encode(cuda, kind, S, L)


@pytest.mark.parametrize("H,S,L", GRID, ids=GRID_IDS)
@pytest.mark.parametrize("erased", W.ERASED, ids=lambda e: "e" + "_".join(map(str, e)))
def test_repair(cuda, order, split, erased, H, S, L):
    split(H)
    W.check_repair(cuda, erased, S, L)


@pytest.mark.parametrize("H,S,L", GRID, ids=GRID_IDS)
def test_apply_streaming(cuda, order, split, H, S, L):
    assert "HRS_STREAM" not in os.environ, "HRS_STREAM changes the route this case is checked for: unset it"
    split(H)
    W.check_apply(cuda, S, L, W.KERNELS["apply_stream"])


def test_apply_chunked_accumulate_in_a_child_process(cuda):
    """HRS_STREAM is read once per process: the 16 + 4 input accumulate
    launches of the same apply run in one fresh child started with
    HRS_STREAM=0, over every (H, order, shape)."""
    # 24 small cases after python, torch and the library have started (a few seconds in all);
    # 120 s is many times that for a busy machine; a child still running then hangs.
    env = {k: v for k, v in os.environ.items() if k not in ("HRS_WINDOW_SPLIT", "HRS_TASK_ORDER")}
    child = subprocess.run([sys.executable, os.path.join(W.ROOT, "tests", "window_split_cases.py"), "stream0"],
                           cwd=W.ROOT, env={**env, "HRS_STREAM": "0"}, timeout=120, capture_output=True, text=True)
    assert child.returncode == 0, child.stdout[-2000:] + child.stderr[-4000:]
    lines = [json.loads(line) for line in child.stdout.splitlines() if line.startswith("{")]
    assert [(x["split"], x["order"], x["S"], x["L"]) for x in lines] == W.CASES
    assert all(x["error"] is None for x in lines), [x for x in lines if x["error"]]


# ------------------------------------------------------------ guarded arena

class WideArena(Arena):
    """An arena whose rows have at least `margin` guard bytes before and
    after them: the row pitch carries the margin, the first row starts that
    far in, and a last input row no call touches keeps the final output row's
    far side covered beyond the arena's own 4 KiB."""

    def __init__(self, S, L, margin, seed):
        super().__init__(S, L, seed=seed)
        self.row_pitch = (L + margin + 15) // 16 * 16
        self.base = (margin + 15) // 16 * 16
        self.margin = margin

    def close(self):
        self.add("far_side", "input")
        assert self.row_pitch - self.L >= self.margin and self.base >= self.margin


def _finish(torch, arena, flat, outputs):
    torch.cuda.synchronize()
    d = arena.diff(flat.cpu().numpy(), arena.expected(outputs))
    assert d is None, d


ARENA_SHAPES = {2048: (3, 4096 + 2048 + 96), 65536: (2, 131072 + 2048 + 96)}  # group + window + tail, 16-byte aligned rows


@pytest.mark.parametrize("H", sorted(ARENA_SHAPES))
def test_encode_in_guarded_arena(cuda, split, H):
    split(H)
    S, L = ARENA_SHAPES[H]
    k, p = W.K, W.P
    arena = WideArena(S, L, margin=H, seed=H + 1)
    dnames = arena.add_rows("data", k, "input")
    pnames = arena.add_rows("parity", p, "output")
    arena.close()
    pre = [arena.pre(n) for n in dnames]
    par = [C.encode_bulk(k, p, [pre[i][s] for i in range(k)]) for s in range(S)]
    want = {pnames[o]: np.stack([par[s][o] for s in range(S)]) for o in range(p)}
    code = HipReedSolomonCode(k, p, device=0)
    flat, v = arena.to_device()
    assert arena.aligned16()
    device.encode_rows(code, [v[n] for n in dnames], [v[n] for n in pnames])
    assert code.lastKernel() == W.KERNELS["rs"]
    _finish(cuda, arena, flat, want)


@pytest.mark.parametrize("H", sorted(ARENA_SHAPES))
def test_single_loss_repair_in_guarded_arena(cuda, split, H):
    split(H)
    S, L = ARENA_SHAPES[H]
    k, p, n = W.K, W.P, W.N
    erased = [4]
    arena = WideArena(S, L, margin=H, seed=H + 2)
    snames = arena.add_rows("loc", n, "input")
    onames = arena.add_rows("out", 1, "output")
    arena.close()
    to_read = sorted(C.locations_to_read(k, p, erased))
    ntr = [x for x in range(n) if x not in to_read]
    pre = [arena.pre(x) for x in snames]
    zero = np.zeros(L, np.uint8)
    want = {onames[0]: np.empty((S, L), np.uint8)}
    for s in range(S):
        reads = [pre[x][s] if x in to_read else zero for x in range(n)]
        want[onames[0]][s] = C.decode_bulk5(k, p, reads, erased, to_read, ntr)[0]
    code = HipReedSolomonCode(k, p, device=0)
    flat, _ = arena.to_device()
    assert arena.aligned16()
    device.decode_stripes(code, arena.stack(flat, snames), erased, ntr, arena.stack(flat, onames))
    assert code.lastKernel() == W.KERNELS[1]
    _finish(cuda, arena, flat, want)
