"""Footprint of hrs_decode_batch_ragged_dev, by the arena convention of
DESIGN.md §4 (gpu_arena.py): the n cells and the output rows of every stripe
lie in one guarded arena, the call runs on strided views of its device copy,
and ONE comparison of the whole arena against the pre-call image, with exactly
the leading valid bytes of each stripe's outputs replaced, shows that the
survivors (their unused tails included), the guards, the output bytes at or
beyond each length and the output rows past a stripe's losses are untouched.
Placements: row starts shifted by 0 or 1 byte, stripes packed or 5 bytes
apart; only the first is 16-byte aligned and takes the vector kernel, the
others end in the byte-granular one."""
import numpy as np
import pytest

from gpu_arena import POISON, Arena
from lambdafs_amd import device
from ragged_repair_inputs import (BYTEWISE, WINDOW, code_id, decode_ref, expected_kernel, length_classes, lost_of,
                                  make_code, patterns, to_read)

pytestmark = pytest.mark.gpu

PLACEMENTS = {"aligned": (0, 0), "shift": (1, 0), "pad": (0, 5), "shift_pad": (1, 5)}
CODES = [("rs", 10, 4, 0), ("nrs", 6, 3, 0), ("rs", 12, 4, 0), ("xor", 4, 1, 0)]
LENGTHS = [2 * WINDOW, 2 * WINDOW + 80, 80]
S = 5


def _inputs(cfg, L):
    k, p = cfg[1], cfg[2]
    n = k + p
    V = length_classes(L)
    valid = np.array([[V[(5 * s + 3 * l) % len(V)] for l in range(n)] for s in range(S)], np.uint32)
    pats = patterns(cfg, p, seed=11)[::-1]  # p losses first; with S > p + 1 the rotation comes round
    erased = np.full((S, p), -1, np.int32)
    for s in range(S):
        erased[s, :len(pats[s % len(pats)])] = pats[s % len(pats)]
    valid[S - 1, :p] = L  # the last stripe is a file tail that lost data cell 0: half full, half empty
    valid[S - 1, p:p + k // 2] = L
    valid[S - 1, p + k // 2:] = 0
    erased[S - 1] = [p] + [-1] * (p - 1)
    return erased, valid


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("place", list(PLACEMENTS))
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("cfg", CODES, ids=code_id)
def test_ragged_repair_footprint(cuda, cfg, L, place, mode):
    torch = cuda
    k, p = cfg[1], cfg[2]
    n = k + p
    shift, pad = PLACEMENTS[place]
    arena = Arena(S, L, shift=shift, stripe_pad=pad, seed=1000 * k + 10 * p + L % 7)
    cells = arena.add_rows("cell", n, "input")  # hops order
    outs = arena.add_rows("out", p, "output")
    erased, valid = _inputs(cfg, L)
    pre = [arena.pre(name) for name in cells]
    want = {name: np.full((S, L), POISON, np.uint8) for name in outs}
    for s in range(S):
        lost = lost_of(erased[s])
        if not lost:
            continue
        tr = to_read(cfg, lost)
        reads = [pre[x][s].copy() for x in range(n)]
        for x in tr:
            reads[x][int(valid[s, x]):] = 0
        ref = decode_ref(cfg, reads, lost, tr)
        for t, e in enumerate(lost):
            v = int(valid[s, e])
            want[outs[t]][s, :v] = ref[t][:v]
    code = make_code(cfg, mode)
    flat, _ = arena.to_device()
    device.decode_batch_ragged(code, arena.stack(flat, cells), erased, arena.stack(flat, outs), valid)
    kernel = code.lastKernel()
    torch.cuda.synchronize()
    d = arena.diff(flat.cpu().numpy(), arena.expected(want))
    assert d is None, d
    vector = mode == 0 and place == "aligned" and L >= WINDOW
    assert kernel == (expected_kernel(cfg, erased) if vector else BYTEWISE)
