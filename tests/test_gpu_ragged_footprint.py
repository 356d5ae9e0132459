"""Footprint of hrs_encode_ragged_dev, by the arena convention of DESIGN.md §4
(gpu_arena.py): the parity and data rows of every stripe lie in one guarded
arena, the call runs on strided views of its device copy, and ONE comparison
of the whole arena against the pre-call image with exactly the parity rows
replaced shows that the data cells (their unused tails included), the guards
and everything else are untouched. Placements: row starts shifted by 0 or 1
byte, stripes packed or 5 bytes apart; only the first is 16-byte aligned and
takes the vector kernel, the others end in the byte-granular one."""
import numpy as np
import pytest

from gpu_arena import Arena
from lambdafs_amd import device
from ragged_inputs import BYTEWISE, WINDOW, code_id, make_code, ref_parity, valid_classes, vector_kernel

pytestmark = pytest.mark.gpu

PLACEMENTS = {"aligned": (0, 0), "shift": (1, 0), "pad": (0, 5), "shift_pad": (1, 5)}
CODES = [("rs", 10, 4, 0), ("nrs", 6, 3, 0), ("rs", 12, 4, 0), ("xor", 4, 1, 0)]
LENGTHS = [2 * WINDOW, 2 * WINDOW + 80, 80]
S = 4


def _valid(k, L):
    V = valid_classes(L)
    v = np.array([[V[(5 * s + 3 * j) % len(V)] for j in range(k)] for s in range(S)], np.uint32)
    v[S - 1, : k // 2] = L  # the last stripe is a file tail: half full, half empty
    v[S - 1, k // 2:] = 0
    return v


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("place", list(PLACEMENTS))
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("cfg", CODES, ids=code_id)
def test_ragged_encode_footprint(cuda, cfg, L, place, mode):
    torch = cuda
    k, p = cfg[1], cfg[2]
    shift, pad = PLACEMENTS[place]
    arena = Arena(S, L, shift=shift, stripe_pad=pad, seed=1000 * k + 10 * p + L % 7)
    pnames = arena.add_rows("parity", p, "output")  # hops order: parity first
    dnames = arena.add_rows("data", k, "input")
    valid = _valid(k, L)
    pre = [arena.pre(n) for n in dnames]
    par = []
    for s in range(S):
        rows = [pre[j][s].copy() for j in range(k)]
        for j in range(k):
            rows[j][int(valid[s, j]):] = 0
        par.append(ref_parity(cfg, rows))
    want = {pnames[o]: np.stack([par[s][o] for s in range(S)]) for o in range(p)}
    code = make_code(cfg, mode)
    flat, _ = arena.to_device()
    device.encode_stripes_ragged(code, arena.stack(flat, pnames + dnames), valid)
    kernel = code.lastKernel()
    torch.cuda.synchronize()
    d = arena.diff(flat.cpu().numpy(), arena.expected(want))
    assert d is None, d
    vector = mode == 0 and place == "aligned" and L >= WINDOW
    assert kernel == (vector_kernel(cfg) if vector else BYTEWISE)
