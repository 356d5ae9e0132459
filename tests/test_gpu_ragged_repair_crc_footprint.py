"""Footprint of hrs_decode_batch_ragged_crc_dev, by the arena convention of
DESIGN.md §4 (gpu_arena.py): the n cells and the output rows of every stripe
lie in one guarded arena, the call runs on strided views of its device copy,
and ONE comparison of the whole arena against the pre-call image, with exactly
the leading valid bytes of each stripe's outputs replaced, shows that the
survivors (their unused tails included), the guards, the output bytes at or
beyond each length and the output rows past a stripe's losses are untouched.
The CRC words lie in a guarded array of their own: nothing outside crc_out is
written, and every word inside equals zlib over the cell's bytes. Output
lengths include a boundary at the last byte of a window and one at its first.
Placements: row starts shifted by 0 or 1 byte, stripes packed or 5 bytes apart;
only the first is 16-byte aligned and takes the fused kernel, the others end in
the byte-granular repair and the window pass."""
import zlib

import numpy as np
import pytest

from gpu_arena import POISON, Arena
from lambdafs_amd import device
from ragged_repair_inputs import BYTEWISE, WINDOW, code_id, decode_ref, expected_kernel, lost_of, make_code, to_read
from test_gpu_ragged_repair_crc import fused_kernel
from test_gpu_ragged_repair_footprint import PLACEMENTS, S, _inputs

pytestmark = pytest.mark.gpu

CODES = [("rs", 10, 4, 0), ("nrs", 6, 3, 0), ("xor", 4, 1, 0)]
LENGTHS = [2 * WINDOW, 2 * WINDOW + 80, 80]
GUARD = 64  # words around crc_out
CRC_POISON = 0x7E7E7E7E


def _lengths(cfg, L):
    """The sibling's batch; the first output of stripes 0 and 2 ends at the last byte of a window and at the first of one."""
    erased, valid = _inputs(cfg, L)
    if L >= 2 * WINDOW:  # stripes 0 and 2 lost something under every code here
        valid[0, lost_of(erased[0])[0]] = 2 * WINDOW - 1
        valid[2, lost_of(erased[2])[0]] = WINDOW + 1
    return erased, valid


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("place", list(PLACEMENTS))
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("cfg", CODES, ids=code_id)
def test_ragged_repair_crc_footprint(cuda, cfg, L, place, mode):
    torch = cuda
    k, p = cfg[1], cfg[2]
    n = k + p
    shift, pad = PLACEMENTS[place]
    arena = Arena(S, L, shift=shift, stripe_pad=pad, seed=1000 * k + 10 * p + L % 7)
    cells = arena.add_rows("cell", n, "input")  # hops order
    outs = arena.add_rows("out", p, "output")
    erased, valid = _lengths(cfg, L)
    pre = [arena.pre(name) for name in cells]
    want = {name: np.full((S, L), POISON, np.uint8) for name in outs}
    seeds = np.random.default_rng(L + k).integers(0, 2**32, (S, p), dtype=np.uint32)
    crcs = seeds.copy()
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
            crcs[s, t] = zlib.crc32(ref[t][:v].tobytes(), int(seeds[s, t]))
    code = make_code(cfg, mode)
    flat, _ = arena.to_device()
    words = np.full(GUARD + S * p + GUARD, CRC_POISON, np.uint32)
    words[GUARD:GUARD + S * p] = seeds.ravel()
    dwords = torch.from_numpy(words.view(np.int32).copy()).to("cuda:0")
    inner = dwords[GUARD:GUARD + S * p].view(S, p)
    got = device.decode_batch_ragged_crc(code, arena.stack(flat, cells), erased, arena.stack(flat, outs), valid,
                                         crc_in=inner, crc_out=inner)  # in place, inside the guards
    assert got is inner
    kernel = code.lastKernel()
    torch.cuda.synchronize()
    d = arena.diff(flat.cpu().numpy(), arena.expected(want))
    assert d is None, d
    after = dwords.cpu().numpy().view(np.uint32)
    assert (after[:GUARD] == CRC_POISON).all() and (after[GUARD + S * p:] == CRC_POISON).all()
    bad = np.argwhere(after[GUARD:GUARD + S * p].reshape(S, p) != crcs)
    assert bad.size == 0, (bad[0], valid[bad[0][0]], erased[bad[0][0]])
    aligned = mode == 0 and place == "aligned" and L >= WINDOW
    fused = fused_kernel(cfg, erased) if aligned and L % WINDOW == 0 else None
    assert kernel == (fused or (expected_kernel(cfg, erased) if aligned else BYTEWISE))
