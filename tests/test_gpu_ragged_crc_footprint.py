"""Footprint of hrs_encode_ragged_crc_dev, by the arena convention of
DESIGN.md §4 (gpu_arena.py): the parity and data rows of every stripe lie in
one guarded arena and the CRC words in another; the call runs on strided views
of the device copies, and ONE comparison per arena against the pre-call image
with exactly the parity rows, and exactly crc_out, replaced shows that the
data cells (their unused tails included), crc_in when it is a distinct array,
the guards and everything else are untouched. Both routes: the aligned
placement on whole windows takes the fused kernel in mode 0, everything else
(a shifted or padded placement, a row tail, mode 1, a code without a static
network) the ragged encode, the ragged window pass and the fold."""
import zlib

import numpy as np
import pytest

from gpu_arena import Arena, CrcArena
from lambdafs_amd import _lib
from ragged_crc_inputs import fused_kernel
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


@pytest.mark.parametrize("mode,with_in", [(0, True), (0, False), (1, True)])
@pytest.mark.parametrize("place", list(PLACEMENTS))
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("cfg", CODES, ids=code_id)
def test_ragged_encode_crc_footprint(cuda, cfg, L, place, mode, with_in):
    torch = cuda
    k, p = cfg[1], cfg[2]
    shift, pad = PLACEMENTS[place]
    arena = Arena(S, L, shift=shift, stripe_pad=pad, seed=1000 * k + 10 * p + L % 7)
    pnames = arena.add_rows("parity", p, "output")  # hops order: parity first
    dnames = arena.add_rows("data", k, "input")
    words = CrcArena(S, k + p, with_in, seed=k + L)
    valid = _valid(k, L)
    cin = words.crc_in()
    pre = [arena.pre(n) for n in dnames]
    par, crcs = [], np.zeros((S, k + p), np.uint32)
    for s in range(S):
        rows = [pre[j][s].copy() for j in range(k)]
        for j in range(k):
            rows[j][int(valid[s, j]):] = 0
        par.append(ref_parity(cfg, rows))
        for r, row in enumerate(rows + list(par[s])):
            crcs[s, r] = zlib.crc32(np.asarray(row, np.uint8).tobytes(), int(cin[s, r]) if with_in else 0)
    want = {pnames[o]: np.stack([par[s][o] for s in range(S)]) for o in range(p)}
    code = make_code(cfg, mode)
    flat, views = arena.to_device()
    wflat, in_ptr, out_ptr = words.to_device()
    ins = _lib.ptr_array([views[n].data_ptr() for n in dnames])
    outs = _lib.ptr_array([views[n].data_ptr() for n in pnames])
    code._check(_lib.lib().hrs_encode_ragged_crc_dev(code._handle(), ins, arena.stripe_stride, outs,
                                                     arena.stripe_stride, L, S, valid.ctypes.data, in_ptr, out_ptr,
                                                     torch.cuda.current_stream().cuda_stream))
    kernel = code.lastKernel()
    torch.cuda.synchronize()
    d = arena.diff(flat.cpu().numpy(), arena.expected(want))
    assert d is None, d
    d = words.diff(wflat.cpu().numpy(), words.expected(crcs))
    assert d is None, d
    static = cfg[0] != "xor"
    if static and mode == 0 and place == "aligned" and L % WINDOW == 0:
        assert kernel == fused_kernel(cfg)
    else:
        assert kernel == (vector_kernel(cfg) if static and place == "aligned" and L >= WINDOW else BYTEWISE)
