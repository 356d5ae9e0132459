"""Footprint of hrs_decode_batch_crc_dev ("Footprint tests"): the
stripes and outputs in a guarded uint8 arena, crc_in / crc_out in a guarded
int32 arena (tests/gpu_arena.py). One comparison of each whole arena against
its pre-call image with exactly these replaced: the present output rows (the
oracle's), and ALL S * E CRC words (zlib for the present outputs, the crc_in
value for the absent ones). Guards, inputs, crc_in and the absent outputs'
poison stay intact."""
import zlib

import numpy as np
import pytest

from gpu_arena import POISON, Arena, CrcArena
from lambdafs_amd import HipReedSolomonCode, _lib
from oracle import rs_oracle as C

pytestmark = pytest.mark.gpu

K, P = 10, 4
LISTS = ((5,), (0, 13), (), (2, 7, 11))  # per-stripe losses; E = 4: every stripe has absent outputs
E = 4

# (L, shift, stripe pad, with crc_in, kernel)
CASES = {
    "whole_windows_aligned": (2048 * 3, 0, 0, True, "batch_decode_crc_kernel<3, 12, 768>"),
    "whole_windows_fresh": (2048, 0, 0, False, "batch_decode_crc_kernel<3, 12, 768>"),
    "tail": (2048 * 3 + 100, 0, 0, True, "batch_bitsliced_kernel<3, 12, true>"),
    "shift_1": (2048 * 3, 1, 0, True, "batch_bytewise_kernel"),
    "stripe_pad_5": (2048 * 3, 0, 5, False, "batch_bytewise_kernel"),
}


@pytest.mark.parametrize("name", list(CASES))
def test_decode_batch_crc_footprint(cuda, name):
    torch = cuda
    L, shift, pad, with_in, kernel = CASES[name]
    n, S = K + P, len(LISTS)
    arena = Arena(S, L, shift=shift, stripe_pad=pad, seed=L + shift + pad)
    snames = arena.add_rows("loc", n, "input")
    onames = arena.add_rows("out", E, "output")
    pre = [arena.pre(x) for x in snames]
    zero = np.zeros(L, np.uint8)
    crcs = CrcArena(S, E, with_in, seed=L)
    start = crcs.crc_in()
    words = np.zeros((S, E), np.uint32) if start is None else start.copy()
    er = np.full((S, E), -1, dtype=np.int32)
    want = {o: np.full((S, L), POISON, np.uint8) for o in onames}
    for s, erased in enumerate(LISTS):
        erased = list(erased)
        er[s, :len(erased)] = erased
        if not erased:
            continue
        to_read = sorted(C.locations_to_read(K, P, erased))
        ntr = [x for x in range(n) if x not in to_read or x in erased]
        ref = C.decode_bulk5(K, P, [zero if x in ntr else pre[x][s] for x in range(n)], erased, to_read, ntr)
        for t in range(len(erased)):
            want[onames[t]][s] = ref[t]
            words[s, t] = zlib.crc32(np.asarray(ref[t], np.uint8).tobytes(), int(words[s, t]))
    code = HipReedSolomonCode(K, P, device=0)
    flat, _ = arena.to_device()
    cflat, cin, cout = crcs.to_device()
    st, out = arena.stack(flat, snames), arena.stack(flat, onames)
    code._check(_lib.lib().hrs_decode_batch_crc_dev(
        code._handle(), st.data_ptr(), st.stride(1), st.stride(0), er.ctypes.data, E, out.data_ptr(), out.stride(1),
        out.stride(0), L, S, cin, cout, torch.cuda.current_stream().cuda_stream))
    got_kernel = code.lastKernel()
    torch.cuda.synchronize()
    d = arena.diff(flat.cpu().numpy(), arena.expected(want))
    assert d is None, d
    d = crcs.diff(cflat.cpu().numpy(), crcs.expected(words))
    assert d is None, d
    assert got_kernel == kernel, got_kernel
