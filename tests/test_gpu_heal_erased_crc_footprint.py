"""Footprint of hrs_heal_erased_crc_dev ("Footprint tests"): the
stripes in a guarded uint8 arena, the reports and the CRC words in guarded
int32 arenas (tests/gpu_arena.py). One comparison of the whole arena against
its pre-call image with exactly the erased cells and the planted bytes
replaced by the oracle-encoded stripes; the report and CRC buffers are written
only inside their 4 + n and n words per stripe. Each case runs with the erased
cells pre-filled with 0xA5 and with 0x00: lost cells are never read, so the
results are identical."""
import random

import numpy as np
import pytest

import heal_erased_inputs as H
from gpu_arena import Arena, CrcArena
from lambdafs_amd import HipReedSolomonCode, _lib
from test_gpu_scrub_crc import crcs_of

pytestmark = pytest.mark.gpu

K, P, S = 10, 4, 7
N = K + P

# name -> (L, shift, stripe_pad, kernel mode, hrs_last_kernel, with crc_in)
CASES = {
    "fused": (2 * H.WINDOW, 0, 0, 3, "heal_erased_crc_kernel<4>", True),
    "fused_fresh": (2 * H.WINDOW, 0, 0, 3, "heal_erased_crc_kernel<4>", False),
    "windows_and_tail": (H.WINDOW + 100, 0, 0, 3, "heal_erased_kernel<4>", True),
    "shift_1": (H.WINDOW + 100, 1, 0, 3, "heal_erased_bytewise_kernel<4>", True),
    "mode_2": (2 * H.WINDOW, 0, 0, 2, "heal_erased_bytewise_kernel<4>", False),
}


def _run(torch, name, fill):
    L, shift, pad, mode, kernel, with_in = CASES[name]
    clean = H.clean_stripes(K, P, S, L, 21)
    pats = H.seven_patterns(K, P, random.Random(L + shift + pad))
    bad, planted = H.plant(K, P, clean, pats, H.columns_of(L), seed=L)
    bad = np.array(bad)
    for s in range(S):
        bad[s, pats[s], :] = fill
    arena = Arena(S, L, shift=shift, stripe_pad=pad, seed=L + shift)
    names = arena.add_rows("loc", N, "input")
    flat, _ = arena.to_device()
    st = arena.stack(flat, names)
    st.copy_(torch.from_numpy(bad).to("cuda:0"))  # the damaged stripes replace the random rows
    pre = flat.cpu().numpy()
    reps = CrcArena(S, 4 + N, False)  # its "crc_out" block is the reports, report_stride = 4 + n
    rflat, _, rout = reps.to_device()
    crcs = CrcArena(S, N, with_in, seed=L)
    cflat, cin, cout = crcs.to_device()
    code = HipReedSolomonCode(K, P, device=0)
    code.setKernelMode(mode)
    rows = _lib.ptr_array([st.data_ptr() + l * st.stride(1) for l in range(N)])
    arr = H.erased_array(pats)
    code._check(_lib.lib().hrs_heal_erased_crc_dev(code._handle(), rows, st.stride(0), L, S, arr.ctypes.data,
                                                   arr.shape[1], rout, 4 + N, cin, cout,
                                                   torch.cuda.current_stream().cuda_stream))
    assert code.lastKernel() == kernel
    torch.cuda.synchronize()
    exp = pre.copy()
    for l, x in enumerate(names):
        for s in range(S):
            o = arena.offset(x, s)
            assert (exp[o:o + L] == bad[s, l]).all()
            exp[o:o + L] = clean[s, l]
    want = H.planted_reports(N, S, planted)
    # exactly the erased cells (where they differ from their fill) and the planted bytes
    filled = sum(int(np.count_nonzero(clean[s, pats[s]] != fill)) for s in range(S))
    assert np.count_nonzero(exp != pre) == filled + int(want[:, 3].sum()) and want[:, 3].sum() > 0
    after = flat.cpu().numpy()
    d = arena.diff(after, exp)
    assert d is None, d
    d = reps.diff(rflat.cpu().numpy(), reps.expected(want))
    assert d is None, d
    words = cflat.cpu().numpy()
    d = crcs.diff(words, crcs.expected(crcs_of(clean, crcs.crc_in())))
    assert d is None, d
    return after, rflat.cpu().numpy(), words


@pytest.mark.parametrize("name", list(CASES))
def test_heal_erased_crc_footprint(cuda, name):
    a5 = _run(cuda, name, H.FILL)
    zero = _run(cuda, name, 0x00)
    for x, y in zip(a5, zero):
        assert (x == y).all()
