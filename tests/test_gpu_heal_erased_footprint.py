"""Footprint of hrs_heal_erased_dev ("Footprint tests"): the stripes
in a guarded uint8 arena, the reports in a guarded int32 arena
(tests/gpu_arena.py). One comparison of the whole arena against its pre-call
image with exactly the erased cells and the planted bytes replaced by the
oracle-encoded stripes: guards, untouched survivors and every byte around the
cells stay as they were. Parity sizes 5, 6 and 7 run a window plus a tail,
aligned and one byte off, against hrs_heal_erased_host."""
import random

import numpy as np
import pytest

import heal_erased_inputs as H
from gpu_arena import Arena, CrcArena
from lambdafs_amd import HipReedSolomonCode, _lib
from test_gpu_heal_erased import NONE_DEV

pytestmark = pytest.mark.gpu

K, P, S = 10, 4, 7
N = K + P

# name -> (L, shift, stripe_pad, kernel mode, hrs_last_kernel)
CASES = {
    "whole_windows": (2 * H.WINDOW, 0, 0, 0, "heal_erased_kernel<4>"),
    "windows_and_tail": (H.WINDOW + 100, 0, 0, 0, "heal_erased_kernel<4>"),
    "tail_only": (100, 0, 0, 0, "heal_erased_bytewise_kernel<4>"),
    "shift_1": (H.WINDOW + 100, 1, 0, 0, "heal_erased_bytewise_kernel<4>"),
    "stride_pad_5": (H.WINDOW + 100, 0, 5, 0, "heal_erased_bytewise_kernel<4>"),
    "mode_2": (2 * H.WINDOW, 0, 0, 2, "heal_erased_bytewise_kernel<4>"),
}


# the parity sizes on heal_tail's rolled bit loop whose second coefficient word is partly filled
WIDE = [(6, 5), (7, 6), (10, 7)]
WIDE_CASES = {
    "windows_and_tail": (H.WINDOW + 100, 0, "heal_erased_kernel"),
    "shift_1": (H.WINDOW + 100, 1, "heal_erased_bytewise_kernel"),
}


@pytest.mark.parametrize("name", list(CASES))
def test_heal_erased_footprint(cuda, name):
    L, shift, pad, mode, kernel = CASES[name]
    _footprint(cuda, K, P, L, shift, pad, mode, kernel)


@pytest.mark.parametrize("name", list(WIDE_CASES))
@pytest.mark.parametrize("k,p", WIDE)
def test_heal_erased_footprint_wide_parity(cuda, k, p, name):
    L, shift, kernel = WIDE_CASES[name]
    _footprint(cuda, k, p, L, shift, 0, 0, f"{kernel}<{p}>")


def _footprint(torch, K, P, L, shift, pad, mode, kernel):
    N = K + P
    clean = H.clean_stripes(K, P, S, L, 21)
    pats = H.seven_patterns(K, P, random.Random(L + shift + pad))
    bad, planted = H.plant(K, P, clean, pats, H.columns_of(L), seed=L)
    if P <= 4:
        after, want = clean, H.planted_reports(N, S, planted)
    else:  # the byte-exact reference where the locator may leave a column within capacity unresolved
        after, want = H.host_reference(HipReedSolomonCode(K, P, device=NONE_DEV), bad, pats)
        assert int(want[:, 1].sum()) * 20 <= len(planted)
    arena = Arena(S, L, shift=shift, stripe_pad=pad, seed=L + shift)
    names = arena.add_rows("loc", N, "input")
    flat, _ = arena.to_device()
    st = arena.stack(flat, names)
    st.copy_(torch.from_numpy(bad).to("cuda:0"))  # the damaged stripes replace the random rows
    pre = flat.cpu().numpy()
    reps = CrcArena(S, 4 + N, False)  # its "crc_out" block is the reports, report_stride = 4 + n
    rflat, _, rout = reps.to_device()
    code = HipReedSolomonCode(K, P, device=0)
    code.setKernelMode(mode)
    rows = _lib.ptr_array([st.data_ptr() + l * st.stride(1) for l in range(N)])
    arr = H.erased_array(pats)
    code._check(_lib.lib().hrs_heal_erased_dev(code._handle(), rows, st.stride(0), L, S, arr.ctypes.data, arr.shape[1],
                                               rout, 4 + N, torch.cuda.current_stream().cuda_stream))
    assert code.lastKernel() == kernel
    torch.cuda.synchronize()
    exp = pre.copy()
    for l, x in enumerate(names):
        for s in range(S):
            o = arena.offset(x, s)
            assert (exp[o:o + L] == bad[s, l]).all()
            exp[o:o + L] = after[s, l]
    # exactly the erased cells (where they differ from their 0xA5 fill) and the planted bytes
    filled = sum(int(np.count_nonzero(after[s, pats[s]] != H.FILL)) for s in range(S))
    assert np.count_nonzero(exp != pre) == filled + int(want[:, 3].sum()) and want[:, 3].sum() > 0
    d = arena.diff(flat.cpu().numpy(), exp)
    assert d is None, d
    d = reps.diff(rflat.cpu().numpy(), reps.expected(want))
    assert d is None, d
