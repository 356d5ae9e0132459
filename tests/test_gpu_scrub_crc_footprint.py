"""Footprint of hrs_scrub_crc_dev and hrs_heal_crc_dev ("Footprint
tests"): the stripes in a guarded uint8 arena, crc_in / crc_out and the
reports in guarded int32 arenas (tests/gpu_arena.py). One comparison of each
whole arena against its pre-call image. Scrub: only the reports and all S * n
CRC words change. Heal: additionally exactly the bytes the oracle says are
patched. Guards, crc_in and every unpatched byte stay intact."""
import numpy as np
import pytest

from gpu_arena import Arena, CrcArena
from lambdafs_amd import HipReedSolomonCode, _lib
from test_gpu_scrub_crc import _heal_inputs, crcs_of, expected_kernel

pytestmark = pytest.mark.gpu

K, P, S = 10, 4, 3
N = K + P

# (L, shift, with crc_in)
CASES = {
    "fused_aligned": (2048 * 3, 0, True),
    "fused_fresh": (2048, 0, False),
    "tail": (2048 * 3 + 100, 0, True),
    "shift_1": (2048 * 3, 1, False),
}


@pytest.mark.parametrize("heal", [False, True], ids=["scrub", "heal"])
@pytest.mark.parametrize("name", list(CASES))
def test_scrub_crc_footprint(cuda, name, heal):
    torch = cuda
    L, shift, with_in = CASES[name]
    host, want_rep, healed, heal_rep = _heal_inputs(K, P, L)
    arena = Arena(S, L, shift=shift, seed=L + shift)
    names = arena.add_rows("loc", N, "input")
    flat, _ = arena.to_device()
    st = arena.stack(flat, names)
    st.copy_(torch.from_numpy(np.array(host)).to("cuda:0"))  # the corrupted codewords replace the random rows
    pre = flat.cpu().numpy()
    crcs = CrcArena(S, N, with_in, seed=L)
    reps = CrcArena(S, 4 + N, False)  # its "crc_out" block is the reports, report_stride = 4 + n
    cflat, cin, cout = crcs.to_device()
    rflat, _, rout = reps.to_device()
    code = HipReedSolomonCode(K, P, device=0)
    rows = _lib.ptr_array([st.data_ptr() + l * st.stride(1) for l in range(N)])
    fn = _lib.lib().hrs_heal_crc_dev if heal else _lib.lib().hrs_scrub_crc_dev
    code._check(fn(code._handle(), rows, st.stride(0), L, S, rout, 4 + N, cin, cout,
                   torch.cuda.current_stream().cuda_stream))
    kernel = code.lastKernel()
    torch.cuda.synchronize()
    cells = healed if heal else host
    exp = pre.copy()
    for l, x in enumerate(names):
        for s in range(S):
            o = arena.offset(x, s)
            assert (exp[o:o + L] == host[s, l]).all()
            exp[o:o + L] = cells[s, l]
    if heal:
        assert np.count_nonzero(exp != pre) == int(heal_rep[:, 3].sum()) > 0  # exactly the patched bytes
    d = arena.diff(flat.cpu().numpy(), exp)
    assert d is None, d
    d = crcs.diff(cflat.cpu().numpy(), crcs.expected(crcs_of(cells, crcs.crc_in())))
    assert d is None, d
    d = reps.diff(rflat.cpu().numpy(), reps.expected(heal_rep if heal else want_rep))
    assert d is None, d
    assert kernel == expected_kernel(K, P, L, shift, 0, 0, heal), kernel
