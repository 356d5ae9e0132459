"""Footprint of the ragged scrub and heal kernels by the arena convention
(tests/gpu_arena.py, DESIGN.md "Footprint tests"): the stripes lie in one
guarded arena, the reports in a guarded word arena, and after a heal the WHOLE
arena is compared with the pre-call image in which exactly the patched bytes
are replaced. The batches of tests/ragged_scrub_inputs.py put cell boundaries
at a window's last and first byte (lengths 2047, 2048, 2049) and non-zero junk
behind every length; shift = 1 with stripe pad 5 takes the byte-granular
kernels over unaligned rows."""
import numpy as np
import pytest

import ragged_scrub_inputs as R
from gpu_arena import Arena, CrcArena
from lambdafs_amd import HipReedSolomonCode, _lib

pytestmark = pytest.mark.gpu

# name -> (k, p, L, shift, stripe pad, kernel mode, the heal's kernel)
CASES = {
    "vector": (10, 4, R.L_BIG, 0, 0, 0, "heal_ragged_kernel<4>"),
    "vector_padded": (6, 3, R.L_BIG, 0, 16, 3, "heal_ragged_kernel<3>"),
    "unaligned": (10, 4, R.L_BIG, 1, 5, 0, "heal_ragged_bytewise_kernel<4>"),
    "tail_only": (12, 4, R.L_TAIL, 0, 0, 0, "heal_ragged_bytewise_kernel<4>"),
    "wide_parity": (20, 8, R.L_BIG, 0, 0, 0, "heal_ragged_kernel<8>"),
    "bytewise_mode": (9, 5, R.L_BIG, 0, 0, 2, "heal_ragged_bytewise_kernel<5>"),
}


@pytest.mark.parametrize("name", list(CASES))
def test_ragged_heal_footprint(cuda, name):
    torch = cuda
    k, p, L, shift, pad, mode, kernel = CASES[name]
    n = k + p
    stored, valid, healed, rep, _, _, _ = R.batch(k, p, L)
    S = stored.shape[0]
    arena = Arena(S, L, shift=shift, stripe_pad=pad, seed=L + shift)
    names = arena.add_rows("loc", n, "input")
    flat, _ = arena.to_device()
    st = arena.stack(flat, names)
    st.copy_(torch.from_numpy(np.array(stored)).to("cuda:0"))
    pre = flat.cpu().numpy()
    reps = CrcArena(S, 4 + n, False)  # its "crc_out" block is the reports, report_stride = 4 + n
    rflat, _, rout = reps.to_device()
    code = HipReedSolomonCode(k, p, device=0)
    code.setKernelMode(mode)
    rows = _lib.ptr_array([st.data_ptr() + l * st.stride(1) for l in range(n)])
    v = np.ascontiguousarray(valid)
    stream = torch.cuda.current_stream().cuda_stream
    # the scrub: nothing in the arena changes
    code._check(_lib.lib().hrs_scrub_ragged_dev(code._handle(), rows, st.stride(0), L, S, v.ctypes.data, rout, 4 + n,
                                                stream))
    assert code.lastKernel() == kernel.replace("heal_", "scrub_", 1)
    d = arena.diff(flat.cpu().numpy(), pre)
    assert d is None, d
    d = reps.diff(rflat.cpu().numpy(), reps.expected(R.scrub_report(rep)))
    assert d is None, d
    # the heal: exactly the patched bytes
    code._check(_lib.lib().hrs_heal_ragged_dev(code._handle(), rows, st.stride(0), L, S, v.ctypes.data, rout, 4 + n,
                                               stream))
    assert code.lastKernel() == kernel
    exp = pre.copy()
    for l, x in enumerate(names):
        for s in range(S):
            o = arena.offset(x, s)
            assert (exp[o:o + L] == stored[s, l]).all()
            exp[o:o + L] = healed[s, l]
    assert np.count_nonzero(exp != pre) == int(rep[:, 3].sum()) > 0
    d = arena.diff(flat.cpu().numpy(), exp)
    assert d is None, d
    d = reps.diff(rflat.cpu().numpy(), reps.expected(np.array(rep)))
    assert d is None, d
