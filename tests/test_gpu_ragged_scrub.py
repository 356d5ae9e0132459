"""The ragged scrub and heal on the device (hrs_scrub_ragged_dev,
hrs_heal_ragged_dev; include/hrs.h "ragged scrub and heal") against the
oracle's expectations of tests/ragged_scrub_inputs.py: every code, lengths of
every class at every placement, demoted and mixed columns, seeded non-zero
junk behind every length, every byte of every cell compared after a heal.
Each case runs a scrub through the C ABI (report_stride > 4 + n, the padding
words checked), a heal and a second heal through the Python mirror on ONE
handle, so the handle's two table slots are reused. Kernel modes 0, 2 and 3
with the kernel names asserted; the all-full route; unaligned rows."""
import numpy as np
import pytest

import ragged_scrub_inputs as R
from lambdafs_amd import HipReedSolomonCode, _lib, device
from test_gpu_heal import _device_view, _outside_unchanged
from test_gpu_scrub import _u32

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A
SPARE = 3  # report_stride = 4 + n + SPARE


def kernel_name(op, p, mode, L, shift=0):
    vector = mode != 2 and L >= R.WINDOW and shift == 0
    return f"{op}_ragged_kernel<{p}>" if vector else f"{op}_ragged_bytewise_kernel<{p}>"


def scrub_abi(torch, code, view, valid, fn=None):
    """hrs_scrub_ragged_dev (or fn) on the view's rows into strided reports whose spare words must survive."""
    S, n, L = view.shape
    rows = _lib.ptr_array([view.data_ptr() + l * view.stride(1) for l in range(n)])
    rep = torch.full((S, 4 + n + SPARE), FILL, dtype=torch.int32, device="cuda:0")
    v = np.ascontiguousarray(valid, dtype=np.uint32)
    fn = fn or _lib.lib().hrs_scrub_ragged_dev
    code._check(fn(code._handle(), rows, view.stride(0), L, S, v.ctypes.data, rep.data_ptr(), 4 + n + SPARE,
                   torch.cuda.current_stream().cuda_stream))
    raw = _u32(rep)
    assert (raw[:, 4 + n:] == FILL).all(), "words past 4 + n of a report were written"
    return raw[:, :4 + n]


def run_case(torch, k, p, L, mode, shift=0):
    stored, valid, healed, rep, rep2, _, _ = R.batch(k, p, L)
    code = HipReedSolomonCode(k, p, device=0)
    code.setKernelMode(mode)
    big, view = _device_view(torch, stored, shift)
    before = big.clone()
    got = scrub_abi(torch, code, view, valid)
    assert code.lastKernel() == kernel_name("scrub", p, mode, L, shift)
    assert R.mismatch(got, R.scrub_report(rep), "scrub reports") is None
    assert torch.equal(big, before), "the scrub wrote into the stripes"
    got = _u32(device.heal_stripes_ragged(code, view, valid))
    assert code.lastKernel() == kernel_name("heal", p, mode, L, shift)
    d = R.mismatch(view.cpu().numpy(), healed, "healed bytes")
    assert d is None, d
    assert _outside_unchanged(big, before, stored.shape, shift)
    d = R.mismatch(got, rep, "heal reports")
    assert d is None, d
    after_first = big.clone()
    got = scrub_abi(torch, code, view, valid, _lib.lib().hrs_heal_ragged_dev)
    assert torch.equal(big, after_first), "the second heal stored something"
    assert R.mismatch(got, rep2, "second heal reports") is None
    assert R.mismatch(_u32(device.scrub_stripes_ragged(code, view, valid)), R.scrub_report(rep2), "mirror scrub") is None


@pytest.mark.parametrize("mode", [0, 2, 3])
@pytest.mark.parametrize("k,p,L", R.all_cases())
def test_ragged_scrub_and_heal_match_oracle(cuda, k, p, L, mode):
    run_case(cuda, k, p, L, mode)


@pytest.mark.parametrize("k,p", [(10, 4), (6, 3), (20, 8)])
def test_unaligned_rows_take_the_bytewise_kernel(cuda, k, p):
    run_case(cuda, k, p, R.L_BIG, 0, shift=1)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_all_full_batch_equals_the_plain_calls(cuda, mode):
    """Every entry equal to len: modes 0 and 1 take the plain route and name
    its kernel, 2 and 3 keep the ragged kernels; all four equal hrs_heal_dev
    word for word and byte for byte (nothing can be demoted)."""
    torch = cuda
    k, p, L = 10, 4, R.L_BIG
    n = k + p
    stored = R.batch(k, p, L)[0]
    S = stored.shape[0]
    full = np.full((S, n), L, np.uint32)
    code = HipReedSolomonCode(k, p, device=0)
    code.setKernelMode(0)
    _, plain = _device_view(torch, stored)
    want_scrub = _u32(device.scrub_stripes(code, plain))
    want_heal = _u32(device.heal_stripes(code, plain))
    want = plain.cpu().numpy()
    assert want_heal[:, 3].sum() > 0
    code.setKernelMode(mode)
    _, view = _device_view(torch, stored)
    got = _u32(device.scrub_stripes_ragged(code, view, full))
    names = {0: "scrub_kernel<4>", 1: "scrub_kernel<4>", 2: "scrub_ragged_bytewise_kernel<4>", 3: "scrub_ragged_kernel<4>"}
    assert code.lastKernel() == names[mode]
    assert R.mismatch(got, want_scrub, "scrub reports") is None
    got = _u32(device.heal_stripes_ragged(code, view, full))
    assert code.lastKernel() == names[mode].replace("scrub_", "heal_", 1)
    assert R.mismatch(got, want_heal, "heal reports") is None
    assert R.mismatch(view.cpu().numpy(), want, "healed bytes") is None
