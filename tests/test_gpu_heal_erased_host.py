"""GPU tests of hrs_heal_erased_batch_host and hrs_heal_erased_batch_host_crc
over runtime-pinned stripes (healed in place across the host link) and
pageable ones (staged through the host-batch pipeline in chunks of 2 stripes,
so the 3 slots and the 2 pattern-table slots are reused): RS(12,4), S = 9,
L = 4096 and 4096 + 100 (a row tail), the patterns of
tests/heal_erased_inputs.py plus two repeats, survivor errors planted within
capacity and, in stripe 8, one past it. Bytes are the oracle-encoded stripes
(stripe 8: hrs_heal_erased_host), reports the planted counts, CRCs zlib over
the expected bytes. One run repeats everything with HRS_ZEROCOPY=0 (the
copy-engine route) in a fresh child process."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import heal_erased_inputs as H  # noqa: E402
from lambdafs_amd import HipReedSolomonCode, TooManyErasedLocations, device  # noqa: E402
from test_gpu_scrub_crc import crcs_of  # noqa: E402

pytestmark = pytest.mark.gpu

K, P, S = 12, 4, 9
N = K + P
LENGTHS = [2 * H.WINDOW, 2 * H.WINDOW + 100]
PAD = 0x3C
OVER = 8  # the stripe with columns past capacity
NONE_DEV = -2  # HRS_DEVICE_NONE
_cache = {}


def _inputs(L):
    """(damaged, patterns, expected bytes, expected reports) [S, n, L]: stripes
    0-6 as the device tests have them (seven patterns, errors within
    capacity), stripe 7 repeats pattern 1 with errors, stripe 8 repeats
    pattern 2 with one error past capacity in every planted column: those
    columns stay as they are, the reference is hrs_heal_erased_host."""
    if L in _cache:
        return _cache[L]
    rnd = random.Random(1009 * K + P + L)
    pats = H.seven_patterns(K, P, rnd)
    pats = pats + [pats[1], pats[2]]
    clean = H.clean_stripes(K, P, S, L, 31)
    bad, planted = H.plant(K, P, clean, pats, H.columns_of(L), seed=L)
    over, _ = H.plant(K, P, clean, pats, H.columns_of(L), over=1, seed=L + 1)
    bad[OVER] = over[OVER]
    after = np.array(clean)
    reps = H.planted_reports(N, S, [x for x in planted if x[0] != OVER])
    code = HipReedSolomonCode(K, P, device=NONE_DEV)
    ref, ref_rep = H.host_reference(code, bad[OVER:OVER + 1], [pats[OVER]])
    after[OVER], reps[OVER] = ref[0], ref_rep[0]
    assert reps[OVER, 1] > 0 and (after[OVER] != clean[OVER]).any()  # unresolved columns, left as they were
    assert reps[7, 3] > 0 and reps[6, 0] == 0
    _cache[L] = (bad, pats, after, reps)
    return _cache[L]


def _alloc(torch, L, pinned):
    """A [S, n, L] view of a padded host buffer (row pitch a multiple of 16,
    above L), the padding filled with PAD."""
    pitch = (L + 15) // 16 * 16 + 16
    big = torch.empty((S, N, pitch), dtype=torch.uint8, pin_memory=True).numpy() if pinned \
        else np.empty((S, N, pitch), np.uint8)
    big[...] = PAD
    return big, big[:, :, :L]


def _check_written(view, big, bad, pats, after, reps, L):
    assert (view == after).all(), np.argwhere(view != after)[:4].tolist()
    assert (big[:, :, L:] == PAD).all()  # the sentinel
    # a cell that is neither erased nor blamed is its input, byte for byte, also
    # where that differs from the clean stripe (stripe 8's unresolved columns)
    differs = 0
    for s in range(S):
        for l in range(N):
            if l not in pats[s] and reps[s, 4 + l] == 0:
                assert (view[s, l] == bad[s, l]).all(), (s, l)
                differs += int((bad[s, l] != H.clean_stripes(K, P, S, L, 31)[s, l]).any())
    assert differs > 0


def check_host_calls(torch, L, pinned, path):
    bad, pats, after, want = _inputs(L)
    code = HipReedSolomonCode(K, P, device=0)
    arr = H.erased_array(pats)
    start = np.random.default_rng(L).integers(0, 1 << 32, (S, N), dtype=np.uint32)
    results = []
    for fill in (H.FILL, 0x00):  # lost cells are never read: the same result whatever they hold
        src = np.array(bad)
        for s in range(S):
            src[s, pats[s], :] = fill
        big, view = _alloc(torch, L, pinned)
        view[...] = src
        rep = device.heal_erased_batch_host(code, view, arr)
        assert code.lastHostPath() == path
        assert code.lastKernel() == "heal_erased_kernel<4>"
        assert rep.dtype == np.uint32 and rep.tolist() == want.tolist()
        _check_written(view, big, src, pats, after, want, L)
        results.append((view.copy(), rep))
        for crc_in, alias in ((start, False), (None, False), (start, True)):
            big, view = _alloc(torch, L, pinned)
            view[...] = src
            words = None if crc_in is None else crc_in.copy()
            rep, crc = device.heal_erased_batch_host_crc(code, view, pats, crc_in=words,
                                                         crc_out=words if alias else None)
            assert code.lastHostPath() == path
            assert code.lastKernel() in ("heal_erased_kernel<4>", "heal_erased_crc_kernel<4>")
            assert rep.tolist() == want.tolist()
            assert crc.dtype == np.uint32 and crc.tolist() == crcs_of(after, crc_in).tolist()
            assert (crc is words) == alias and (alias or words is None or (words == crc_in).all())
            _check_written(view, big, src, pats, after, want, L)
        results.append((view.copy(), rep, crc))
        # the fused kernel (kernel mode 3) where the shape allows it
        code.setKernelMode(3)
        big, view = _alloc(torch, L, pinned)
        view[...] = src
        rep, crc = device.heal_erased_batch_host_crc(code, view, arr, crc_in=start)
        code.setKernelMode(0)
        assert code.lastKernel() == ("heal_erased_crc_kernel<4>" if L % H.WINDOW == 0 else "heal_erased_kernel<4>")
        assert rep.tolist() == want.tolist() and crc.tolist() == crcs_of(after, start).tolist()
        _check_written(view, big, src, pats, after, want, L)
        # a second call stores no survivor byte and returns the same CRCs
        rep2, crc2 = device.heal_erased_batch_host_crc(code, view, arr, crc_in=start)
        assert not rep2[:, 3].any() and not rep2[:, 4:].any() and (view == after).all()
        assert crc2.tolist() == crc.tolist()
    for x, y in zip(results[:2], results[2:]):
        assert all((a == b).all() for a, b in zip(x, y))
    # a stripe with too many erasures in the middle of the batch: refused before any copy
    big, view = _alloc(torch, L, pinned)
    view[...] = bad
    image = big.copy()
    worse = [list(e) for e in pats]
    worse[4] = [0, 1, 2, 3, 4]
    for call in (device.heal_erased_batch_host, device.heal_erased_batch_host_crc):
        with pytest.raises(TooManyErasedLocations, match="stripe 4"):
            call(code, view, worse)
        assert (big == image).all()


@pytest.fixture
def two_stripe_chunks(monkeypatch):
    for name in ("HRS_ZEROCOPY", "HRS_HBATCH_DUPLEX", "HRS_HOST_NT"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("HRS_HBATCH_BYTES", str(2 * N * (max(LENGTHS) + 256)))


@pytest.mark.parametrize("pinned", [True, False], ids=["pinned", "pageable"])
@pytest.mark.parametrize("L", LENGTHS)
def test_host_batches_restore_the_stripes(cuda, two_stripe_chunks, L, pinned):
    check_host_calls(cuda, L, pinned, "pinned" if pinned else "staged")


def test_nothing_erased_is_the_host_heal(cuda, two_stripe_chunks):
    """max_erased == 0 is hrs_heal_batch_host / hrs_heal_batch_host_crc."""
    L = LENGTHS[0]
    clean = H.clean_stripes(K, P, S, L, 31)
    none = [[] for _ in range(S)]
    bad, planted = H.plant(K, P, clean, none, H.columns_of(L), clean_stripes_=(), seed=2)
    code = HipReedSolomonCode(K, P, device=0)
    a, b, c = np.array(bad), np.array(bad), np.array(bad)
    want, want_crc = device.heal_batch_host_crc(code, a)
    kernel = code.lastKernel()
    empty = np.zeros((S, 0), np.int32)
    rep, crc = device.heal_erased_batch_host_crc(code, b, empty)
    assert code.lastKernel() == kernel and code.lastHostPath() == "staged"
    assert (a == b).all() and (a == clean).all() and rep.tolist() == want.tolist() and crc.tolist() == want_crc.tolist()
    assert device.heal_erased_batch_host(code, c, empty).tolist() == want.tolist() and (c == clean).all()
    assert code.lastKernel() == "heal_kernel<4>"


def test_copy_engine_route_in_a_child_process(cuda, two_stripe_chunks):
    """HRS_ZEROCOPY=0 from the start of a fresh process: pinned stripes DMA'd
    chunk by chunk, pageable ones through staging, kernels on device images
    whose erased rows hold whatever the slot held before."""
    env = dict(os.environ, HRS_ZEROCOPY="0")
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True,
                         timeout=240)
    assert out.returncode == 0 and "copy engine ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


if __name__ == "__main__":
    import torch
    assert os.environ.get("HRS_ZEROCOPY") == "0" and torch.cuda.is_available()
    for length in LENGTHS:
        for pin in (True, False):
            check_host_calls(torch, length, pin, "copy_engine")
    print("copy engine ok")
