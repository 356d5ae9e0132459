"""GPU tests of hrs_scrub_batch_host_crc and hrs_heal_batch_host_crc over
runtime-pinned stripes (read and healed in place across the host link) and
pageable ones (staged through the host-batch pipeline in chunks of 2 stripes,
so the 3 slots are reused): RS(12,4), S = 9, L = 4096 (the fused kernel) and
4096 + 100 (a row tail: two passes). The same assertions as on the device:
reports and healed bytes from the oracle, CRCs from zlib over the expected
bytes. One run repeats everything with HRS_ZEROCOPY=0 (the copy-engine route)
in a fresh child process."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from lambdafs_amd import HipReedSolomonCode, device  # noqa: E402
from oracle import rs_oracle as C  # noqa: E402
from test_gpu_scrub_crc import crcs_of  # noqa: E402
from test_heal_host import heal_expected  # noqa: E402

pytestmark = pytest.mark.gpu

K, P, S = 12, 4, 9
N = K + P
LENGTHS = [4096, 4096 + 100]
PAD = 0x3C
_cache = {}


def _inputs(L):
    """(stripes, healed stripes, reports of the heal) [S, n, L]: stripe 1 with
    single wrong bytes at the window edges, stripe 4 with a replaced cell,
    stripe 7 with a 3-error column the oracle cannot resolve plus one flipped
    bit, stripe 8 with a wrong last byte; the rest clean."""
    if L in _cache:
        return _cache[L]
    rng = np.random.default_rng(1204 + L)
    rnd = random.Random(1204 + L)
    host = np.empty((S, N, L), np.uint8)
    host[:, P:] = rng.integers(0, 256, (S, K, L), dtype=np.uint8)
    for s in range(S):
        host[s, :P] = np.stack(C.encode_bulk(K, P, [host[s, P + c] for c in range(K)]))
    for c, l in ((0, 0), (2047, 5), (2048, N - 1), (L - 1, 3)):
        host[1, l, c] ^= rnd.randrange(1, 256)
    host[4, 9] = rng.integers(0, 256, L, dtype=np.uint8)
    for _ in range(400):
        c = rnd.randrange(1, L)
        trial = host[7, :, c].copy()
        for l in rnd.sample(range(N), 3):
            trial[l] ^= rnd.randrange(1, 256)
        if not C.compute_error_locations(K, P, trial.tolist())[0]:
            host[7, :, c] = trial
            break
    else:
        raise AssertionError("no unresolved 3-error column found")
    host[7, 2, 0] ^= 0x40
    host[8, N - 1, L - 1] ^= 1
    healed = host.copy()
    rep = np.zeros((S, 4 + N), np.uint32)
    rep[:, 2] = 0xFFFFFFFF
    for s in (1, 4, 7, 8):
        healed[s], rep[s] = heal_expected(K, P, host[s])
    assert rep[7, 1] == 1 and rep[4, 4 + 9] >= L - 40 and not rep[0, [0, 1, 3]].any()
    _cache[L] = (host, healed, rep)
    return _cache[L]


def _alloc(torch, L, pinned):
    """A [S, n, L] view of a padded host buffer (row pitch a multiple of 16,
    above L), the padding filled with PAD."""
    pitch = (L + 15) // 16 * 16 + 16
    big = torch.empty((S, N, pitch), dtype=torch.uint8, pin_memory=True).numpy() if pinned \
        else np.empty((S, N, pitch), np.uint8)
    big[...] = PAD
    return big, big[:, :, :L]


def check_host_calls(torch, L, pinned, path):
    host, healed, want = _inputs(L)
    code = HipReedSolomonCode(K, P, device=0)
    fused = L % 2048 == 0
    start = np.random.default_rng(L).integers(0, 1 << 32, (S, N), dtype=np.uint32)
    scrub_rep = want.copy()
    scrub_rep[:, 3] = 0
    for crc_in, alias in ((start, False), (None, False), (start, True)):
        big, view = _alloc(torch, L, pinned)
        view[...] = host
        words = None if crc_in is None else crc_in.copy()
        rep, crc = device.scrub_batch_host_crc(code, view, crc_in=words, crc_out=words if alias else None)
        assert code.lastHostPath() == path
        assert code.lastKernel() == ("scrub_crc_kernel<4>" if fused else "scrub_kernel<4>")
        assert rep.dtype == np.uint32 and rep.tolist() == scrub_rep.tolist()
        assert crc.dtype == np.uint32 and crc.tolist() == crcs_of(host, crc_in).tolist()
        assert (crc is words) == alias and (alias or words is None or (words == crc_in).all())
        assert (view == host).all() and (big[:, :, L:] == PAD).all()  # a scrub writes nothing

        words = None if crc_in is None else crc_in.copy()
        rep, crc = device.heal_batch_host_crc(code, view, crc_in=words, crc_out=words if alias else None)
        assert code.lastHostPath() == path
        assert code.lastKernel() == ("heal_crc_kernel<4>" if fused else "heal_kernel<4>")
        assert rep.tolist() == want.tolist()
        assert (view == healed).all()
        assert crc.tolist() == crcs_of(healed, crc_in).tolist()  # the cells as they are now
        # nothing outside the cells with a nonzero count in word 4 + l changed
        assert (big[:, :, L:] == PAD).all()
        for s in range(S):
            for l in range(N):
                if want[s, 4 + l] == 0:
                    assert (view[s, l] == host[s, l]).all(), (s, l)
        # a second heal stores nothing and returns the same CRCs
        rep2, crc2 = device.heal_batch_host_crc(code, view, crc_in=crc_in)
        assert not rep2[:, 3].any() and not rep2[:, 4:].any() and (view == healed).all()
        assert crc2.tolist() == crcs_of(healed, crc_in).tolist()


@pytest.fixture
def two_stripe_chunks(monkeypatch):
    for name in ("HRS_ZEROCOPY", "HRS_HBATCH_DUPLEX", "HRS_HOST_NT"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("HRS_HBATCH_BYTES", str(2 * N * (max(LENGTHS) + 256)))


@pytest.mark.parametrize("pinned", [True, False], ids=["pinned", "pageable"])
@pytest.mark.parametrize("L", LENGTHS)
def test_host_batches_match_oracle_and_zlib(cuda, two_stripe_chunks, L, pinned):
    check_host_calls(cuda, L, pinned, "pinned" if pinned else "staged")


def test_copy_engine_route_in_a_child_process(cuda, two_stripe_chunks):
    """HRS_ZEROCOPY=0 from the start of a fresh process: pinned stripes DMA'd
    chunk by chunk, pageable ones through staging, kernels on device images."""
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
