"""hrs_scrub_ragged_batch_host and hrs_heal_ragged_batch_host over pageable and
pinned host memory, with HRS_ZEROCOPY=0 (both duplex settings) and with short
chunks through several slots, against the oracle's expectations of
tests/ragged_scrub_inputs.py.

A FULL batch of junk goes first on the same handle, so the slot images hold
stale non-zero bytes behind everything a ragged chunk copies in: only the
kernels' masking keeps them out of the reports, and a copy-back of more than a
cell's valid bytes would put them into the caller's memory. The caller's
stripes lie in a larger guarded buffer that is compared whole: it changes in
exactly the patched bytes."""
import numpy as np
import pytest

import ragged_scrub_inputs as R
from lambdafs_amd import HipReedSolomonCode, device
from test_gpu_heal import _guarded

pytestmark = pytest.mark.gpu

K, P, L = 10, 4, R.L_BIG
N = K + P


def _stale_first(code, shape):
    """A full batch of non-zero junk through the same handle's slots."""
    junk = np.random.default_rng(5).integers(1, 256, shape, dtype=np.uint8)
    rep = device.scrub_batch_host(code, junk)
    assert rep[:, 0].min() > 0


def _check(code, torch, pinned, path, k=K, p=P, L=L):
    stored, valid, healed, rep, rep2, _, _ = R.batch(k, p, L)
    vector = L >= R.WINDOW
    _stale_first(code, stored.shape)
    big, view, arg = _guarded(stored, pinned, torch)
    before = big.copy()
    got = device.scrub_batch_host_ragged(code, arg, valid)
    assert code.lastHostPath() == path
    assert code.lastKernel() == (f"scrub_ragged_kernel<{p}>" if vector else f"scrub_ragged_bytewise_kernel<{p}>")
    d = R.mismatch(got, R.scrub_report(rep), "scrub reports")
    assert d is None, d
    assert (big == before).all(), "the scrub changed the caller's memory"
    got = device.heal_batch_host_ragged(code, arg, valid)
    assert code.lastHostPath() == path
    assert code.lastKernel() == (f"heal_ragged_kernel<{p}>" if vector else f"heal_ragged_bytewise_kernel<{p}>")
    d = R.mismatch(got, rep, "heal reports")
    assert d is None, d
    want = before.copy()
    want[:, :k + p, :L] = healed
    d = R.mismatch(big, want, "the caller's memory, guards and junk included")
    assert d is None, d
    assert np.count_nonzero(big != before) == int(rep[:, 3].sum()) > 0
    got = device.heal_batch_host_ragged(code, arg, valid)  # nothing left to store
    assert R.mismatch(got, rep2, "second heal reports") is None and (big == want).all()


def test_pinned_runs_in_place(cuda):
    _check(HipReedSolomonCode(K, P, device=0), cuda, True, "pinned")


@pytest.mark.parametrize("chunk_stripes", [None, 2])
def test_pageable_staged(cuda, monkeypatch, chunk_stripes):
    """One chunk, and chunks of two stripes, so that the 3 slots are refilled
    after their healed cells have left."""
    if chunk_stripes:
        monkeypatch.setenv("HRS_HBATCH_BYTES", str(chunk_stripes * N * (L + 256)))
    _check(HipReedSolomonCode(K, P, device=0), cuda, False, "staged")


def test_pageable_tail_only_cells(cuda, monkeypatch):
    monkeypatch.setenv("HRS_HBATCH_BYTES", str(3 * 16 * 256))
    _check(HipReedSolomonCode(12, 4, device=0), cuda, False, "staged", 12, 4, R.L_TAIL)


@pytest.mark.parametrize("duplex", ["0", "1"])
def test_copy_engine(cuda, monkeypatch, duplex):
    """Zero copy switched off: only each cell's valid bytes go up, only the
    dirty cells' valid bytes come back; chunks of three stripes."""
    monkeypatch.setenv("HRS_ZEROCOPY", "0")
    monkeypatch.setenv("HRS_HBATCH_DUPLEX", duplex)
    monkeypatch.setenv("HRS_HBATCH_BYTES", str(3 * N * (L + 256)))
    code = HipReedSolomonCode(K, P, device=0)
    for pinned in (True, False):
        _check(code, cuda, pinned, "copy_engine")


def test_all_full_host_batch_takes_the_plain_route(cuda):
    code = HipReedSolomonCode(K, P, device=0)
    stored = R.batch(K, P, L)[0]
    full = np.full(stored.shape[:2], L, np.uint32)
    a, b = np.array(stored), np.array(stored)
    want = device.heal_batch_host(code, a)
    got = device.heal_batch_host_ragged(code, b, full)
    assert code.lastKernel() == "heal_kernel<4>"
    assert got.tolist() == want.tolist() and (a == b).all()
