"""GPU tests of stripe healing (hrs_heal_dev / hrs_heal_batch_host). Expected
bytes come from the oracle, column by column: with
ok, locs, after = computeErrorLocations(column), the healed column is `after`
if ok, else the column as it was (also where the oracle wrote into it before
returning false). The report is the scrub's report of the input, plus word 3 =
the bytes that differ before and after."""
import random

import numpy as np
import pytest

from lambdafs_amd import HipReedSolomonCode, _lib, device
from oracle import rs_oracle as C
from test_gpu_scrub import LENGTHS, NONE, SHAPES, S, _stripes, _u32
from test_heal_host import heal_expected

pytestmark = pytest.mark.gpu

_cache = {}


def _search(k, p, clean, rnd, errors, accept):
    """A corruption of the codeword `clean` with `errors` wrong symbols whose
    oracle outcome (ok, found, after, trial) satisfies accept; 400 tries."""
    n = k + p
    for _ in range(400):
        trial = list(clean)
        for l in rnd.sample(range(n), errors):
            trial[l] ^= rnd.randrange(1, 256)
        ok, found, after = C.compute_error_locations(k, p, list(trial))
        if accept(ok, found, after, trial):
            return trial
    raise AssertionError(f"RS({k},{p}): no such column in 400 tries")


def _inputs(k, p, L):
    """The scrub test's corrupted stripes [S, n, L] plus the planted columns,
    and what the oracle makes of them; built once per (shape, L), read only.
    Stripe 0 (clean in the scrub test) carries the planted columns: at column
    L - 1, for p >= 2, one that the oracle calls unresolved after writing into
    its data ((3,2) has none: there, one it calls unresolved and leaves alone);
    at column 0, for (20,8) and L > 1, a two-error column that the oracle
    resolves with three locations."""
    key = (k, p, L)
    if key in _cache:
        return _cache[key]
    n = k + p
    base, _ = _stripes(k, p, L)
    host = base.copy()
    rnd = random.Random(15485863 * k + 32452843 * p + L)
    planted = {}
    if p >= 2:
        c = L - 1
        clean = host[0, :, c].tolist()
        if (k, p) == (3, 2):
            trial = _search(k, p, clean, rnd, 2, lambda ok, found, after, t: not ok and after == t)
        else:
            trial = _search(k, p, clean, rnd, p // 2 + 1, lambda ok, found, after, t: not ok and after != t)
        host[0, :, c] = trial
        planted["unresolved"] = c
    if (k, p) == (20, 8) and L > 1:
        clean = host[0, :, 0].tolist()
        host[0, :, 0] = _search(k, p, clean, rnd, 2, lambda ok, found, after, t: ok and len(found) == 3)
        planted["spurious"] = (0, clean)
    want = np.empty_like(host)
    rep = np.empty((S, 4 + n), dtype=np.uint32)
    for s in range(S):
        want[s], rep[s] = heal_expected(k, p, host[s])
    host.setflags(write=False)
    want.setflags(write=False)
    rep.setflags(write=False)
    _cache[key] = (host, want, rep, planted)
    return _cache[key]


def _device_view(torch, host, shift=0):
    """host[S, n, L] as a view of a larger random device tensor: padding after
    each row (pitch a multiple of 16), a spare row per stripe (so the stripe
    stride leaves a gap), rows offset by `shift`. Returns (big, view)."""
    s, n, L = host.shape
    pitch = ((L + shift + 15) // 16) * 16 + 16
    g = torch.Generator(device="cuda:0")
    g.manual_seed(L + shift)
    big = torch.randint(0, 256, (s, n + 1, pitch), dtype=torch.uint8, device="cuda:0", generator=g)
    view = big[:, :n, shift:shift + L]
    view.copy_(torch.from_numpy(np.array(host)).to("cuda:0"))
    assert view.stride(0) == (n + 1) * pitch and view.stride(1) == pitch
    return big, view


def _outside_unchanged(big, before, view_shape, shift=0):
    """Every byte of `big` outside the view equals `before`."""
    s, n, L = view_shape
    a, b = big.clone(), before.clone()
    a[:, :n, shift:shift + L] = 0
    b[:, :n, shift:shift + L] = 0
    return bool((a == b).all())


def _kernel_name(p, mode, L, shift=0):
    vector = mode == 0 and L >= 2048 and shift == 0
    return f"heal_kernel<{p}>" if vector else f"heal_bytewise_kernel<{p}>"


def _check_planted(k, p, L, host, want, rep, planted, got):
    if p >= 2:
        c = planted["unresolved"]
        ok, _, after = C.compute_error_locations(k, p, host[0, :, c].tolist())
        assert not ok
        assert (after != host[0, :, c].tolist()) == ((k, p) != (3, 2))  # the oracle wrote into it (bar (3,2))
        assert (got[0, :, c] == host[0, :, c]).all()                     # heal did not
        assert rep[0, 1] >= 1
    if "spurious" in planted:
        c, clean = planted["spurious"]
        ok, found, after = C.compute_error_locations(k, p, host[0, :, c].tolist())
        assert ok and len(found) == 3 and after == clean
        assert got[0, :, c].tolist() == clean
        assert int(rep[0, 4:].sum()) > int(rep[0, 3])  # locations blamed > bytes changed


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("k,p", SHAPES)
def test_heal_matches_oracle(cuda, k, p, L, mode):
    torch = cuda
    n = k + p
    host, want, want_rep, planted = _inputs(k, p, L)
    assert ((k, p) == (20, 8) and L > 1) == ("spurious" in planted) and (p >= 2) == ("unresolved" in planted)
    code = HipReedSolomonCode(k, p, device=0)
    code.setKernelMode(mode)
    big, view = _device_view(torch, host)
    before = big.clone()
    # the scrub of the same input: word 3 stays 0, its own kernels, nothing written
    scrubbed = _u32(device.scrub_stripes(code, view))
    assert code.lastKernel() == _kernel_name(p, mode, L).replace("heal_", "scrub_")
    assert not scrubbed[:, 3].any() and torch.equal(big, before)
    rep = _u32(device.heal_stripes(code, view))
    assert code.lastKernel() == _kernel_name(p, mode, L)
    got = view.cpu().numpy()
    print(f"RS({k},{p}) L={L} mode={mode}: kernel {code.lastKernel()}, report heads {rep[:, :4].tolist()}")
    assert (got == want).all()
    assert _outside_unchanged(big, before, host.shape)
    others = [w for w in range(4 + n) if w != 3]
    assert rep[:, others].tolist() == scrubbed[:, others].tolist()
    assert rep.tolist() == want_rep.tolist()
    assert rep[:, 3].tolist() == [int(np.count_nonzero(host[s] != got[s])) for s in range(S)]
    _check_planted(k, p, L, host, want, rep, planted, got)
    # the same through explicit row views
    big2, view2 = _device_view(torch, host)
    rows = _u32(device.heal_rows(code, [view2[:, l, :] for l in range(n)]))
    assert rows.tolist() == want_rep.tolist() and (view2.cpu().numpy() == want).all()


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("k,p", SHAPES)
def test_heal_is_idempotent(cuda, k, p, mode):
    """A second heal changes no byte and stores nothing: the bad columns left
    are the first call's unresolved ones, and no location is blamed."""
    L = 2049
    host, want, want_rep, _ = _inputs(k, p, L)
    code = HipReedSolomonCode(k, p, device=0)
    code.setKernelMode(mode)
    big, view = _device_view(cuda, host)
    first = _u32(device.heal_stripes(code, view))
    after_first = big.clone()
    second = _u32(device.heal_stripes(code, view))
    assert cuda.equal(big, after_first)
    assert not second[:, 3].any() and not second[:, 4:].any()
    assert second[:, 0].tolist() == second[:, 1].tolist() == first[:, 1].tolist()
    assert first[:, 1].any()


def test_heal_past_erasure_decoding(cuda):
    """RS(10,4), L = 2049: one single-byte error at each of the 14 locations,
    each in another column (13 in the vector window, one in the tail). More
    locations are blamed than erasure decoding repairs (scrub_to_erased gives
    up); heal restores the stripe exactly."""
    torch = cuda
    k, p, L = 10, 4, 2049
    n = k + p
    rng = np.random.default_rng(1014)
    data = [rng.integers(0, 256, L, dtype=np.uint8) for _ in range(k)]
    clean = np.stack([np.stack(C.encode_bulk(k, p, data) + data)] * 2)  # stripe 1 stays clean
    host = clean.copy()
    cols = [0, 15, 16, 100, 511, 1023, 1024, 1025, 1500, 2000, 2032, 2046, 2047, 2048]
    assert len(cols) == n and cols[-1] >= 2048
    for l, c in enumerate(cols):
        host[0, l, c] ^= 1 + (37 * l) % 255
    code = HipReedSolomonCode(k, p, device=0)
    big, view = _device_view(torch, host)
    before = big.clone()
    rep = _u32(device.heal_stripes(code, view))
    assert code.lastKernel() == "heal_kernel<4>"
    assert (view.cpu().numpy() == clean).all() and _outside_unchanged(big, before, host.shape)
    assert rep[0, :4].tolist() == [n, 0, 0, n] and rep[0, 4:].tolist() == [1] * n
    assert rep[1].tolist() == [0, 0, NONE, 0] + [0] * n
    assert np.count_nonzero(rep[0, 4:]) > p
    with pytest.raises(ValueError, match="blamed locations"):
        device.scrub_to_erased(rep, p)


@pytest.mark.parametrize("k,p,L", [(10, 4, 4129), (6, 3, 2049)])
def test_heal_unaligned_rows_and_report_stride(cuda, k, p, L):
    """Rows shifted by one byte take the byte-granular kernel; a report_stride
    of 4 + n + 3 leaves the three words after each report alone."""
    torch = cuda
    n = k + p
    host, want, want_rep, _ = _inputs(k, p, L)
    code = HipReedSolomonCode(k, p, device=0)
    big, view = _device_view(torch, host, shift=1)
    assert view.data_ptr() % 16 == 1
    before = big.clone()
    rep = torch.full((S, 4 + n + 3), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    rows = _lib.ptr_array([view.data_ptr() + l * view.stride(1) for l in range(n)])
    code._check(_lib.lib().hrs_heal_dev(code._handle(), rows, view.stride(0), L, S, rep.data_ptr(), 4 + n + 3,
                                        torch.cuda.current_stream().cuda_stream))
    got = _u32(rep)
    assert code.lastKernel() == f"heal_bytewise_kernel<{p}>"
    assert got[:, :4 + n].tolist() == want_rep.tolist()
    assert (got[:, 4 + n:] == 0x5A5A5A5A).all()
    assert (view.cpu().numpy() == want).all() and _outside_unchanged(big, before, host.shape, shift=1)


def test_heal_rejects_equal_row_pointers(cuda):
    torch = cuda
    k, p, L = 3, 2, 64
    n = k + p
    code = HipReedSolomonCode(k, p, device=0)
    st = torch.zeros((1, n, L), dtype=torch.uint8, device="cuda:0")
    rep = torch.zeros((1, 4 + n), dtype=torch.int32, device="cuda:0")
    rows = _lib.ptr_array([st.data_ptr() + (1 if l == 4 else l) * L for l in range(n)])
    assert _lib.lib().hrs_heal_dev(code._handle(), rows, n * L, L, 1, rep.data_ptr(), 4 + n, None) == _lib.HRS_EINVAL


@pytest.mark.parametrize("mode", [0, 2])
def test_heal_widest_code_n255(cuda, mode):
    """RS(247,8), n = 255: the last entry of the row table is patched (location
    254 is blamed in stripe 1), one window + tail, both kernels."""
    k, p, L = 247, 8, 2049
    host, want, want_rep, planted = _inputs(k, p, L)
    assert want_rep[1, 4 + 254] >= 1 and (host[1, 254] != want[1, 254]).any() and want_rep[:, 1].any()
    code = HipReedSolomonCode(k, p, device=0)
    code.setKernelMode(mode)
    big, view = _device_view(cuda, host)
    before = big.clone()
    rep = _u32(device.heal_stripes(code, view))
    got = view.cpu().numpy()
    assert code.lastKernel() == _kernel_name(p, mode, L)
    assert (got == want).all() and _outside_unchanged(big, before, host.shape)
    assert rep.tolist() == want_rep.tolist()
    _check_planted(k, p, L, host, want, rep, planted, got)


# ------------------------------------------------------------ host batch

HB = dict(k=12, p=4, L=4129, S=5, guard=0xC3)


def _host_batch():
    """RS(12,4), L = 4129, 5 stripes, as (stripes [S, n, L], healed, reports):
    0 clean; 1 single-byte errors in both windows and the tail; 2 one whole
    cell replaced; 3 an unresolved column, a double error and a single one;
    4 clean."""
    if "hb" in _cache:
        return _cache["hb"]
    k, p, L, ns = HB["k"], HB["p"], HB["L"], HB["S"]
    n = k + p
    rng = np.random.default_rng(4129)
    rnd = random.Random(4129)
    host = np.zeros((ns, n, L), dtype=np.uint8)
    for s in range(ns):
        data = [rng.integers(0, 256, L, dtype=np.uint8) for _ in range(k)]
        host[s] = np.stack(C.encode_bulk(k, p, data) + data)
    for l, c in [(0, 0), (15, 2047), (4, 2048), (7, 4095), (3, 4096), (12, L - 1)]:
        host[1, l, c] ^= rnd.randrange(1, 256)
    host[2, 9] = rng.integers(0, 256, L, dtype=np.uint8)
    host[3, :, 77] = _search(k, p, host[3, :, 77].tolist(), rnd, 3, lambda ok, found, after, t: not ok and after != t)
    host[3, 1, 3000] ^= 0x11
    host[3, 14, 3000] ^= 0x80
    host[3, 5, 4100] ^= 0xFF
    want = np.empty_like(host)
    rep = np.empty((ns, 4 + n), dtype=np.uint32)
    for s in range(ns):
        want[s], rep[s] = heal_expected(k, p, host[s])
    assert not rep[0, [0, 1, 3]].any() and rep[2, 3] >= L - 40 and rep[3, :4].tolist() == [3, 1, 77, 3]
    assert (want[[0, 4]] == host[[0, 4]]).all() and (want[3, :, 77] == host[3, :, 77]).all()
    _cache["hb"] = (host, want, rep)
    return _cache["hb"]


def _guarded(host, pinned, torch):
    """host[S, n, L] inside a larger buffer full of the guard byte: padding
    after each row (row stride a multiple of 16) and a spare row per stripe.
    Returns (big, view) as numpy arrays over pageable or pinned memory, and
    the object to hand to heal_batch_host."""
    s, n, L = host.shape
    pitch = ((L + 15) // 16) * 16 + 16
    if pinned:
        t = torch.full((s, n + 1, pitch), HB["guard"], dtype=torch.uint8).pin_memory()
        big = t.numpy()
        arg = t[:, :n, :L]
    else:
        big = np.full((s, n + 1, pitch), HB["guard"], dtype=np.uint8)
        arg = big[:, :n, :L]
    big[:, :n, :L] = host
    return big, big[:, :n, :L], arg


def _guards_intact(big, n, L):
    return bool((big[:, n] == HB["guard"]).all() and (big[:, :, L:] == HB["guard"]).all())


def _check_host_batch(code, torch, pinned, path):
    host, want, want_rep = _host_batch()
    n, L = host.shape[1], host.shape[2]
    big, view, arg = _guarded(host, pinned, torch)
    got = device.heal_batch_host(code, arg)
    assert code.lastHostPath() == path
    assert code.lastKernel() == "heal_kernel<4>"
    assert got.dtype == np.uint32 and got.tolist() == want_rep.tolist()
    assert (view == want).all()
    assert _guards_intact(big, n, L)
    again = device.heal_batch_host(code, arg)  # nothing left to store
    assert not again[:, 3].any() and again[:, 0].tolist() == want_rep[:, 1].tolist() and (view == want).all()


def test_heal_batch_host_pinned(cuda):
    code = HipReedSolomonCode(HB["k"], HB["p"], device=0)
    _check_host_batch(code, cuda, True, "pinned")


@pytest.mark.parametrize("chunk_stripes", [None, 1])
def test_heal_batch_host_pageable(cuda, monkeypatch, chunk_stripes):
    """Staged through the pinned slots (one chunk, and chunks of one stripe so
    that the 3 slots are refilled after their healed cells have left): only
    the cells with a blamed location are copied back, so the clean stripes'
    memory (guards included) is compared byte for byte with what it held."""
    if chunk_stripes:
        monkeypatch.setenv("HRS_HBATCH_BYTES", str(chunk_stripes * (HB["k"] + HB["p"]) * (HB["L"] + 256)))
    code = HipReedSolomonCode(HB["k"], HB["p"], device=0)
    _check_host_batch(code, cuda, False, "staged")
    host, want, _ = _host_batch()
    big, view, arg = _guarded(host, False, cuda)
    before = big.copy()
    device.heal_batch_host(code, arg)
    assert (big[[0, 4]] == before[[0, 4]]).all()
    changed = np.argwhere((big != before).any(axis=2))  # (stripe, row) cells that differ at all
    assert {tuple(x) for x in changed.tolist()} <= {(1, 0), (1, 15), (1, 4), (1, 7), (1, 3), (1, 12), (2, 9), (3, 1),
                                                    (3, 14), (3, 5)}


@pytest.mark.parametrize("duplex", ["0", "1"])
def test_heal_batch_host_copy_engine(cuda, monkeypatch, duplex):
    """Zero copy switched off: H2D -> heal kernels on the device image -> D2H
    of the healed cells only, for pinned and for pageable stripes, chunks of
    one stripe so that the 3 slots are reused by the 5 stripes."""
    n, L = HB["k"] + HB["p"], HB["L"]
    code = HipReedSolomonCode(HB["k"], HB["p"], device=0)
    monkeypatch.setenv("HRS_ZEROCOPY", "0")
    monkeypatch.setenv("HRS_HBATCH_DUPLEX", duplex)
    monkeypatch.setenv("HRS_HBATCH_BYTES", str(n * (L + 256)))
    for pinned in (True, False):
        _check_host_batch(code, cuda, pinned, "copy_engine")
