"""hrs_heal_erased_dev on the GPU (heal_erased_kernel<P> and
heal_erased_bytewise_kernel<P>, hrs_heal_erased.hip): seven stripes of two
windows plus a tail, each with its own erasure pattern, survivor errors within
capacity planted at window, piece and row edges. Expected bytes are the
oracle-encoded stripes themselves and the reports are counted from the planted
list; at parity_size 5 to 8, where the reference locator may leave a few
columns within capacity unresolved, the byte-exact reference is
hrs_heal_erased_host.
The CPU test at the top checks the inputs without a device."""
import random

import numpy as np
import pytest

import heal_erased_inputs as H
from lambdafs_amd import HipReedSolomonCode, HrsError, TooManyErasedLocations, _lib, device

L = 2 * H.WINDOW + 33
SHAPES = [(10, 4), (12, 4), (6, 3), (3, 2), (4, 1), (20, 8), (6, 5), (7, 6), (10, 7)]
NONE_DEV = -2  # HRS_DEVICE_NONE
SPARE = 3


def _case(k, p, over=0, seed=1):
    rnd = random.Random(1009 * k + p + seed)
    pats = H.seven_patterns(k, p, rnd)
    clean = H.clean_stripes(k, p, 7, L, seed)
    bad, planted = H.plant(k, p, clean, pats, H.columns_of(L), over=over, seed=seed)
    return clean, bad, pats, planted


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _aligned(torch, host):
    """host[S, n, L] on the device as a view with a 16-byte multiple row pitch
    (rows and stripe stride aligned whatever L is)."""
    S, n, length = host.shape
    big = torch.full((S, n, (length + 15) // 16 * 16), 0xC3, dtype=torch.uint8, device="cuda:0")
    view = big[:, :, :length]
    view.copy_(torch.from_numpy(np.array(host)).to("cuda:0"))
    assert view.data_ptr() % 16 == 0 and view.stride(0) % 16 == 0 and view.stride(1) % 16 == 0
    return view


def _unresolved_share(k, p, bad, clean, pats, planted):
    """(host result, host reports, unresolved within-capacity columns, planted columns)."""
    code = HipReedSolomonCode(k, p, device=NONE_DEV)
    after, reps = H.host_reference(code, bad, pats)
    # a resolved column within capacity is the codeword again; an unresolved one keeps its damage
    wrong = int((after != clean).any(axis=1).sum())
    assert wrong == int(reps[:, 1].sum())
    return after, reps, wrong, len(planted)


@pytest.mark.parametrize("k,p", SHAPES + [(247, 8)])
def test_inputs_within_capacity(k, p):
    """No device: the patterns cover what the issue lists, the planted errors
    are within capacity, and hrs_heal_erased_host restores them: all of them
    and with exactly the planted reports at p <= 4; at p > 4 all but the
    unresolved columns, which stay below 5 % of the planted ones."""
    n = k + p
    clean, bad, pats, planted = _case(k, p)
    assert [len(e) for e in pats] == [0, 1, 1, min(2, p), p - 1, p, 1]
    assert pats[1][0] >= p and pats[2] == [0] and n - 1 in pats[3]
    assert all((bad[s, pats[s]] == H.FILL).all() for s in range(7))
    assert (bad[6][[l for l in range(n) if l not in pats[6]]] == clean[6][[l for l in range(n) if l not in pats[6]]]).all()
    cols = {c for _, c, _ in planted}
    if p >= 2:
        assert cols == set(H.columns_of(L)) >= {0, 15, 16, 1023, 1024, 2047, 2048, L - 1}
    if p >= 3:  # capacity is left beside an erasure
        assert any(l - 1 in pats[s] or l + 1 in pats[s] for s, _, errs in planted for l in errs)
        assert len({s for s, c, _ in planted if c == 0}) >= 2  # one column of two stripes
    for s, _, errs in planted:
        assert 1 <= len(errs) <= (p - len(pats[s])) // 2 and not set(errs) & set(pats[s])
    after, reps, unresolved, total = _unresolved_share(k, p, bad, clean, pats, planted)
    print(f"RS({k},{p}): {total} planted columns, {unresolved} unresolved on the host")
    if p <= 4:
        assert (after == clean).all()
        assert reps.tolist() == H.planted_reports(n, 7, planted).tolist()
    else:
        assert unresolved * 20 <= total


def _run(torch, k, p, mode, bad, pats, spare=0):
    """One hrs_heal_erased_dev call: (bytes after [S, n, L], reports, kernel)."""
    n, S = k + p, bad.shape[0]
    code = HipReedSolomonCode(k, p, device=0)
    code.setKernelMode(mode)
    st = _aligned(torch, bad)
    if spare:
        rep = torch.full((S, 4 + n + spare), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
        rows = _lib.ptr_array([st.data_ptr() + l * st.stride(1) for l in range(n)])
        arr = H.erased_array(pats)
        code._check(_lib.lib().hrs_heal_erased_dev(code._handle(), rows, st.stride(0), bad.shape[2], S, arr.ctypes.data,
                                                   arr.shape[1], rep.data_ptr(), 4 + n + spare,
                                                   torch.cuda.current_stream().cuda_stream))
        raw = _u32(rep)
        assert (raw[:, 4 + n:] == 0x5A5A5A5A).all(), "words past 4 + n of a report were written"
        reports = raw[:, :4 + n]
    else:
        reports = _u32(device.heal_erased_stripes(code, st, pats))
    return st, reports, code


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("k,p", SHAPES)
def test_heal_erased_restores_the_stripes(cuda, k, p, mode):
    n = k + p
    clean, bad, pats, planted = _case(k, p)
    st, reports, code = _run(cuda, k, p, mode, bad, pats)
    assert code.lastKernel() == (f"heal_erased_kernel<{p}>" if mode == 0 else f"heal_erased_bytewise_kernel<{p}>")
    got = st.cpu().numpy()
    if p <= 4:
        assert (got == clean).all(), np.argwhere(got != clean)[:4].tolist()
        assert reports.tolist() == H.planted_reports(n, 7, planted).tolist()
    else:
        after, reps, unresolved, total = _unresolved_share(k, p, bad, clean, pats, planted)
        assert (got == after).all(), np.argwhere(got != after)[:4].tolist()
        assert reports.tolist() == reps.tolist()
        assert unresolved * 20 <= total
    # a second call finds the survivors consistent wherever the first resolved: it stores no survivor byte
    arr = H.erased_array(pats)
    again = _u32(device.heal_erased_stripes(code, st, arr))
    assert not again[:, 3].any() and (st.cpu().numpy() == got).all()
    if p <= 4:
        assert again.tolist() == H.planted_reports(n, 7, []).tolist()


@pytest.mark.gpu
def test_heal_erased_widest_code(cuda):
    """RS(247,8), n = 255 (the widest code), once."""
    k, p = 247, 8
    clean, bad, pats, planted = _case(k, p)
    after, reps, unresolved, total = _unresolved_share(k, p, bad, clean, pats, planted)
    st, reports, code = _run(cuda, k, p, 0, bad, pats)
    assert code.lastKernel() == "heal_erased_kernel<8>"
    got = st.cpu().numpy()
    assert (got == after).all(), np.argwhere(got != after)[:4].tolist()
    assert reports.tolist() == reps.tolist() and unresolved * 20 <= total


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 2])
def test_nothing_erased_is_the_heal(cuda, mode):
    """e = 0 through the new kernels (max_erased 1, every entry -1) against
    hrs_heal_dev on the same input, columns past capacity included."""
    torch = cuda
    k, p = 10, 4
    clean = H.clean_stripes(k, p, 7, L, 1)
    none = [[] for _ in range(7)]
    bad, planted = H.plant(k, p, clean, none, H.columns_of(L), clean_stripes_=(), seed=2)
    more, _ = H.plant(k, p, clean, none, [5, 1030, L - 2], over=1, clean_stripes_=(), seed=3)
    bad[:, :, [5, 1030, L - 2]] = more[:, :, [5, 1030, L - 2]]
    st, reports, code = _run(torch, k, p, mode, bad, none)
    assert "heal_erased" in code.lastKernel()
    ref = _aligned(torch, bad)
    want = _u32(device.heal_stripes(code, ref))
    assert torch.equal(st, ref) and reports.tolist() == want.tolist()
    assert want[:, 1].all() and want[:, 3].all()
    # max_erased == 0 is hrs_heal_dev itself
    st0 = _aligned(torch, bad)
    rep0 = torch.empty((7, 4 + k + p), dtype=torch.int32, device="cuda:0")
    rows = _lib.ptr_array([st0.data_ptr() + l * st0.stride(1) for l in range(k + p)])
    code._check(_lib.lib().hrs_heal_erased_dev(code._handle(), rows, st0.stride(0), L, 7, None, 0, rep0.data_ptr(),
                                               4 + k + p, torch.cuda.current_stream().cuda_stream))
    assert torch.equal(st0, ref) and _u32(rep0).tolist() == want.tolist()
    assert code.lastKernel().startswith("heal_kernel" if mode == 0 else "heal_bytewise_kernel")


@pytest.mark.gpu
@pytest.mark.parametrize("k,p", [(10, 4), (6, 3)])
def test_clean_survivors_give_the_batch_repair_rows(cuda, k, p):
    torch = cuda
    n = k + p
    clean = H.clean_stripes(k, p, 7, L, 1)
    pats = H.seven_patterns(k, p, random.Random(5))
    bad, _ = H.plant(k, p, clean, pats, [], seed=0)
    code = HipReedSolomonCode(k, p, device=0)
    st = _aligned(torch, bad)
    arr = H.erased_array(pats, p)
    out = torch.zeros((7, p, L), dtype=torch.uint8, device="cuda:0")
    device.decode_batch(code, st, arr, out)
    reports = _u32(device.heal_erased_stripes(code, st, arr))
    assert reports.tolist() == H.planted_reports(n, 7, []).tolist()
    got = st.cpu().numpy()
    rows = out.cpu().numpy()
    for s, E in enumerate(pats):
        for t, l in enumerate(E):
            assert (got[s, l] == rows[s, t]).all(), (s, l)
    assert (got == clean).all()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("k,p", [(10, 4), (6, 3), (20, 8), (6, 5), (7, 6), (10, 7)])
def test_one_past_capacity_matches_the_host(cuda, k, p, mode):
    n = k + p
    clean, bad, pats, planted = _case(k, p, over=1, seed=4)
    code = HipReedSolomonCode(k, p, device=NONE_DEV)
    after, reps = H.host_reference(code, bad, pats)
    st, reports, _ = _run(cuda, k, p, mode, bad, pats)
    got = st.cpu().numpy()
    assert (got == after).all(), np.argwhere(got != after)[:4].tolist()
    assert reports.tolist() == reps.tolist()
    assert reps[:, 1].sum() > 0
    # the survivors of a stripe whose bad columns are all unresolved are untouched
    for s in range(7):
        if reps[s, 0] and reps[s, 0] == reps[s, 1]:
            keep = [l for l in range(n) if l not in pats[s]]
            assert (got[s, keep] == bad[s, keep]).all() and reps[s, 3] == 0 and not reps[s, 4:].any()


@pytest.mark.gpu
def test_unaligned_rows_and_report_stride(cuda):
    """Rows one byte off 16-byte alignment, a stripe stride 5 bytes off, and
    reports of 4 + n + 3 words: the byte-granular kernel, same results."""
    torch = cuda
    k, p = 10, 4
    n = k + p
    clean, bad, pats, planted = _case(k, p)
    pitch = n * L + 5
    flat = torch.full((1 + 7 * pitch + 64,), 0xC3, dtype=torch.uint8, device="cuda:0")
    st = torch.as_strided(flat, (7, n, L), (pitch, L, 1), 1)
    st.copy_(torch.from_numpy(bad).to("cuda:0"))
    before = flat.clone()
    code = HipReedSolomonCode(k, p, device=0)
    rep = torch.full((7, 4 + n + SPARE), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    rows = _lib.ptr_array([st.data_ptr() + l * L for l in range(n)])
    arr = H.erased_array(pats)
    code._check(_lib.lib().hrs_heal_erased_dev(code._handle(), rows, pitch, L, 7, arr.ctypes.data, arr.shape[1],
                                               rep.data_ptr(), 4 + n + SPARE, torch.cuda.current_stream().cuda_stream))
    assert code.lastKernel() == "heal_erased_bytewise_kernel<4>"
    raw = _u32(rep)
    assert (raw[:, 4 + n:] == 0x5A5A5A5A).all()
    assert raw[:, :4 + n].tolist() == H.planted_reports(n, 7, planted).tolist()
    assert (st.cpu().numpy() == clean).all()
    st.copy_(torch.from_numpy(bad).to("cuda:0"))
    assert torch.equal(flat, before)  # nothing outside the cells moved
    # aligned rows, strided reports: the vector kernel
    _, reports, _ = _run(torch, k, p, 0, bad, pats, spare=SPARE)
    assert reports.tolist() == H.planted_reports(n, 7, planted).tolist()


@pytest.mark.gpu
def test_bad_arguments_are_rejected_on_a_device_handle(cuda):
    torch = cuda
    k, p = 10, 4
    n = k + p
    code = HipReedSolomonCode(k, p, device=0)
    st = torch.zeros((2, n, 64), dtype=torch.uint8, device="cuda:0")
    with pytest.raises(TooManyErasedLocations):
        device.heal_erased_stripes(code, st, [[0], [0, 1, 2, 3, 4]])
    with pytest.raises(HrsError):
        device.heal_erased_stripes(code, st, [[0], [n]])
    with pytest.raises(HrsError):
        device.heal_erased_stripes(code, st, [[0], [2, 2]])
    rep = torch.zeros((2, 4 + n), dtype=torch.int32, device="cuda:0")
    twice = _lib.ptr_array([st.data_ptr() + (0 if l == 3 else l) * 64 for l in range(n)])
    arr = H.erased_array([[0], [1]])
    assert _lib.lib().hrs_heal_erased_dev(code._handle(), twice, n * 64, 64, 2, arr.ctypes.data, 1, rep.data_ptr(),
                                          4 + n, None) == _lib.HRS_EINVAL
    torch.cuda.synchronize()
    assert not st.any() and not rep.any()


# ---- many dirty windows per wave (after test_gpu_scrub_waves.py, small)

def _waves_case():
    k, p, S, Lw = 10, 4, 40, 3 * H.WINDOW + 33
    rnd = random.Random(77)
    clean = H.clean_stripes(k, p, S, Lw, 9)
    base = H.seven_patterns(k, p, rnd)
    pats = [base[rnd.randrange(6)] if s % 4 else sorted(rnd.sample(range(k + p), rnd.randrange(0, 3))) for s in range(S)]
    cols = sorted({w * H.WINDOW + c for w in range(3) for c in (0, 517, 2047)} | {Lw - 1})
    quiet = tuple(s for s in range(S) if s % 5 == 3)  # clean survivors
    bad, planted = H.plant(k, p, clean, pats, cols, clean_stripes_=quiet, seed=11)
    return k, p, clean, bad, pats, planted


def test_waves_inputs():
    k, p, clean, bad, pats, planted = _waves_case()
    dirty = {(s, c // H.WINDOW) for s, c, _ in planted if c < 3 * H.WINDOW}
    assert len(dirty) >= 40 and len({tuple(e) for e in pats}) >= 6
    after, reps = H.host_reference(HipReedSolomonCode(k, p, device=NONE_DEV), bad, pats)
    assert (after == clean).all() and reps.tolist() == H.planted_reports(k + p, 40, planted).tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("order", [1, 32])
def test_many_dirty_windows_per_wave(cuda, monkeypatch, order):
    """RS(10,4), 40 stripes of 3 windows + 33 bytes with mixed patterns, most
    of them dirty in every window: under HRS_TASK_ORDER 32 one block
    runs all 120 windows, 30 per wave, stripe after stripe."""
    monkeypatch.setenv("HRS_TASK_ORDER", str(order))
    k, p, clean, bad, pats, planted = _waves_case()
    st, reports, code = _run(cuda, k, p, 0, bad, pats)
    assert code.lastKernel() == "heal_erased_kernel<4>"
    got = st.cpu().numpy()
    assert (got == clean).all(), np.argwhere(got != clean)[:4].tolist()
    assert reports.tolist() == H.planted_reports(k + p, 40, planted).tolist()
