"""GPU tests of checked repair (hrs_repair_checked_dev): bytes, verdicts,
erased_out, reports and CRCs against hrs_repair_checked_host stripe by stripe,
all compared exactly, over small shapes that hit the kernels' edges (whole
windows, windows plus tail, byte-granular only, layouts offset by one byte,
kernel mode 2, n = 20 past the fused scrub's 16 rows); the cross-check with the
existing device calls; batches with no stripe listed, every stripe listed and
one stripe; many listed windows per wave; the footprint in guarded arenas;
repetition on one handle; and a non-default stream. The inputs and their
recipes are tests/repair_checked_inputs.py. The references are computed once
per shape and shared."""
import numpy as np
import pytest

import repair_checked_inputs as R
from gpu_arena import POISON_WORD, Arena, CrcArena
from lambdafs_amd import HipReedSolomonCode, _lib, device

pytestmark = pytest.mark.gpu

S = 37
LISTED = (0, 5, 6, 13, 20, 21, 22, 30, S - 1)  # both ends, pairs, a run and lone stripes
LENGTHS = [2048, 2 * 2048 + 80, 100]
NONE = -2

_batches, _refs = {}, {}


def batch(k, p, L, nstripes=S, listed=LISTED, seed=0):
    key = (k, p, L, nstripes, tuple(listed), seed)
    if key not in _batches:
        st, stored = R.mix(k, p, L, nstripes, set(listed), seed)
        st.setflags(write=False)
        stored.setflags(write=False)
        _batches[key] = (st, stored)
    return _batches[key]


def host_reference(k, p, stripes, stored, join, key=None):
    """hrs_repair_checked_host stripe by stripe on a host-only handle."""
    if key is not None and (key, join) in _refs:
        return _refs[(key, join)]
    code = HipReedSolomonCode(k, p, device=NONE)
    n = k + p
    out = np.array(stripes)
    ns = len(out)
    verdicts = np.zeros(ns, dtype=np.int64)
    erased = np.zeros((ns, p), dtype=np.int64)
    reports = np.zeros((ns, 4 + n), dtype=np.int64)
    crcs = np.zeros((ns, n), dtype=np.int64)
    for s in range(ns):
        rows = [np.ascontiguousarray(out[s, l]) for l in range(n)]
        verdicts[s], erased[s], reports[s], crcs[s] = device.repair_checked_host(code, rows, stored[s], join)
        out[s] = np.stack(rows)
    ref = (out, verdicts, erased, reports, crcs)
    if key is not None:
        _refs[(key, join)] = ref
    return ref


def u32(t):
    return t.cpu().numpy().astype(np.int64) & 0xFFFFFFFF


def to_device(torch, stripes, offset):
    """The batch on the device: contiguous, or a [S, n, L] view one byte into a [S, n, L + 1] tensor."""
    ns, n, L = stripes.shape
    if not offset:
        return torch.from_numpy(np.array(stripes)).to("cuda:0")
    base = torch.zeros((ns, n, L + 1), dtype=torch.uint8, device="cuda:0")
    view = base[:, :, 1:]
    view.copy_(torch.from_numpy(np.array(stripes)).to("cuda:0"))
    return view


def stored_tensor(torch, stored):
    return torch.from_numpy(np.array(stored).view(np.int32)).to("cuda:0")


def check(torch, got, st, ref, what):
    out, verdicts, erased, reports, crcs = ref
    gv, ge, gr, gc = got
    torch.cuda.synchronize()
    assert u32(gv).tolist() == verdicts.tolist(), what
    assert ge.cpu().numpy().tolist() == erased.tolist(), what
    assert (u32(gr) == reports).all(), what
    assert (u32(gc) == crcs).all(), what
    assert (st.cpu().numpy() == out).all(), what


@pytest.mark.parametrize("join", [False, True])
@pytest.mark.parametrize("layout,mode", [("aligned", 0), ("offset", 0), ("aligned", 2)])
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("k,p", R.CODES)
def test_repair_checked_equals_the_host_call(cuda, k, p, L, layout, mode, join):
    torch = cuda
    stripes, stored = batch(k, p, L)
    ref = host_reference(k, p, stripes, stored, join, key=(k, p, L, S, LISTED, 0))
    assert set(ref[1].tolist()) >= {R.CLEAN, R.REPAIRED, R.TOOMANY}  # a mix: listed and unlisted stripes
    code = HipReedSolomonCode(k, p, device=0)
    code.setKernelMode(mode)
    st = to_device(torch, stripes, layout == "offset")
    got = device.repair_checked_stripes(code, st, stored_tensor(torch, stored), join_syndromes=join)
    check(torch, got, st, ref, f"RS({k},{p}) L={L} {layout} mode {mode} join={join}")
    # pass 1's kernel, as hrs_scrub_crc_dev names it
    vec = layout == "aligned" and mode == 0 and L >= 2048
    fused = vec and L % 2048 == 0 and 2 <= p <= 4 and k + p <= 16
    want = f"scrub_crc_kernel<{p}>" if fused else f"scrub_kernel<{p}>" if vec else f"scrub_bytewise_kernel<{p}>"
    assert code.lastKernel() == want
    # the unlisted stripes are byte-identical
    unlisted = np.isin(ref[1], [R.CLEAN, R.TOOMANY, R.AMBIGUOUS])
    assert (st.cpu().numpy()[unlisted] == stripes[unlisted]).all()


def test_all_six_verdicts_in_one_batch(cuda):
    """RS(3,2) and RS(10,4) between them give every verdict on the device."""
    torch = cuda
    seen = set()
    for k, p in ((3, 2), (10, 4)):
        stripes, stored = batch(k, p, 2 * 2048 + 80)
        code = HipReedSolomonCode(k, p, device=0)
        for join in (False, True):
            st = to_device(torch, stripes, False)
            v = device.repair_checked_stripes(code, st, stored_tensor(torch, stored), join_syndromes=join)[0]
            seen |= set(u32(v).tolist())
    assert seen == {R.CLEAN, R.REPAIRED, R.RESTAMP, R.FAILED, R.TOOMANY, R.AMBIGUOUS}


@pytest.mark.parametrize("join", [False, True])
@pytest.mark.parametrize("k,p,L", [(10, 4, 2 * 2048 + 80), (12, 8, 2 * 2048 + 80), (6, 3, 2048)])
def test_listed_stripes_equal_the_existing_device_calls(cuda, k, p, L, join):
    """scrub_stripes_crc, checksums_to_erased, heal_erased_stripes_crc on the
    listed stripes gathered into their own tensor: the same bytes, reports,
    erased sets and CRCs."""
    torch = cuda
    stripes, stored = batch(k, p, L)
    code = HipReedSolomonCode(k, p, device=0)
    st = to_device(torch, stripes, False)
    verdicts, erased, reports, crcs = device.repair_checked_stripes(code, st, stored_tensor(torch, stored), join)
    torch.cuda.synchronize()
    listed = np.flatnonzero(np.isin(u32(verdicts), [R.REPAIRED, R.RESTAMP, R.FAILED]))
    assert len(listed) >= len(LISTED) - 2
    before = to_device(torch, stripes, False)
    r1, c1 = device.scrub_stripes_crc(code, before)
    idx = torch.from_numpy(listed).to("cuda:0")
    want_e = device.checksums_to_erased(c1[idx], stored[listed], p, r1[idx] if join else None)
    gathered = before[idx].contiguous()
    r2, c2 = device.heal_erased_stripes_crc(code, gathered, want_e)
    torch.cuda.synchronize()
    assert erased.cpu().numpy()[listed].tolist() == want_e.tolist()
    assert torch.equal(st[idx], gathered) and torch.equal(reports[idx], r2) and torch.equal(crcs[idx], c2)
    rest = np.setdiff1d(np.arange(S), listed)
    ridx = torch.from_numpy(rest).to("cuda:0")
    assert torch.equal(reports[ridx], r1[ridx]) and torch.equal(crcs[ridx], c1[ridx]) and torch.equal(st[ridx], before[ridx])


@pytest.mark.parametrize("join", [False, True])
@pytest.mark.parametrize("name,nstripes,listed", [("none_listed", 9, ()), ("all_listed", 9, tuple(range(9))),
                                                  ("one_listed_stripe", 1, (0,)), ("one_clean_stripe", 1, ())])
@pytest.mark.parametrize("k,p,L", [(10, 4, 2 * 2048 + 80), (3, 2, 100)])
def test_batches_at_the_edges_of_the_list(cuda, k, p, L, name, nstripes, listed, join):
    torch = cuda
    if name == "none_listed":  # all clean
        one, st1 = R.recipe("clean", k, p, L, 3)
        stripes, stored = np.repeat(one[None], nstripes, 0), np.repeat(st1[None], nstripes, 0)
    else:
        stripes, stored = batch(k, p, L, nstripes, listed, seed=11)
    ref = host_reference(k, p, stripes, stored, join)
    if name == "none_listed":
        assert (ref[1] == R.CLEAN).all()
    if name == "all_listed" and not join:  # joined, three cells of garbage pass p (the documented contrast)
        assert np.isin(ref[1], [R.REPAIRED, R.RESTAMP, R.FAILED]).all()
    code = HipReedSolomonCode(k, p, device=0)
    st = to_device(torch, stripes, False)
    got = device.repair_checked_stripes(code, st, stored_tensor(torch, stored), join_syndromes=join)
    check(torch, got, st, ref, f"{name} RS({k},{p}) L={L} join={join}")


@pytest.mark.parametrize("order", [0, 1, 32])
@pytest.mark.parametrize("k,p", [(10, 4), (12, 8)])
def test_many_listed_windows_per_wave(cuda, monkeypatch, k, p, order):
    """16 windows per cell: under HRS_TASK_ORDER 32 one wave of the listed heal
    walks 32 windows in a row, which belong to scattered listed stripes that
    are neighbours only in the list; no stripe's report may leak into
    another's. Orders 0 and 1 run the same batch in the other two schedules."""
    torch = cuda
    L = 16 * 2048
    stripes, stored = batch(k, p, L)
    ref = host_reference(k, p, stripes, stored, False, key=(k, p, L, S, LISTED, 0))
    monkeypatch.setenv("HRS_TASK_ORDER", str(order))
    code = HipReedSolomonCode(k, p, device=0)
    st = to_device(torch, stripes, False)
    got = device.repair_checked_stripes(code, st, stored_tensor(torch, stored))
    check(torch, got, st, ref, f"RS({k},{p}) order {order}")


@pytest.mark.parametrize("order", [0, 1])
def test_more_listed_windows_than_waves(cuda, monkeypatch, order):
    """129 listed stripes of 16 windows: 2,064 listed windows, more than the
    2,048 waves of the largest grid the launcher picks (two blocks of four
    waves on each of 256 CUs), so that some waves come back for a second window
    a whole grid further on. (HRS_ZC_BLOCKS cannot shrink the grid here: it
    caps zero-copy launches over host memory only, and this call has no
    host-batch form.)"""
    torch = cuda
    k, p, L, ns = 3, 2, 16 * 2048, 132
    listed = tuple(s for s in range(ns) if s not in (1, 50, ns - 1))
    stripes, stored = batch(k, p, L, ns, listed, seed=3)
    ref = host_reference(k, p, stripes, stored, False, key=(k, p, L, ns, listed, 3))
    assert int(np.isin(ref[1], [R.REPAIRED, R.RESTAMP, R.FAILED]).sum()) == len(listed)
    monkeypatch.setenv("HRS_TASK_ORDER", str(order))
    code = HipReedSolomonCode(k, p, device=0)
    st = to_device(torch, stripes, False)
    got = device.repair_checked_stripes(code, st, stored_tensor(torch, stored))
    check(torch, got, st, ref, f"RS({k},{p}) {ns} stripes order {order}")


# name -> (L, shift, stripe_pad, kernel mode)
FOOTPRINT = {
    "whole_windows": (2 * 2048, 0, 0, 0),
    "windows_and_tail": (2048 + 100, 0, 0, 0),
    "tail_only": (100, 0, 0, 0),
    "shift_1": (2048 + 100, 1, 0, 0),
    "stride_pad_5": (2048 + 100, 0, 5, 0),
    "mode_2": (2 * 2048, 0, 0, 2),
}


@pytest.mark.parametrize("join", [False, True])
@pytest.mark.parametrize("name", list(FOOTPRINT))
def test_repair_checked_footprint(cuda, name, join):
    """The whole call in guarded arenas: the cells, and reports (with a report
    stride three words wider than 4 + n), verdicts, erased_out and crc_out each
    between guard words. One comparison per arena against the pre-call image
    with exactly the reference's values put in: no other byte or word changes,
    the words past 4 + n of every report included, and the cells of the
    stripes that are not listed stay as they were."""
    torch = cuda
    k, p, ns = 10, 4, 9
    n = k + p
    L, shift, pad, mode = FOOTPRINT[name]
    stripes, stored = batch(k, p, L, ns, (0, 3, 4, 8), seed=5)
    ref_out, verdicts, erased, reports, crcs = host_reference(k, p, stripes, stored, join)
    arena = Arena(ns, L, shift=shift, stripe_pad=pad, seed=L + shift)
    names = arena.add_rows("loc", n, "input")
    flat, _ = arena.to_device()
    st = arena.stack(flat, names)
    st.copy_(torch.from_numpy(np.array(stripes)).to("cuda:0"))
    pre = flat.cpu().numpy()
    wide = 4 + n + 3
    areps, averd, aerased, acrc = CrcArena(ns, wide, False), CrcArena(ns, 1, False), CrcArena(ns, p, False), CrcArena(ns, n, False)
    (rflat, _, rout), (vflat, _, vout), (eflat, _, eout), (cflat, _, cout) = (a.to_device() for a in (areps, averd, aerased, acrc))
    sdev = stored_tensor(torch, stored)
    code = HipReedSolomonCode(k, p, device=0)
    code.setKernelMode(mode)
    rows = _lib.ptr_array([st.data_ptr() + l * st.stride(1) for l in range(n)])
    code._check(_lib.lib().hrs_repair_checked_dev(code._handle(), rows, st.stride(0), L, ns, sdev.data_ptr(),
                                                  1 if join else 0, vout, eout, rout, wide, cout,
                                                  torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    exp = pre.copy()
    for l, x in enumerate(names):
        for s in range(ns):
            o = arena.offset(x, s)
            exp[o:o + L] = ref_out[s, l]
    d = arena.diff(flat.cpu().numpy(), exp)
    assert d is None, d
    wide_reports = np.full((ns, wide), POISON_WORD, dtype=np.uint32)
    wide_reports[:, : 4 + n] = reports
    for a, f, want in ((areps, rflat, wide_reports), (averd, vflat, verdicts[:, None]),
                       (aerased, eflat, erased.astype(np.int32).view(np.uint32)), (acrc, cflat, crcs)):
        d = a.diff(f.cpu().numpy(), a.expected(np.asarray(want, dtype=np.uint32)))
        assert d is None, d
    assert (sdev.cpu().numpy().view(np.uint32) == stored).all()


@pytest.mark.parametrize("join", [False, True])
def test_second_call_and_smaller_batch_on_one_handle(cuda, join):
    """A second call on the output leaves the bytes as they are and patches
    nothing; then a smaller batch on the same handle, after the larger one,
    gives exactly its own reference: a count or a list left over from the
    larger call would show."""
    torch = cuda
    k, p, L = 10, 4, 2 * 2048 + 80
    stripes, stored = batch(k, p, L)
    code = HipReedSolomonCode(k, p, device=0)
    st = to_device(torch, stripes, False)
    sdev = stored_tensor(torch, stored)
    first = device.repair_checked_stripes(code, st, sdev, join_syndromes=join)
    check(torch, first, st, host_reference(k, p, stripes, stored, join, key=(k, p, L, S, LISTED, 0)), "first call")
    after = st.cpu().numpy()
    second = device.repair_checked_stripes(code, st, sdev, join_syndromes=join)
    check(torch, second, st, host_reference(k, p, after, stored, join), "second call")
    assert (st.cpu().numpy() == after).all() and not u32(second[2])[:, device.SCRUB_PATCHED].any()
    small, small_stored = batch(k, p, L, 5, (1, 3), seed=23)
    st2 = to_device(torch, small, False)
    third = device.repair_checked_stripes(code, st2, stored_tensor(torch, small_stored), join_syndromes=join)
    check(torch, third, st2, host_reference(k, p, small, small_stored, join), "smaller batch after a larger one")


def test_on_a_stream_of_its_own(cuda):
    """Inputs produced on a non-default stream just before the call, results
    read on that stream: right without any synchronisation by the caller."""
    torch = cuda
    k, p, L = 10, 4, 2 * 2048 + 80
    stripes, stored = batch(k, p, L)
    ref = host_reference(k, p, stripes, stored, False, key=(k, p, L, S, LISTED, 0))
    code = HipReedSolomonCode(k, p, device=0)
    src = torch.from_numpy(np.array(stripes)).to("cuda:0")
    ssrc = stored_tensor(torch, stored)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        st = torch.empty_like(src)
        sdev = torch.empty_like(ssrc)
        for _ in range(3):  # work in front of the call on its stream
            st.copy_(src.flip(0))
        st.copy_(src)
        sdev.copy_(ssrc)
        got = device.repair_checked_stripes(code, st, sdev)
        host = [t.to("cpu", non_blocking=False) for t in (*got, st)]  # ordered behind the call on this stream
    out, verdicts, erased, reports, crcs = ref
    assert (host[0].numpy().astype(np.int64) & 0xFFFFFFFF).tolist() == verdicts.tolist()
    assert host[1].numpy().tolist() == erased.tolist()
    assert ((host[2].numpy().astype(np.int64) & 0xFFFFFFFF) == reports).all()
    assert ((host[3].numpy().astype(np.int64) & 0xFFFFFFFF) == crcs).all()
    assert (host[4].numpy() == out).all()
    torch.cuda.synchronize()
