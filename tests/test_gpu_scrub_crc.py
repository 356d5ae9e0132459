"""GPU tests of scrub / heal + CRC-32 on the device (hrs_scrub_crc_dev,
hrs_heal_crc_dev). Reports and healed bytes are the oracle's, built exactly as
tests/test_gpu_scrub.py and the heal tests build them (their helpers are
imported); every expected CRC is zlib.crc32 over the expected bytes, continued
from the crc_in word: the cells as they were for the scrub, the cells after
the write-back for the heal."""
import random
import zlib

import numpy as np
import pytest

from lambdafs_amd import HipReedSolomonCode, _lib, device
from oracle import rs_oracle as C
from test_gpu_scrub import NONE, S, _stripes, _u32
from test_heal_host import heal_expected

pytestmark = pytest.mark.gpu

WINDOW = 2048
SHAPES = [(10, 4), (12, 4), (6, 3), (3, 2), (4, 1), (20, 8)]  # the last two pin the two-pass route
# name -> (L, row shift, stripe-stride pad)
LAYOUTS = {
    "one_window": (WINDOW, 0, 0),
    "three_windows": (3 * WINDOW, 0, 0),
    "tail": (3 * WINDOW + 100, 0, 0),
    "one_byte": (1, 0, 0),
    "below_a_window": (WINDOW - 1, 0, 0),
    "shift_1": (3 * WINDOW, 1, 0),
    "stride_pad_5": (3 * WINDOW, 0, 5),
}


def crcs_of(cells, start=None):
    """zlib CRC-32 of cells[S, n, L], continued from start[S, n] (uint32) if given."""
    s, n, _ = cells.shape
    return np.array([[zlib.crc32(cells[i, l].tobytes(), 0 if start is None else int(start[i, l])) for l in range(n)]
                     for i in range(s)], dtype=np.uint32)


_healed = {}


def _heal_inputs(k, p, L):
    """(stripes, scrub reports, healed stripes, heal reports), once per shape."""
    key = (k, p, L)
    if key not in _healed:
        host, want = _stripes(k, p, L)
        healed = np.empty_like(host)
        rep = np.empty((S, 4 + k + p), np.uint32)
        for s in range(S):
            healed[s], rep[s] = heal_expected(k, p, host[s])
        _healed[key] = (host, want, healed, rep)
    return _healed[key]


def fused(k, p, L, shift=0, pad=0, mode=0):
    return 2 <= p <= 4 and k + p <= 16 and L % WINDOW == 0 and shift == 0 and pad % 16 == 0 and mode in (0, 3)


def sibling_kernel(p, L, shift, pad, mode, heal):
    vector = mode != 2 and L >= WINDOW and shift == 0 and pad % 16 == 0
    return ("heal" if heal else "scrub") + ("_kernel" if vector else "_bytewise_kernel") + f"<{p}>"


def expected_kernel(k, p, L, shift, pad, mode, heal):
    if fused(k, p, L, shift, pad, mode):
        return ("heal" if heal else "scrub") + f"_crc_kernel<{p}>"
    return sibling_kernel(p, L, shift, pad, mode, heal)


def place(torch, host, shift, pad):
    """host[S, n, L] as a strided view of a flat random device buffer: row
    pitch a multiple of 16, a spare row per stripe, the stripe stride padded
    by `pad`, rows offset by `shift`. Returns (flat, view)."""
    s, n, L = host.shape
    pitch = ((L + shift + 15) // 16) * 16 + 16
    stride = (n + 1) * pitch + pad
    g = torch.Generator(device="cuda:0")
    g.manual_seed(L + shift + pad)
    flat = torch.randint(0, 256, (64 + s * stride,), dtype=torch.uint8, device="cuda:0", generator=g)
    assert flat.data_ptr() % 16 == 0
    view = torch.as_strided(flat, (s, n, L), (stride, pitch, 1), 32 + shift)
    view.copy_(torch.from_numpy(np.array(host)).to("cuda:0"))
    return flat, view


def call(torch, code, view, heal, crc_in=None, alias=False):
    """One raw entry-point call; crc_in: uint32 [S, n] or None; alias: crc_out
    is the crc_in array itself. Returns (reports, crcs) as uint32 arrays."""
    s, n, L = view.shape
    rep = torch.full((s, 4 + n), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    cin = None if crc_in is None else torch.from_numpy(crc_in.view(np.int32).copy()).to("cuda:0")
    out = cin if alias else torch.full((s, n), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    rows = _lib.ptr_array([view.data_ptr() + l * view.stride(1) for l in range(n)])
    fn = _lib.lib().hrs_heal_crc_dev if heal else _lib.lib().hrs_scrub_crc_dev
    code._check(fn(code._handle(), rows, view.stride(0), L, s, rep.data_ptr(), 4 + n,
                   None if cin is None else cin.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream))
    if cin is not None and not alias:
        assert (_u32(cin) == crc_in).all()  # crc_in is only read
    return _u32(rep), _u32(out)


def crc_modes(n, seed):
    """(crc_in, alias): random running CRCs, a fresh CRC32 (NULL), crc_out = crc_in."""
    start = np.random.default_rng(seed).integers(0, 1 << 32, (S, n), dtype=np.uint32)
    return [(start, False), (None, False), (start, True)]


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("k,p", SHAPES)
def test_scrub_crc_matches_oracle_and_zlib(cuda, k, p, layout):
    torch = cuda
    L, shift, pad = LAYOUTS[layout]
    n = k + p
    host, want = _stripes(k, p, L)
    code = HipReedSolomonCode(k, p, device=0)
    flat, view = place(torch, host, shift, pad)
    before = flat.clone()
    for mode in (0, 2):
        code.setKernelMode(mode)
        for crc_in, alias in crc_modes(n, L + n):
            rep, crc = call(torch, code, view, False, crc_in, alias)
            assert code.lastKernel() == expected_kernel(k, p, L, shift, pad, mode, False)
            assert rep.tolist() == want.tolist()
            assert crc.tolist() == crcs_of(host, crc_in).tolist()
            assert torch.equal(flat, before)  # a scrub writes nothing
    # the Python mirror, through the stripes tensor and through row views
    code.setKernelMode(0)
    if pad == 0:
        rep, crc = device.scrub_stripes_crc(code, view)
        assert _u32(rep).tolist() == want.tolist() and _u32(crc).tolist() == crcs_of(host).tolist()
        assert crc.dtype == torch.int32 and tuple(crc.shape) == (S, n)
    start = crc_modes(n, 5)[0][0]
    cin = torch.from_numpy(start.view(np.int32)).to("cuda:0")
    rep, crc = device.scrub_rows_crc(code, [view[:, l, :] for l in range(n)], crc_in=cin)
    assert _u32(rep).tolist() == want.tolist() and _u32(crc).tolist() == crcs_of(host, start).tolist()
    ref = device.crc32_rows(code, [view[:, l, :] for l in range(n)], crc_in=cin)
    assert torch.equal(ref, crc)  # hops order: exactly crc32_rows over the n rows


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("k,p", SHAPES)
def test_heal_crc_matches_oracle_and_zlib(cuda, k, p, layout):
    """Bytes and reports as the plain heal's expectation; CRCs of the post-heal
    bytes: stripe 2 has a replaced row (every window dirty) and a column the
    locator leaves as it was. A second heal_crc stores nothing and returns the
    same CRCs."""
    torch = cuda
    L, shift, pad = LAYOUTS[layout]
    n = k + p
    host, _, healed, want_rep = _heal_inputs(k, p, L)
    if p <= 4:
        assert want_rep[2, 1] >= 1  # an unresolved column, left as it was
    if p >= 2 and L > 1:
        assert (healed[2] != host[2]).any()
    code = HipReedSolomonCode(k, p, device=0)
    for mode in (0, 2):
        code.setKernelMode(mode)
        for crc_in, alias in crc_modes(n, L + n + 1):
            flat, view = place(torch, host, shift, pad)
            before = flat.clone()
            rep, crc = call(torch, code, view, True, crc_in, alias)
            assert code.lastKernel() == expected_kernel(k, p, L, shift, pad, mode, True)
            got = view.cpu().numpy()
            assert (got == healed).all()
            assert rep.tolist() == want_rep.tolist()
            assert crc.tolist() == crcs_of(healed, crc_in).tolist()
            view.copy_(torch.from_numpy(np.array(host)).to("cuda:0"))
            assert torch.equal(flat, before)  # nothing outside the cells was written
            if alias:
                continue
            view.copy_(torch.from_numpy(healed).to("cuda:0"))
            rep2, crc2 = call(torch, code, view, True, crc_in, False)
            assert (view.cpu().numpy() == healed).all()
            assert not rep2[:, 3].any() and not rep2[:, 4:].any()
            assert rep2[:, 0].tolist() == rep2[:, 1].tolist() == rep[:, 1].tolist()
            assert crc2.tolist() == crc.tolist()
    code.setKernelMode(0)
    if pad == 0:
        _, view = place(torch, host, shift, pad)
        rep, crc = device.heal_stripes_crc(code, view)
        assert _u32(rep).tolist() == want_rep.tolist() and _u32(crc).tolist() == crcs_of(healed).tolist()
    _, view = place(torch, host, shift, pad)
    rep, crc = device.heal_rows_crc(code, [view[:, l, :] for l in range(n)])
    assert _u32(rep).tolist() == want_rep.tolist() and _u32(crc).tolist() == crcs_of(healed).tolist()
    assert (view.cpu().numpy() == healed).all()


def test_kernel_mode_3_and_block_width(cuda, monkeypatch):
    """Kernel mode 3 takes the fused kernel like mode 0; the 512-thread form
    (8 rows in flight) gives the same words as the 1,024-thread one."""
    torch = cuda
    k, p, L = 10, 4, 3 * WINDOW
    host, want, healed, want_rep = _heal_inputs(k, p, L)
    code = HipReedSolomonCode(k, p, device=0)
    code.setKernelMode(3)
    for threads in ("1024", "512"):
        monkeypatch.setenv("HRS_SCRUB_CRC_THREADS", threads)
        _, view = place(torch, host, 0, 0)
        rep, crc = call(torch, code, view, False)
        assert code.lastKernel() == "scrub_crc_kernel<4>"
        assert rep.tolist() == want.tolist() and crc.tolist() == crcs_of(host).tolist()
        rep, crc = call(torch, code, view, True)
        assert code.lastKernel() == "heal_crc_kernel<4>"
        assert rep.tolist() == want_rep.tolist() and crc.tolist() == crcs_of(healed).tolist()
        assert (view.cpu().numpy() == healed).all()


# ------------------------------------------------------------ wave hand-over

WAVE_K, WAVE_P, WAVE_S, WAVE_NWIN = 10, 4, 40, 30
_waves = {}


def _wave_inputs():
    """RS(10,4), 40 stripes x 30 windows of codeword columns by construction,
    then planted columns (1, 2 and 3 errors) as tests/test_gpu_scrub_waves.py
    plants them: a quarter of the stripes clean (the first and the last among
    them), the others dirty in a random half of their windows, so that the
    waves of the launch meet runs of dirty windows, stripe changes between two
    of them and dirty - clean - dirty gaps (asserted in the test). Expected
    bytes and reports come from the oracle column by column."""
    if _waves:
        return _waves
    from test_gpu_scrub_waves import _column_report, _plant
    k, p, ns, nwin = WAVE_K, WAVE_P, WAVE_S, WAVE_NWIN
    n, L = k + p, nwin * WINDOW
    rng = np.random.default_rng([11, k, p, ns, L])
    rnd = random.Random(424243)
    host = np.empty((ns, n, L), dtype=np.uint8)
    host[:, p:] = rng.integers(0, 256, (ns, k, L), dtype=np.uint8)
    for s in range(ns):
        host[s, :p] = np.stack(C.encode_bulk(k, p, [host[s, p + c] for c in range(k)]))
    healed = host.copy()
    rep = np.zeros((ns, 4 + n), dtype=np.uint32)
    rep[:, 2] = NONE
    inner = list(range(1, ns - 1))
    rnd.shuffle(inner)
    clean = {0, ns - 1} | set(inner[:ns // 4 - 2])
    dirty = [set() for _ in range(ns)]
    for s in range(ns):
        if s in clean:
            continue
        dirty[s] = set(rnd.sample(range(nwin), nwin // 2))
        for w in sorted(dirty[s]):
            inside = set(rnd.sample(range(WINDOW), rnd.randint(1, 3))) | ({0} if w % 7 == 0 else {WINDOW - 1})
            for c in sorted(w * WINDOW + x for x in inside):
                column = _plant(k, p, host[s, :, c].tolist(), rnd, rnd.choice([1, 2, 3]))
                host[s, :, c] = column
                ok, _, after = _column_report(k, p, rep[s], c, list(column))
                healed[s, :, c] = after if ok else column
        rep[s, 3] = np.count_nonzero(healed[s] != host[s])
    assert rep[:, 1].any() and rep[:, 3].any()
    _waves.update(host=host, healed=healed, rep=rep, dirty=dirty, crc=crcs_of(host), healed_crc=crcs_of(healed))
    return _waves


def _wave_runs(ntasks, order, grid, wpb):
    """wave_tasks (hrs_device.hpp) restated: the tasks of every wave, in order."""
    waves = []
    for b in range(grid):
        for w in range(wpb):
            if order >= 1:
                t0, end, jump, chunk = b * order * wpb + w, ntasks, grid * order * wpb, order
            else:
                per = -(-ntasks // grid)
                t0, end, jump, chunk = per * b + w, min(per * b + per, ntasks), 0, 0xFFFFFFFF
            tasks, j = [], 0
            while True:
                q = j // chunk
                t = t0 + q * jump + (j - q * chunk) * wpb
                if t >= end:
                    break
                tasks.append(t)
                j += 1
            waves.append(tasks)
    return waves


@pytest.mark.parametrize("order", [1, 0, 2, 32])
def test_wave_handover(cuda, monkeypatch, order):
    """Every one of the 560 cell CRCs against zlib, for scrub_crc and heal_crc,
    under each window order: one window's raw words or dirty mark leaking into
    the wave's next task would show here. Under order 32 a wave runs up to 32
    windows; the run, hand-over and gap it meets are asserted of the schedule."""
    torch = cuda
    w = _wave_inputs()
    k, p, ns, nwin = WAVE_K, WAVE_P, WAVE_S, WAVE_NWIN
    host, healed = w["host"], w["healed"]
    ntasks, wpb = ns * nwin, 16
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    runs = _wave_runs(ntasks, order, min(-(-ntasks // wpb), cus), wpb)
    assert sorted(t for r in runs for t in r) == list(range(ntasks))  # every window once
    if order == 32:
        shown = set()
        for r in runs:
            seq = [(t % nwin in w["dirty"][t // nwin], t // nwin) for t in r]
            for i in range(len(seq) - 1):
                if seq[i][0] and seq[i + 1][0] and seq[i][1] != seq[i + 1][1]:
                    shown.add("handover")
                if i + 2 < len(seq) and seq[i][0] and not seq[i + 1][0] and seq[i + 2][0]:
                    shown.add("gap")
            if sum(d for d, _ in seq) >= 3 and len({s for d, s in seq if d}) >= 2:
                shown.add("run")
        assert shown == {"run", "handover", "gap"}
    monkeypatch.setenv("HRS_TASK_ORDER", str(order))
    code = HipReedSolomonCode(k, p, device=0)
    st = torch.from_numpy(host).to("cuda:0")
    rep, crc = device.scrub_stripes_crc(code, st)
    assert code.lastKernel() == "scrub_crc_kernel<4>"
    got = _u32(rep)
    others = [x for x in range(4 + k + p) if x != 3]
    assert got[:, others].tolist() == w["rep"][:, others].tolist() and not got[:, 3].any()
    assert (_u32(crc) == w["crc"]).all()
    assert (st.cpu().numpy() == host).all()
    rep, crc = device.heal_stripes_crc(code, st)
    assert code.lastKernel() == "heal_crc_kernel<4>"
    assert _u32(rep).tolist() == w["rep"].tolist()
    assert (st.cpu().numpy() == healed).all()
    bad = np.argwhere(_u32(crc) != w["healed_crc"])
    assert bad.size == 0, f"stale or foreign raw words in (stripe, location) {bad[:8].tolist()}"


# ------------------------------------------------------------- end to end

def test_scrub_crc_to_erasures_to_repair(cuda):
    """RS(10,4), L = 2 x 2 KiB, S = 4. The stored checksums come from
    encode_batch_host_crc, permuted to hops order. Stripe 0: a column with 3
    wrong cells, which the syndromes cannot resolve at p = 4 (checked here
    with the oracle) but the checksums name; stripe 1: one flipped bit; stripe
    2: a stale parity cell, rewritten together with its stored checksum, which
    only the report names; stripe 3 clean. scrub_stripes_crc ->
    checksums_to_erased -> decode_batch_crc gives the cells and their stored
    checksums back."""
    torch = cuda
    k, p, L, ns = 10, 4, 2 * WINDOW, 4
    n = k + p
    code = HipReedSolomonCode(k, p, device=0)
    rng = np.random.default_rng(20261)
    orig = rng.integers(0, 256, (ns, n, L), dtype=np.uint8)
    enc = device.encode_batch_host_crc(code, orig)  # parity in place; [S, n] data first
    stored = np.concatenate([enc[:, k:], enc[:, :k]], axis=1)  # hops order: parity first
    assert stored.tolist() == crcs_of(orig).tolist()
    bad = orig.copy()
    # stripe 0: three wrong cells in one column, searched (seeded) until the oracle calls it unresolved
    rnd = random.Random(77)
    for _ in range(400):
        c = rnd.randrange(L)
        locs = sorted(rnd.sample(range(n), 3))
        trial = orig[0, :, c].copy()
        for l in locs:
            trial[l] ^= rnd.randrange(1, 256)
        ok, _, _ = C.compute_error_locations(k, p, trial.tolist())
        if not ok:
            bad[0, :, c] = trial
            break
    else:
        raise AssertionError("no unresolved 3-error column found")
    bad[1, 7, 1234] ^= 0x10
    bad[2, 1] = rng.integers(0, 256, L, dtype=np.uint8)  # stale parity cell ...
    stored[2, 1] = zlib.crc32(bad[2, 1].tobytes())       # ... whose checksum was updated with it
    st = torch.from_numpy(bad).to("cuda:0")
    rep, crc = device.scrub_stripes_crc(code, st)
    assert code.lastKernel() == "scrub_crc_kernel<4>"
    r = _u32(rep)
    assert r[0, :2].tolist() == [1, 1] and not r[0, 4:].any()  # unresolved by the syndromes
    assert (_u32(crc)[2] == stored[2]).all() and r[2, 4 + 1] > 0  # the checksums agree, the report names parity 1
    with pytest.raises(ValueError, match="unresolved"):
        device.scrub_to_erased(rep, p)
    erased = device.checksums_to_erased(crc, stored, p, reports=rep)
    assert erased[0].tolist() == locs + [-1] and erased[1].tolist() == [7, -1, -1, -1]
    assert erased[2].tolist() == [1, -1, -1, -1] and erased[3].tolist() == [-1] * p
    out = torch.zeros((ns, p, L), dtype=torch.uint8, device="cuda:0")
    out_crc = _u32(device.decode_batch_crc(code, st, erased, out))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for s in range(ns):
        for t, l in enumerate(x for x in erased[s] if x >= 0):
            assert (got[s, t] == orig[s, l]).all(), (s, l)
            if s < 2:
                assert out_crc[s, t] == stored[s, l], (s, l)
    assert out_crc[2, 0] == zlib.crc32(orig[2, 1].tobytes())  # the true parity, not the stale cell's checksum
