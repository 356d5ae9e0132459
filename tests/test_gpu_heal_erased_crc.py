"""hrs_heal_erased_crc_dev on the GPU (heal_erased_crc_kernel<P>,
hrs_heal_erased_crc.hip, and the two-pass route): the inputs of
tests/heal_erased_inputs.py as they stand, seven stripes with seven erasure
patterns and survivor errors planted at window, piece and row edges. Expected
bytes are the oracle-encoded stripes and the reports the counts of the planted
list (parity_size above 4: hrs_heal_erased_host, byte for byte); every expected CRC
is zlib.crc32 over the expected bytes, continued from the crc_in word. L = 4096
is the fused shape (kernel mode 3 pins the fused kernel, mode 2 the byte-granular
one, mode 0 takes what was measured faster), L = 4096 + 100 adds a row tail and
so takes two passes."""
import random

import numpy as np
import pytest

import heal_erased_inputs as H
from lambdafs_amd import HipReedSolomonCode, _lib, device
from test_gpu_heal_erased import _aligned, _u32
from test_gpu_scrub_crc import crcs_of

pytestmark = pytest.mark.gpu

SHAPES = [(10, 4), (12, 4), (6, 3), (3, 2), (4, 1), (20, 8), (247, 8), (6, 5), (7, 6), (10, 7)]
LENGTHS = [2 * H.WINDOW, 2 * H.WINDOW + 100]
NONE_DEV = -2  # HRS_DEVICE_NONE
S = 7
_cases = {}


def _case(k, p, L, over=0, seed=1, columns=None):
    """(clean, damaged, patterns, planted, bytes after, reports): the last two
    are the clean stripes and the planted counts at p <= 4 within capacity
    (tests/cpp/heal_erased_logic asserts full resolution there) and
    hrs_heal_erased_host's otherwise."""
    key = (k, p, L, over, seed, None if columns is None else tuple(columns))
    if key not in _cases:
        rnd = random.Random(1009 * k + p + seed)
        pats = H.seven_patterns(k, p, rnd)
        clean = H.clean_stripes(k, p, S, L, seed)
        bad, planted = H.plant(k, p, clean, pats, H.columns_of(L) if columns is None else columns, over=over, seed=seed)
        if p <= 4 and not over:
            after, reps = clean, H.planted_reports(k + p, S, planted)
        else:
            after, reps = H.host_reference(HipReedSolomonCode(k, p, device=NONE_DEV), bad, pats)
        _cases[key] = (clean, bad, pats, planted, after, reps)
    return _cases[key]


def fused_shape(k, p, L):
    return 2 <= p <= 4 and k + p <= 16 and L % H.WINDOW == 0


def expected_kernels(k, p, L, mode):
    """The names hrs_last_kernel may report: one, except in mode 0 on a fused
    shape, where the measured routing decides between the two."""
    if mode == 2:
        return {f"heal_erased_bytewise_kernel<{p}>"}
    sibling = f"heal_erased_kernel<{p}>"
    if not fused_shape(k, p, L):
        return {sibling}
    return {f"heal_erased_crc_kernel<{p}>"} if mode == 3 else {sibling, f"heal_erased_crc_kernel<{p}>"}


def call(torch, code, view, pats, crc_in=None, alias=False, max_erased=None):
    """One raw entry-point call; crc_in: uint32 [S, n] or None; alias: crc_out
    is the crc_in array itself. Returns (reports, crcs) as uint32 arrays."""
    s, n, L = view.shape
    rep = torch.full((s, 4 + n), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    cin = None if crc_in is None else torch.from_numpy(crc_in.view(np.int32).copy()).to("cuda:0")
    out = cin if alias else torch.full((s, n), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    rows = _lib.ptr_array([view.data_ptr() + l * view.stride(1) for l in range(n)])
    arr = H.erased_array(pats)
    me = arr.shape[1] if max_erased is None else max_erased
    code._check(_lib.lib().hrs_heal_erased_crc_dev(code._handle(), rows, view.stride(0), L, s,
                                                   arr.ctypes.data if me else None, me, rep.data_ptr(), 4 + n,
                                                   None if cin is None else cin.data_ptr(), out.data_ptr(),
                                                   torch.cuda.current_stream().cuda_stream))
    if cin is not None and not alias:
        assert (_u32(cin) == crc_in).all()  # crc_in is only read
    return _u32(rep), _u32(out)


def crc_modes(s, n, seed):
    """(crc_in, alias): random running CRCs, a fresh CRC32 (NULL), crc_out = crc_in."""
    start = np.random.default_rng(seed).integers(0, 1 << 32, (s, n), dtype=np.uint32)
    return [(start, False), (None, False), (start, True)]


@pytest.mark.parametrize("mode", [3, 2, 0])
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("k,p", SHAPES)
def test_heal_erased_crc_matches_oracle_and_zlib(cuda, k, p, L, mode):
    torch = cuda
    n = k + p
    clean, bad, pats, planted, after, reps = _case(k, p, L)
    code = HipReedSolomonCode(k, p, device=0)
    code.setKernelMode(mode)
    for crc_in, alias in crc_modes(S, n, L + n):
        st = _aligned(torch, bad)
        rep, crc = call(torch, code, st, pats, crc_in, alias)
        assert code.lastKernel() in expected_kernels(k, p, L, mode), code.lastKernel()
        got = st.cpu().numpy()
        assert (got == after).all(), np.argwhere(got != after)[:4].tolist()
        assert rep.tolist() == reps.tolist()
        assert crc.tolist() == crcs_of(after, crc_in).tolist()
    # a second call stores nothing and returns the same CRCs
    rep2, crc2 = call(torch, code, st, pats, crc_in, False)
    assert not rep2[:, 3].any() and (st.cpu().numpy() == got).all()
    assert crc2.tolist() == crc.tolist()
    if p <= 4:
        assert rep2.tolist() == H.planted_reports(n, S, []).tolist()


# name -> (columns, over): what the fused kernel takes from registers and what from memory
VARIANTS = {
    "edges": (None, 0),            # every window of a stripe with errors is dirty; stripes 5 (e = p) and 6 are clean
    "one_patched_byte": ([100], 0),  # window 0 with one patched column, window 1 clean, in every stripe with capacity
    "clean_survivors": ([], 0),    # every window clean: the erased rows' words all come from registers
    "unresolved": (None, 1),       # one error past capacity: columns left as they are
}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("k,p,threads", [(10, 4, 512), (6, 3, 1024), (6, 3, 512)])
def test_fused_crcs_are_those_of_the_tensor_read_back(cuda, monkeypatch, k, p, threads, variant):
    """Kernel mode 3 at L = 4096: CRCs against zlib over the tensor AS READ
    BACK, so a stale raw word cannot hide behind an expectation. Covers a clean
    window of a stripe with erasures, a window with one patched survivor,
    columns left unresolved, the e = p stripe (stripe 5) and the stripe with no
    erasure (stripe 0) inside a batch with max_erased > 0. Both block widths
    where both are built (P = 4 has the 512-thread form only)."""
    torch = cuda
    monkeypatch.setenv("HRS_HEAL_ERASED_CRC_THREADS", str(threads))
    n, L = k + p, 2 * H.WINDOW
    columns, over = VARIANTS[variant]
    clean, bad, pats, planted, after, reps = _case(k, p, L, over=over, seed=4 if over else 1, columns=columns)
    assert pats[0] == [] and len(pats[5]) == p and len(pats[6]) == 1
    code = HipReedSolomonCode(k, p, device=0)
    code.setKernelMode(3)
    start = np.random.default_rng(n).integers(0, 1 << 32, (S, n), dtype=np.uint32)
    st = _aligned(torch, bad)
    rep, crc = call(torch, code, st, pats, start)
    assert code.lastKernel() == f"heal_erased_crc_kernel<{p}>"
    got = st.cpu().numpy()
    assert crc.tolist() == crcs_of(got, start).tolist()
    assert (got == after).all(), np.argwhere(got != after)[:4].tolist()
    assert rep.tolist() == reps.tolist()
    if over:
        assert reps[:, 1].sum() > 0 and (after != clean).any()
    if variant == "one_patched_byte":
        assert reps[:, 3].sum() > 0 and reps[:, 0].max() == 1


def test_nothing_erased_is_heal_crc(cuda):
    """max_erased == 0 is hrs_heal_crc_dev: bytes, reports and CRC words."""
    torch = cuda
    k, p, L = 10, 4, 2 * H.WINDOW
    n = k + p
    clean = H.clean_stripes(k, p, S, L, 1)
    none = [[] for _ in range(S)]
    bad, _ = H.plant(k, p, clean, none, H.columns_of(L), clean_stripes_=(), seed=2)
    more, _ = H.plant(k, p, clean, none, [5, 1030, L - 2], over=1, clean_stripes_=(), seed=3)
    bad[:, :, [5, 1030, L - 2]] = more[:, :, [5, 1030, L - 2]]
    code = HipReedSolomonCode(k, p, device=0)
    start = np.random.default_rng(3).integers(0, 1 << 32, (S, n), dtype=np.uint32)
    cin = torch.from_numpy(start.view(np.int32).copy()).to("cuda:0")
    ref = _aligned(torch, bad)
    want_rep, want_crc = device.heal_stripes_crc(code, ref, cin)
    kernel = code.lastKernel()
    st = _aligned(torch, bad)
    rep, crc = call(torch, code, st, none, start, max_erased=0)
    assert code.lastKernel() == kernel == "heal_crc_kernel<4>"
    assert torch.equal(st, ref) and rep.tolist() == _u32(want_rep).tolist() and crc.tolist() == _u32(want_crc).tolist()
    assert rep[:, 1].all() and rep[:, 3].all()


@pytest.mark.parametrize("mode", [3, 2])
@pytest.mark.parametrize("L", LENGTHS)
def test_equals_heal_erased_then_crc32(cuda, L, mode):
    """The new call against hrs_heal_erased_dev followed by hrs_crc32_dev over
    the n rows, one column past capacity included; the Python mirrors."""
    torch = cuda
    k, p = 12, 4
    n = k + p
    clean, bad, pats, planted, after, reps = _case(k, p, L, over=1, seed=4)
    code = HipReedSolomonCode(k, p, device=0)
    code.setKernelMode(mode)
    start = np.random.default_rng(5).integers(0, 1 << 32, (S, n), dtype=np.uint32)
    cin = torch.from_numpy(start.view(np.int32).copy()).to("cuda:0")
    ref = _aligned(torch, bad)
    want_rep = device.heal_erased_stripes(code, ref, pats)
    want_crc = device.crc32_rows(code, [ref[:, l] for l in range(n)], cin)
    st = _aligned(torch, bad)
    rep, crc = device.heal_erased_stripes_crc(code, st, pats, cin)
    assert torch.equal(st, ref) and torch.equal(rep, want_rep) and torch.equal(crc, want_crc)
    st2 = _aligned(torch, bad)
    rep2, crc2 = device.heal_erased_rows_crc(code, [st2[:, l] for l in range(n)], H.erased_array(pats), cin)
    assert torch.equal(st2, ref) and torch.equal(rep2, want_rep) and torch.equal(crc2, want_crc)
    assert (st.cpu().numpy() == after).all() and _u32(rep).tolist() == reps.tolist()


# ---- many windows per wave (after test_gpu_heal_erased.py)

def _waves_case():
    k, p, s, Lw = 10, 4, 40, 3 * H.WINDOW
    rnd = random.Random(77)
    clean = H.clean_stripes(k, p, s, Lw, 9)
    base = H.seven_patterns(k, p, rnd)
    pats = [base[rnd.randrange(6)] if i % 4 else sorted(rnd.sample(range(k + p), rnd.randrange(0, 3))) for i in range(s)]
    cols = sorted({w * H.WINDOW + c for w in range(3) for c in (0, 517, 2047)})
    quiet = tuple(i for i in range(s) if i % 5 == 3)  # clean survivors
    bad, planted = H.plant(k, p, clean, pats, cols, clean_stripes_=quiet, seed=11)
    return k, p, clean, bad, pats, planted


@pytest.mark.parametrize("order", [1, 32])
def test_many_windows_per_wave(cuda, monkeypatch, order):
    """RS(10,4), 40 stripes of 3 windows with mixed patterns, most of them
    dirty in every window: under HRS_TASK_ORDER 32 one block runs all 120
    windows stripe after stripe, 15 per wave of its 8 (heal_erased_kernel's
    4-wave block ran 30). All 40 * n CRCs against zlib."""
    torch = cuda
    monkeypatch.setenv("HRS_TASK_ORDER", str(order))
    k, p, clean, bad, pats, planted = _waves_case()
    n = k + p
    assert len({(s, c // H.WINDOW) for s, c, _ in planted}) >= 40 and len({tuple(e) for e in pats}) >= 6
    code = HipReedSolomonCode(k, p, device=0)
    code.setKernelMode(3)
    start = np.random.default_rng(order).integers(0, 1 << 32, (40, n), dtype=np.uint32)
    st = _aligned(torch, bad)
    rep, crc = call(torch, code, st, pats, start)
    assert code.lastKernel() == "heal_erased_crc_kernel<4>"
    got = st.cpu().numpy()
    assert (got == clean).all(), np.argwhere(got != clean)[:4].tolist()
    assert rep.tolist() == H.planted_reports(n, 40, planted).tolist()
    assert crc.tolist() == crcs_of(clean, start).tolist()
