"""hrs_decode_batch_ragged_crc_dev on the GPU: the bytes of the ragged repair
(ragged_repair_inputs.expected: the oracle's decodeBulk over zero-filled
survivors, each output cut at its length, `out` a sentinel elsewhere) and the
CRC-32 of every rebuilt cell over EXACTLY its length,
zlib.crc32(want[s, t, :v], crc_in[s, t]), word for word: with crc_in None, a
seeded crc_in, and crc_out being crc_in. Every code kind, cell lengths of whole
2 KiB windows (the fused kernel where the shape has one) and of windows plus an
80-byte tail (two passes), through the C ABI and the Python mirror; kernel
names and modes 1 / 2 / 3; the all-full batch and the batch one entry short of
full; cells of more than 64 windows (the fold holds two windows per lane) on
both routes; table-slot reuse over back-to-back calls."""
import functools
import zlib

import numpy as np
import pytest

from lambdafs_amd import _lib, device
from ragged_repair_inputs import (BYTEWISE, CODES, SENTINEL, class_batch, code_id, expected, expected_kernel,
                                  fresh_stripes, full_batch, lost_of, make_code, mismatch)

pytestmark = pytest.mark.gpu

LENGTHS = [4096, 4096 + 80]
SRC = CODES[-1]
CASES = [(cfg, 4 if cfg == SRC else cfg[2]) for cfg in CODES] + [(SRC, SRC[2])]
FUSED = "batch_ragged_crc_kernel<%d, %d, 768>"


def case_id(case):
    return "%s_upto%d" % (code_id(case[0]), case[1])


def fused_kernel(cfg, erased):
    """The fused kernel's name for the batch, or None when its shape has none
    (more than 4 losses, more than 12 survivors read, more than 8 at 4 losses)."""
    name = expected_kernel(cfg, erased)
    if name == BYTEWISE:
        return None
    nout, ninb = (int(x) for x in name[name.index("<") + 1:-1].split(","))
    return FUSED % (nout, ninb) if ninb <= (8 if nout == 4 else 12) else None


def seeded(shape, seed=5):
    return np.random.default_rng(seed).integers(0, 2**32, shape, dtype=np.uint32)


def expected_crcs(want, erased, valid, crc_in=None):
    """crc[S, E]: zlib over the first valid bytes of each rebuilt cell, continued
    from crc_in; an entry past its stripe's losses keeps crc_in (0 without)."""
    S, E = erased.shape
    crc = np.zeros((S, E), np.uint32) if crc_in is None else np.array(crc_in, np.uint32)
    for s in range(S):
        for t, e in enumerate(lost_of(erased[s])):
            crc[s, t] = zlib.crc32(want[s, t, :int(valid[s, e])].tobytes(), int(crc[s, t]))
    return crc


@functools.lru_cache(maxsize=None)
def class_crcs(cfg, L, max_loss, with_in):
    _, erased, valid, want = class_batch(cfg, L, max_loss)
    out = expected_crcs(want, erased, valid, seeded(erased.shape) if with_in else None)
    out.setflags(write=False)
    return out


def crc_mismatch(got, want):
    bad = np.argwhere(got != want)
    if bad.size == 0:
        return None
    s, t = (int(x) for x in bad[0])
    return "%d CRCs differ; first: stripe %d output %d: got %#010x, want %#010x" % (len(bad), s, t, got[s, t],
                                                                                    want[s, t])


def as_i32(torch, a):
    return torch.from_numpy(np.array(a, np.uint32).view(np.int32)).to("cuda:0")


def _run(torch, code, stripes, erased, valid, via, crcs="none"):
    """(out bytes, crc words, kernel). crcs: "none" (fresh), "in" (a seeded crc_in), "alias" (crc_out is crc_in)."""
    t = torch.from_numpy(np.array(stripes)).to("cuda:0")
    S, E, L = t.shape[0], erased.shape[1], t.shape[2]
    out = torch.full((S, E, L), SENTINEL, dtype=torch.uint8, device="cuda:0")
    cin = None if crcs == "none" else as_i32(torch, seeded((S, E)))
    cout = cin if crcs == "alias" else torch.full((S, E), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    if via == "abi":
        e = np.ascontiguousarray(erased, dtype=np.int32)
        v = np.ascontiguousarray(np.array(valid), dtype=np.uint32)
        st = _lib.lib().hrs_decode_batch_ragged_crc_dev(
            code._handle(), t.data_ptr(), L, t.shape[1] * L, e.ctypes.data, E, out.data_ptr(), L, E * L, L, S,
            v.ctypes.data, None if cin is None else cin.data_ptr(), cout.data_ptr(),
            torch.cuda.current_stream().cuda_stream)
        v[...] = 0xFFFFFFFF  # the caller's array is free as soon as the call returns
        code._check(st)
    else:
        got = device.decode_batch_ragged_crc(code, t, np.array(erased), out, valid, crc_in=cin, crc_out=cout)
        assert got is cout
    kernel = code.lastKernel()
    torch.cuda.synchronize()
    assert (t.cpu().numpy() == stripes).all()  # survivors are never written
    return out.cpu().numpy(), cout.cpu().numpy().view(np.uint32), kernel


def check(got, want_bytes, want_crcs, erased, valid, what=None):
    d = mismatch(got[0], want_bytes, erased, valid)
    assert d is None, (what, d)
    d = crc_mismatch(got[1], want_crcs)
    assert d is None, (what, d)


@pytest.mark.parametrize("via,crcs", [("abi", "none"), ("abi", "alias"), ("mirror", "in")])
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_ragged_repair_crc_matches_the_oracle_and_zlib(cuda, case, L, via, crcs):
    cfg, max_loss = case
    stripes, erased, valid, want = class_batch(cfg, L, max_loss)
    got = _run(cuda, make_code(cfg), stripes, erased, valid, via, crcs)
    fused = fused_kernel(cfg, erased)
    ragged = expected_kernel(cfg, erased)
    assert (ragged == BYTEWISE) == (max_loss > 4)  # src beyond 4 losses is byte-granular
    if cfg[0] in ("rs", "nrs"):  # outside the fused set: 4 losses that read more than 8 survivors
        assert (fused is None) == (max_loss == 4 and cfg[1] > 8)
    assert got[2] == (fused if L % 2048 == 0 and fused else ragged)
    check(got, want, class_crcs(cfg, L, max_loss, crcs != "none"), erased, valid)


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_kernel_modes_give_equal_bytes_and_crcs(cuda, case, L):
    """Modes 1 and 2 never fuse (2 with the byte-granular repair), mode 3 fuses where mode 0 does."""
    cfg, max_loss = case
    stripes, erased, valid, want = class_batch(cfg, L, max_loss)
    ragged = expected_kernel(cfg, erased)
    fused = fused_kernel(cfg, erased) if L % 2048 == 0 else None
    for mode, wanted in ((1, ragged), (2, BYTEWISE), (3, fused or ragged)):
        got = _run(cuda, make_code(cfg, mode), stripes, erased, valid, "mirror", "in")
        assert got[2] == wanted, mode
        check(got, want, class_crcs(cfg, L, max_loss, True), erased, valid, mode)


@pytest.mark.parametrize("via", ["abi", "mirror"])
def test_fourteen_survivors_take_two_passes(cuda, via):
    """RS(14,2): 14 survivors per pattern, beyond the fused kernels' 12."""
    cfg = ("rs", 14, 2, 0)
    for L in LENGTHS:
        stripes, erased, valid, want = class_batch(cfg, L)
        got = _run(cuda, make_code(cfg), stripes, erased, valid, via, "in")
        assert got[2] == "batch_ragged_kernel<2, 16>" and fused_kernel(cfg, erased) is None
        check(got, want, class_crcs(cfg, L, None, True), erased, valid, L)


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("cfg", [CODES[0], CODES[2], CODES[6]], ids=code_id)
def test_all_full_batch_takes_the_plain_route(cuda, cfg, L):
    """Modes 0 and 1: hrs_decode_batch_crc_dev's route, kernel and CRCs (over len
    bytes, which then is each cell's length); modes 2 and 3 keep the ragged kernels."""
    torch = cuda
    stripes, erased, valid, want = full_batch(cfg, L)
    t = torch.from_numpy(np.array(stripes)).to("cuda:0")
    cin = as_i32(torch, seeded(erased.shape))
    plain_names, plain_crcs = {}, None
    for mode in (0, 1):
        plain = make_code(cfg, mode)
        out = torch.full(want.shape, SENTINEL, dtype=torch.uint8, device="cuda:0")
        crc = device.decode_batch_crc(plain, t, np.array(erased), out, crc_in=cin)
        plain_names[mode] = plain.lastKernel()
        torch.cuda.synchronize()
        plain_crcs = crc.cpu().numpy().view(np.uint32)
    want_crcs = expected_crcs(want, erased, valid, seeded(erased.shape))
    assert crc_mismatch(plain_crcs, want_crcs) is None  # the two references of this test agree
    ragged = expected_kernel(cfg, erased)
    fused = fused_kernel(cfg, erased) if L % 2048 == 0 else None
    for mode, name in ((0, plain_names[0]), (1, plain_names[1]), (2, BYTEWISE), (3, fused or ragged)):
        got = _run(torch, make_code(cfg, mode), stripes, erased, valid, "abi", "in")
        assert got[2] == name, mode
        check(got, want, want_crcs, erased, valid, mode)
    assert all(n and "ragged" not in n for n in plain_names.values())


def test_one_entry_short_of_full_takes_the_ragged_route(cuda):
    """The all-full route needs EVERY entry at len, the ignored ones too."""
    cfg = CODES[0]
    for L in LENGTHS:
        stripes, erased, valid, _ = full_batch(cfg, L)
        valid = np.array(valid)
        valid[-1, 0] = L - 1
        want = expected(cfg, stripes, erased, valid)
        got = _run(cuda, make_code(cfg), stripes, erased, valid, "mirror")
        ragged = expected_kernel(cfg, erased)  # up to 4 losses at 10 survivors: outside the fused set
        assert got[2] == ((fused_kernel(cfg, erased) if L % 2048 == 0 else None) or ragged) and "ragged" in got[2]
        check(got, want, expected_crcs(want, erased, valid), erased, valid, L)


def test_a_batch_that_lost_nothing_runs_only_the_fold(cuda):
    cfg, L = CODES[0], LENGTHS[0]
    stripes = fresh_stripes(cfg, 3, L, seed=4)
    erased = np.full((3, 2), -1, np.int32)
    valid = np.full((3, 14), L // 2, np.uint32)
    want = np.full((3, 2, L), SENTINEL, np.uint8)
    for crcs in ("none", "in", "alias"):
        got = _run(cuda, make_code(cfg), stripes, erased, valid, "abi", crcs)
        check(got, want, expected_crcs(want, erased, valid, None if crcs == "none" else seeded((3, 2))), erased, valid)


# the model's 63-66-window classes (tests/cpp/ragged_repair_crc_model.cpp) and the ends
LONG_CLASSES = [0, 1, 2047] + [n * 2048 + d for n in (63, 64, 65, 66) for d in (-1, 0, 1)]


@functools.lru_cache(maxsize=None)
def long_batch(cfg, L):
    """8 stripes that lost data cell 0, output and survivor lengths walking the long classes."""
    k, p = cfg[1], cfg[2]
    n, S = k + p, 8
    V = sorted({min(v, L) for v in LONG_CLASSES + [L - 1, L]})
    erased = np.full((S, 1), p, np.int32)
    valid = np.array([[V[(2 * s + 5 * l) % len(V)] for l in range(n)] for s in range(S)], np.uint32)
    valid[:, p] = [V[(3 * s + 7) % len(V)] for s in range(S)]  # the outputs
    valid[0, p], valid[1, p], valid[2, p] = 65 * 2048 + 1, 64 * 2048, 63 * 2048 - 1
    st = fresh_stripes(cfg, S, L, seed=3)
    want = expected(cfg, st, erased, valid)
    crcs = expected_crcs(want, erased, valid, seeded(erased.shape))
    for a in (st, erased, valid, want, crcs):
        a.setflags(write=False)
    return st, erased, valid, want, crcs


@pytest.mark.parametrize("L", [66 * 2048, 66 * 2048 + 80])
@pytest.mark.parametrize("cfg", [("rs", 3, 2, 0), ("rs", 10, 4, 0)], ids=code_id)
def test_cells_of_more_than_64_windows(cuda, cfg, L):
    """The fold with two 2 KiB windows per lane (fused) and the window pass with
    its tail window (two passes), on both routes at the whole-window length."""
    stripes, erased, valid, want, crcs = long_batch(cfg, L)
    fused = fused_kernel(cfg, erased)
    for mode in ((0, 1) if L % 2048 == 0 else (0,)):
        got = _run(cuda, make_code(cfg, mode), stripes, erased, valid, "abi", "in")
        assert got[2] == (fused if mode == 0 and L % 2048 == 0 else expected_kernel(cfg, erased))
        check(got, want, crcs, erased, valid, mode)


def test_repeated_calls_reuse_the_table_slots(cuda):
    """Five calls back to back on one handle and stream, each with its own
    valid array overwritten right after the call."""
    torch = cuda
    cfg, L = CODES[0], LENGTHS[0]
    stripes, erased, valid, want = class_batch(cfg, L)
    base = class_crcs(cfg, L, cfg[2], False)
    code = make_code(cfg)
    runs = []
    for i in range(5):
        t = torch.from_numpy(np.roll(np.array(stripes), i, axis=0)).to("cuda:0")
        out = torch.full(want.shape, SENTINEL, dtype=torch.uint8, device="cuda:0")
        crc = torch.zeros(erased.shape, dtype=torch.int32, device="cuda:0")
        e = np.ascontiguousarray(np.roll(np.array(erased), i, axis=0))
        v = np.ascontiguousarray(np.roll(np.array(valid), i, axis=0))
        st = _lib.lib().hrs_decode_batch_ragged_crc_dev(
            code._handle(), t.data_ptr(), L, t.shape[1] * L, e.ctypes.data, e.shape[1], out.data_ptr(), L,
            e.shape[1] * L, L, t.shape[0], v.ctypes.data, None, crc.data_ptr(), torch.cuda.current_stream().cuda_stream)
        v[...] = 0xFFFFFFFF
        code._check(st)
        runs.append((t, out, crc))
    torch.cuda.synchronize()
    for i, (_, out, crc) in enumerate(runs):
        got = (out.cpu().numpy(), crc.cpu().numpy().view(np.uint32))
        check(got, np.roll(want, i, axis=0), np.roll(base, i, axis=0), np.roll(erased, i, axis=0),
              np.roll(valid, i, axis=0), i)
