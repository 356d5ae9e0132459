"""Footprint tests of the device entry points (hrs_encode_dev, hrs_decode_dev,
hrs_apply_dev, hrs_decode_batch_dev, hrs_encode_crc_dev, hrs_decode_crc_dev,
hrs_crc32_dev): every byte a call could touch lives in a guarded arena
(gpu_arena.py), and each case asserts two things:

- the whole arena after the call equals the pre-call arena with exactly the
  output rows replaced by a host reference computed from the PRE-call bytes
  (the oracle's encodeBulk / decodeBulk, GF(2^8) products from the oracle's
  multiply, zlib.crc32): outputs right, guards intact, inputs untouched,
  output rows the call must not write still poisoned;
- hrs_last_kernel names the kernel the case is meant to exercise. The names
  in the tables are literals read off the dispatch source (run_apply in
  hrs_dispatch.cpp, the CRC routes in hrs_crc_api.cpp, launch_batch in
  hrs_batch_api.cpp, the launch_* functions of the .hip files), not computed
  by a second planner.

Placements: "aligned" and "gap16" (16 spare bytes per stripe) keep rows and
strides on 16-byte boundaries, so the vector kernels run; "shift" (rows start
at an odd address) and "pad5" (stripe stride not a multiple of 16) must end in
the byte-granular kernel.
"""
import zlib
from collections import namedtuple

import numpy as np
import pytest

from gpu_arena import POISON, Arena, CrcArena
from lambdafs_amd import HipNativeReedSolomonCode, HipReedSolomonCode, HipXORCode, _lib, device
from oracle import rs_oracle as C

PLACEMENTS = {"aligned": (0, 0), "gap16": (0, 16), "shift": (1, 0), "pad5": (0, 5)}
UNALIGNED = ("shift", "pad5")

BIG = 32768 + 2048 + 5
LENGTHS = (1, 15, 16, 17, 2047, 2048, 2049, 4096 + 17, BIG, 32768, 65536)  # the last two: fused kernels, CRC

BYTEWISE = "bytewise_kernel"
BATCH_BYTEWISE = "batch_bytewise_kernel"

# family: the kernel family the case belongs to (what its aligned placement
# runs); kernel: what hrs_last_kernel must say ("x*": starts with x).
Case = namedtuple("Case", "entry family cfg L place kernel")


def _cases(entry, family, cfg, rows):
    return [Case(entry, family, cfg, L, place, kernel) for L, place, kernel in rows]


# hrs_encode_dev. cfg = (code, k, p, kernel mode)
ENCODE = (
    _cases("encode", "encode_static_kernel", ("rs", 10, 4, 0), [
        (2048, "aligned", "encode_static_kernel<10, 4>"),
        (2049, "gap16", "encode_static_kernel<10, 4>"),
        (4096 + 17, "aligned", "encode_static_kernel<10, 4>"),
        (BIG, "aligned", "encode_static_kernel<10, 4>"),
        (17, "aligned", BYTEWISE),
        (2049, "shift", BYTEWISE),
        (4096 + 17, "pad5", BYTEWISE),
    ])
    + _cases("encode", "encode_cauchy_kernel", ("nrs", 10, 4, 0), [
        (2048, "aligned", "encode_cauchy_kernel<10, 4>"),
        (4096 + 17, "aligned", "encode_cauchy_kernel<10, 4>"),
        (15, "aligned", BYTEWISE),
        (2049, "shift", BYTEWISE),
        (2049, "pad5", BYTEWISE),
    ])
    + _cases("encode", "bitsliced_kernel", ("rs", 10, 4, 1), [
        (2048, "aligned", "bitsliced_kernel<4, 12>"),
        (2049, "aligned", "bitsliced_kernel<4, 12>"),
        (16, "aligned", BYTEWISE),
        (2049, "shift", BYTEWISE),
        (4096 + 17, "pad5", BYTEWISE),
    ])
    + _cases("encode", "bitsliced_pipe_kernel", ("rs", 5, 2, 0), [
        (2048, "aligned", "bitsliced_pipe_kernel<2, 8>"),
        (4096 + 17, "gap16", "bitsliced_pipe_kernel<2, 8>"),
        (1, "aligned", BYTEWISE),
        (2049, "shift", BYTEWISE),
        (2049, "pad5", BYTEWISE),
    ])
    + _cases("encode", "bitsliced_stream_kernel", ("rs", 20, 7, 0), [
        (2048, "aligned", "bitsliced_stream_kernel<7, 4>"),
        (2049, "aligned", "bitsliced_stream_kernel<7, 4>"),
        (2047, "aligned", BYTEWISE),
        (4096 + 17, "shift", BYTEWISE),
        (2049, "pad5", BYTEWISE),
    ])
    # 9 outputs = chunks of 8 + 1, 40 inputs = chunks of 32 + 8 (accumulating): the last launch has one output
    + _cases("encode", "bitsliced_stream_kernel", ("rs", 40, 9, 0), [
        (2049, "aligned", "bitsliced_stream_kernel<1, 4>"),
        (BIG, "aligned", "bitsliced_stream_kernel<1, 4>"),
        (2049, "shift", BYTEWISE),
    ])
    # 20 inputs: xor_kernel<16>, then xor_kernel<4> accumulating, each with its byte-granular tail
    + _cases("encode", "xor_kernel", ("xor", 20, 1, 0), [
        (2048, "aligned", "xor_kernel<4>"),
        (2049, "aligned", "xor_kernel<4>"),
        (4096 + 17, "gap16", "xor_kernel<4>"),
        (17, "aligned", BYTEWISE),
        (2049, "shift", BYTEWISE),
        (2049, "pad5", BYTEWISE),
    ])
    + _cases("encode", "bytewise_kernel", ("rs", 10, 4, 2), [
        (1, "aligned", BYTEWISE),
        (2049, "aligned", BYTEWISE),
        (4096 + 17, "gap16", BYTEWISE),
    ])
)

# hrs_decode_dev, RS(10,4). cfg = erased locations
DECODE = (
    _cases("decode", "bitsliced_pipe_kernel", (5,), [
        (2048, "aligned", "bitsliced_pipe_kernel<1, 12>"),
        (2049, "aligned", "bitsliced_pipe_kernel<1, 12>"),
        (4096 + 17, "gap16", "bitsliced_pipe_kernel<1, 12>"),
        (17, "aligned", BYTEWISE),
        (2049, "shift", BYTEWISE),
        (2049, "pad5", BYTEWISE),
    ])
    + _cases("decode", "bitsliced_kernel", (0, 5, 9, 13), [
        (2048, "aligned", "bitsliced_kernel<4, 12>"),
        (4096 + 17, "gap16", "bitsliced_kernel<4, 12>"),
        (15, "aligned", BYTEWISE),
        (2049, "shift", BYTEWISE),
        (4096 + 17, "pad5", BYTEWISE),
    ])
)

# hrs_apply_dev. cfg = matrix kind (see _apply_matrix)
APPLY = (
    # 2 x 5, column 2 all zero and its input pointer NULL: 4 live inputs
    _cases("apply", "bitsliced_pipe_kernel", "zero_column", [
        (2049, "aligned", "bitsliced_pipe_kernel<2, 4>"),
        (2049, "shift", BYTEWISE),
    ])
    # 2 x 3 of zeros: hipMemset, no kernel
    + _cases("apply", None, "all_zero", [
        (2049, "aligned", ""),
        (17, "shift", ""),
    ])
    # one row of 17 ones: xor_kernel<16>, then xor_kernel<4> accumulating, with tails
    + _cases("apply", "xor_kernel", "ones_1x17", [
        (2049, "aligned", "xor_kernel<4>"),
        (2049, "pad5", BYTEWISE),
    ])
    # 6 outputs, 9 inputs: more than the 8 the resident kernels take with wide outputs
    + _cases("apply", "bitsliced_stream_kernel", "random_6x9", [
        (2048, "aligned", "bitsliced_stream_kernel<6, 4>"),
        (4096 + 17, "aligned", "bitsliced_stream_kernel<6, 4>"),
        (2049, "shift", BYTEWISE),
        (2049, "pad5", BYTEWISE),
    ])
)

# hrs_decode_batch_dev. cfg = (k, p, kernel mode, per-stripe erasure lists)
BATCH_10_4 = ((5,), (0, 13), ())
BATCH_20_7 = ((0, 3, 8, 12, 19, 22, 26), (1, 2, 6, 7, 20, 25, 26), (4, 21))
BATCH = (
    _cases("decode_batch", "batch_bitsliced_kernel", (10, 4, 0, BATCH_10_4), [
        (2048, "aligned", "batch_bitsliced_kernel<2, 12, true>"),
        (2049, "aligned", "batch_bitsliced_kernel<2, 12, true>"),
        (4096 + 17, "gap16", "batch_bitsliced_kernel<2, 12, true>"),
        (17, "aligned", BATCH_BYTEWISE),
        (2047, "aligned", BATCH_BYTEWISE),
        (2049, "shift", BATCH_BYTEWISE),
        (2049, "pad5", BATCH_BYTEWISE),
    ])
    + _cases("decode_batch", "batch_bytewise_kernel", (10, 4, 2, BATCH_10_4), [
        (2049, "aligned", BATCH_BYTEWISE),
    ])
    + _cases("decode_batch", "batch_stream_kernel", (20, 7, 0, BATCH_20_7), [
        (2048, "aligned", "batch_stream_kernel<7, 4>"),
        (2049, "aligned", "batch_stream_kernel<7, 4>"),
        (2049, "shift", BATCH_BYTEWISE),
        (4096 + 17, "pad5", BATCH_BYTEWISE),
    ])
)

# hrs_encode_crc_dev, RS(10,4) mode 3. cfg = (stripes, with crc_in[, (code, k, p, kernel mode)])
ENCODE_CRC = [
    Case("encode_crc", "encode_crc", cfg, L, place, kernel) for cfg, L, place, kernel in [
        ((3, False), 2048, "aligned", "encode_crc*"),
        ((3, True), 2048, "gap16", "encode_crc*"),
        ((3, True), 32768, "aligned", "encode_crc*"),
        ((1, False), 65536, "aligned", "encode_crc*"),
        ((3, True), 2049, "aligned", "encode_static_kernel<10, 4>"),   # two passes: encode, then the CRC pass
        ((3, False), 4096 + 17, "aligned", "encode_static_kernel<10, 4>"),
        ((3, False), 2049, "shift", BYTEWISE),
        ((3, True), 2048, "shift", BYTEWISE),
        ((3, True), 2048, "pad5", BYTEWISE),
        # a (k, p) inside kFusedMaxK / kFusedMaxP that no fused kernel is built for: two passes on whole windows
        ((3, False, ("rs", 5, 2, 0)), 2048, "aligned", "bitsliced_pipe_kernel<2, 8>"),
    ]
]

# hrs_decode_crc_dev, RS(10,4). cfg = (erased locations, with crc_in)
DECODE_CRC = [
    Case("decode_crc", "decode_crc", cfg, L, place, kernel) for cfg, L, place, kernel in [
        (((5,), False), 2048, "aligned", "decode_crc*"),
        (((0, 13), True), 2048, "aligned", "decode_crc*"),
        (((5,), True), 32768, "aligned", "decode_crc*"),
        (((0, 13), False), 32768, "gap16", "decode_crc*"),
        (((5,), True), 2049, "aligned", "bitsliced_pipe_kernel<1, 12>"),  # the apply, then the CRC pass
        (((0, 13), False), 2049, "aligned", "bitsliced_pipe_kernel<2, 12>"),
        (((5,), False), 2048, "shift", BYTEWISE),
        (((5,), True), 2049, "shift", BYTEWISE),
        (((0, 13), True), 2048, "pad5", BYTEWISE),
        # 4 outputs from 10 live inputs, more than the 8 the fused repair takes: two passes on whole windows
        (((0, 5, 9, 13), False), 2048, "aligned", "bitsliced_kernel<4, 12>"),
    ]
]

# hrs_crc32_dev: 5 rows; hrs_last_kernel is not set by this entry point
CRC32 = [Case("crc32", None, (i + j) % 2 == 1, L, place, None)
         for i, L in enumerate(LENGTHS) for j, place in enumerate(("aligned", "shift"))]

TABLE = ENCODE + DECODE + APPLY + BATCH + ENCODE_CRC + DECODE_CRC + CRC32

FAMILIES = ("encode_static_kernel", "encode_cauchy_kernel", "xor_kernel", "bitsliced_kernel", "bitsliced_pipe_kernel",
            "bitsliced_stream_kernel", "bytewise_kernel", "batch_bitsliced_kernel", "batch_stream_kernel",
            "batch_bytewise_kernel", "encode_crc", "decode_crc")
BYTE_GRANULAR = ("bytewise_kernel", "batch_bytewise_kernel")


def check_table(table=TABLE):
    """A condition on the table, not on the GPU: every kernel family is
    named by a case, has a case whose length leaves a row tail, and, if it is
    a vector family, has both unaligned placements ending in the byte-granular
    kernel. Every length of the list is used."""
    for fam in FAMILIES:
        mine = [c for c in table if c.family == fam]
        named = [c for c in mine if c.kernel is not None and
                 (c.kernel[:-1] == fam if c.kernel.endswith("*") else c.kernel.split("<")[0] == fam)]
        assert named, f"no case names {fam}"
        assert any(c.L % 2048 for c in mine), f"{fam}: no case with a row tail"
        if fam in BYTE_GRANULAR:
            continue
        assert any(c.L % 2048 and c.L > 2048 for c in mine if c.place not in UNALIGNED), f"{fam}: no windows + tail"
        assert any(c.L % 2048 == 0 for c in named), f"{fam}: no case of whole windows"
        for place in UNALIGNED:
            assert any(c.place == place and c.kernel in BYTE_GRANULAR for c in mine), \
                f"{fam}: no {place} case that ends in the byte-granular kernel"
    for c in table:
        assert c.L in LENGTHS and c.place in PLACEMENTS, c
        if c.place in UNALIGNED and c.kernel:
            assert c.kernel in BYTE_GRANULAR, c
    assert {c.L for c in table} == set(LENGTHS)


check_table()

pytestmark = pytest.mark.gpu


def _id(c):
    return f"{c.family}-{c.cfg}-{c.L}-{c.place}".replace(" ", "")


def _arena(S, L, place, seed):
    shift, pad = PLACEMENTS[place]
    return Arena(S, L, shift=shift, stripe_pad=pad, seed=seed)


def _kernel_ok(got, want):
    return got.startswith(want[:-1]) if want.endswith("*") else got == want


def _finish(torch, arena, flat, outputs, code=None, kernel=None):
    """The two assertions of every case."""
    got_kernel = code.lastKernel() if code is not None else None
    torch.cuda.synchronize()
    d = arena.diff(flat.cpu().numpy(), arena.expected(outputs))
    assert d is None, d
    if kernel is not None:
        assert _kernel_ok(got_kernel, kernel), (got_kernel, kernel)


def _finish_crc(crc_arena, crc_flat, words):
    d = crc_arena.diff(crc_flat.cpu().numpy(), crc_arena.expected(words))
    assert d is None, d


def _make_code(kind, k, p, mode):
    cls = {"rs": HipReedSolomonCode, "nrs": HipNativeReedSolomonCode, "xor": HipXORCode}[kind]
    code = cls(k, p, device=0)
    code.setKernelMode(mode)
    return code


def _ref_encode(kind, k, p, data):
    if kind == "rs":
        return C.encode_bulk(k, p, data)
    if kind == "nrs":
        return C.nrs_encode_bulk(k, p, data)
    return [C.xor_encode_bulk(k, data)]


def _encode_outputs(arena, kind, k, p, dnames, pnames):
    pre = [arena.pre(n) for n in dnames]
    par = [_ref_encode(kind, k, p, [pre[i][s] for i in range(k)]) for s in range(arena.S)]
    return {pnames[o]: np.stack([par[s][o] for s in range(arena.S)]) for o in range(p)}


# ------------------------------------------------------------ hrs_encode_dev

@pytest.mark.parametrize("case", ENCODE, ids=_id)
def test_encode_footprint(cuda, case):
    kind, k, p, mode = case.cfg
    arena = _arena(3, case.L, case.place, seed=k * 1000 + p * 10 + mode)
    dnames = arena.add_rows("data", k, "input")
    pnames = arena.add_rows("parity", p, "output")
    want = _encode_outputs(arena, kind, k, p, dnames, pnames)
    code = _make_code(kind, k, p, mode)
    flat, v = arena.to_device()
    device.encode_rows(code, [v[n] for n in dnames], [v[n] for n in pnames])
    _finish(cuda, arena, flat, want, code, case.kernel)


# ------------------------------------------------------------ hrs_decode_dev

def _decode_setup(arena, erased):
    """14 non-codeword rows (every coefficient of the decode matrix counts)
    and the oracle's decodeBulk of each stripe's pre-call survivors."""
    k, p = 10, 4
    n = k + p
    snames = arena.add_rows("loc", n, "input")
    onames = arena.add_rows("out", len(erased), "output")
    to_read = sorted(C.locations_to_read(k, p, list(erased)))
    ntr = [x for x in range(n) if x not in to_read]
    pre = [arena.pre(x) for x in snames]
    zero = np.zeros(arena.L, np.uint8)
    want = {o: np.empty((arena.S, arena.L), np.uint8) for o in onames}
    for s in range(arena.S):
        reads = [pre[x][s] if x in to_read else zero for x in range(n)]
        ref = C.decode_bulk5(k, p, reads, list(erased), to_read, ntr)
        for t, o in enumerate(onames):
            want[o][s] = ref[t]
    return snames, onames, ntr, want


@pytest.mark.parametrize("case", DECODE, ids=_id)
def test_decode_footprint(cuda, case):
    erased = list(case.cfg)
    arena = _arena(3, case.L, case.place, seed=len(erased))
    snames, onames, ntr, want = _decode_setup(arena, erased)
    code = HipReedSolomonCode(10, 4, device=0)
    flat, _ = arena.to_device()
    # rows at not_to_read locations go to the library as NULL
    device.decode_stripes(code, arena.stack(flat, snames), erased, ntr, arena.stack(flat, onames))
    _finish(cuda, arena, flat, want, code, case.kernel)


# ------------------------------------------------------------- hrs_apply_dev

_mul = []


def _gf_products(m, x):
    """out[o] = XOR_i m[o, i] * x[i] over [S, L] rows, from the oracle's multiply."""
    if not _mul:
        _mul.append(np.array([[C.gf_mul(a, b) for b in range(256)] for a in range(256)], dtype=np.uint8))
    out = [np.zeros_like(next(r for r in x if r is not None)) for _ in range(m.shape[0])]
    for o in range(m.shape[0]):
        for i, r in enumerate(x):
            if m[o, i]:
                out[o] ^= _mul[0][m[o, i]][r]
    return out


def _apply_matrix(kind):
    """(matrix, indices of the inputs passed as NULL)."""
    rng = np.random.default_rng(len(kind))
    if kind == "zero_column":
        m = rng.integers(0, 256, (2, 5), dtype=np.uint8)
        m[:, 2] = 0
        assert all(m[:, i].any() for i in (0, 1, 3, 4))
        return m, (2,)
    if kind == "all_zero":
        return np.zeros((2, 3), np.uint8), ()
    if kind == "ones_1x17":
        return np.ones((1, 17), np.uint8), ()
    m = rng.integers(0, 256, (6, 9), dtype=np.uint8)
    assert m.any(axis=0).all() and kind == "random_6x9"
    return m, ()


@pytest.mark.parametrize("case", APPLY, ids=_id)
def test_apply_footprint(cuda, case):
    m, null = _apply_matrix(case.cfg)
    nout, nin = m.shape
    arena = _arena(3, case.L, case.place, seed=nout * 100 + nin)
    xnames = [None if i in null else arena.add(f"x{i}", "input") for i in range(nin)]  # no region for a NULL input
    ynames = arena.add_rows("y", nout, "output")
    ref = _gf_products(m, [None if n is None else arena.pre(n) for n in xnames])
    code = HipReedSolomonCode(10, 4, device=0)
    flat, v = arena.to_device()
    device.apply_rows(code, m, [None if n is None else v[n] for n in xnames], [v[n] for n in ynames])
    _finish(cuda, arena, flat, dict(zip(ynames, ref)), code, case.kernel)


# ------------------------------------------------------ hrs_decode_batch_dev

@pytest.mark.parametrize("case", BATCH, ids=lambda c: f"{c.family}-{c.cfg[:3]}-{c.L}-{c.place}".replace(" ", ""))
def test_decode_batch_footprint(cuda, case):
    k, p, mode, lists = case.cfg
    n, S = k + p, len(lists)
    E = max(len(e) for e in lists)
    arena = _arena(S, case.L, case.place, seed=n)
    snames = arena.add_rows("loc", n, "input")
    onames = arena.add_rows("out", E, "output")
    er = np.full((S, E), -1, dtype=np.int32)
    pre = [arena.pre(x) for x in snames]
    zero = np.zeros(arena.L, np.uint8)
    # rows past a stripe's own erasures, and the stripe with none, keep their poison
    want = {o: np.full((S, arena.L), POISON, np.uint8) for o in onames}
    for s, erased in enumerate(lists):
        erased = list(erased)
        er[s, :len(erased)] = erased
        if not erased:
            continue
        to_read = sorted(C.locations_to_read(k, p, erased))
        ntr = [x for x in range(n) if x not in to_read or x in erased]
        reads = [zero if x in ntr else pre[x][s] for x in range(n)]
        ref = C.decode_bulk5(k, p, reads, erased, to_read, ntr)
        for t in range(len(erased)):
            want[onames[t]][s] = ref[t]
    code = _make_code("rs", k, p, mode)
    flat, _ = arena.to_device()
    device.decode_batch(code, arena.stack(flat, snames), er, arena.stack(flat, onames))
    _finish(cuda, arena, flat, want, code, case.kernel)


# ---------------------------------------------- CRC entry points (via _lib)

def _ptrs(views, names):
    return _lib.ptr_array([None if n is None else views[n].data_ptr() for n in names])


def _stride(arena):
    return arena.stripe_stride if arena.S > 1 else arena.L


def _crc_words(rows, crc_in):
    """zlib CRC-32 of rows[r][s] -> [S, nrows] uint32, continuing crc_in."""
    S = rows[0].shape[0]
    out = np.empty((S, len(rows)), np.uint32)
    for s in range(S):
        for r, row in enumerate(rows):
            out[s, r] = zlib.crc32(row[s].tobytes(), 0 if crc_in is None else int(crc_in[s, r]))
    return out


@pytest.mark.parametrize("case", ENCODE_CRC, ids=_id)
def test_encode_crc_footprint(cuda, case):
    torch = cuda
    S, with_in = case.cfg[:2]
    kind, k, p, mode = case.cfg[2] if len(case.cfg) > 2 else ("rs", 10, 4, 3)
    arena = _arena(S, case.L, case.place, seed=case.L)
    dnames = arena.add_rows("data", k, "input")
    pnames = arena.add_rows("parity", p, "output")
    want = _encode_outputs(arena, kind, k, p, dnames, pnames)
    crcs = CrcArena(S, k + p, with_in, seed=case.L)
    words = _crc_words([arena.pre(x) for x in dnames] + [want[x] for x in pnames], crcs.crc_in())
    code = _make_code(kind, k, p, mode)
    flat, v = arena.to_device()
    cflat, cin, cout = crcs.to_device()
    code._check(_lib.lib().hrs_encode_crc_dev(code._handle(), _ptrs(v, dnames), _stride(arena), _ptrs(v, pnames),
                                              _stride(arena), case.L, S, cin, cout,
                                              torch.cuda.current_stream().cuda_stream))
    _finish(torch, arena, flat, want, code, case.kernel)
    _finish_crc(crcs, cflat, words)  # exactly S * (k + p) words written, crc_in and the guard words intact


@pytest.mark.parametrize("case", DECODE_CRC, ids=_id)
def test_decode_crc_footprint(cuda, case):
    torch = cuda
    erased, with_in = list(case.cfg[0]), case.cfg[1]
    arena = _arena(3, case.L, case.place, seed=case.L + len(erased))
    snames, onames, ntr, want = _decode_setup(arena, erased)
    crcs = CrcArena(3, len(erased), with_in, seed=case.L)
    words = _crc_words([want[o] for o in onames], crcs.crc_in())
    code = HipReedSolomonCode(10, 4, device=0)
    flat, v = arena.to_device()
    cflat, cin, cout = crcs.to_device()
    rows = _ptrs(v, [None if x in ntr else snames[x] for x in range(14)])
    code._check(_lib.lib().hrs_decode_crc_dev(
        code._handle(), rows, _stride(arena), _ptrs(v, onames), _stride(arena), _lib.int_array(erased), len(erased),
        _lib.int_array(ntr), len(ntr), case.L, 3, cin, cout, torch.cuda.current_stream().cuda_stream))
    _finish(torch, arena, flat, want, code, case.kernel)
    _finish_crc(crcs, cflat, words)


@pytest.mark.parametrize("case", CRC32, ids=lambda c: f"{c.L}-{c.place}-{'in' if c.cfg else 'noin'}")
def test_crc32_footprint(cuda, case):
    torch = cuda
    S, nrows = 3, 5
    arena = _arena(S, case.L, case.place, seed=case.L)
    names = arena.add_rows("row", nrows, "input")
    crcs = CrcArena(S, nrows, case.cfg, seed=case.L)
    words = _crc_words([arena.pre(x) for x in names], crcs.crc_in())
    code = HipReedSolomonCode(10, 4, device=0)
    flat, v = arena.to_device()
    cflat, cin, cout = crcs.to_device()
    code._check(_lib.lib().hrs_crc32_dev(code._handle(), _ptrs(v, names), nrows, _stride(arena), case.L, S, cin, cout,
                                         torch.cuda.current_stream().cuda_stream))
    _finish(torch, arena, flat, {})  # the rows are unchanged
    _finish_crc(crcs, cflat, words)


# -------------------------------------------------- hrs_last_kernel is fresh

def _encode_once(torch, code, L, place):
    arena = _arena(3, L, place, seed=L)
    dnames = arena.add_rows("data", 10, "input")
    pnames = arena.add_rows("parity", 4, "output")
    flat, v = arena.to_device()
    device.encode_rows(code, [v[n] for n in dnames], [v[n] for n in pnames])
    kernel = code.lastKernel()
    _finish(torch, arena, flat, _encode_outputs(arena, "rs", 10, 4, dnames, pnames))
    return kernel


def _batch_once(torch, code, L, place):
    arena = _arena(3, L, place, seed=L)
    snames = arena.add_rows("loc", 14, "input")
    onames = arena.add_rows("out", 2, "output")
    flat, _ = arena.to_device()
    er = np.array([[5, -1], [0, 13], [-1, -1]], dtype=np.int32)
    device.decode_batch(code, arena.stack(flat, snames), er, arena.stack(flat, onames))
    kernel = code.lastKernel()
    torch.cuda.synchronize()
    return kernel


@pytest.mark.parametrize("entry", ["encode", "decode_batch"])
def test_last_kernel_names_the_latest_call(cuda, entry):
    """A call whose only launch is the byte-granular kernel (short rows,
    unaligned rows) names it, on a fresh handle and after a call that ran a
    vector kernel; it used to leave the previous call's name (or "")."""
    once, vector, bytewise = {
        "encode": (_encode_once, "encode_static_kernel<10, 4>", BYTEWISE),
        "decode_batch": (_batch_once, "batch_bitsliced_kernel<2, 12, true>", BATCH_BYTEWISE),
    }[entry]
    fresh = HipReedSolomonCode(10, 4, device=0)
    assert fresh.lastKernel() == ""
    assert once(cuda, fresh, 100, "aligned") == bytewise
    code = HipReedSolomonCode(10, 4, device=0)
    assert once(cuda, code, 4096, "aligned") == vector
    assert once(cuda, code, 100, "aligned") == bytewise
    assert once(cuda, code, 4096, "aligned") == vector
    assert once(cuda, code, 4096, "shift") == bytewise
