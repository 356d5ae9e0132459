"""Inputs and expectations of the ragged encode tests (test_gpu_ragged*.py).

A batch is stripes[S, n, L] in hops order (parity first) and valid[S, k]. The
data cells hold seeded random NON-ZERO bytes throughout, so a byte at or
beyond `valid` that reaches a parity byte shows; the parity rows hold a poison
byte. The expectation is the oracle's encodeBulk of the code's kind over
zero-filled copies of the data cells, nothing else. Everything is built once
per key and handed out read-only."""
import functools

import numpy as np

from oracle import rs_oracle as C

WINDOW = 2048  # kWindowBytes
POISON = 0xA5
VECTOR = "encode_ragged_kernel<%d, %d>"
BYTEWISE = "encode_ragged_bytewise_kernel"

# (kind, k, p, src parities): the six shapes with a compile-time network, then
# the codes that only have the byte-granular kernel
STATIC = [("rs", 3, 2, 0), ("rs", 6, 3, 0), ("rs", 10, 4, 0), ("rs", 12, 4, 0), ("nrs", 10, 4, 0), ("nrs", 6, 3, 0)]
RUNTIME = [("rs", 5, 3, 0), ("xor", 4, 1, 0), ("src", 10, 6, 2)]


def code_id(cfg):
    return "%s_%d_%d" % cfg[:3]


def make_code(cfg, mode=0, device=0):
    from lambdafs_amd import (HipNativeReedSolomonCode, HipReedSolomonCode, HipSimpleRegeneratingCode, HipXORCode)
    kind, k, p, s = cfg
    if kind == "src":
        code = HipSimpleRegeneratingCode(k, p, s, device=device)
    else:
        code = {"rs": HipReedSolomonCode, "nrs": HipNativeReedSolomonCode, "xor": HipXORCode}[kind](k, p, device=device)
    code.setKernelMode(mode)
    return code


def vector_kernel(cfg):
    return VECTOR % cfg[1:3] if cfg in STATIC else BYTEWISE


def ref_parity(cfg, rows):
    """The oracle's encodeBulk of the code over k full rows: p rows."""
    kind, k, p, s = cfg
    if kind == "rs":
        return C.encode_bulk(k, p, rows)
    if kind == "nrs":
        return C.nrs_encode_bulk(k, p, rows)
    if kind == "xor":
        return [C.xor_encode_bulk(k, rows)]
    return C.src_encode_bulk(k, p, s, rows)


def zero_filled(data, valid):
    """data[S, k, L] as the reference's readTillEnd leaves the buffers."""
    z = np.array(data, copy=True)
    for s in range(z.shape[0]):
        for j in range(z.shape[1]):
            z[s, j, int(valid[s, j]):] = 0
    return z


def expected(cfg, stripes, valid):
    """stripes[S, n, L] with exactly the parity rows replaced by the oracle's."""
    p = cfg[2]
    want = np.array(stripes, copy=True)
    z = zero_filled(stripes[:, p:], valid)
    for s in range(want.shape[0]):
        want[s, :p] = np.stack(ref_parity(cfg, list(z[s])))
    return want


def fresh_stripes(cfg, S, L, seed):
    k, p = cfg[1], cfg[2]
    st = np.full((S, k + p, L), POISON, np.uint8)
    st[:, p:] = np.random.default_rng([seed, k, p, S, L]).integers(1, 256, (S, k, L), dtype=np.uint8)
    return st


def valid_classes(L):
    return sorted({min(v, L) for v in (0, 1, 15, 16, 17, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, L - 1, L)})


def class_valid(k, L):
    """3 |V| stripes, row j of stripe i at V[(i + 3 j) mod |V|]: every row
    position meets every class and consecutive rows differ; then the file-tail
    stripes (the first m cells full, the rest empty, m = 0..k, which includes
    the all-zero and the all-full stripe), then one more of each of those two."""
    V = valid_classes(L)
    rows = [[V[(i + 3 * j) % len(V)] for j in range(k)] for i in range(3 * len(V))]
    rows += [[L] * m + [0] * (k - m) for m in range(k + 1)]
    rows += [[0] * k, [L] * k]
    return np.array(rows, np.uint32)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def class_batch(cfg, L):
    """(stripes, valid, want) of the class batch of a code at cell length L."""
    valid = class_valid(cfg[1], L)
    st = fresh_stripes(cfg, len(valid), L, seed=1)
    return _frozen(st, valid, expected(cfg, st, valid))


@functools.lru_cache(maxsize=None)
def full_batch(cfg, L, S=5):
    """An all-full batch: (stripes, valid, want)."""
    valid = np.full((S, cfg[1]), L, np.uint32)
    st = fresh_stripes(cfg, S, L, seed=2)
    return _frozen(st, valid, expected(cfg, st, valid))


def mismatch(got, want, p):
    """None, or where got[S, n, L] first differs from want."""
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    if bad.size == 0:
        return None
    s, l, c = (int(x) for x in bad[0])
    what = "parity row %d" % l if l < p else "DATA cell %d (must never be written)" % (l - p)
    return "%d bytes differ; first: stripe %d %s byte %d: got %#x, want %#x" % (
        len(bad), s, what, c, int(got[s, l, c]), int(want[s, l, c]))
