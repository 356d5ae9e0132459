"""Inputs and expectations of the ragged repair tests (test_gpu_ragged_repair*.py).

A batch is stripes[S, n, L] in hops order (parity first), erased[S, E]
(ascending per stripe, -1 padded) and valid[S, n]. EVERY cell holds seeded
random NON-ZERO bytes throughout (non-codeword rows, so every coefficient of
every pattern's matrix counts), tails behind `valid` included: a byte at or
beyond a survivor's length that reaches an output shows. `out` starts as a
sentinel and every byte of it is compared, so a byte written at or beyond an
output's length shows too. The expectation is the oracle's decodeBulk of the
code's kind over zero-filled copies of the survivors, with the survivor lists
tests/test_batch_decode.py derives (locationsToReadForDecode; everything else
not read), each output cut at its length. Everything is built once per key and
handed out read-only."""
import functools
import random

import numpy as np

from oracle import rs_oracle as C
from ragged_inputs import code_id, make_code  # noqa: F401  (re-exported)

WINDOW = 2048  # kWindowBytes
SENTINEL = 0x5C
VECTOR = "batch_ragged_kernel<%d, %d>"
BYTEWISE = "batch_ragged_bytewise_kernel"

# (kind, k, p, src parities)
CODES = [("rs", 10, 4, 0), ("rs", 6, 3, 0), ("rs", 3, 2, 0), ("rs", 12, 4, 0), ("rs", 5, 3, 0), ("nrs", 10, 4, 0),
         ("xor", 4, 1, 0), ("src", 10, 6, 2)]


def to_read(cfg, lost):
    """The survivors the repair of `lost` reads, ascending; None when the code cannot repair it."""
    kind, k, p, s = cfg
    tr = C.src_locations_to_read(k, p, s, lost) if kind == "src" else C.locations_to_read(k, p, lost)
    return None if tr is None else sorted(tr)


def decode_ref(cfg, reads, lost, tr):
    """The oracle's decodeBulk of the code: reads[n] full rows (only those in tr are used)."""
    kind, k, p, s = cfg
    n = k + p
    ntr = [x for x in range(n) if x not in tr]
    if kind == "nrs":
        return C.nrs_decode_bulk(k, p, [reads[x] if x in tr else None for x in range(n)], lost, ntr)
    rows = [reads[x] if x in tr else np.zeros_like(reads[0]) for x in range(n)]
    if kind == "rs":
        return C.decode_bulk5(k, p, rows, lost, tr, ntr)
    if kind == "xor":
        return [C.xor_decode_bulk(k, rows, lost[0])]
    return C.src_decode_bulk(k, p, s, rows, lost, tr, ntr)


@functools.lru_cache(maxsize=None)
def live_inputs(cfg, lost):
    """The survivors the plan of the pattern `lost` (a tuple) reads, ascending,
    which is the plan's input order: the oracle decodes n unit rows, so byte x
    of output t is the coefficient (t, x), and a survivor is live when its
    column is not all zero."""
    if not lost:
        return ()
    n = cfg[1] + cfg[2]
    unit = [np.eye(n, dtype=np.uint8)[x] for x in range(n)]
    m = np.stack(decode_ref(cfg, unit, list(lost), to_read(cfg, list(lost))))
    return tuple(int(x) for x in np.flatnonzero((m != 0).any(axis=0)))


def plan_shape(cfg, lost):
    """(outputs, live inputs) of the pattern `lost` (a tuple)."""
    return len(lost), len(live_inputs(cfg, lost))


def lost_of(erased_row):
    return [int(x) for x in erased_row if x >= 0]


def expected_kernel(cfg, erased):
    """The name hrs_last_kernel reports for a ragged batch with whole windows
    and an aligned layout (include/hrs.h, "ragged repair": Kernels)."""
    shapes = [plan_shape(cfg, tuple(lost_of(r))) for r in erased]
    nout, nin = max(a for a, _ in shapes), max(b for _, b in shapes)
    if nout > 4 or nin > 16:
        return BYTEWISE
    return VECTOR % (nout, 4 if nin <= 4 else 8 if nin <= 8 else 12 if nin <= 12 else 16)


def expected(cfg, stripes, erased, valid):
    """out[S, E, L]: the sentinel, except the first valid[s, e] bytes of each
    output, which are the oracle's over the zero-filled survivors."""
    S, n, L = stripes.shape
    want = np.full((S, erased.shape[1], L), SENTINEL, np.uint8)
    for s in range(S):
        lost = lost_of(erased[s])
        if not lost:
            continue
        tr = to_read(cfg, lost)
        reads = [np.array(stripes[s, x]) for x in range(n)]
        for x in tr:
            reads[x][int(valid[s, x]):] = 0
        ref = decode_ref(cfg, reads, lost, tr)
        for t, e in enumerate(lost):
            v = int(valid[s, e])
            want[s, t, :v] = ref[t][:v]
    return want


def fresh_stripes(cfg, S, L, seed):
    return np.random.default_rng([seed, cfg[1], cfg[2], S, L]).integers(1, 256, (S, cfg[1] + cfg[2], L), dtype=np.uint8)


def length_classes(L):
    return sorted({min(v, L) for v in (0, 1, 15, 16, 17, 1024, 1025, 2047, 2048, 2049, L - 1, L)})


def patterns(cfg, max_loss, seed=7):
    """One seeded repairable erasure list of every size 0..max_loss."""
    n = cfg[1] + cfg[2]
    rnd = random.Random(seed * 1000 + n)
    pats = []
    for ne in range(max_loss + 1):
        while True:
            lost = sorted(rnd.sample(range(n), ne))
            if to_read(cfg, lost) is not None:
                pats.append(lost)
                break
    return pats


def class_batch_inputs(cfg, L, max_loss):
    """(erased, valid): stripe i has pattern i mod P of patterns() and cell l
    the length class (i div P + 3 l) mod |V|, over P |V| stripes: under every
    pattern every location, so every input position and every output position,
    meets every class, and neighbouring cells differ. Then the file-tail
    stripes: the first k div 3 data cells full, one half full, the rest empty,
    every parity cell full; one lost data cell 0, one lost the last (empty) data
    cell, whose output is dead throughout, and one nothing."""
    k, p = cfg[1], cfg[2]
    n = k + p
    V = length_classes(L)
    pats = patterns(cfg, max_loss)
    E = max(1, max_loss)
    er, va = [], []
    for i in range(len(pats) * len(V)):
        er.append(pats[i % len(pats)])
        va.append([V[(i // len(pats) + 3 * l) % len(V)] for l in range(n)])
    m = k // 3
    tail = [L] * p + [L] * m + [L // 2] + [0] * (k - m - 1)
    for lost in ([p], [n - 1], []):
        er.append(lost)
        va.append(tail)
    erased = np.full((len(er), E), -1, np.int32)
    for i, lost in enumerate(er):
        erased[i, :len(lost)] = lost
    return erased, np.array(va, np.uint32)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def class_batch(cfg, L, max_loss=None):
    """(stripes, erased, valid, want) of the class batch of a code at cell
    length L with up to max_loss losses per stripe (default: p)."""
    erased, valid = class_batch_inputs(cfg, L, cfg[2] if max_loss is None else max_loss)
    st = fresh_stripes(cfg, len(valid), L, seed=1)
    return _frozen(st, erased, valid, expected(cfg, st, erased, valid))


@functools.lru_cache(maxsize=None)
def full_batch(cfg, L, S=6):
    """An all-full batch with every loss count: (stripes, erased, valid, want)."""
    pats = patterns(cfg, min(cfg[2], 4), seed=9)
    erased = np.full((S, max(len(x) for x in pats)), -1, np.int32)
    for i in range(S):
        erased[i, :len(pats[i % len(pats)])] = pats[i % len(pats)]
    valid = np.full((S, cfg[1] + cfg[2]), L, np.uint32)
    st = fresh_stripes(cfg, S, L, seed=2)
    return _frozen(st, erased, valid, expected(cfg, st, erased, valid))


def mismatch(got, want, erased, valid):
    """None, or where got[S, E, L] first differs from want."""
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    if bad.size == 0:
        return None
    s, t, c = (int(x) for x in bad[0])
    lost = lost_of(erased[s])
    v = int(valid[s, lost[t]]) if t < len(lost) else 0
    what = "inside" if c < v else "BEYOND (must never be written)"
    return "%d bytes differ; first: stripe %d (lost %s) output %d byte %d, %s its length %d: got %#x, want %#x" % (
        len(bad), s, lost, t, c, what, v, int(got[s, t, c]), int(want[s, t, c]))
