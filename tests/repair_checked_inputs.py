"""Inputs and the Python restatement of checked repair (hrs_repair_checked_host,
hrs_repair_checked_dev), shared by the CPU and the GPU tests.

The restatement is written on its own from the rule in include/hrs.h: zlib
CRCs, pass 1's report from device.heal_host on a copy (word 3 cleared: a scrub
stores nothing), steps 1-3 in Python, device.heal_erased_host on the erased
set, step 6. It shares no code with the call under test beyond those two older
host calls.

The recipes are few-column damage: a damaged cell gets random nonzero XORs in
the columns {0, 15, 1023, 2048, L - 1} of its row; "restamped" means that the
stored checksum is the CRC of the damaged cell. Only numpy, zlib and the
oracle (through heal_erased_inputs)."""
import zlib

import numpy as np

import heal_erased_inputs as hei
from lambdafs_amd import device

CLEAN, REPAIRED, RESTAMP, FAILED, TOOMANY, AMBIGUOUS = range(6)
NONE = 0xFFFFFFFF
CODES = [(3, 2), (6, 3), (10, 4), (4, 1), (12, 8), (6, 5), (7, 6), (10, 7)]


def crc(row):
    return zlib.crc32(np.ascontiguousarray(row).tobytes()) & 0xFFFFFFFF


def restate(code, rows, stored, join):
    """The rule over one stripe: rows (list of n writable uint8 arrays) are
    left as the call must leave them. Returns (verdict, erased [p], report
    [4 + n], crcs [n], listed, (pass-1 crcs, pass-1 report))."""
    n, p = len(rows), code.paritySize()
    c1 = np.array([crc(r) for r in rows], dtype=np.uint32)
    r1 = device.heal_host(code, [r.copy() for r in rows])
    r1[device.SCRUB_PATCHED] = 0
    d = [l for l in range(n) if c1[l] != stored[l]]
    b = sorted(set(d) | ({l for l in range(n) if r1[4 + l] != 0} if join else set()))
    erased = np.full(p, -1, dtype=np.int32)
    first = (c1.copy(), r1.copy())
    if not d and r1[1] > 0:
        return AMBIGUOUS, erased, r1, c1, False, first
    if not d and r1[0] == 0:
        return CLEAN, erased, r1, c1, False, first
    if len(b) > p:
        return TOOMANY, erased, r1, c1, False, first
    erased[: len(b)] = b
    r2 = device.heal_erased_host(code, rows, b)
    c2 = np.array([crc(r) for r in rows], dtype=np.uint32)
    f = [l for l in range(n) if c2[l] != stored[l]]
    if not f:
        verdict = REPAIRED
    elif not set(f) & set(d) and r2[1] == 0:
        verdict = RESTAMP
    else:
        verdict = FAILED
    return verdict, erased, r2, c2, True, first


def columns(L):
    return sorted({0, 15, 1023, 2048, L - 1} & set(range(L)))


def _damage(stripe, cell, cols, rng):
    for c in cols:
        stripe[cell, c] ^= rng.integers(1, 256, dtype=np.uint8)


def clean(k, p, L, seed=0):
    """One clean stripe [n, L] (a copy) and its true checksums."""
    st = np.array(hei.clean_stripes(k, p, 1, L, 100 + seed)[0])
    return st, np.array([crc(r) for r in st], dtype=np.uint32)


def recipe(kind, k, p, L, seed=0):
    """(stripe [n, L], stored [n]) of a recipe, or None where the recipe does
    not apply to the code: 'clean'; 'repaired' (p damaged cells, true
    checksums); 'garbage1' (one cell of garbage); 'toomany' (p + 1 damaged
    cells); 'restamp' (parity cell 0 damaged and restamped); 'failed'
    (RS(10,4): cells 2, 3, 8 damaged, cell 11 damaged in one of their columns
    and restamped); 'ambiguous' (RS(3,2): cells 0 and 3 damaged in the same
    columns, both restamped); 'garbage3' (RS(10,4): three cells of garbage)."""
    n = k + p
    rng = np.random.default_rng([seed, k, p, L, sum(map(ord, kind))])
    st, stored = clean(k, p, L, seed)
    cols = columns(L)
    if kind == "clean":
        pass
    elif kind == "repaired":
        for cell in rng.choice(n, p, replace=False):
            _damage(st, cell, cols, rng)
    elif kind == "garbage1":
        st[int(rng.integers(n))] = rng.integers(0, 256, L, dtype=np.uint8)
    elif kind == "toomany":
        for cell in rng.choice(n, p + 1, replace=False):
            _damage(st, cell, cols, rng)
    elif kind == "restamp":
        _damage(st, 0, cols, rng)
        stored[0] = crc(st[0])
    elif kind == "failed":
        if (k, p) != (10, 4):
            return None
        for cell in (2, 3, 8):
            _damage(st, cell, cols, rng)
        _damage(st, 11, cols[1:2], rng)
        stored[11] = crc(st[11])
    elif kind == "ambiguous":
        if (k, p) != (3, 2):
            return None
        for cell in (0, 3):
            _damage(st, cell, cols, rng)
            stored[cell] = crc(st[cell])
    elif kind == "garbage3":
        if (k, p) != (10, 4):
            return None
        for cell in (1, 5, 12):
            st[cell] = rng.integers(0, 256, L, dtype=np.uint8)
    else:
        raise ValueError(kind)
    return st, stored


KINDS = ["clean", "repaired", "garbage1", "toomany", "restamp", "failed", "ambiguous", "garbage3"]
# what the recipes give with checksums alone (p >= 2): no step of these depends on a column the locator may mis-resolve
EXPECTED = {"clean": CLEAN, "repaired": REPAIRED, "garbage1": REPAIRED, "toomany": TOOMANY, "restamp": RESTAMP,
            "failed": FAILED, "garbage3": REPAIRED}


def mix(k, p, L, S, listed_at, seed=0):
    """A batch [S, n, L] with its stored checksums [S, n]: stripes in
    `listed_at` take the damaging recipes that apply to the code in turn, the
    others alternate between clean, too many and (RS(3,2)) ambiguous."""
    n = k + p
    st = np.empty((S, n, L), dtype=np.uint8)
    stored = np.empty((S, n), dtype=np.uint32)
    hot = [kd for kd in ("repaired", "restamp", "garbage1", "failed", "garbage3") if recipe(kd, k, p, L) is not None]
    cold = ["clean", "toomany", "clean"] + (["ambiguous"] if (k, p) == (3, 2) else [])
    hi = ci = 0
    for s in range(S):
        if s in listed_at:
            kind, hi = hot[hi % len(hot)], hi + 1
        else:
            kind, ci = cold[ci % len(cold)], ci + 1
        st[s], stored[s] = recipe(kind, k, p, L, seed + s)
    return st, stored


def reference(code, stripes, stored, join):
    """restate() stripe by stripe: (bytes [S, n, L], verdicts [S], erased
    [S, p], reports [S, 4 + n], crcs [S, n], listed [S] bool)."""
    S, n, _ = stripes.shape
    p = code.paritySize()
    out = np.array(stripes)
    verdicts = np.zeros(S, dtype=np.int64)
    erased = np.zeros((S, p), dtype=np.int64)
    reports = np.zeros((S, 4 + n), dtype=np.int64)
    crcs = np.zeros((S, n), dtype=np.int64)
    listed = np.zeros(S, dtype=bool)
    for s in range(S):
        rows = [np.ascontiguousarray(out[s, l]) for l in range(n)]
        v, e, r, c, li, _ = restate(code, rows, stored[s], join)
        out[s] = np.stack(rows)
        verdicts[s], erased[s], reports[s], crcs[s], listed[s] = v, e, r, c, li
    return out, verdicts, erased, reports, crcs, listed
