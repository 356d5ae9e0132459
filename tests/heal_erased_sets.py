"""Inputs of the every-erased-set tests (tests/test_gpu_heal_erased_sets.py):
one stripe per erased set of a code, all sets of the code in one batch. The
clean stripes are 8 oracle-encoded stripes repeated cyclically, the erased
cells are filled with 0xA5, and heal_erased_inputs.plant puts survivor errors
at the window's and the tail's edges; every third stripe keeps clean survivors.
L = 2048 + 33 is one window and a byte-granular tail, the smallest length at
which both kernels run for every set; L = 2048 is the fused CRC kernel's shape.

What depends on the erased set in a walk (the per-group mask byte, the spare
row that dead load slots read, gamma and loc in the locator, the P x P matrix
of tv = M S) is a function of the set alone, so one stripe per set covers it.
Only numpy, zlib and the oracle (through heal_erased_inputs)."""
import itertools
import random
import zlib

import numpy as np

import heal_erased_inputs as H

L = H.WINDOW + 33
L_FUSED = H.WINDOW
BASE = 8      # distinct clean stripes
SEEDED = 40   # seeded sets of each size above 2 (sampled codes)
SEED = 1

EXHAUSTIVE = [(10, 4), (6, 3), (3, 2), (4, 1)]  # every subset of size 0 .. p
SAMPLED = [(6, 5), (7, 6), (10, 7), (20, 8)]
WIDEST = (247, 8)
# around the mask-word edges (32, 64, ...), location n - 1 = 254 and both ends of the tables
WIDEST_FIXED = [[31, 32], [63, 64], [30, 31, 32, 33], [254], [0, 254], list(range(247, 255)), list(range(8)),
                [95, 96, 127, 128, 159, 160, 191, 192]]
WIDEST_SEEDED = 10


def named_sets(k, p):
    """The sets a sampled code gets by name: all parity lost (the spare row is
    location p; at p = 8 the first load group is empty), the last p locations,
    and at RS(20,8) the whole second load group."""
    n = k + p
    named = [list(range(p)), list(range(n - p, n))]
    if (k, p) == (20, 8):
        named.append(list(range(8, 16)))
    return named


def erased_sets(k, p):
    """The code's list of erased sets (ascending location lists); the empty
    set comes first where the list has it (every code but the widest)."""
    n = k + p
    if (k, p) in EXHAUSTIVE:
        return [list(c) for e in range(p + 1) for c in itertools.combinations(range(n), e)]
    rnd = random.Random(7919 * k + p)
    if (k, p) == WIDEST:
        sets = [list(e) for e in WIDEST_FIXED]
        while len(sets) < len(WIDEST_FIXED) + WIDEST_SEEDED:
            e = sorted(rnd.sample(range(n), rnd.randrange(1, p + 1)))
            if e not in sets:
                sets.append(e)
        return sets
    if (k, p) not in SAMPLED:
        raise ValueError(f"no set list for RS({k},{p})")
    sets = [list(c) for e in range(3) for c in itertools.combinations(range(n), e)]
    named = named_sets(k, p)
    for e in range(3, p + 1):
        drawn = []
        while len(drawn) < SEEDED:
            c = sorted(rnd.sample(range(n), e))
            if c not in drawn and c not in named:
                drawn.append(c)
        sets += drawn
    return sets + named


def columns_of(length):
    return sorted({0, 1023, 2047, 2048, length - 1} & set(range(length)))


def crc(row, start=0):
    return zlib.crc32(np.ascontiguousarray(row).tobytes(), int(start)) & 0xFFFFFFFF


class Case:
    """sets; clean, bad [S, n, L]; planted (heal_erased_inputs.plant's list);
    clean_crcs [S, n]: zlib over the clean cells."""

    def __init__(self, k, p, length, over):
        self.k, self.p, self.n, self.length, self.over = k, p, k + p, length, over
        self.sets = erased_sets(k, p)
        self.S = len(self.sets)
        base = H.clean_stripes(k, p, BASE, length, SEED)
        turn = np.arange(self.S) % BASE
        self.clean = base[turn]
        self.clean.setflags(write=False)
        quiet = frozenset(range(0, self.S, 3))
        self.bad, self.planted = H.plant(k, p, self.clean, self.sets, columns_of(length), over=over,
                                         clean_stripes_=quiet, seed=SEED)
        self.bad.setflags(write=False)
        base_crcs = np.array([[crc(base[s, l]) for l in range(self.n)] for s in range(BASE)], dtype=np.uint32)
        self.clean_crcs = base_crcs[turn]

    def erased(self, width=None):
        return H.erased_array(self.sets, width)

    def planted_reports(self):
        return H.planted_reports(self.n, self.S, self.planted)

    def stored(self):
        """The checksums checked repair is given: the clean cells' CRCs, and a
        survivor with planted errors restamped with the CRC of the damaged cell
        (else it would join the doubted cells)."""
        stored = self.clean_crcs.copy()
        for s, l in sorted({(s, l) for s, _, errs in self.planted for l in errs}):
            stored[s, l] = crc(self.bad[s, l])
        return stored


_cases = {}


def case(k, p, length=L, over=0):
    """The code's batch, cached; the cache holds one code at a time (RS(10,4)'s
    batch is 40 MB)."""
    key = (k, p, length, over)
    if key not in _cases:
        if any(c[:2] != (k, p) for c in _cases):
            _cases.clear()
        _cases[key] = Case(k, p, length, over)
    return _cases[key]
