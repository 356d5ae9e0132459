"""Inputs of the heal-with-known-erasures GPU tests, built from the oracle's
encoder alone and cached: stripes of codeword columns, one erasure pattern per
stripe, erased cells pre-filled with 0xA5, and a list of planted survivor
errors. What a call must leave behind is the clean stripes themselves, and
the reports are counted from the planted list. Only numpy and the oracle."""
import random

import numpy as np

from oracle import rs_oracle as C

WINDOW = 2048
NONE = 0xFFFFFFFF
FILL = 0xA5


def clean_stripes(k, p, S, L, seed):
    """[S, n, L] codeword columns (hops order, parity first), read-only."""
    key = ("clean", k, p, S, L, seed)
    if key not in _cache:
        rng = np.random.default_rng([seed, k, p, S, L])
        st = np.empty((S, k + p, L), dtype=np.uint8)
        st[:, p:] = rng.integers(0, 256, (S, k, L), dtype=np.uint8)
        for s in range(S):
            st[s, :p] = np.stack(C.encode_bulk(k, p, [st[s, p + c] for c in range(k)]))
        st.setflags(write=False)
        _cache[key] = st
    return _cache[key]


_cache = {}


def seven_patterns(k, p, rnd):
    """The seven erased sets of the GPU tests: none; a data cell; parity 0; two
    cells with location n - 1; p - 1 cells; p cells; one cell (this stripe's
    survivors stay clean). Sizes are cut to p."""
    n = k + p
    pats = [[], [p + rnd.randrange(k)], [0], sorted([rnd.randrange(1, n - 1), n - 1])[-min(2, p):],
            sorted(rnd.sample(range(n), p - 1)), sorted(rnd.sample(range(n), p)), [rnd.randrange(n)]]
    return pats


def columns_of(L):
    """Planted columns: window and piece edges, the row's last byte, and three
    columns of lane 5 (two bytes of one word, one of its second piece)."""
    return sorted({0, 15, 16, 1023, 1024, 2047, 2048, L - 1, 81, 83, 1110} & set(range(L)))


def plant(k, p, clean, patterns, columns, over=0, clean_stripes_=(6,), seed=0):
    """(damaged [S, n, L], planted) for clean[S, n, L]: stripe s loses
    patterns[s] (cells filled with 0xA5); at every column of `columns` each
    stripe with capacity cap = (p - e) // 2 >= 1 (stripes in clean_stripes_
    excepted) gets 1 .. cap survivor errors in turn, or cap + 1 when over = 1
    (then also where cap = 0, as long as a spare syndrome is left: e < p).
    planted: list of (stripe, column, {location: xor value}). The first
    planted column of a stripe with erasures hits a survivor next to an erased
    location."""
    S, n, _ = clean.shape
    rnd = random.Random(seed * 7919 + 131 * k + p)
    bad = np.array(clean)
    planted = []
    for s in range(S):
        E = patterns[s]
        bad[s, E, :] = FILL
        cap = (p - len(E)) // 2
        if s in clean_stripes_ or (cap == 0 and not (over and len(E) < p)):
            continue
        survivors = [l for l in range(n) if l not in E]
        for i, c in enumerate(columns):
            t = cap + 1 if over else 1 + i % cap
            t = min(t, len(survivors))
            locs = rnd.sample(survivors, t)
            if i == 0 and E:
                near = [l for l in survivors if l - 1 in E or l + 1 in E]
                if near and near[0] not in locs:
                    locs[0] = near[0]
            errs = {l: rnd.randrange(1, 256) for l in locs}
            for l, x in errs.items():
                bad[s, l, c] ^= x
            planted.append((s, c, errs))
    return bad, planted


def planted_reports(n, S, planted):
    """Reports [S, 4 + n] when every planted column resolves to exactly its errors."""
    rep = np.zeros((S, 4 + n), dtype=np.uint32)
    rep[:, 2] = NONE
    for s, c, errs in planted:
        rep[s, 0] += 1
        rep[s, 2] = min(int(rep[s, 2]), c)
        rep[s, 3] += len(errs)
        for l in errs:
            rep[s, 4 + l] += 1
    return rep


def erased_array(patterns, width=None):
    width = width or max(1, max(len(e) for e in patterns))
    arr = np.full((len(patterns), width), -1, dtype=np.int32)
    for s, e in enumerate(patterns):
        arr[s, : len(e)] = e
    return arr


def host_reference(code, bad, patterns):
    """hrs_heal_erased_host stripe by stripe: (after [S, n, L], reports [S, 4 + n])."""
    from lambdafs_amd import device
    S, n, _ = bad.shape
    out = np.array(bad)
    reps = np.zeros((S, 4 + n), dtype=np.uint32)
    for s in range(S):
        rows = [out[s, l].copy() for l in range(n)]
        reps[s] = device.heal_erased_host(code, rows, patterns[s])
        out[s] = np.stack(rows)
    return out, reps
