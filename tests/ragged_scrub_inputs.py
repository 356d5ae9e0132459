"""Inputs and expectations of the ragged scrub and heal tests (include/hrs.h,
"ragged scrub and heal"), from the oracle alone: encode_bulk makes the
codewords, compute_error_locations judges every column that is not one, and
the demotion rule is applied here to its (ok, locations, post-call data).
Nothing comes from hrs_heal_ragged_host or from a kernel.

A batch is stored[S, n, L] (what lies in memory), valid[S, n] and, from
expect(), healed[S, n, L], the heal's reports[S, 4 + n] and the classes of its
columns. Every cell holds seeded NON-ZERO junk from its valid on, so a kernel
that reads one byte too many sees a bad column, and every byte of every cell
is compared after a heal.

Stripe kinds of batch(k, p, L):
  low   every length <= v, locations 0 and p - 1 (parity cells) at v: the
        columns from v on lie beyond every length;
  top   location n - 1 (the first Horner step) at v, both sides of the
        group-of-8 edge (locations n - 9 and n - 8) at v and another class;
  run   a dead run at the top (n - 1 and n - 2 empty), n - 3 at v;
  gap   a dead cell (n - 2) between live ones, n - 3 at v;
  zero  every length 0;
  short parity made from FULL cells, then one or two cells given a shorter
        valid than their data: the demoted columns, some with a real error in
        a live cell on top (mixed).
v runs over length_classes(L). The low / top / run / gap stripes are codewords
of their zero-filled cells, with planted columns: 1 .. p / 2 wrong bytes in
live cells (patched), p / 2 + 1 (unresolved, as the oracle decides), one of
them just below a cell's boundary and one at it; every fourth stripe is left
a codeword.
"""
import random

import numpy as np

from oracle import rs_oracle as C

WINDOW = 2048  # kWindowBytes
NONE = 0xFFFFFFFF

# one each of P = 5, 6, 7 beside the issue's codes
CODES = [(4, 1), (3, 2), (6, 3), (10, 4), (12, 4), (20, 8), (9, 5), (8, 6), (7, 7)]
WIDE = (247, 8)  # L = 2048 + 33, 2 stripes
L_BIG, L_TAIL = 2 * WINDOW + 77, 77


def length_classes(L):
    return sorted({v for v in (0, 1, 15, 16, 17, 1023, 1024, 1025, 2047, 2048, 2049, L - 1, L) if 0 <= v <= L})


def _specs(k, p, L):
    """(kind, v) per stripe."""
    if (k, p) == WIDE:
        return [("low", 1025), ("short", L - 40)]
    cl = length_classes(L)
    specs = [("low", v) for v in cl] + [("top", v) for v in cl]
    specs += [("run" if i % 2 == 0 else "gap", v) for i, v in enumerate(cl) if i % 2 == 0 or i % 4 == 1]
    specs += [("zero", 0)] + [("short", v) for v in ((min(2040, L - 47), L - 20, L - 33) if L > WINDOW else (30, 50, 60))]
    return specs


def _lengths(kind, v, k, p, L, rnd, idx):
    n = k + p
    cl = length_classes(L)
    lens = [L] * n
    if kind == "low":
        below = [x for x in cl if x <= v]
        for l in range(p, n):
            lens[l] = rnd.choice(below)
        lens[p + rnd.randrange(k)] = v if idx % 2 else lens[p]
        for l in range(p):
            lens[l] = max(lens[p:]) if l not in (0, p - 1) else v
    elif kind == "top":
        for l in range(p, n):
            lens[l] = rnd.choice(cl)
        lens[n - 1] = v
        if n >= 9 and n - 9 >= p:
            lens[n - 9], lens[n - 8] = (v, rnd.choice(cl)) if idx % 2 else (rnd.choice(cl), v)
        elif n >= 9:  # the edge lies among the parity cells: consistent only from the longest data cell on
            for l in range(p, n):
                lens[l] = min(lens[l], v)
            for l in (n - 9, n - 8):
                lens[l] = v if l < p else lens[l]
    elif kind in ("run", "gap"):
        for l in range(p, n):
            lens[l] = rnd.choice(cl)
        lens[n - 1] = 0 if kind == "run" else L
        if k >= 3:
            lens[n - 2], lens[n - 3] = 0, v
        else:
            lens[n - 2] = v
    elif kind == "zero":
        lens = [0] * n
    return lens


def _junk(rng, shape):
    return rng.integers(1, 256, shape, dtype=np.uint8)


def _oracle_column(k, p, column, c, lens):
    """(bad, resolved, blamed, post-call data, demoted, mixed) of the zero-filled
    column `column` at byte c of a stripe with the lengths `lens`."""
    ok, found, after = C.compute_error_locations(k, p, list(column))
    if ok and not found:
        return None
    err = {l: after[l] ^ column[l] for l in found}
    virtual = [l for l in found if err[l] and c >= lens[l]]
    live = [l for l in found if err[l] and c < lens[l]]
    demoted = ok and bool(virtual)
    return ok and not demoted, sorted(found), err, after, demoted, demoted and bool(live)


def expect(k, p, stored, valid, codeword, full=False):
    """(healed, reports, classes) of the stored stripes under the ragged heal
    rule. `codeword`[S, n, L]: what the zero-filled stripes are where nobody
    touched them; only columns that differ from it go through the oracle
    (full = True: every column)."""
    S, n, L = stored.shape
    zf = stored.copy()
    for s in range(S):
        for l in range(n):
            zf[s, l, valid[s, l]:] = 0
    healed = stored.copy()
    rep = np.zeros((S, 4 + n), dtype=np.uint32)
    rep[:, 2] = NONE
    classes = dict(clean=0, patched=0, unresolved=0, demoted=0, mixed=0, boundary_patched=0, beyond_bad=0)
    classes["bad"] = [[] for _ in range(S)]  # the bad columns of each stripe
    for s in range(S):
        lens = [int(x) for x in valid[s]]
        cols = range(L) if full else np.flatnonzero((zf[s] != codeword[s]).any(axis=0))
        classes["clean"] += L - len(cols)
        for c in (int(x) for x in cols):
            column = zf[s, :, c].tolist()
            got = _oracle_column(k, p, column, c, lens)
            if got is None:
                classes["clean"] += 1
                continue
            resolved, found, err, after, demoted, mixed = got
            rep[s, 0] += 1
            rep[s, 2] = min(int(rep[s, 2]), c)
            classes["bad"][s].append(c)
            if not resolved:
                rep[s, 1] += 1
                classes["demoted" if demoted else "unresolved"] += 1
                classes["mixed"] += mixed
                continue
            stores = 0
            for l in found:
                rep[s, 4 + l] += 1
                if err[l]:
                    assert c < lens[l]
                    healed[s, l, c] = after[l]
                    stores += 1
            rep[s, 3] += stores
            if stores:
                classes["patched"] += 1
                lo = c // WINDOW * WINDOW
                if c < L // WINDOW * WINDOW and any(lo < v < lo + WINDOW for v in lens):
                    classes["boundary_patched"] += 1
        # a column beyond every length whose junk would be bad if read
        most = max(lens)
        if most < L:
            c = most
            ok, found, _ = C.compute_error_locations(k, p, stored[s, :, c].tolist())
            classes["beyond_bad"] += not (ok and not found)
    return healed, rep, classes


_cache = {}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def batch(k, p, L):
    """stored, valid, healed, rep (the heal's), rep2 (a second heal's), classes, kinds; built once, read-only."""
    key = (k, p, L)
    if key in _cache:
        return _cache[key]
    n = k + p
    specs = _specs(k, p, L)
    S = len(specs)
    rng = np.random.default_rng([k, p, L, 77])
    rnd = random.Random(k * 1009 + p * 31 + L)
    valid = np.zeros((S, n), dtype=np.uint32)
    stored = np.empty((S, n, L), dtype=np.uint8)
    codeword = np.empty((S, n, L), dtype=np.uint8)
    for s, (kind, v) in enumerate(specs):
        data = rng.integers(0, 256, (k, L), dtype=np.uint8)
        if kind == "short":
            lens = [L] * n
        else:
            lens = _lengths(kind, v, k, p, L, rnd, s)
            for j in range(k):
                data[j, lens[p + j]:] = 0
        par = np.stack(C.encode_bulk(k, p, list(data)))
        codeword[s] = np.concatenate([par, data])
        for l in range(p):  # a consistent parity cell reaches at least as far as the data
            assert kind == "short" or lens[l] >= max(lens[p:]) or not par[l, lens[l]:].any()
        stored[s] = codeword[s]
        if kind == "short":  # shorter than the data the parity was made from
            cells = [p + rnd.randrange(k)] if s % 3 == 0 else [rnd.randrange(p)] if s % 3 == 1 else \
                [p + j for j in rnd.sample(range(k), 2 if p in (4, 5, 8) else 1)]
            for i, l in enumerate(cells):
                lens[l] = v - 7 * i
            if p >= 4:  # mixed: a real error in a live cell of a column that is demoted anyway
                for c in rnd.sample(range(max(lens[l] for l in cells), L), 3):
                    l = rnd.choice([x for x in range(n) if x not in cells])
                    stored[s, l, c] ^= rnd.randrange(1, 256)
        elif s % 4 != 2:  # every fourth stripe stays a codeword: clean windows between dirty ones
            cols = set(rnd.sample(range(L), min(L, 6)))
            for l in range(n):  # the last live byte of a cell and the first dead one
                if 0 < lens[l] <= L and rnd.random() < 0.5:
                    cols |= {lens[l] - 1} | ({lens[l]} if lens[l] < L else set())
            for i, c in enumerate(sorted(cols)):
                live = [l for l in range(n) if c < lens[l]]
                errors = [1, max(1, p // 2), p // 2 + 1][i % 3]
                if len(live) < errors:
                    continue
                for l in rnd.sample(live, errors):
                    stored[s, l, c] ^= rnd.randrange(1, 256)
        valid[s] = lens
        for l in range(n):
            stored[s, l, lens[l]:] = _junk(rng, L - lens[l])
    healed, rep, classes = expect(k, p, stored, valid, codeword, full=L <= L_TAIL and n <= 32)
    _, rep2, _ = expect(k, p, healed, valid, codeword)
    _cache[key] = _frozen(stored, valid, healed, rep, rep2) + (classes, [kind for kind, _ in specs])
    return _cache[key]


def all_cases():
    return [(k, p, L) for k, p in CODES for L in (L_BIG, L_TAIL)] + [(*WIDE, WINDOW + 33)]


def scrub_report(rep):
    out = np.array(rep)
    out[:, 3] = 0
    return out


def required_classes(p, L):
    """What a batch of parity size p and cells of L bytes can hold: nothing is
    patched (or demoted) at p = 1, a mixed column needs two blamed locations,
    a boundary window needs a window."""
    need = ["clean", "unresolved", "beyond_bad"]
    if p >= 2:
        need += ["patched", "demoted"] + (["boundary_patched"] if L >= WINDOW else [])
    if p >= 4:
        need += ["mixed"]
    return need


def mismatch(got, want, what):
    if np.array_equal(got, want):
        return None
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    idx = tuple(int(x) for x in bad[0])
    return f"{what}: {len(bad)} entries differ, first at {idx}: got {int(got[idx])}, want {int(want[idx])}"
