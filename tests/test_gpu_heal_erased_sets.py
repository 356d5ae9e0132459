"""Heal with known erasures over every erased set (tests/heal_erased_sets.py):
one stripe per set, all sets of a code in one batch, one call per case, every
comparison exact. RS(10,4), RS(6,3), RS(3,2) and RS(4,1) run every subset of
size 0 .. p; RS(6,5), RS(7,6), RS(10,7) and RS(20,8) every set of size <= 2,
40 seeded sets of each larger size and the sets that move the spare row or
empty a load group; RS(247,8) a list around the mask-word edges.

  1. hrs_heal_erased_dev within capacity, kernel modes 0 and 2;
  2. the same call one error past capacity;
  3. hrs_heal_erased_crc_dev pinned to the fused kernel (mode 3) at L = 2048;
  4. hrs_repair_checked_dev from checksums alone, so that the device's pattern
     builder (repair::fill_pattern in repair_plan_kernel) makes every pattern.

At p <= 4 within capacity the expected bytes are the oracle-encoded stripes and
the reports the counts of the planted list; otherwise the byte-exact reference
is hrs_heal_erased_host. The expectations of 4 come from the oracle, zlib and
the planted list alone. The CPU tests at the top check the inputs without a
device."""
import itertools
from math import comb

import numpy as np
import pytest

import heal_erased_inputs as H
import heal_erased_sets as ES
import repair_checked_inputs as R
from lambdafs_amd import HipReedSolomonCode, device
from test_gpu_heal_erased import _aligned, _u32
from test_gpu_heal_erased_crc import call

NONE_DEV = -2  # HRS_DEVICE_NONE
ALL = ES.EXHAUSTIVE + ES.SAMPLED + [ES.WIDEST]
PAST = [(10, 4), (6, 3), (6, 5), (20, 8)]
FUSED = [(10, 4), (6, 3), (3, 2)]
CHECKED = ES.EXHAUSTIVE + [(6, 5), (10, 7), (20, 8)]
JOINED = [(10, 4), (6, 3)]

_refs = {}


def host_reference(c):
    """hrs_heal_erased_host over the case's stripes, once; one code's at a time."""
    key = (c.k, c.p, c.length, c.over)
    if key not in _refs:
        if any(r[:2] != (c.k, c.p) for r in _refs):
            _refs.clear()
        _refs[key] = H.host_reference(HipReedSolomonCode(c.k, c.p, device=NONE_DEV), c.bad, c.sets)
    return _refs[key]


def expected(c):
    """(bytes after, reports) of a heal of the case."""
    if c.p <= 4 and not c.over:
        return c.clean, c.planted_reports()
    return host_reference(c)


def modes(codes, values=(0, 2)):
    """Cases code by code, so that a code's inputs are built once."""
    return [(k, p, m) for k, p in codes for m in values]


# ---- the inputs, no device

@pytest.mark.parametrize("k,p", ALL)
def test_set_lists_are_the_enumeration(k, p):
    n = k + p
    sets = ES.erased_sets(k, p)
    assert all(e == sorted(set(e)) and len(e) <= p and all(0 <= l < n for l in e) for e in sets)
    assert len({tuple(e) for e in sets}) == len(sets)  # no set twice
    if (k, p) in ES.EXHAUSTIVE:
        assert len(sets) == sum(comb(n, e) for e in range(p + 1)) == {(10, 4): 1471, (6, 3): 130, (3, 2): 16, (4, 1): 6}[k, p]
        assert sets == [list(c) for e in range(p + 1) for c in itertools.combinations(range(n), e)]
    elif (k, p) in ES.SAMPLED:
        small = 1 + n + comb(n, 2)
        named = [list(range(p)), list(range(n - p, n))] + ([list(range(8, 16))] if (k, p) == (20, 8) else [])
        assert sets[:small] == [list(c) for e in range(3) for c in itertools.combinations(range(n), e)]
        assert [len(e) for e in sets[small:small + 40 * (p - 2)]] == [e for e in range(3, p + 1) for _ in range(40)]
        assert sets[small + 40 * (p - 2):] == named
    else:
        fixed = [[31, 32], [63, 64], [30, 31, 32, 33], [254], [0, 254], list(range(247, 255)), list(range(8)),
                 [95, 96, 127, 128, 159, 160, 191, 192]]
        assert sets[:len(fixed)] == fixed and len(sets) == len(fixed) + 10 and all(sets)
    if (k, p) != ES.WIDEST:  # every location is the lowest and the highest member of some set
        assert {e[0] for e in sets if e} == {e[-1] for e in sets if e} == set(range(n))
    assert ES.erased_sets(k, p) == sets  # seeded


@pytest.mark.parametrize("k,p", ALL)
def test_inputs_within_capacity(k, p):
    """The batch is what the module says, and hrs_heal_erased_host restores
    it: at p <= 4 every stripe to the oracle's bytes with exactly the planted
    reports; at p > 4 all but the unresolved columns, which stay within the
    project's cap of 5 % of the planted ones, and a stripe without one is the
    oracle's again. Measured: none of 355 planted columns at RS(6,5), none of
    570 at RS(7,6), none of 910 at RS(10,7), 6 of 1,890 (0.32 %) at RS(20,8),
    none of 40 at RS(247,8)."""
    n = k + p
    c = ES.case(k, p)
    assert c.clean.shape == c.bad.shape == (c.S, n, ES.L) and ES.L == 2048 + 33
    assert (c.clean[ES.BASE:] == c.clean[:-ES.BASE]).all() and len({c.clean[s].tobytes() for s in range(min(c.S, 8))}) == min(c.S, 8)
    for s in range(min(c.S, ES.BASE)):  # the oracle's codewords
        ref = H.C.encode_bulk(k, p, [c.clean[s, p + j] for j in range(k)])
        assert all((c.clean[s, r] == ref[r]).all() for r in range(p))
    touched = np.zeros(c.bad.shape, dtype=bool)
    for s, e in enumerate(c.sets):
        assert (c.bad[s, e] == H.FILL).all()
        touched[s, e] = True
        # an erased cell is doubted by its checksum
        assert all(ES.crc(c.bad[s, l]) != c.clean_crcs[s, l] == ES.crc(c.clean[s, l]) for l in e)
    cols = set(ES.columns_of(ES.L))
    assert cols == {0, 1023, 2047, 2048, ES.L - 1}
    for s, col, errs in c.planted:
        assert s % 3 and col in cols and 1 <= len(errs) <= (p - len(c.sets[s])) // 2 and not set(errs) & set(c.sets[s])
        for l, x in errs.items():
            assert c.bad[s, l, col] == c.clean[s, l, col] ^ x and x
            touched[s, l, col] = True
    assert (c.bad[~touched] == c.clean[~touched]).all()
    # every stripe with capacity that is not a quiet one is planted at every column
    want = {(s, col) for s, e in enumerate(c.sets) if s % 3 and (p - len(e)) // 2 >= 1 for col in cols}
    assert {(s, col) for s, col, _ in c.planted} == want
    after, reps = host_reference(c)
    wrong = int((after != c.clean).any(axis=1).sum())
    assert wrong == int(reps[:, 1].sum())
    print(f"RS({k},{p}): {c.S} sets, {len(c.planted)} planted columns, {wrong} unresolved on the host")
    if p <= 4:
        assert (after == c.clean).all() and reps.tolist() == c.planted_reports().tolist()
    else:
        assert wrong * 20 <= len(c.planted)
        solved = reps[:, 1] == 0  # a stripe without an unresolved column is the oracle's, its bad columns the planted ones
        assert (after[solved] == c.clean[solved]).all() and (reps[solved, :4] == c.planted_reports()[solved, :4]).all()
        print("  sets with an unresolved column:", [c.sets[s] for s in np.flatnonzero(~solved)])


@pytest.mark.parametrize("k,p", PAST)
def test_inputs_one_past_capacity(k, p):
    """Every stripe with a spare syndrome (e < p) that is not a quiet one gets
    one error more than it can correct in every planted column, and the host
    leaves at least one of them unresolved: the sets with e = p - 1 reach the
    locator with their own gamma."""
    c = ES.case(k, p, over=1)
    planted = {s for s, _, _ in c.planted}
    assert planted == {s for s, e in enumerate(c.sets) if s % 3 and len(e) < p}
    assert any(len(c.sets[s]) == p - 1 for s in planted)
    for s, _, errs in c.planted:
        assert len(errs) == min((p - len(c.sets[s])) // 2 + 1, k + p - len(c.sets[s]))
    _, reps = host_reference(c)
    assert all(reps[s, 1] > 0 for s in planted)


def test_fused_inputs():
    """L = 2048: the planted columns are the window's own, all within it."""
    assert ES.columns_of(ES.L_FUSED) == [0, 1023, 2047] and ES.L_FUSED == H.WINDOW
    c = ES.case(3, 2, ES.L_FUSED)
    assert c.bad.shape == (16, 5, 2048)


# ---- 1 and 2: hrs_heal_erased_dev

def _heal(torch, c, mode):
    code = HipReedSolomonCode(c.k, c.p, device=0)
    code.setKernelMode(mode)
    st = _aligned(torch, c.bad)
    reports = _u32(device.heal_erased_stripes(code, st, c.erased()))
    assert code.lastKernel() == (f"heal_erased_kernel<{c.p}>" if mode == 0 else f"heal_erased_bytewise_kernel<{c.p}>")
    return st.cpu().numpy(), reports


def _same(got, reports, after, reps, c):
    bad = np.flatnonzero((got != after).any(axis=(1, 2)) | (reports != reps).any(axis=1))
    assert bad.size == 0, [(int(s), c.sets[s]) for s in bad[:6]]


@pytest.mark.gpu
@pytest.mark.parametrize("k,p,mode", modes(ALL))
def test_every_set_heals(cuda, k, p, mode):
    c = ES.case(k, p)
    after, reps = expected(c)
    got, reports = _heal(cuda, c, mode)
    _same(got, reports, after, reps, c)


@pytest.mark.gpu
@pytest.mark.parametrize("k,p,mode", modes(PAST))
def test_every_set_one_past_capacity(cuda, k, p, mode):
    c = ES.case(k, p, over=1)
    after, reps = host_reference(c)
    got, reports = _heal(cuda, c, mode)
    _same(got, reports, after, reps, c)


# ---- 3: the fused CRC kernel

@pytest.mark.gpu
@pytest.mark.parametrize("k,p,running", modes(FUSED, (False, True)))
def test_every_set_fused_crc(cuda, k, p, running):
    torch = cuda
    c = ES.case(k, p, ES.L_FUSED)
    after, reps = expected(c)
    assert after is c.clean
    start = np.random.default_rng(k + p).integers(0, 1 << 32, (c.S, c.n), dtype=np.uint32) if running else None
    code = HipReedSolomonCode(k, p, device=0)
    code.setKernelMode(3)
    st = _aligned(torch, c.bad)
    rep, crcs = call(torch, code, st, c.sets, start)
    assert code.lastKernel() == f"heal_erased_crc_kernel<{p}>"
    _same(st.cpu().numpy(), rep, after, reps, c)
    if running:  # zlib over the clean cells, continued from the running CRCs
        want = np.array([[ES.crc(c.clean[s, l], start[s, l]) for l in range(c.n)] for s in range(c.S)], dtype=np.uint32)
    else:
        want = c.clean_crcs
    bad = np.flatnonzero((crcs != want).any(axis=1))
    assert bad.size == 0, [(int(s), c.sets[s]) for s in bad[:6]]


# ---- 4: checked repair, the device builds the patterns

def _checked(torch, c, mode, join):
    code = HipReedSolomonCode(c.k, c.p, device=0)
    code.setKernelMode(mode)
    st = _aligned(torch, c.bad)  # a 16-byte row pitch: mode 0 runs the window kernels and the byte-granular tail
    stored = torch.from_numpy(c.stored().view(np.int32)).to("cuda:0")
    verdicts, erased, reports, crcs = device.repair_checked_stripes(code, st, stored, join_syndromes=join)
    torch.cuda.synchronize()
    # pass 1's kernel, as hrs_scrub_crc_dev names it: L = 2048 + 33 is no fused shape
    assert code.lastKernel() == (f"scrub_kernel<{c.p}>" if mode == 0 else f"scrub_bytewise_kernel<{c.p}>")
    return st.cpu().numpy(), _u32(verdicts), erased.cpu().numpy(), _u32(reports), _u32(crcs)


def _first(c, *pairs):
    """Asserts got == want for every pair, naming the first sets that differ."""
    for what, got, want in pairs:
        assert np.shape(got) == np.shape(want), what
        got, want = np.asarray(got).reshape(c.S, -1), np.asarray(want).reshape(c.S, -1)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (what, [(int(s), c.sets[s], got[s].tolist()[:12], want[s].tolist()[:12]) for s in bad[:4]])


def _checked_host(c, stored, join, stripes):
    """hrs_repair_checked_host on the named stripes: {stripe: (verdict, erased, bytes, report, crcs)}."""
    code = HipReedSolomonCode(c.k, c.p, device=NONE_DEV)
    out = {}
    for s in stripes:
        rows = [c.bad[s, l].copy() for l in range(c.n)]
        v, e, r, crcs = device.repair_checked_host(code, rows, stored[s], join)
        out[int(s)] = (v, e, np.stack(rows), r, crcs)
    return out


def _checked_expectation(c):
    """(verdicts, erased_out, bytes, reports, crc_out) with checksums alone,
    from the oracle, zlib and the planted list: RESTAMP for a stripe with
    planted survivors (its restamped cells differ once they are fixed), CLEAN
    for the empty set with clean survivors, REPAIRED for every other stripe;
    the clean stripes and their CRCs. At p > 4 the reports are
    hrs_heal_erased_host's, and the few stripes in which it leaves a column
    unresolved take hrs_repair_checked_host's results whole."""
    planted = {s for s, _, _ in c.planted}
    assert c.sets[0] == [] and 0 not in planted
    verdicts = np.array([R.RESTAMP if s in planted else R.REPAIRED if c.sets[s] else R.CLEAN for s in range(c.S)],
                        dtype=np.uint32)
    erased, after, crcs = c.erased(c.p), c.clean, c.clean_crcs
    if c.p <= 4:
        return verdicts, erased, after, c.planted_reports(), crcs
    reps = np.array(host_reference(c)[1])
    hard = np.flatnonzero(reps[:, 1])
    assert hard.size * 20 <= len(planted)
    if hard.size:
        after, crcs = np.array(after), np.array(crcs)
        for s, (v, e, rows, r, cr) in _checked_host(c, c.stored(), False, hard).items():
            verdicts[s], erased[s], after[s], reps[s], crcs[s] = v, e, rows, r, cr
    return verdicts, erased, after, reps, crcs


@pytest.mark.parametrize("k,p", CHECKED)
def test_checked_expectations_hold_on_the_host(k, p):
    """No device: hrs_repair_checked_host gives the expectation for every set,
    and all three verdicts occur."""
    c = ES.case(k, p)
    verdicts, erased, after, reps, crcs = _checked_expectation(c)
    assert set(verdicts.tolist()) >= ({R.CLEAN, R.REPAIRED, R.RESTAMP} if p >= 3 else {R.CLEAN, R.REPAIRED})
    ref = _checked_host(c, c.stored(), False, range(c.S))
    _first(c, *((what, np.stack([np.asarray(ref[s][i]) for s in range(c.S)]), want) for i, (what, want) in enumerate(
        (("verdicts", verdicts), ("erased_out", erased), ("bytes", after), ("reports", reps), ("crc_out", crcs)))))


@pytest.mark.gpu
@pytest.mark.parametrize("k,p,mode", modes(CHECKED))
def test_every_set_checked_repair(cuda, k, p, mode):
    """Checksums alone: the doubted cells are exactly the erased set, which the
    plan kernel turns into the stripe's pattern on the device. A stripe with
    planted survivors comes back RESTAMP (its restamped cells now differ), the
    empty set with clean survivors CLEAN, every other stripe REPAIRED."""
    c = ES.case(k, p)
    verdicts, erased, after, reps, crcs = _checked_expectation(c)
    got, gv, ge, gr, gc = _checked(cuda, c, mode, False)
    _first(c, ("verdicts", gv, verdicts), ("erased_out", ge, erased), ("bytes", got, after), ("reports", gr, reps),
           ("crc_out", gc, crcs))


@pytest.mark.gpu
@pytest.mark.parametrize("k,p", JOINED)
def test_every_set_checked_repair_joined(cuda, k, p):
    """With the syndromes joined the doubted cells are the erased set and what
    pass 1's locator blamed: against hrs_repair_checked_host stripe by stripe,
    whatever verdict it gives."""
    c = ES.case(k, p)
    ref = _checked_host(c, c.stored(), True, range(c.S))
    verdicts, erased, out, reps, crcs = (np.stack([np.asarray(ref[s][i]) for s in range(c.S)]) for i in range(5))
    assert len(set(verdicts.tolist())) >= 2
    got, gv, ge, gr, gc = _checked(cuda, c, 0, True)
    _first(c, ("verdicts", gv, verdicts), ("erased_out", ge, erased), ("bytes", got, out), ("reports", gr, reps),
           ("crc_out", gc, crcs))
