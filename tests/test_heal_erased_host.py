"""CPU tests of heal with known erasures: hrs_heal_erased_host (one stripe on
the host through the code the kernels run, host-only handles) against a
pure-Python restatement of the rule in include/hrs.h (syndromes of the
survivors, modified syndromes, the reference locator with its elimination
quirks, the Vandermonde solve), written on its own and sharing nothing with
the product; the argument rules of both entry points; the CPU program. No GPU
call runs here."""
import os
import random
import subprocess

import numpy as np
import pytest

from lambdafs_amd import HipReedSolomonCode, _lib, device
from oracle import rs_oracle as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = -2  # HRS_DEVICE_NONE
SCRUB_NONE = 0xFFFFFFFF

# ---- GF(2^8), polynomial 0x11D, alpha = 2
EXP, LOG = [0] * 510, [0] * 256
_v = 1
for _i in range(255):
    EXP[_i] = EXP[_i + 255] = _v
    LOG[_v] = _i
    _v <<= 1
    if _v & 0x100:
        _v ^= 0x11D


def mul(a, b):
    return 0 if a == 0 or b == 0 else EXP[LOG[a] + LOG[b]]


def div(a, b):
    """a / b with the reference's a / 0 = 0."""
    return 0 if a == 0 or b == 0 else EXP[LOG[a] + 255 - LOG[b]]


def apow(e):
    return EXP[e % 255]


def vandermonde_solve(xs, ys):
    """v with sum_j v[j] xs[j]^i = ys[i], i < len(xs) (GaloisField.solveVandermondeSystem)."""
    m = len(xs)
    v = list(ys[:m])
    for i in range(m - 1):
        for j in range(m - 1, i, -1):
            v[j] ^= mul(xs[i], v[j - 1])
    for i in range(m - 1, -1, -1):
        for j in range(i + 1, m):
            v[j] = div(v[j], xs[j] ^ xs[j - i - 1])
        for j in range(i, m - 1):
            v[j] ^= v[j + 1]
    return v


def locate(n, syn):
    """computeErrorLocations on len(syn) syndromes over n locations:
    (returned boolean, locations ascending, error values)."""
    p = len(syn)
    t, w = p // 2, p // 2 + 1
    m = [[syn[i + j] for j in range(w)] for i in range(t)]
    for i in range(t):  # the row-wise pivot search of GaloisField.gaussianElimination
        piv = next((j for j in range(i, t) if m[i][j] != 0), None)
        if piv is None:
            continue
        m[i], m[piv] = m[piv], m[i]
        pivot = m[i][i]
        for c in range(i, w):
            m[i][c] = div(m[i][c], pivot)
        for r in range(i + 1, t):
            lead = m[r][i]
            for c in range(i, w):
                m[r][c] ^= mul(lead, m[i][c])
    for i in range(t - 1, -1, -1):
        for r in range(i):
            lead = m[r][i]
            for c in range(i, w):
                m[r][c] ^= mul(lead, m[i][c])
    poly = [1] + [m[t - 1 - i][t] for i in range(t)]
    locs = []
    for l in range(n):
        root, v, y = EXP[255 - l], 0, 1
        for c in poly:
            v ^= mul(c, y)
            y = mul(root, y)
        if v == 0 and len(locs) < 4:
            locs.append(l)
    if not locs:
        return False, [], []
    err = vandermonde_solve([apow(l) for l in locs], syn)
    for i in range(p):
        v = syn[i]
        for l, e in zip(locs, err):
            v ^= mul(e, apow(l * i))
        if v:
            return False, locs, err
    return True, locs, err


def heal_erased_expected(k, p, stripe, erased):
    """(stripe after the call [n, L], report [4 + n]) by steps 1-5 of include/hrs.h."""
    n = k + p
    E = sorted(erased)
    e, pp = len(E), p - len(E)
    gamma = [1]
    for m in E:  # times (1 + alpha^m x)
        gamma = [a ^ mul(b, apow(m)) for a, b in zip(gamma + [0], [0] + gamma)]
    want = stripe.copy()
    rep = [0, 0, SCRUB_NONE, 0] + [0] * n
    for c in range(stripe.shape[1]):
        d = [0 if l in E else int(stripe[l, c]) for l in range(n)]
        S = [0] * p
        for i in range(p):
            for l in range(n):
                S[i] ^= mul(apow(i * l), d[l])
        T = [0] * pp
        for i in range(pp):
            for j in range(e + 1):
                T[i] ^= mul(gamma[j], S[i + e - j])
        if any(T):
            rep[0] += 1
            rep[2] = min(rep[2], c)
            ok, locs, errs = locate(n, T) if pp >= 2 else (False, [], [])
            if ok and not set(locs) & set(E):
                for l, err in zip(locs, errs):
                    scale = 1
                    for m in E:
                        scale = mul(scale, apow(l) ^ apow(m))
                    u = div(err, scale)
                    rep[4 + l] += 1
                    if u:
                        want[l, c] ^= u
                        rep[3] += 1
                    for i in range(p):
                        S[i] ^= mul(u, apow(l * i))
            else:
                rep[1] += 1
        for m, v in zip(E, vandermonde_solve([apow(m) for m in E], S)):
            want[m, c] = v
    return want, rep


def _codewords(k, p, L, rnd):
    cols = []
    for _ in range(L):
        msg = [rnd.randrange(256) for _ in range(k)]
        cols.append(C.encode(k, p, msg) + msg)
    return np.array(cols, dtype=np.uint8).T.copy()


def _damaged(k, p, L, e, rnd):
    """(stripe [n, L], clean, erased, per-column error counts): column c carries
    c % (cap + 2) survivor errors, cap = (p - e) // 2, so 0 .. one past capacity."""
    n = k + p
    clean = _codewords(k, p, L, rnd)
    erased = rnd.sample(range(n), e)
    stripe = clean.copy()
    stripe[erased, :] = 0xA5
    cap = (p - e) // 2
    counts = [min(c % (cap + 2), n - e) for c in range(L)]
    rnd.shuffle(counts)
    survivors = [l for l in range(n) if l not in erased]
    for c, t in enumerate(counts):
        for l in rnd.sample(survivors, t):
            stripe[l, c] ^= rnd.randrange(1, 256)
    return stripe, clean, erased, counts


def _call(code, stripe, erased):
    rows = [stripe[l].copy() for l in range(stripe.shape[0])]
    rep = device.heal_erased_host(code, rows, erased)
    return np.stack(rows), [int(x) for x in rep]


SHAPES = [(10, 4), (6, 3), (3, 2), (20, 8), (6, 5), (7, 6), (10, 7)]


@pytest.mark.parametrize("k,p", SHAPES)
def test_heal_erased_host_matches_the_restatement(k, p):
    n, L = k + p, 257
    code = HipReedSolomonCode(k, p, device=NONE)
    rnd = random.Random(7919 * k + p)
    seen_unresolved = False
    for e in range(p + 1):
        stripe, clean, erased, counts = _damaged(k, p, L, e, rnd)
        want, want_rep = heal_erased_expected(k, p, stripe, erased)
        got, rep = _call(code, stripe, erased)
        assert rep == want_rep, (e, erased)
        assert (got == want).all(), (e, erased)
        cap = (p - e) // 2
        within = np.array([t <= cap for t in counts])
        if p <= 4:  # every column within capacity is the codeword again
            assert (got[:, within] == clean[:, within]).all()
            assert rep[1] <= int((~within).sum())
        assert all(rep[4 + l] == 0 for l in erased)
        seen_unresolved |= rep[1] > 0
        # past capacity no survivor of an unresolved column moves: nothing but
        # the blamed bytes and the erased cells changed
        changed = got != stripe
        changed[erased, :] = False
        assert int(changed.sum()) == rep[3]
    assert seen_unresolved


def test_heal_erased_host_nothing_erased_is_heal_host():
    k, p, L = 10, 4, 257
    rnd = random.Random(3)
    stripe, _, _, _ = _damaged(k, p, L, 0, rnd)
    code = HipReedSolomonCode(k, p, device=NONE)
    got, rep = _call(code, stripe, [])
    rows = [stripe[l].copy() for l in range(k + p)]
    hrep = device.heal_host(code, rows)
    assert (np.stack(rows) == got).all() and [int(x) for x in hrep] == rep
    assert rep[0] > rep[1] > 0 and rep[3] > 0


def test_heal_erased_calls_check_arguments_before_the_device():
    lib = _lib.lib()
    k, p, L, ns = 3, 2, 64, 2
    n = k + p
    code = HipReedSolomonCode(k, p, device=NONE)
    h = code._h
    buf = np.zeros((ns, n, L), dtype=np.uint8)
    rep = np.zeros((ns, 4 + n), dtype=np.uint32)
    rows = _lib.ptr_array([buf.ctypes.data + l * L for l in range(n)])

    def dev(handle, rws, erased, max_erased, length=L, stripes=ns, stride=4 + n):
        arr = np.ascontiguousarray(np.array(erased, dtype=np.int32).reshape(-1))
        return lib.hrs_heal_erased_dev(handle, rws, n * L, length, stripes, arr.ctypes.data, max_erased,
                                       rep.ctypes.data, stride, None)

    def host(handle, rws, erased, num=None, length=L):
        return lib.hrs_heal_erased_host(handle, rws, length, _lib.int_array(erased), len(erased) if num is None else num,
                                        rep.ctypes.data)

    ok = [[0, -1], [4, 1]]
    # the scrub's code rules
    from lambdafs_amd import HipNativeReedSolomonCode
    nrs = HipNativeReedSolomonCode(k, p, device=NONE)
    assert dev(nrs._h, rows, ok, 2) == _lib.HRS_EINVAL and b"rs code only" in lib.hrs_last_error(nrs._h)
    assert host(nrs._h, rows, [0]) == _lib.HRS_EINVAL
    wide = HipReedSolomonCode(3, 9, device=NONE)
    wbuf = np.zeros((1, 12, L), dtype=np.uint8)
    wrows = _lib.ptr_array([wbuf.ctypes.data + l * L for l in range(12)])
    assert host(wide._h, wrows, [0]) == _lib.HRS_EINVAL and b"parity_size <= 8" in lib.hrs_last_error(wide._h)
    # too many erasures in one stripe
    assert dev(h, rows, [[0, -1, -1], [0, 1, 2]], 3) == _lib.HRS_ETOOMANY
    assert b"stripe 1" in lib.hrs_last_error(h)
    assert host(h, rows, [0, 1, 2]) == _lib.HRS_ETOOMANY
    # a location outside [0, n), a repeated one, a negative max_erased
    assert dev(h, rows, [[0, -1], [n, -1]], 2) == _lib.HRS_EINVAL and b"outside" in lib.hrs_last_error(h)
    assert host(h, rows, [n]) == _lib.HRS_EINVAL
    assert dev(h, rows, [[0, -1], [3, 3]], 2) == _lib.HRS_EINVAL and b"twice" in lib.hrs_last_error(h)
    assert host(h, rows, [3, 3]) == _lib.HRS_EINVAL
    assert dev(h, rows, ok, -1) == _lib.HRS_EINVAL
    assert host(h, rows, [0], num=-1) == _lib.HRS_EINVAL
    # rows: NULL, equal; a short report stride
    holed = _lib.ptr_array([None if l == 1 else buf.ctypes.data + l * L for l in range(n)])
    assert dev(h, holed, ok, 2) == _lib.HRS_EINVAL and b"row 1 is NULL" in lib.hrs_last_error(h)
    twice = _lib.ptr_array([buf.ctypes.data + (0 if l == 3 else l) * L for l in range(n)])
    assert dev(h, twice, ok, 2) == _lib.HRS_EINVAL and b"rows 0 and 3 are one pointer" in lib.hrs_last_error(h)
    assert host(h, twice, [0]) == _lib.HRS_EINVAL
    assert dev(h, rows, ok, 2, stride=4 + n - 1) == _lib.HRS_EINVAL and b"report_stride" in lib.hrs_last_error(h)
    # the erasure lists are checked even for an empty job, which then touches nothing
    assert dev(h, rows, [[0, -1], [3, 3]], 2, length=0) == _lib.HRS_EINVAL
    assert dev(h, rows, ok, 2, length=0) == _lib.HRS_OK
    assert dev(h, rows, ok, 2, stripes=0) == _lib.HRS_OK
    assert host(h, rows, [0], length=0) == _lib.HRS_OK
    assert not rep.any() and not buf.any()
    # good arguments: no device behind this handle, with and without erasures
    assert dev(h, rows, ok, 2) == _lib.HRS_EDEVICE
    assert dev(h, rows, ok, 0) == _lib.HRS_EDEVICE
    assert not rep.any()
    # while the host form runs on it (all-zero columns are codewords); a list ends at the first negative entry
    buf[0, 4] = 0xA5
    assert host(h, rows, [4, -1, 77]) == _lib.HRS_OK
    assert rep[0].tolist() == [0, 0, SCRUB_NONE, 0] + [0] * n and not buf.any()


def test_heal_erased_logic_program():
    """tests/cpp/heal_erased_logic.cpp: uniqueness, capacity at p <= 4 and e = 0
    against hrs_heal_host over seeded columns up to n = 255 (also part of the
    `make asan` run)."""
    exe = os.path.join(ROOT, "tests", "cpp", "heal_erased_logic")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", ROOT, "tests/cpp/heal_erased_logic"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "heal_erased_logic: 0 mismatches" in out.stdout


def test_abi_name_sets_agree():
    """The new entry points are declared, bound and exported."""
    import ctypes
    import re
    src = open(os.path.join(ROOT, "include", "hrs.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(hrs_[a-z0-9_]+)\s*\(", src))
    assert {"hrs_heal_erased_dev", "hrs_heal_erased_host"} <= declared
    assert declared == set(_lib.EXPORTS)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(lib, name) for name in declared)
    hpp = open(os.path.join(ROOT, "include", "hrs.hpp")).read()
    assert "hrs_heal_erased_dev(" in hpp and "hrs_heal_erased_host(" in hpp


def test_library_holds_the_heal_erased_kernels():
    blob = open(_lib.LIB_PATH, "rb").read()
    for p in range(1, 9):
        assert b"heal_erased_kernelILi%dEE" % p in blob
        assert b"heal_erased_bytewise_kernelILi%dEE" % p in blob
