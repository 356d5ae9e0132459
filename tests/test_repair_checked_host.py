"""CPU tests of checked repair: hrs_repair_checked_host (one stripe on the host,
host-only handles) against the Python restatement of the rule in
tests/repair_checked_inputs.py (zlib CRCs, device.heal_host on a copy, steps
1-3 in Python, device.heal_erased_host, step 6); agreement of erased_out with
device.checksums_to_erased; all six verdicts; the whole-cell contrast between
the two modes; the argument rules of both entry points; the CPU program. No
GPU call runs here."""
import os
import subprocess

import numpy as np
import pytest

import repair_checked_inputs as R
from lambdafs_amd import HipReedSolomonCode, _lib, device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = -2  # HRS_DEVICE_NONE
LENGTHS = [100, 2 * 2048 + 80]


def _call(code, stripe, stored, join):
    rows = [np.ascontiguousarray(stripe[l]).copy() for l in range(stripe.shape[0])]
    v, e, r, c = device.repair_checked_host(code, rows, stored, join_syndromes=join)
    return np.stack(rows), v, e, r, c


@pytest.mark.parametrize("join", [False, True])
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("k,p", R.CODES)
def test_repair_checked_host_equals_the_restatement(k, p, L, join):
    code = HipReedSolomonCode(k, p, device=NONE)
    n = k + p
    for kind in R.KINDS:
        for seed in range(2):
            made = R.recipe(kind, k, p, L, seed)
            if made is None:
                continue
            stripe, stored = made
            got, v, e, r, c = _call(code, stripe, stored, join)
            rows = [stripe[l].copy() for l in range(n)]
            wv, we, wr, wc, listed, (c1, r1) = R.restate(code, rows, stored, join)
            what = f"RS({k},{p}) L={L} join={join} {kind} seed {seed}"
            print(what, "verdict", v, "restated", wv, "erased", e.tolist())
            assert v == wv, what
            assert (got == np.stack(rows)).all(), what
            assert e.tolist() == we.tolist() and r.tolist() == wr.tolist() and c.tolist() == wc.tolist(), what
            if listed:  # the rule checksums_to_erased states, on pass 1's values
                want = device.checksums_to_erased(c1[None], stored[None], p, r1[None] if join else None)[0]
                assert e.tolist() == want.tolist(), what
            else:  # never written
                assert (got == stripe).all() and (e == -1).all(), what
            if not join and p >= 2 and kind in R.EXPECTED:
                assert v == R.EXPECTED[kind], what


def test_all_six_verdicts_occur():
    """A condition on the inputs: over the recipes every verdict is produced
    (checked on the restatement, so it holds whatever the call does)."""
    seen = set()
    for k, p in R.CODES:
        code = HipReedSolomonCode(k, p, device=NONE)
        for kind in R.KINDS:
            made = R.recipe(kind, k, p, 100)
            if made is None:
                continue
            stripe, stored = made
            for join in (False, True):
                seen.add(R.restate(code, [stripe[l].copy() for l in range(k + p)], stored, join)[0])
    assert seen == {R.CLEAN, R.REPAIRED, R.RESTAMP, R.FAILED, R.TOOMANY, R.AMBIGUOUS}


def test_whole_cell_garbage_contrasts_the_two_modes():
    """Three cells of whole-cell garbage at RS(10,4), inside the code's
    capacity: checksums alone repair the stripe byte-exact; with the syndromes
    joined the verdict is whatever the restatement says (the locator blames
    sound cells in the columns it mis-resolves)."""
    k, p, L = 10, 4, 2 * 2048 + 80
    code = HipReedSolomonCode(k, p, device=NONE)
    good, _ = R.clean(k, p, L, 0)
    stripe, stored = R.recipe("garbage3", k, p, L, 0)
    got, v, e, r, c = _call(code, stripe, stored, False)
    assert v == R.REPAIRED and (got == good).all() and e.tolist() == [1, 5, 12, -1]
    assert c.tolist() == stored.tolist()
    got, v, e, r, c = _call(code, stripe, stored, True)
    rows = [stripe[l].copy() for l in range(k + p)]
    wv = R.restate(code, rows, stored, True)[0]
    print("join mode on three garbage cells: verdict", v, "erased", e.tolist())
    assert v == wv and (got == np.stack(rows)).all()


def test_repair_checked_calls_check_arguments_before_the_device():
    lib = _lib.lib()
    k, p, L, ns = 3, 2, 64, 2
    n = k + p
    code = HipReedSolomonCode(k, p, device=NONE)
    h = code._h
    buf = np.zeros((ns, n, L), dtype=np.uint8)
    rep = np.zeros((ns, 4 + n), dtype=np.uint32)
    crcs = np.zeros((ns, n + 1), dtype=np.uint32).reshape(-1)  # room to shift stored against crc_out
    stored = np.zeros(ns * n, dtype=np.uint32)
    verdicts = np.full(ns, 77, dtype=np.uint32)
    erased = np.full((ns, p), 77, dtype=np.int32)
    rows = _lib.ptr_array([buf.ctypes.data + l * L for l in range(n)])

    def dev(handle, rws, flags=0, length=L, stripes=ns, stride=4 + n, st=stored.ctypes.data, vd=verdicts.ctypes.data,
            rp=rep.ctypes.data, co=crcs.ctypes.data, er=erased.ctypes.data):
        return lib.hrs_repair_checked_dev(handle, rws, n * L, length, stripes, st, flags, vd, er, rp, stride, co, None)

    def host(handle, rws, flags=0, length=L, st=stored.ctypes.data, vd=verdicts.ctypes.data, rp=rep.ctypes.data,
             co=crcs.ctypes.data):
        return lib.hrs_repair_checked_host(handle, rws, length, st, flags, vd, erased.ctypes.data, rp, co)

    def untouched():
        return not rep.any() and not crcs.any() and (verdicts == 77).all() and (erased == 77).all() and not buf.any()

    # the scrub's code rules
    from lambdafs_amd import HipNativeReedSolomonCode
    nrs = HipNativeReedSolomonCode(k, p, device=NONE)
    assert dev(nrs._h, rows) == _lib.HRS_EINVAL and b"rs code only" in lib.hrs_last_error(nrs._h)
    assert host(nrs._h, rows) == _lib.HRS_EINVAL
    # rows: NULL, equal; a short report stride
    holed = _lib.ptr_array([None if l == 1 else buf.ctypes.data + l * L for l in range(n)])
    assert dev(h, holed) == _lib.HRS_EINVAL and b"row 1 is NULL" in lib.hrs_last_error(h)
    twice = _lib.ptr_array([buf.ctypes.data + (0 if l == 3 else l) * L for l in range(n)])
    assert dev(h, twice) == _lib.HRS_EINVAL and b"rows 0 and 3 are one pointer" in lib.hrs_last_error(h)
    assert host(h, twice) == _lib.HRS_EINVAL
    assert dev(h, rows, stride=4 + n - 1) == _lib.HRS_EINVAL and b"report_stride" in lib.hrs_last_error(h)
    # a flag bit other than bit 0, also on an empty call (argument errors come first)
    for bad in (2, 3, 4, 1 << 30, -2):
        assert dev(h, rows, flags=bad) == _lib.HRS_EINVAL and b"flags" in lib.hrs_last_error(h)
        assert host(h, rows, flags=bad) == _lib.HRS_EINVAL
    assert dev(h, rows, flags=2, length=0) == _lib.HRS_EINVAL
    # NULL arrays with work to do
    assert dev(h, rows, st=None) == _lib.HRS_EINVAL and b"stored is NULL" in lib.hrs_last_error(h)
    assert dev(h, rows, vd=None) == _lib.HRS_EINVAL and b"verdicts is NULL" in lib.hrs_last_error(h)
    assert dev(h, rows, co=None) == _lib.HRS_EINVAL and b"crc_out is NULL" in lib.hrs_last_error(h)
    assert dev(h, rows, rp=None) == _lib.HRS_EINVAL
    assert host(h, rows, st=None) == _lib.HRS_EINVAL and host(h, rows, vd=None) == _lib.HRS_EINVAL
    assert host(h, rows, co=None) == _lib.HRS_EINVAL
    # crc_out overlapping stored: the same array, or shifted by one word
    assert dev(h, rows, st=crcs.ctypes.data) == _lib.HRS_EINVAL and b"overlap" in lib.hrs_last_error(h)
    assert dev(h, rows, st=crcs.ctypes.data + 4) == _lib.HRS_EINVAL
    assert host(h, rows, st=crcs.ctypes.data) == _lib.HRS_EINVAL
    assert host(h, rows, st=crcs.ctypes.data + 4 * (n - 1)) == _lib.HRS_EINVAL
    assert untouched()
    # the empty call touches nothing and needs no array but the reports
    assert dev(h, rows, length=0) == _lib.HRS_OK and dev(h, rows, stripes=0) == _lib.HRS_OK
    assert dev(h, rows, length=0, st=None, vd=None, co=None, er=None) == _lib.HRS_OK
    assert host(h, rows, length=0) == _lib.HRS_OK
    assert untouched()
    # good arguments: no device behind this handle, in either mode, with and without erased_out
    assert dev(h, rows) == _lib.HRS_EDEVICE and dev(h, rows, flags=1) == _lib.HRS_EDEVICE
    assert dev(h, rows, er=None) == _lib.HRS_EDEVICE
    assert untouched()
    # while the host form runs on it: all-zero columns are codewords, and zlib's CRC of 64 zero bytes is stored
    import zlib
    stored[:] = zlib.crc32(bytes(L))
    assert host(h, rows) == _lib.HRS_OK
    assert verdicts[0] == R.CLEAN and (erased[0] == -1).all() and (crcs[:n] == stored[:n]).all()
    assert rep[0].tolist() == [0, 0, R.NONE, 0] + [0] * n and not buf.any()


def test_repair_checked_logic_program():
    """tests/cpp/repair_checked_logic.cpp: the pattern builder the plan kernel
    shares against a construction of its own over every erased set of RS(3,2)
    and RS(6,3) and 200 of RS(12,8), and hrs_repair_checked_host's verdicts
    (also part of the `make asan` run)."""
    exe = os.path.join(ROOT, "tests", "cpp", "repair_checked_logic")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", ROOT, "tests/cpp/repair_checked_logic"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "repair_checked_logic ok" in out.stdout
