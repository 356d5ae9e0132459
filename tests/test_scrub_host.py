"""CPU tests of stripe scrubbing: the host locator (hrs_compute_error_locations,
lambdafs_amd/csrc/hrs_locator.hpp — the code the scrub kernels run on their
bad columns) against the oracle's computeErrorLocations, the argument rules
of the scrub entry points on host-only handles, and the report -> erasure
list helper. No coding call runs here."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from lambdafs_amd import HipReedSolomonCode, HrsError, _lib, device
from oracle import rs_oracle as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = -2  # HRS_DEVICE_NONE

SHAPES = [(10, 4), (12, 4), (6, 3), (3, 2), (4, 1), (20, 8), (40, 7)]
WORDS_PER_KIND = 60


def _cases(k, p):
    """Seeded words with 0, 1, 2 and 3 corrupted locations, plus 2-error words
    whose two error values are equal (S_0 = 0): (kind, word, true locations)."""
    n = k + p
    rnd = random.Random(1000 * k + p)
    out = []
    for kind in ("e0", "e1", "e2", "e3", "eq2"):
        errors = {"e0": 0, "e1": 1, "e2": 2, "e3": 3, "eq2": 2}[kind]
        for _ in range(WORDS_PER_KIND):
            msg = [rnd.randrange(256) for _ in range(k)]
            word = C.encode(k, p, msg) + msg
            locs = sorted(rnd.sample(range(n), errors))
            same = rnd.randrange(1, 256)
            for l in locs:
                word[l] ^= same if kind == "eq2" else rnd.randrange(1, 256)
            out.append((kind, word, set(locs)))
    return out


def _oracle_class(kind, ok, found, truth):
    if ok and not found:
        return "clean_equal" if kind == "eq2" else "clean"
    if ok:
        return "exact" if found == truth else "wrong_set"
    return f"unresolved_{min(len(found), 1)}"


@pytest.fixture(scope="module")
def oracle_outcomes():
    """The oracle's answer for every case, computed once: {(k, p): [(kind, word,
    truth, ok, found, mutated)]}."""
    res = {}
    for k, p in SHAPES:
        rows = []
        for kind, word, truth in _cases(k, p):
            ok, found, mutated = C.compute_error_locations(k, p, list(word))
            rows.append((kind, word, truth, ok, found, mutated))
        res[(k, p)] = rows
    return res


def test_oracle_outcomes_cover_every_class(oracle_outcomes):
    """The case list is not vacuous: the oracle itself returns every class of
    outcome somewhere in it, the reference's odd ones included."""
    seen = {}
    for (k, p), rows in oracle_outcomes.items():
        for kind, _, truth, ok, found, _ in rows:
            seen.setdefault(_oracle_class(kind, ok, found, truth), set()).add((k, p))
    assert seen.get("exact")
    assert (20, 8) in seen.get("wrong_set", set())          # resolved, with locations that were never corrupted
    assert seen.get("unresolved_0") and seen.get("unresolved_1")
    assert (4, 1) in seen.get("clean_equal", set())         # equal error values: S_0 = 0, p = 1 sees nothing
    assert seen.get("clean")


@pytest.mark.parametrize("k,p", SHAPES)
def test_locator_matches_oracle(oracle_outcomes, k, p):
    code = HipReedSolomonCode(k, p, device=NONE)
    for kind, word, _, ok, found, mutated in oracle_outcomes[(k, p)]:
        data = list(word)
        locs = {99}
        got = code.computeErrorLocations(data, locs)
        assert (got, locs, data) == (ok, found, mutated), (kind, word)


def test_p1_any_nonzero_syndrome_is_unresolved():
    code = HipReedSolomonCode(4, 1, device=NONE)
    word = C.encode(4, 1, [1, 2, 3, 4]) + [1, 2, 3, 4]
    word[2] ^= 0x55
    locs = set()
    assert code.computeErrorLocations(word, locs) is False and locs == set()


def _raw_locate(code, data):
    n = len(data)
    locs = (ctypes.c_int * max(1, n))()
    nloc, res = ctypes.c_int(0), ctypes.c_int(0)
    return _lib.lib().hrs_compute_error_locations(code._h, _lib.int_array(data), locs, ctypes.byref(nloc),
                                                  ctypes.byref(res))


def test_compute_error_locations_argument_errors():
    lib = _lib.lib()
    code = HipReedSolomonCode(3, 2, device=NONE)
    for bad in (256, -1):
        assert _raw_locate(code, [0, 0, bad, 0, 0]) == _lib.HRS_EINVAL
        assert b"outside [0, 255]" in lib.hrs_last_error(code._h)
    with pytest.raises(HrsError) as ei:
        code.computeErrorLocations([0, 0, 0, 0, 300], set())
    assert ei.value.status == _lib.HRS_EINVAL
    wide = HipReedSolomonCode(3, 9, device=NONE)
    assert _raw_locate(wide, [0] * 12) == _lib.HRS_EINVAL
    assert b"parity_size <= 8" in lib.hrs_last_error(wide._h)
    from lambdafs_amd import HipXORCode
    xor = HipXORCode(4, 1, device=NONE)
    assert _raw_locate(xor, [0] * 5) == _lib.HRS_EINVAL
    assert b"rs code only" in lib.hrs_last_error(xor._h)


def test_scrub_calls_check_arguments_before_the_device():
    """Family, p > 8, NULL rows and a short report_stride are HRS_EINVAL even
    on a host-only handle; with good arguments the two coding calls then fail
    with HRS_EDEVICE; empty jobs are HRS_OK."""
    lib = _lib.lib()
    k, p = 3, 2
    n = k + p
    code = HipReedSolomonCode(k, p, device=NONE)
    h = code._h
    buf = np.zeros((2, n, 64), dtype=np.uint8)
    rep = np.zeros((2, 4 + n), dtype=np.uint32)
    rows = _lib.ptr_array([buf.ctypes.data + l * 64 for l in range(n)])
    # short report stride
    assert lib.hrs_scrub_dev(h, rows, n * 64, 64, 2, rep.ctypes.data, 4 + n - 1, None) == _lib.HRS_EINVAL
    assert b"report_stride" in lib.hrs_last_error(h)
    assert lib.hrs_scrub_batch_host(h, buf.ctypes.data, 64, n * 64, 64, 2, rep.ctypes.data, 3) == _lib.HRS_EINVAL
    assert b"report_stride" in lib.hrs_last_error(h)
    # a NULL row
    holed = _lib.ptr_array([None if l == 1 else buf.ctypes.data + l * 64 for l in range(n)])
    assert lib.hrs_scrub_dev(h, holed, n * 64, 64, 2, rep.ctypes.data, 4 + n, None) == _lib.HRS_EINVAL
    assert b"row 1 is NULL" in lib.hrs_last_error(h)
    assert lib.hrs_scrub_batch_host(h, None, 64, n * 64, 64, 2, rep.ctypes.data, 4 + n) == _lib.HRS_EINVAL
    # empty jobs touch nothing
    assert lib.hrs_scrub_dev(h, rows, n * 64, 0, 2, rep.ctypes.data, 4 + n, None) == _lib.HRS_OK
    assert lib.hrs_scrub_dev(h, rows, n * 64, 64, 0, rep.ctypes.data, 4 + n, None) == _lib.HRS_OK
    assert lib.hrs_scrub_batch_host(h, buf.ctypes.data, 64, n * 64, 0, 2, rep.ctypes.data, 4 + n) == _lib.HRS_OK
    # good arguments: no device behind this handle
    assert lib.hrs_scrub_dev(h, rows, n * 64, 64, 2, rep.ctypes.data, 4 + n, None) == _lib.HRS_EDEVICE
    assert lib.hrs_scrub_batch_host(h, buf.ctypes.data, 64, n * 64, 64, 2, rep.ctypes.data, 4 + n) == _lib.HRS_EDEVICE
    assert not rep.any()
    with pytest.raises(HrsError) as ei:
        device.scrub_batch_host(code, buf)
    assert ei.value.status == _lib.HRS_EDEVICE
    # other families and p > 8
    wide = HipReedSolomonCode(3, 9, device=NONE)
    wbuf = np.zeros((1, 12, 64), dtype=np.uint8)
    wrep = np.zeros((1, 16), dtype=np.uint32)
    assert lib.hrs_scrub_batch_host(wide._h, wbuf.ctypes.data, 64, 12 * 64, 64, 1, wrep.ctypes.data, 16) == _lib.HRS_EINVAL
    assert b"parity_size <= 8" in lib.hrs_last_error(wide._h)
    from lambdafs_amd import HipNativeReedSolomonCode
    nrs = HipNativeReedSolomonCode(3, 2, device=NONE)
    assert lib.hrs_scrub_dev(nrs._h, rows, n * 64, 64, 2, rep.ctypes.data, 4 + n, None) == _lib.HRS_EINVAL
    assert b"rs code only" in lib.hrs_last_error(nrs._h)


def test_widest_handle_n255():
    """RS(247,8): n = 255 is the most hrs_create admits (k + p < 256). The
    locator agrees with the oracle there, errors at the last location
    included, and the scrub calls take the handle (their row table and
    histogram hold 255 locations): arguments pass, then HRS_EDEVICE."""
    lib = _lib.lib()
    k, p = 247, 8
    n = k + p
    code = HipReedSolomonCode(k, p, device=NONE)
    rnd = random.Random(255)
    outcomes = set()
    for trial in range(60):
        msg = [rnd.randrange(256) for _ in range(k)]
        word = C.encode(k, p, msg) + msg
        locs = {n - 1} | set(rnd.sample(range(n - 1), trial % 5))
        for l in locs:
            word[l] ^= rnd.randrange(1, 256)
        ok, found, mutated = C.compute_error_locations(k, p, list(word))
        data, got_locs = list(word), set()
        got = code.computeErrorLocations(data, got_locs)
        assert (got, got_locs, data) == (ok, found, mutated), word
        outcomes.add((ok, (n - 1) in found))
    assert (True, True) in outcomes and any(not ok for ok, _ in outcomes)
    buf = np.zeros((1, n, 16), dtype=np.uint8)
    rep = np.zeros((1, 4 + n), dtype=np.uint32)
    rows = _lib.ptr_array([buf.ctypes.data + l * 16 for l in range(n)])
    assert lib.hrs_scrub_dev(code._h, rows, n * 16, 16, 1, rep.ctypes.data, 4 + n, None) == _lib.HRS_EDEVICE
    assert lib.hrs_scrub_dev(code._h, rows, n * 16, 16, 1, rep.ctypes.data, 4 + n - 1, None) == _lib.HRS_EINVAL
    assert lib.hrs_scrub_batch_host(code._h, buf.ctypes.data, 16, n * 16, 16, 1, rep.ctypes.data,
                                    4 + n) == _lib.HRS_EDEVICE
    with pytest.raises(HrsError):  # one more location is no handle at all
        HipReedSolomonCode(248, 8, device=NONE)


def test_scrub_batch_host_rejects_overlapping_cells():
    """Strides under which cells overlap are HRS_EINVAL (a read-only pass would
    otherwise report on the wrong bytes silently); both packings pass the
    check and reach HRS_EDEVICE on a host-only handle."""
    lib = _lib.lib()
    k, p, L, ns = 3, 2, 64, 4
    n = k + p
    code = HipReedSolomonCode(k, p, device=NONE)
    buf = np.zeros(ns * n * L, dtype=np.uint8)
    rep = np.zeros((ns, 4 + n), dtype=np.uint32)

    def call(row_stride, stripe_stride, stripes=ns):
        return lib.hrs_scrub_batch_host(code._h, buf.ctypes.data, row_stride, stripe_stride, L, stripes,
                                        rep.ctypes.data, 4 + n)

    for row_stride, stripe_stride in [(L - 1, n * L), (L, n * L - 1), (L, L), (L, 0), (ns * L - 1, L), (0, n * L)]:
        assert call(row_stride, stripe_stride) == _lib.HRS_EINVAL, (row_stride, stripe_stride)
        assert b"cells overlap" in lib.hrs_last_error(code._h)
    assert call(L, n * L) == _lib.HRS_EDEVICE        # [S, n, L]
    assert call(ns * L, L) == _lib.HRS_EDEVICE       # [n, S, L]
    assert call(L, 0, stripes=1) == _lib.HRS_EDEVICE  # one stripe: its stride is not used


def test_scrub_to_erased():
    n, p = 14, 4
    rep = np.zeros((4, 4 + n), dtype=np.uint32)
    rep[:, 2] = 0xFFFFFFFF
    rep[1, [0, 2, 4 + 13, 4 + 0]] = [7, 5, 3, 4]           # locations 0 and 13
    rep[2, [0, 2, 4 + 5]] = [1 << 20, 0, 1 << 20]          # one whole cell
    rep[3, [0, 2, 4 + 1, 4 + 2, 4 + 3, 4 + 9]] = [9, 1, 2, 2, 2, 3]
    want = [[-1, -1, -1, -1], [0, 13, -1, -1], [5, -1, -1, -1], [1, 2, 3, 9]]
    got = device.scrub_to_erased(rep, p)
    assert got.dtype == np.int32 and got.tolist() == want
    # the int32 view the device helpers return (uint32 bits)
    assert device.scrub_to_erased(rep.view(np.int32), p).tolist() == want
    unresolved = rep.copy()
    unresolved[2, 1] = 1
    with pytest.raises(ValueError, match="stripe 2.*unresolved"):
        device.scrub_to_erased(unresolved, p)
    many = rep.copy()
    many[3, 4 + 11] = 1
    with pytest.raises(ValueError, match="stripe 3.*5 blamed"):
        device.scrub_to_erased(many, p)
    with pytest.raises(ValueError):
        device.scrub_to_erased(np.zeros((2, 4), dtype=np.uint32), p)


def test_scrub_logic_program():
    """tests/cpp/scrub_logic.cpp: 22,000 seeded words (shapes up to n = 255)
    through the C ABI against the oracle (also part of the `make asan` run)."""
    exe = os.path.join(ROOT, "tests", "cpp", "scrub_logic")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", ROOT, "tests/cpp/scrub_logic"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout


def test_library_holds_the_scrub_kernels():
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"scrub_kernel" in blob and b"scrub_bytewise_kernel" in blob
