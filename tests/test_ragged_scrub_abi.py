"""CPU tests of the argument rules of the ragged scrub and heal entry points
on a host-only handle, in the order include/hrs.h states them: the handle, the
sibling's gate (code, reports, rows; heal's NULL-row and equal-rows rule, the
host batches' overlapping-cells rule), valid, the empty batch, the valid
entries (the stripe and location named), then the device. Each case also
breaks every later rule, so the order itself is tested. A refused or empty call
touches nothing. And the names in hrs.hpp and libhrs.map, the Python mirror,
and the kernels in the library."""
import ctypes
import fnmatch
import os
import re

import numpy as np
import pytest

from lambdafs_amd import HipReedSolomonCode, HrsError, _lib, device

NONE = -2  # HRS_DEVICE_NONE
K, P, S, L = 10, 4, 3, 256
N = K + P
FILL = 0xA5
DEV = ("hrs_scrub_ragged_dev", "hrs_heal_ragged_dev")
BATCH = ("hrs_scrub_ragged_batch_host", "hrs_heal_ragged_batch_host")
ONE = "hrs_heal_ragged_host"
NAMES = DEV + BATCH + (ONE,)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Buffers:
    """A small host batch under a fill pattern (host addresses: no call here
    gets as far as a device), reports and a valid array that breaks rule 5."""

    def __init__(self):
        self.st = np.full((S, N, L), FILL, np.uint8)
        self.rep = np.full((S, 4 + N), FILL, np.uint32)
        self.valid = np.full((S, N), L // 2, np.uint32)
        self.valid[1, 5] = L + 1  # rule 5, broken in every case that tests an earlier rule

    def untouched(self):
        return bool((self.st == FILL).all() and (self.rep == FILL).all() and self.valid[1, 5] == L + 1)


def call(name, h, b, *, cells=True, reports=True, valid=True, nstripes=S, length=L, stride=None, row_null=None,
         row_equal=False, report_stride=4 + N):
    """One call; the keywords replace an argument by NULL or break it."""
    lib = _lib.lib()
    v = b.valid.ctypes.data if valid else None
    r = b.rep.ctypes.data if reports else None
    if name in BATCH:
        return getattr(lib, name)(h, b.st.ctypes.data if cells else None, L if stride is None else stride, N * L, length,
                                  nstripes, v, r, report_stride)
    ptrs = [b.st.ctypes.data + l * L for l in range(N)]
    if row_null is not None:
        ptrs[row_null] = None
    if row_equal:
        ptrs[3] = ptrs[7]
    rows = _lib.ptr_array(ptrs) if cells else None
    if name == ONE:
        return lib.hrs_heal_ragged_host(h, rows, length, v, r)
    return getattr(lib, name)(h, rows, N * L, length, nstripes, v, r, report_stride, None)


def last_error(code):
    return _lib.lib().hrs_last_error(code._handle()).decode()


@pytest.fixture
def code():
    return HipReedSolomonCode(K, P, device=NONE)


def test_the_symbols_are_declared_exported_and_mirrored():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "hrs.h")).read()
    hpp = open(os.path.join(ROOT, "include", "hrs.hpp")).read()
    version_script = open(os.path.join(ROOT, "lambdafs_amd", "csrc", "libhrs.map")).read()
    patterns = re.findall(r"^\s*([A-Za-z_*]+);", version_script.split("local:")[0], flags=re.M)
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.EXPORTS
        assert name + "(" in header and name + "(" in hpp
        assert any(fnmatch.fnmatchcase(name, pat) for pat in patterns), (name, patterns)
    for name in ("scrub_stripes_ragged", "heal_stripes_ragged", "scrub_batch_host_ragged", "heal_batch_host_ragged",
                 "heal_host_ragged"):
        assert hasattr(device, name)
    assert "ragged scrub and heal" in header and "DEMOTION" in header


def test_library_holds_the_ragged_scrub_kernels():
    blob = open(_lib.LIB_PATH, "rb").read()
    for p in range(1, 9):
        for heal in (0, 1):
            assert b"19scrub_ragged_kernelILi%dELb%dEE" % (p, heal) in blob
            assert b"28scrub_ragged_bytewise_kernelILi%dELb%dEE" % (p, heal) in blob


@pytest.mark.parametrize("name", NAMES)
def test_rule_1_null_handle(name):
    b = Buffers()
    assert call(name, None, b, cells=False, reports=False, valid=False) == _lib.HRS_EINVAL
    assert b.untouched()


@pytest.mark.parametrize("name", NAMES)
def test_rule_2_the_siblings_gate(code, name):
    b = Buffers()
    h = code._handle()
    assert call(name, h, b, cells=False, valid=False) == _lib.HRS_EINVAL and "NULL" in last_error(code)
    assert call(name, h, b, reports=False, valid=False) == _lib.HRS_EINVAL and "NULL" in last_error(code)
    if name != ONE:
        assert call(name, h, b, valid=False, report_stride=3 + N) == _lib.HRS_EINVAL
        assert "report_stride" in last_error(code)
    if name in BATCH:
        assert call(name, h, b, valid=False, stride=L - 1) == _lib.HRS_EINVAL and "overlap" in last_error(code)
    else:
        assert call(name, h, b, valid=False, row_null=4) == _lib.HRS_EINVAL and "row 4 is NULL" in last_error(code)
        st = call(name, h, b, valid=False, row_equal=True)
        if name == DEV[0]:  # the scrub reads only: equal rows are its caller's business, so the next rule answers
            assert st == _lib.HRS_EINVAL and "valid is NULL" in last_error(code)
        else:
            assert st == _lib.HRS_EINVAL and "one pointer" in last_error(code)
    assert b.untouched()
    for k, p, kw in [(10, 9, {})]:  # p > 8: the code's rule comes before valid
        wide = HipReedSolomonCode(k, p, device=NONE)
        n = k + p
        rows = _lib.ptr_array([b.st.ctypes.data + l for l in range(n)])
        lib = _lib.lib()
        st = lib.hrs_heal_ragged_host(wide._handle(), rows, 4, None, b.rep.ctypes.data)
        assert st == _lib.HRS_EINVAL and "parity_size" in _lib.lib().hrs_last_error(wide._handle()).decode()
    assert b.untouched()


@pytest.mark.parametrize("name", NAMES)
def test_rule_3_null_valid_comes_before_the_empty_batch(code, name):
    b = Buffers()
    h = code._handle()
    assert call(name, h, b, valid=False) == _lib.HRS_EINVAL and "valid is NULL" in last_error(code)
    assert call(name, h, b, valid=False, length=0) == _lib.HRS_EINVAL and "valid is NULL" in last_error(code)
    if name != ONE:
        assert call(name, h, b, valid=False, nstripes=0) == _lib.HRS_EINVAL
    assert b.untouched()


@pytest.mark.parametrize("name", NAMES)
def test_rule_4_the_empty_batch_touches_nothing(code, name):
    b = Buffers()  # its valid breaks rule 5, the handle has no device: neither is looked at
    h = code._handle()
    assert call(name, h, b, length=0) == _lib.HRS_OK
    if name != ONE:
        assert call(name, h, b, nstripes=0) == _lib.HRS_OK
    assert b.untouched()


@pytest.mark.parametrize("name", NAMES)
def test_rule_5_valid_entries_then_6_the_device(code, name):
    b = Buffers()
    h = code._handle()
    if name == ONE:
        b.valid[0, 5] = L + 1
        assert call(name, h, b) == _lib.HRS_EINVAL
        assert "stripe 0 location 5" in last_error(code) and str(L + 1) in last_error(code)
        b.valid[0, 5] = L
        assert (b.st == FILL).all() and (b.rep == FILL).all()
        assert call(name, h, b) == _lib.HRS_OK  # works on a host-only handle
        return
    assert call(name, h, b) == _lib.HRS_EINVAL
    assert "stripe 1 location 5" in last_error(code) and str(L + 1) in last_error(code)
    assert b.untouched()
    b.valid[1, 5] = L
    assert call(name, h, b) == _lib.HRS_EDEVICE
    assert (b.st == FILL).all() and (b.rep == FILL).all()


def test_mirror_refuses_a_valid_array_of_the_wrong_shape(code):
    rows = [np.zeros(8, np.uint8) for _ in range(N)]
    with pytest.raises(ValueError):
        device.heal_host_ragged(code, rows, np.zeros(N - 1, np.uint32))
    with pytest.raises(ValueError):
        device.scrub_batch_host_ragged(code, np.zeros((S, N, 8), np.uint8), np.zeros((S, K), np.uint32))
    with pytest.raises(HrsError) as ei:
        device.scrub_batch_host_ragged(code, np.zeros((S, N, 8), np.uint8), np.full((S, N), 8, np.uint32))
    assert ei.value.status == _lib.HRS_EDEVICE
