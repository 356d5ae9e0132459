"""CPU tests of the boundary of heal with known erasures over host batches and
with block CRC-32s (hrs_heal_erased_crc_dev, hrs_heal_erased_batch_host,
hrs_heal_erased_batch_host_crc): exported and declared in both headers; on a
host-only handle the sibling calls' refusals, settled before any device is
selected; the Python wrappers' own checks; and the build's resource report of
the fused kernel (no scratch)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from lambdafs_amd import HipReedSolomonCode, HrsError, TooManyErasedLocations, _lib, device
from test_abi import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = -2  # HRS_DEVICE_NONE
NAMES = ("hrs_heal_erased_crc_dev", "hrs_heal_erased_batch_host", "hrs_heal_erased_batch_host_crc")
CRC_NAMES = (NAMES[0], NAMES[2])
HOST_NAMES = NAMES[1:]
K, P, S, L = 10, 4, 3, 4096
N = K + P
W = 4 + N
ERASED = [[2], [], [0, 13]]


def test_symbols_exported_and_declared():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name
    assert set(NAMES) <= set(declared_symbols())
    with open(os.path.join(ROOT, "include", "hrs.hpp")) as f:
        hpp = f.read()
    for name in NAMES:
        assert name + "(" in hpp, name


def _erased(lists, width=None):
    width = width or max(1, max(len(e) for e in lists))
    arr = np.full((len(lists), width), -1, np.int32)
    for s, e in enumerate(lists):
        arr[s, : len(e)] = e
    return arr


def _calls(code, crc_in, crc_out, erased=ERASED, max_erased=None, nstripes=S, length=L, report_stride=W, rows=None,
           row_stride=L, stripe_stride=None, reports=None, stripes=None):
    """The three entry points over one host batch (the _dev form is only ever
    asked for its argument checks here): {name: status}."""
    lib, h = _lib.lib(), code._handle()
    n = code.stripeSize() + code.paritySize()
    st = np.zeros((S, n, L), np.uint8) if stripes is None else stripes
    rep = np.zeros((S, report_stride + 4), np.uint32) if reports is None else reports
    ptrs = _lib.ptr_array([st.ctypes.data + l * L for l in range(n)] if rows is None else rows)
    arr = None if erased is None else _erased(erased)
    ep = None if arr is None else arr.ctypes.data
    me = (0 if arr is None else arr.shape[1]) if max_erased is None else max_erased
    host = (h, st.ctypes.data, row_stride, n * L if stripe_stride is None else stripe_stride, length, nstripes, ep, me,
            rep.ctypes.data, report_stride)
    return {
        NAMES[0]: lib.hrs_heal_erased_crc_dev(h, ptrs, n * L, length, nstripes, ep, me, rep.ctypes.data, report_stride,
                                              crc_in, crc_out, None),
        NAMES[1]: lib.hrs_heal_erased_batch_host(*host),
        NAMES[2]: lib.hrs_heal_erased_batch_host_crc(*host, crc_in, crc_out),
    }


@pytest.fixture
def code():
    return HipReedSolomonCode(K, P, device=NONE)


def _msg(c):
    return _lib.lib().hrs_last_error(c._handle())


def test_null_crc_out_is_einval(code):
    got = _calls(code, None, None)
    assert [got[x] for x in CRC_NAMES] == [_lib.HRS_EINVAL] * 2
    assert b"crc_out" in _msg(code)
    assert got[NAMES[1]] == _lib.HRS_EDEVICE  # the call without CRCs has no such argument


def test_overlapping_crc_arrays_are_einval(code):
    words = np.zeros(S * N + 1, np.uint32)
    base = words.ctypes.data
    for cin, cout in ((base, base + 4), (base + 4, base)):
        got = _calls(code, cin, cout)
        assert [got[x] for x in CRC_NAMES] == [_lib.HRS_EINVAL] * 2
        assert b"overlap" in _msg(code)
    got = _calls(code, base, base)  # aliased: valid
    assert [got[x] for x in CRC_NAMES] == [_lib.HRS_EDEVICE] * 2


def test_bad_erased_lists_are_refused_with_the_stripe_named(code):
    words = np.zeros(S * N, np.uint32)
    out = words.ctypes.data
    assert _calls(code, None, out, erased=[[0], [1, 2, 3, 4, 5], []]) == dict.fromkeys(NAMES, _lib.HRS_ETOOMANY)
    assert b"stripe 1" in _msg(code)
    assert _calls(code, None, out, erased=[[0], [], [N]]) == dict.fromkeys(NAMES, _lib.HRS_EINVAL)
    assert b"stripe 2" in _msg(code) and b"outside" in _msg(code)
    assert _calls(code, None, out, erased=[[0], [7, 7], []]) == dict.fromkeys(NAMES, _lib.HRS_EINVAL)
    assert b"stripe 1" in _msg(code) and b"twice" in _msg(code)
    assert _calls(code, None, out, max_erased=-1) == dict.fromkeys(NAMES, _lib.HRS_EINVAL)
    assert b"max_erased" in _msg(code)
    assert _calls(code, None, out, erased=None, max_erased=2) == dict.fromkeys(NAMES, _lib.HRS_EINVAL)
    assert b"max_erased" in _msg(code)
    # the erased list is judged before the CRC arrays, as the sibling judges it before the device
    assert _calls(code, None, None, erased=[[0], [1, 2, 3, 4, 5], []]) == dict.fromkeys(NAMES, _lib.HRS_ETOOMANY)
    # the list runs up to the first negative entry: what follows is not read
    arr = [[2, -1, 99], [-1, 5, 5], [0, 13, -1]]
    assert _calls(code, None, out, erased=arr) == dict.fromkeys(NAMES, _lib.HRS_EDEVICE)


def test_sibling_refusals_come_back_unchanged(code):
    words = np.zeros(S * N, np.uint32)
    out = words.ctypes.data
    from lambdafs_amd import HipNativeReedSolomonCode
    nrs = HipNativeReedSolomonCode(K, P, device=NONE)
    assert _calls(nrs, None, out) == dict.fromkeys(NAMES, _lib.HRS_EINVAL)
    assert b"rs code only" in _msg(nrs)
    wide = HipReedSolomonCode(20, 9, device=NONE)
    assert _calls(wide, None, out, report_stride=4 + 29) == dict.fromkeys(NAMES, _lib.HRS_EINVAL)
    assert b"parity_size <= 8" in _msg(wide)
    # report_stride below 4 + n, also with a bad erased list behind it
    assert _calls(code, None, out, report_stride=W - 1) == dict.fromkeys(NAMES, _lib.HRS_EINVAL)
    assert b"report_stride" in _msg(code)
    assert _calls(code, None, out, report_stride=W - 1, erased=[[N], [], []]) == dict.fromkeys(NAMES, _lib.HRS_EINVAL)
    assert b"report_stride" in _msg(code)
    # _dev: two equal row pointers, a NULL row
    st = np.zeros((S, N, L), np.uint8)
    rows = [st.ctypes.data + l * L for l in range(N)]
    rows[5] = rows[2]
    assert _calls(code, None, out, rows=rows)[NAMES[0]] == _lib.HRS_EINVAL
    rows[5] = None
    assert _calls(code, None, out, rows=rows)[NAMES[0]] == _lib.HRS_EINVAL
    # host batches: overlapping cells
    got = _calls(code, None, out, row_stride=L - 1)
    assert [got[x] for x in HOST_NAMES] == [_lib.HRS_EINVAL] * 2
    assert b"cells overlap" in _msg(code)
    got = _calls(code, None, out, stripe_stride=L)
    assert [got[x] for x in HOST_NAMES] == [_lib.HRS_EINVAL] * 2
    # NULL stripes / reports
    lib, h = _lib.lib(), code._handle()
    arr = _erased(ERASED)
    rep = np.zeros((S, W), np.uint32)
    assert lib.hrs_heal_erased_batch_host(h, None, L, N * L, L, S, arr.ctypes.data, 2, rep.ctypes.data, W) == _lib.HRS_EINVAL
    assert lib.hrs_heal_erased_batch_host_crc(h, st.ctypes.data, L, N * L, L, S, arr.ctypes.data, 2, None, W, None,
                                              out) == _lib.HRS_EINVAL
    assert lib.hrs_heal_erased_crc_dev(None, None, 0, 0, 0, None, 0, None, 0, None, None, None) == _lib.HRS_EINVAL


def test_valid_arguments_on_host_only_handle_are_edevice(code):
    words = np.zeros(2 * S * N, np.uint32)
    rep = np.zeros((S, W + 4), np.uint32)
    st = np.full((S, N, L), 0x11, np.uint8)
    base = words.ctypes.data
    assert _calls(code, None, base, reports=rep, stripes=st) == dict.fromkeys(NAMES, _lib.HRS_EDEVICE)
    assert _calls(code, base + 4 * S * N, base, reports=rep, stripes=st) == dict.fromkeys(NAMES, _lib.HRS_EDEVICE)
    # max_erased == 0 is the heal call: the same answer
    assert _calls(code, None, base, erased=None, reports=rep, stripes=st) == dict.fromkeys(NAMES, _lib.HRS_EDEVICE)
    assert not words.any() and not rep.any() and (st == 0x11).all()  # nothing written


def test_empty_calls_are_ok_and_touch_nothing(code):
    words = np.full(S * N, 0xA5A5A5A5, np.uint32)
    rep = np.full((S, W + 4), 0x5A5A5A5A, np.uint32)
    st = np.full((S, N, L), 0x11, np.uint8)
    out = words.ctypes.data
    for kw in (dict(nstripes=0), dict(length=0)):
        assert _calls(code, None, out, reports=rep, stripes=st, **kw) == dict.fromkeys(NAMES, _lib.HRS_OK)
        assert _calls(code, None, None, reports=rep, stripes=st, **kw) == dict.fromkeys(NAMES, _lib.HRS_OK)
    assert (words == 0xA5A5A5A5).all() and (rep == 0x5A5A5A5A).all() and (st == 0x11).all()
    # a bad list is still refused for an empty row, as hrs_heal_erased_dev does
    assert _calls(code, None, out, length=0, erased=[[N], [], []]) == dict.fromkeys(NAMES, _lib.HRS_EINVAL)


def test_python_wrappers_raise_for_the_same_errors(code):
    st = np.zeros((S, N, L), np.uint8)
    for call in (device.heal_erased_batch_host, device.heal_erased_batch_host_crc):
        with pytest.raises(TooManyErasedLocations):
            call(code, st, [[0], [1, 2, 3, 4, 5], []])
        with pytest.raises(HrsError):
            call(code, st, [[0], [N], []])
        with pytest.raises(HrsError):
            call(code, st, [[0], [2, 2], []])
        with pytest.raises(ValueError):
            call(code, st, [[0], [1]])  # one list per stripe
        with pytest.raises(ValueError):
            call(code, np.zeros((S, N - 1, L), np.uint8), ERASED)
        ro = np.zeros((S, N, L), np.uint8)
        ro.setflags(write=False)
        with pytest.raises(ValueError):
            call(code, ro, ERASED)
        with pytest.raises(HrsError) as err:  # valid arguments: the host-only handle
            call(code, st, ERASED)
        assert err.value.status == _lib.HRS_EDEVICE
    for bad in (np.zeros((S, N + 1), np.uint32), np.zeros((S, N), np.int32), np.zeros((N, S), np.uint32).T):
        with pytest.raises(ValueError):
            device.heal_erased_batch_host_crc(code, st, ERASED, crc_in=bad)
        with pytest.raises(ValueError):
            device.heal_erased_batch_host_crc(code, st, ERASED, crc_out=bad)
    assert "heal_erased_batch_host" in device.checksums_to_erased.__doc__


# ------------------------------------------------------------ build checks

def test_fused_kernels_have_no_scratch():
    """The compiler's resource report for gfx950 (make heal_erased_crc_resources):
    every heal_erased_crc_kernel instantiation that is built shows ScratchSize 0."""
    out = subprocess.run(["make", "-C", ROOT, "--no-print-directory", "heal_erased_crc_resources"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    names = re.findall(r"Function Name: (\S+)", out.stdout)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stdout)]
    assert len(names) == len(scratch)
    fused = [x for x in names if "heal_erased_crc_kernel" in x]
    # P = 2 and 3 at 512 and 1,024 threads, P = 4 at 512 (its 1,024-thread form spills and is not built)
    assert len(fused) == 5 and len(fused) == len(names), names
    assert sum("Li4ELi512E" in x for x in fused) == 1 and not any("Li4ELi1024E" in x for x in fused), fused
    assert all(v == 0 for v in scratch), list(zip(names, scratch))
