"""CPU tests of the scrub / heal + CRC-32 entry points' boundary
(hrs_scrub_crc_dev, hrs_heal_crc_dev, hrs_scrub_batch_host_crc,
hrs_heal_batch_host_crc): exported and declared, and on a host-only handle the
argument rules that are settled before any device is selected; the erasure
list from checksums (device.checksums_to_erased); and the build's resource
report of the fused kernels (no scratch)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from lambdafs_amd import HipReedSolomonCode, _lib, device
from test_abi import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = -2  # HRS_DEVICE_NONE
NAMES = ("hrs_scrub_crc_dev", "hrs_heal_crc_dev", "hrs_scrub_batch_host_crc", "hrs_heal_batch_host_crc")
HOST_NAMES = NAMES[2:]
K, P, S, L = 10, 4, 3, 4096
N = K + P
W = 4 + N


def test_symbols_exported_and_declared():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name
    assert set(declared_symbols()) == set(_lib.EXPORTS)
    with open(os.path.join(ROOT, "include", "hrs.h")) as f:
        header = f.read()
    assert "HOPS ORDER" in header  # the order of crc_out is spelled out where the calls are declared


def _calls(code, crc_in, crc_out, nstripes=S, report_stride=W, rows=None, row_stride=L, stripe_stride=N * L,
           reports=None):
    """The four entry points over one host batch (the _dev forms are only ever
    asked for their argument checks here): {name: status}."""
    lib, h = _lib.lib(), code._handle()
    n = code.stripeSize() + code.paritySize()
    st = np.zeros((S, n, L), np.uint8)
    rep = np.zeros((S, report_stride + 4), np.uint32) if reports is None else reports
    ptrs = _lib.ptr_array([st.ctypes.data + l * L for l in range(n)] if rows is None else rows)
    dev = (h, ptrs, n * L, L, nstripes, rep.ctypes.data, report_stride, crc_in, crc_out, None)
    host = (h, st.ctypes.data, row_stride, stripe_stride if stripe_stride != N * L else n * L, L, nstripes,
            rep.ctypes.data, report_stride, crc_in, crc_out)
    return {
        "hrs_scrub_crc_dev": lib.hrs_scrub_crc_dev(*dev),
        "hrs_heal_crc_dev": lib.hrs_heal_crc_dev(*dev),
        "hrs_scrub_batch_host_crc": lib.hrs_scrub_batch_host_crc(*host),
        "hrs_heal_batch_host_crc": lib.hrs_heal_batch_host_crc(*host),
    }


@pytest.fixture
def code():
    return HipReedSolomonCode(K, P, device=NONE)


def test_null_crc_out_is_einval(code):
    assert _calls(code, None, None) == dict.fromkeys(NAMES, _lib.HRS_EINVAL)
    assert b"crc_out" in _lib.lib().hrs_last_error(code._handle())


def test_overlapping_crc_arrays_are_einval(code):
    """crc_out may be crc_in itself; any other overlap is refused, before the
    device is looked at."""
    words = np.zeros(S * N + 1, np.uint32)
    base = words.ctypes.data
    assert _calls(code, base, base + 4) == dict.fromkeys(NAMES, _lib.HRS_EINVAL)
    assert _calls(code, base + 4, base) == dict.fromkeys(NAMES, _lib.HRS_EINVAL)
    assert _calls(code, base, base) == dict.fromkeys(NAMES, _lib.HRS_EDEVICE)  # aliased: valid


def test_valid_arguments_on_host_only_handle_are_edevice(code):
    words = np.zeros(2 * S * N, np.uint32)
    rep = np.zeros((S, W + 4), np.uint32)
    base = words.ctypes.data
    assert _calls(code, None, base, reports=rep) == dict.fromkeys(NAMES, _lib.HRS_EDEVICE)
    assert _calls(code, base + 4 * S * N, base, reports=rep) == dict.fromkeys(NAMES, _lib.HRS_EDEVICE)
    assert not words.any() and not rep.any()  # nothing written


def test_empty_batch_is_ok_and_touches_nothing(code):
    words = np.full(S * N, 0xA5A5A5A5, np.uint32)
    rep = np.full((S, W + 4), 0x5A5A5A5A, np.uint32)
    assert _calls(code, None, words.ctypes.data, nstripes=0, reports=rep) == dict.fromkeys(NAMES, _lib.HRS_OK)
    assert _calls(code, None, None, nstripes=0, reports=rep) == dict.fromkeys(NAMES, _lib.HRS_OK)
    assert (words == 0xA5A5A5A5).all() and (rep == 0x5A5A5A5A).all()


def test_sibling_refusals_come_back_unchanged(code):
    """The scrub's and the heal's own argument rules hold, with their messages,
    whatever the CRC arrays are."""
    lib = _lib.lib()
    words = np.zeros(S * N, np.uint32)
    out = words.ctypes.data

    def msg(c):
        return lib.hrs_last_error(c._handle())

    # a non-rs code
    from lambdafs_amd import HipNativeReedSolomonCode
    nrs = HipNativeReedSolomonCode(K, P, device=NONE)
    assert _calls(nrs, None, out) == dict.fromkeys(NAMES, _lib.HRS_EINVAL)
    assert b"rs code only" in msg(nrs)
    # parity_size above 8
    wide = HipReedSolomonCode(20, 9, device=NONE)
    assert _calls(wide, None, out, report_stride=4 + 29) == dict.fromkeys(NAMES, _lib.HRS_EINVAL)
    assert b"parity_size <= 8" in msg(wide)
    # a short report_stride
    assert _calls(code, None, out, report_stride=W - 1) == dict.fromkeys(NAMES, _lib.HRS_EINVAL)
    assert b"report_stride" in msg(code)
    # heal: two equal row pointers (the scrub reads them happily and goes on to the device check)
    st = np.zeros((S, N, L), np.uint8)
    rows = [st.ctypes.data + l * L for l in range(N)]
    rows[5] = rows[2]
    got = _calls(code, None, out, rows=rows)
    assert got["hrs_heal_crc_dev"] == _lib.HRS_EINVAL and got["hrs_scrub_crc_dev"] == _lib.HRS_EDEVICE
    rows[5] = None
    got = _calls(code, None, out, rows=rows)
    assert got["hrs_heal_crc_dev"] == got["hrs_scrub_crc_dev"] == _lib.HRS_EINVAL
    # host batches: overlapping cells
    got = _calls(code, None, out, row_stride=L - 1)
    assert [got[x] for x in HOST_NAMES] == [_lib.HRS_EINVAL] * 2
    assert b"cells overlap" in msg(code)
    got = _calls(code, None, out, stripe_stride=L)
    assert [got[x] for x in HOST_NAMES] == [_lib.HRS_EINVAL] * 2


def test_python_mirror_checks_crc_arguments(code):
    """device.py refuses wrong shapes and dtypes before the library is called,
    as decode_batch_host_crc does."""
    st = np.zeros((S, N, L), np.uint8)
    for call in (device.scrub_batch_host_crc, device.heal_batch_host_crc):
        for bad in (np.zeros((S, N + 1), np.uint32), np.zeros((S, N), np.int32), np.zeros((N, S), np.uint32).T):
            with pytest.raises(ValueError):
                call(code, st, crc_in=bad)
            with pytest.raises(ValueError):
                call(code, st, crc_out=bad)
        with pytest.raises(ValueError):
            call(code, np.zeros((S, N - 1, L), np.uint8))
    ro = np.zeros((S, N, L), np.uint8)
    ro.setflags(write=False)
    with pytest.raises(ValueError):
        device.heal_batch_host_crc(code, ro)


# ------------------------------------------------------ checksums_to_erased

def _reports(rows):
    r = np.zeros((len(rows), 4 + 6), np.uint32)
    r[:, 2] = 0xFFFFFFFF
    for s, (unresolved, blamed) in enumerate(rows):
        r[s, 1] = unresolved
        for l in blamed:
            r[s, 4 + l] = 2
        r[s, 0] = unresolved + len(blamed)
    return r


def test_checksums_to_erased_union_order_padding():
    stored = np.arange(4 * 6, dtype=np.uint32).reshape(4, 6) + 0xFFFFFF00  # values past 2^31: sign-proof
    crcs = stored.copy()
    crcs[1, 4] ^= 1
    crcs[1, 0] ^= 0x80000000
    crcs[2, 5] ^= 7
    crcs[3, 3] ^= 1
    assert device.checksums_to_erased(crcs, stored, 3).tolist() == [[-1, -1, -1], [0, 4, -1], [5, -1, -1], [3, -1, -1]]
    # int32 views (what the device calls return) compare as the same bits
    assert device.checksums_to_erased(crcs.view(np.int32), stored, 3).tolist()[1] == [0, 4, -1]
    rep = _reports([(0, []), (0, [2]), (3, [5, 1]), (1, [])])
    got = device.checksums_to_erased(crcs, stored, 3, reports=rep)
    assert got.dtype == np.int32 and got.shape == (4, 3)
    # union, ascending, -1 padded; unresolved columns are no error where a checksum differs
    assert got.tolist() == [[-1, -1, -1], [0, 2, 4], [1, 5, -1], [3, -1, -1]]
    # a stale parity cell: checksums agree, the report names it
    rep = _reports([(0, [1]), (0, []), (0, []), (0, [])])
    assert device.checksums_to_erased(stored, stored, 3, reports=rep).tolist()[0] == [1, -1, -1]


def test_checksums_to_erased_errors():
    stored = np.zeros((2, 6), np.uint32)
    crcs = stored.copy()
    crcs[1, :4] = 1
    with pytest.raises(ValueError, match="stripe 1"):
        device.checksums_to_erased(crcs, stored, 3)
    crcs[1, 3] = 0
    rep = _reports([(0, []), (0, [5])])
    with pytest.raises(ValueError, match="stripe 1"):  # 3 by checksum + 1 by report
        device.checksums_to_erased(crcs, stored, 3, reports=rep)
    assert device.checksums_to_erased(crcs, stored, 4, reports=rep).tolist()[1] == [0, 1, 2, 5]
    # unresolved columns and no checksum differs: neither names the damage
    rep = _reports([(2, []), (0, [])])
    with pytest.raises(ValueError, match="stripe 0"):
        device.checksums_to_erased(stored, stored, 3, reports=rep)
    with pytest.raises(ValueError):
        device.checksums_to_erased(stored, stored[:, :5], 3)
    with pytest.raises(ValueError):
        device.checksums_to_erased(stored, stored, 3, reports=rep[:, :9])


def test_scrub_to_erased_is_unchanged():
    rep = _reports([(0, []), (0, [4, 1]), (0, [0])])
    assert device.scrub_to_erased(rep, 2).tolist() == [[-1, -1], [1, 4], [0, -1]]
    with pytest.raises(ValueError, match="unresolved"):
        device.scrub_to_erased(_reports([(1, [2])]), 2)
    with pytest.raises(ValueError, match="blamed locations"):
        device.scrub_to_erased(_reports([(0, [0, 1, 2])]), 2)


# ------------------------------------------------------------ build checks

def test_fused_kernels_have_no_scratch():
    """The compiler's resource report for gfx950 (make scrub_crc_resources):
    every scrub_crc_kernel instantiation and the redo kernel show ScratchSize 0."""
    out = subprocess.run(["make", "-C", ROOT, "--no-print-directory", "scrub_crc_resources"], capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    names = re.findall(r"Function Name: (\S+)", out.stdout)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stdout)]
    assert len(names) == len(scratch)
    fused = [x for x in names if "scrub_crc_kernel" in x]
    assert len(fused) == 10, names  # P = 2 (512 threads), P = 3 and 4 (512 and 1,024), each as scrub and heal
    assert any("scrub_crc_redo_kernel" in x for x in names)
    assert all(v == 0 for v in scratch), list(zip(names, scratch))
