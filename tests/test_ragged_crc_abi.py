"""CPU tests of the ragged encode + CRC entry points
(hrs_encode_ragged_crc_dev, hrs_encode_ragged_batch_host_crc): declared,
mirrored, exported, and on a host-only handle every argument rule in the order
include/hrs.h states it: the handle, the pointer arguments (valid and crc_out
included), the empty batch (CRC arrays untouched), len, the valid entries and
the row pointers, the overlap of the CRC arrays, then the device. A refused or
empty call touches nothing."""
import ctypes
import os
import re

import numpy as np
import pytest

from lambdafs_amd import HipReedSolomonCode, HrsError, _lib, device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = -2  # HRS_DEVICE_NONE
K, P, S, L = 10, 4, 3, 256
N = K + P
FILL = 0xA5
POISON = 0xC3C3C3C3
NAMES = ("hrs_encode_ragged_crc_dev", "hrs_encode_ragged_batch_host_crc")


@pytest.fixture
def code():
    return HipReedSolomonCode(K, P, device=NONE)


class Buffers:
    """One small host batch under a fill pattern, its row pointer arrays (host
    addresses: no call here gets as far as a device), a valid array and
    poisoned CRC arrays with room to overlap (crc is a view into `words`)."""

    def __init__(self):
        self.st = np.full((S, N, L), FILL, np.uint8)
        self.valid = np.full((S, K), L // 2, np.uint32)
        base = self.st.ctypes.data
        self.ins = _lib.ptr_array([base + (P + j) * L for j in range(K)])
        self.outs = _lib.ptr_array([base + r * L for r in range(P)])
        self.words = np.full(3 * S * N, POISON, np.uint32)
        self.valid_before = self.valid.copy()

    def crc(self, at):
        return self.words[at:at + S * N].ctypes.data

    def untouched(self):
        return bool((self.st == FILL).all() and (self.valid == self.valid_before).all()
                    and (self.words == POISON).all())


def call(name, h, b, *, rows=True, outs=True, valid=True, crc_in=0, crc_out=S * N, nstripes=S, length=L):
    """One call; a False flag replaces an argument by NULL, crc_in / crc_out
    are word offsets into b.words (None: NULL)."""
    v = b.valid.ctypes.data if valid else None
    cin = None if crc_in is None else b.crc(crc_in)
    cout = None if crc_out is None else b.crc(crc_out)
    if name.endswith("_dev"):
        return _lib.lib().hrs_encode_ragged_crc_dev(h, b.ins if rows else None, N * L, b.outs if outs else None,
                                                    N * L, length, nstripes, v, cin, cout, None)
    return _lib.lib().hrs_encode_ragged_batch_host_crc(h, b.st.ctypes.data if rows and outs else None, L, N * L,
                                                       length, nstripes, v, cin, cout)


def last_error(code):
    return _lib.lib().hrs_last_error(code._handle()).decode()


def test_the_symbols_are_declared_exported_and_mirrored():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "hrs.h")).read()
    wrapper = open(os.path.join(ROOT, "include", "hrs.hpp")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.EXPORTS
        assert re.search(r"hrs_status %s\(hrs_codec\* codec" % name, header)
        assert name + "(h_," in wrapper
    assert hasattr(device, "encode_stripes_ragged_crc") and hasattr(device, "encode_batch_host_ragged_crc")
    blob = open(_lib.LIB_PATH, "rb").read()
    for k, p in [(3, 2), (6, 3), (10, 4), (12, 4)]:
        assert b"24encode_ragged_crc_kernelILi%dELi%dENS_2gf12EncodeMatrix" % (k, p) in blob
    for k, p in [(10, 4), (6, 3)]:
        assert b"24encode_ragged_crc_kernelILi%dELi%dENS_2gf12CauchyMatrix" % (k, p) in blob
    assert b"24crc_ragged_window_kernelILb1EE" in blob and b"24crc_ragged_window_kernelILb0EE" in blob


def test_the_header_no_longer_lists_the_crc_forms_as_not_covered():
    header = open(os.path.join(ROOT, "include", "hrs.h")).read()
    for m in re.finditer(r"Not covered, by design:(.*?)\*/", header, re.S):
        assert "CRC forms (" not in m.group(1) and "single-stripe host call" in m.group(1)
        assert "JNI" in m.group(1) and "repair" in m.group(1)


@pytest.mark.parametrize("name", NAMES)
def test_rule_1_null_handle(name):
    b = Buffers()
    for kw in (dict(), dict(nstripes=0), dict(valid=False), dict(rows=False), dict(crc_out=None)):
        assert call(name, None, b, **kw) == _lib.HRS_EINVAL
    assert b.untouched()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("null", ["rows", "outs", "valid", "crc_out"])
def test_rule_2_null_pointers_come_before_the_empty_batch(code, name, null):
    b = Buffers()
    gone = {null: None} if null == "crc_out" else {null: False}
    for kw in (dict(), dict(nstripes=0), dict(length=0)):
        assert call(name, code._handle(), b, **gone, **kw) == _lib.HRS_EINVAL
        assert "NULL" in last_error(code)
    assert b.untouched()


@pytest.mark.parametrize("name", NAMES)
def test_rule_3_empty_batches_touch_nothing(code, name):
    """Neither the valid entries nor the overlap of the CRC arrays is looked
    at, and the poisoned CRC arrays stay as they are."""
    b = Buffers()
    b.valid[1, 2] = L + 1
    b.valid_before = b.valid.copy()
    for kw in (dict(nstripes=0), dict(length=0)):
        assert call(name, code._handle(), b, **kw) == _lib.HRS_OK
        assert call(name, code._handle(), b, crc_in=0, crc_out=1, **kw) == _lib.HRS_OK
    assert b.untouched()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("stripe,row", [(0, 0), (1, 7), (S - 1, K - 1)])
def test_rule_4_valid_beyond_len_comes_before_the_overlap_rule(code, name, stripe, row):
    b = Buffers()
    b.valid[stripe, row] = L + 1
    b.valid_before = b.valid.copy()
    for kw in (dict(), dict(crc_in=0, crc_out=1)):
        assert call(name, code._handle(), b, **kw) == _lib.HRS_EINVAL
        assert f"stripe {stripe} row {row}" in last_error(code) and f"exceeds len {L}" in last_error(code)
    assert b.untouched()


@pytest.mark.parametrize("name", NAMES)
def test_rule_4_len_beyond_uint32(code, name):
    b = Buffers()
    assert call(name, code._handle(), b, length=2**32, crc_in=0, crc_out=1) == _lib.HRS_EINVAL
    assert "exceeds 2^32 - 1" in last_error(code)
    assert b.untouched()


def test_rule_4_null_row_pointer_comes_before_the_overlap_rule(code):
    b = Buffers()
    b.ins[3] = None
    assert call(NAMES[0], code._handle(), b, crc_in=0, crc_out=1) == _lib.HRS_EINVAL
    assert "input row 3 is NULL" in last_error(code)
    b = Buffers()
    b.outs[1] = None
    assert call(NAMES[0], code._handle(), b, crc_in=0, crc_out=1) == _lib.HRS_EINVAL
    assert "output row 1 is NULL" in last_error(code)
    assert b.untouched()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("shift", [1, S * N - 1, -1, -(S * N - 1)])
def test_rule_5_overlapping_crc_arrays_come_before_the_device(code, name, shift):
    b = Buffers()
    assert call(name, code._handle(), b, crc_in=S * N, crc_out=S * N + shift) == _lib.HRS_EINVAL
    assert "device" not in last_error(code)
    assert b.untouched()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("crcs", [dict(), dict(crc_in=None), dict(crc_in=0, crc_out=0), dict(crc_in=S * N, crc_out=0)],
                         ids=["apart", "fresh", "same_array", "adjacent"])
@pytest.mark.parametrize("fill", [0, L // 2, L], ids=["all_dead", "half", "all_full"])
def test_rule_6_valid_arguments_reach_the_device(code, name, fill, crcs):
    b = Buffers()
    b.valid[...] = fill
    b.valid_before = b.valid.copy()
    assert call(name, code._handle(), b, **crcs) == _lib.HRS_EDEVICE
    assert "device" in last_error(code)
    assert _lib.lib().hrs_last_host_path(code._handle()) == b""  # set only on success
    assert b.untouched()


# ---- the Python mirror

def test_mirror_checks_its_arguments_before_the_library(code):
    st = np.zeros((S, N, L), np.uint8)
    valid = np.full((S, K), L // 2, np.uint32)
    with pytest.raises(ValueError, match=r"valid must be \[S, 10\]"):
        device.encode_batch_host_ragged_crc(code, st, valid[:, :-1])
    with pytest.raises(ValueError, match="crc_in"):
        device.encode_batch_host_ragged_crc(code, st, valid, crc_in=np.zeros((S, K), np.uint32))
    with pytest.raises(ValueError, match="crc_out"):
        device.encode_batch_host_ragged_crc(code, st, valid, crc_out=np.zeros((S, N), np.int32))


def test_mirror_passes_valid_arguments_on(code):
    st = np.zeros((S, N, L), np.uint8)
    crc = np.full((S, N), POISON, np.uint32)
    for valid in ([[L // 2] * K] * S, np.full((S, K), L, np.int64)):
        with pytest.raises(HrsError) as ei:
            device.encode_batch_host_ragged_crc(code, st, valid, crc_in=crc, crc_out=crc)
        assert ei.value.status == _lib.HRS_EDEVICE
    with pytest.raises(HrsError) as ei:
        device.encode_batch_host_ragged_crc(code, st, np.full((S, K), L + 1), crc_out=crc)
    assert ei.value.status == _lib.HRS_EINVAL
    assert (crc == POISON).all()
